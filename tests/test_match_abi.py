"""The matching surface (dlco_desc_match / match_device / cross_sqdists, the tool match) on a machine without a GPU: the C ABI
is declared and exported, argument checks that need no device, and the command line's usage rules."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
FUNCS = ["dlco_desc_match", "dlco_desc_match_device", "dlco_desc_cross_sqdists"]
METHODS = ["match", "match_device", "cross_sqdists"]


def test_match_functions_are_declared_and_exported(dlco):
    declared = set(dlco.exported_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", dlco.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    for f in FUNCS:
        assert f in declared, f + " is not declared in include/dlco.h"
        assert f in exported, f + " is not exported by libdlco.so"
    L = dlco.load()
    for f in FUNCS:
        assert getattr(L, f).argtypes is not None, f + " has no ctypes signature"
    for m in METHODS:
        assert callable(getattr(dlco.DescContext, m, None)), "DescContext." + m
    header = open(dlco.HEADER_PATH).read()
    assert "NOT guaranteed to give exactly 0" in header            # the contract the header has to state (unlike pair_sqdists)


def test_match_rejects_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    q, t = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32)
    idx, d, out = np.zeros((3, 2), np.int32), np.zeros((3, 2), np.float32), np.zeros((3, 5), np.float32)
    Qp, Tp, Ip, Dp, Op = q.ctypes.data_as(f32p), t.ctypes.data_as(f32p), idx.ctypes.data_as(i32p), d.ctypes.data_as(f32p), out.ctypes.data_as(f32p)
    vq, vt, vi, vd = (C.c_void_p(a.ctypes.data) for a in (q, t, idx, d))
    INV = dlco.ERR_INVALID
    # a null handle: invalid before anything touches a device
    assert L.dlco_desc_match(None, Qp, 3, Tp, 5, 8, Ip, Dp) == INV
    assert L.dlco_desc_match_device(None, vq, 8, 3, vt, 8, 5, 8, vi, vd) == INV
    assert L.dlco_desc_cross_sqdists(None, Qp, 3, Tp, 5, 8, Op) == INV
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(out.ctypes.data)
    for args in ((None, 3, Tp, 5, 8, Ip, Dp), (Qp, 3, None, 5, 8, Ip, Dp), (Qp, 3, Tp, 5, 8, None, Dp), (Qp, 3, Tp, 5, 8, Ip, None),
                 (Qp, 3, Tp, 5, 0, Ip, Dp), (Qp, 3, Tp, 5, 1025, Ip, Dp), (Qp, 3, Tp, 5, -1, Ip, Dp), (Qp, 0, Tp, 5, 8, Ip, Dp),
                 (Qp, 3, Tp, 0, 8, Ip, Dp), (Qp, -1, Tp, 5, 8, Ip, Dp), (Qp, 3, Tp, 1 << 31, 8, Ip, Dp)):
        assert L.dlco_desc_match(h, *args) == INV, args
    for args in ((None, 3, Tp, 5, 8, Op), (Qp, 3, None, 5, 8, Op), (Qp, 3, Tp, 5, 8, None), (Qp, 3, Tp, 5, 0, Op), (Qp, 3, Tp, 5, 1025, Op),
                 (Qp, 0, Tp, 5, 8, Op), (Qp, 3, Tp, 0, 8, Op), (Qp, (1 << 14) + 1, Tp, 1 << 14, 8, Op)):        # the last: above 2^28 entries
        assert L.dlco_desc_cross_sqdists(h, *args) == INV, args
    for args in ((None, 8, 3, vt, 8, 5, 8, vi, vd), (vq, 8, 3, None, 8, 5, 8, vi, vd), (vq, 8, 3, vt, 8, 5, 8, None, vd),
                 (vq, 8, 3, vt, 8, 5, 8, vi, None), (vq, 8, 3, vt, 8, 5, 0, vi, vd), (vq, 1028, 3, vt, 1028, 5, 1025, vi, vd),
                 (vq, 8, 0, vt, 8, 5, 8, vi, vd), (vq, 8, 3, vt, 8, 0, 8, vi, vd),
                 (vq, 4, 3, vt, 8, 5, 8, vi, vd), (vq, 8, 3, vt, 4, 5, 8, vi, vd),              # a pitch below r
                 (vq, 9, 3, vt, 8, 5, 8, vi, vd), (vq, 8, 3, vt, 10, 5, 8, vi, vd),             # a pitch that is not a multiple of 4
                 (vq, 6, 3, vt, 8, 5, 5, vi, vd)):
        assert L.dlco_desc_match_device(h, *args) == INV, args


def _tool():
    subprocess.check_call(["make", "-s", "-C", CLI])
    return os.path.join(CLI, "match")


def test_match_usage_exits_1():
    tool = _tool()
    full = ["q", "t", "-out", "o"]
    cases = [[], ["only_one"], ["q", "t"], ["q", "-out", "o"], ["-help"] + full, full + ["third_positional"], full + ["-bogus"],
             full + ["-ratio"], full + ["-ratio", "0"], full + ["-ratio", "1.5"], ["q", "t", "-out"]]
    for args in cases:
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, (args, p.returncode, p.stderr)
        assert "Usage: match query_desc_file train_desc_file -out" in p.stdout and "[-ratio f] [-cross] [-device n]" in p.stdout, args
    p = subprocess.run([tool, "q", "t", "-x"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stdout.startswith("ERROR: Invalid -x option.")


def test_match_missing_or_unfit_input_exits_2(tmp_path):
    """A runtime failure is a message on stderr and exit 2, before any device is opened: files that do not exist, tables of
    different widths, a NaN in a table."""
    tool = _tool()
    out = tmp_path / "out"
    p = subprocess.run([tool, str(tmp_path / "no_q"), str(tmp_path / "no_t"), "-out", str(out), "-cross", "-ratio", "0.8"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("match: ") and not out.exists()
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d_, arr in ((a, np.ones((4, 8), np.float32)), (b, np.ones((3, 12), np.float32)), (c, np.full((2, 8), np.nan, np.float32))):
        d_.mkdir()
        np.save(d_ / "Descriptor.npy", arr)
    p = subprocess.run([tool, str(a), str(b), "-out", str(out)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("match: the descriptors differ in size") and not out.exists()
    p = subprocess.run([tool, str(a), str(c), "-out", str(out)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("match: ") and "NaN" in p.stderr and not out.exists()
