"""The learnt-descriptor surface (dlco_desc_set_projection / describe / pair_sqdists / pair_stats, the tools describe and
eval-patches) on a machine without a GPU: the C ABI is declared and exported, argument checks that need no device, and the
command lines' usage rules."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
FUNCS = ["dlco_desc_set_projection", "dlco_desc_projected_size", "dlco_desc_describe", "dlco_desc_describe_device",
         "dlco_desc_pair_sqdists", "dlco_desc_pair_stats"]
METHODS = ["set_projection", "projected_size", "describe", "describe_device", "pair_sqdists", "pair_stats"]


def test_describe_functions_are_declared_and_exported(dlco):
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
        assert hasattr(dlco.DescContext, m), "DescContext." + m
    assert isinstance(dlco.DescContext.projected_size, property)


def test_describe_rejects_null_arguments_without_a_device(dlco):
    L = dlco.load()
    f32p, u8p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    W = np.ones((2, 8), np.float32)
    patches = np.zeros((1, 64, 64), np.uint8)
    pairs = np.zeros((1, 4), np.int32)
    out = np.zeros(8, np.float32)
    lab = np.zeros(1, np.uint8)
    dim, f, a = C.c_int32(), C.c_float(), C.c_double()
    Wp, Pp, Qp, Op, Lp = (W.ctypes.data_as(f32p), patches.ctypes.data_as(u8p), pairs.ctypes.data_as(i32p), out.ctypes.data_as(f32p),
                          lab.ctypes.data_as(u8p))
    # a null handle: invalid before anything touches a device
    assert L.dlco_desc_set_projection(None, Wp, 2, 8) == dlco.ERR_INVALID
    assert L.dlco_desc_projected_size(None) == 0
    assert L.dlco_desc_describe(None, Pp, 1, Op) == dlco.ERR_INVALID
    assert L.dlco_desc_describe_device(None, Pp, 1, C.c_void_p(out.ctypes.data), 8) == dlco.ERR_INVALID
    assert L.dlco_desc_pair_sqdists(None, Pp, 1, Qp, 1, Op, Lp) == dlco.ERR_INVALID
    assert L.dlco_desc_pair_stats(None, Pp, 1, Qp, 1, C.byref(dim), C.byref(f), C.byref(a)) == dlco.ERR_INVALID
    # null data pointers are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(out.ctypes.data)
    assert L.dlco_desc_set_projection(h, None, 2, 8) == dlco.ERR_INVALID
    assert L.dlco_desc_describe(h, None, 1, Op) == dlco.ERR_INVALID
    assert L.dlco_desc_describe(h, Pp, 1, None) == dlco.ERR_INVALID
    assert L.dlco_desc_describe(h, Pp, 0, Op) == dlco.ERR_INVALID
    assert L.dlco_desc_describe_device(h, Pp, 1, None, 8) == dlco.ERR_INVALID
    assert L.dlco_desc_pair_sqdists(h, None, 1, Qp, 1, Op, Lp) == dlco.ERR_INVALID
    assert L.dlco_desc_pair_sqdists(h, Pp, 1, None, 1, Op, Lp) == dlco.ERR_INVALID
    assert L.dlco_desc_pair_sqdists(h, Pp, 1, Qp, 1, None, Lp) == dlco.ERR_INVALID
    assert L.dlco_desc_pair_stats(h, Pp, 1, Qp, 1, C.byref(dim), None, C.byref(a)) == dlco.ERR_INVALID
    assert L.dlco_desc_pair_stats(h, Pp, 1, Qp, 1, C.byref(dim), C.byref(f), None) == dlco.ERR_INVALID
    assert L.dlco_desc_pair_stats(h, None, 1, Qp, 1, C.byref(dim), C.byref(f), C.byref(a)) == dlco.ERR_INVALID


def _tool(name):
    subprocess.check_call(["make", "-s", "-C", CLI])
    return os.path.join(CLI, name)


@pytest.mark.parametrize("name,needs_out", [("describe", True), ("eval-patches", False)])
def test_tools_usage_exits_1(name, needs_out):
    tool = _tool(name)
    full = ["flt", "img", "-prj", "p", "-id", "0", "-pj", "m"] + (["-out", "o"] if needs_out else [])
    cases = [[], ["only_one"], ["flt", "img"], ["flt", "img", "-prj", "p"], ["-help"] + full, full + ["third_positional"], full + ["-bogus"]]
    if needs_out:
        cases.append(full[:-2])                                   # no -out
    for args in cases:
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, (args, p.returncode, p.stderr)
        assert "Usage: %s src_h5_filter_file src_h5_img_file" % name in p.stdout, args
    p = subprocess.run([tool, "flt", "img", "-x"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stdout.startswith("ERROR: Invalid -x option.")


@pytest.mark.parametrize("name,needs_out", [("describe", True), ("eval-patches", False)])
def test_tools_missing_input_exits_2(name, needs_out, tmp_path):
    """A runtime failure (here: files that do not exist) is a message on stderr and exit 2, before any device is opened."""
    tool = _tool(name)
    args = [str(tmp_path / "no_filters"), str(tmp_path / "no_images"), "-prj", str(tmp_path / "no_prj"), "-id", "0", "-pj", str(tmp_path / "no_pj")]
    if needs_out:
        args += ["-out", str(tmp_path / "out")]
    p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith(name + ": ")
