"""The batched-matching surface (dlco_desc_match_pairs and its forms, the DescContext methods, the tool match-pairs) on a machine
without a GPU: the C ABI is declared, exported and bound with the stated signatures, the argument checks that need no device,
the row offsets against numpy, and the paths of the tool that open no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
FUNCS = ["dlco_desc_match_pairs_rows", "dlco_desc_match_pairs", "dlco_desc_match_pairs_device", "dlco_desc_match_pairs_u8",
         "dlco_desc_match_pairs_u8_device", "dlco_desc_match_pairs_slices"]
METHODS = ["match_pairs", "match_pairs_u8", "match_pairs_device", "match_pairs_u8_device", "match_pairs_slices"]
USAGE = "Usage: match-pairs -pairs pairs_file -out dst_h5_filename [-u8] [-ratio f] [-cross] [-device n] desc_file_0 desc_file_1 ..."
f32p, i32p, i64p, u8p = (C.POINTER(t) for t in (C.c_float, C.c_int32, C.c_int64, C.c_uint8))


def test_functions_are_declared_exported_and_bound(dlco):
    declared = set(dlco.exported_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", dlco.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    L = dlco.load()
    for f in FUNCS:
        assert f in declared, f + " is not declared in include/dlco.h"
        assert f in exported, f + " is not exported by libdlco.so"
        assert getattr(L, f).argtypes is not None, f + " has no ctypes signature"
    for m in METHODS:
        assert callable(getattr(dlco.DescContext, m, None)), "DescContext." + m
    assert callable(dlco.match_pairs_rows)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert L.dlco_desc_match_pairs_rows.argtypes == [i64p, i32, i32p, i64, i64p]
    assert L.dlco_desc_match_pairs.argtypes == [vp, f32p, i64p, i32, i32p, i64, i32, i32p, f32p]
    assert L.dlco_desc_match_pairs_device.argtypes == [vp, vp, i64, i64p, i32, i32p, i64, i32, vp, vp]
    assert L.dlco_desc_match_pairs_u8.argtypes == [vp, u8p, i64p, i32, i32p, i64, i32, i32p, i32p]
    assert L.dlco_desc_match_pairs_u8_device.argtypes == [vp, vp, i64, i64p, i32, i32p, i64, i32, vp, vp]
    assert L.dlco_desc_match_pairs_slices.argtypes == [vp, i64p, i32, i32p, i64, i32, i32p]
    # the header states the same parameter lists
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    common = ["const int64_t *seg", "int32_t n_img", "const int32_t *pairs", "int64_t n_pairs"]
    assert params("dlco_desc_match_pairs_rows") == common + ["int64_t *row0"]
    assert params("dlco_desc_match_pairs") == ["dlco_desc_ctx *ctx", "const float *table_host"] + common + ["int32_t r", "int32_t *idx_host", "float *sqdist_host"]
    assert params("dlco_desc_match_pairs_device") == ["dlco_desc_ctx *ctx", "const float *table_dev", "int64_t ld"] + common + [
        "int32_t r", "int32_t *idx_dev", "float *sqdist_dev"]
    assert params("dlco_desc_match_pairs_u8") == ["dlco_desc_ctx *ctx", "const uint8_t *table_u8"] + common + ["int32_t r", "int32_t *idx_host",
                                                                                                            "int32_t *sqdist_host"]
    assert params("dlco_desc_match_pairs_u8_device") == ["dlco_desc_ctx *ctx", "const uint8_t *table_dev", "int64_t ld"] + common + [
        "int32_t r", "int32_t *idx_dev", "int32_t *sqdist_dev"]
    assert params("dlco_desc_match_pairs_slices") == ["dlco_desc_ctx *ctx"] + common + ["int32_t u8", "int32_t *slices"]
    # the header says what is out of scope, and the kernel-time comment covers the call
    raw = " ".join(open(dlco.HEADER_PATH).read().split())
    for words in ("guided forms of the batch", "a batched distance matrix", "seg / pairs in device memory", "a batched verify",
                  "after a match_pairs call, float or _u8, every kernel of the call"):
        assert words in raw, words


def test_calls_reject_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    E = dlco.ERR_INVALID
    tab, tab8 = np.zeros((10, 8), np.float32), np.zeros((10, 16), np.uint8)
    seg, pairs = np.array([0, 3, 3, 10], np.int64), np.array([[0, 2], [2, 0], [1, 2]], np.int32)
    idx, d, d8, sl, row0 = (np.full((10, 2), -5, np.int32), np.full((10, 2), -5, np.float32), np.full((10, 2), -5, np.int32), np.full(3, -5, np.int32),
                            np.full(4, -5, np.int64))
    p = lambda a, t: a.ctypes.data_as(t)
    v = lambda a: C.c_void_p(a.ctypes.data)
    good = dict(seg=p(seg, i64p), n_img=3, pairs=p(pairs, i32p), n_pairs=3, r=8)
    K = ("seg", "n_img", "pairs", "n_pairs")
    arg = lambda kw, keys: [{**good, **kw}[k] for k in keys]
    rows = lambda **kw: L.dlco_desc_match_pairs_rows(*arg({"row0": p(row0, i64p), **kw}, K + ("row0",)))
    host = lambda h, **kw: L.dlco_desc_match_pairs(h, *arg({"t": p(tab, f32p), "idx": p(idx, i32p), "d": p(d, f32p), **kw}, ("t",) + K + ("r", "idx", "d")))
    host8 = lambda h, **kw: L.dlco_desc_match_pairs_u8(h, *arg({"t": p(tab8, u8p), "idx": p(idx, i32p), "d": p(d8, i32p), **kw}, ("t",) + K + ("r", "idx", "d")))
    dev = lambda h, **kw: L.dlco_desc_match_pairs_device(h, *arg({"t": v(tab), "ld": 8, "idx": v(idx), "d": v(d), **kw}, ("t", "ld") + K + ("r", "idx", "d")))
    dev8 = lambda h, **kw: L.dlco_desc_match_pairs_u8_device(h, *arg({"t": v(tab8), "ld": 16, "idx": v(idx), "d": v(d8), **kw}, ("t", "ld") + K + ("r", "idx", "d")))
    slices = lambda h, **kw: L.dlco_desc_match_pairs_slices(h, *arg({"u8": 0, "sl": p(sl, i32p), **kw}, K + ("u8", "sl")))
    with_handle = (host, host8, dev, dev8, slices)
    for f in with_handle:
        assert f(None) == E                                # a null handle: invalid before anything touches a device
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(tab.ctypes.data)
    keep = []                                              # the arrays behind the pointers stay alive
    def segs(a):
        keep.append(np.array(a, np.int64))
        return dict(seg=p(keep[-1], i64p), n_img=len(a) - 1)
    def prs(a):
        keep.append(np.array(a, np.int32))
        return dict(pairs=p(keep[-1], i32p), n_pairs=len(a))
    bad = [dict(seg=None), dict(pairs=None), dict(n_img=0), dict(n_img=-1), dict(n_pairs=0), dict(n_pairs=-3),
           segs([1, 3, 3, 10]), segs([0, 3, 2, 10]), segs([0, 0, 0, 0]), segs([0, 3, 3 + 2 ** 31, 4 + 2 ** 31]),
           prs([[0, 3], [2, 0], [1, 2]]), prs([[0, 2], [-1, 0], [1, 2]]), prs([[0, 2], [2, 0], [1, 2 ** 20]])]
    for kw in bad:
        assert rows(**kw) == E, kw
        for f in with_handle:
            assert f(h, **kw) == E, (f, kw)
    assert rows(row0=None) == E and slices(h, sl=None) == E and slices(h, u8=2) == E and slices(h, u8=-1) == E
    for f in (host, host8, dev, dev8):
        for kw in (dict(t=None), dict(idx=None), dict(d=None), dict(r=0), dict(r=1025), dict(r=-8)):
            assert f(h, **kw) == E, (f, kw)
    for kw in (dict(ld=4), dict(ld=9), dict(ld=10), dict(ld=0), dict(ld=-8), dict(t=C.c_void_p(tab.ctypes.data + 4))):
        assert dev(h, **kw) == E, kw
    for kw in (dict(ld=8, r=16), dict(ld=24), dict(ld=20), dict(ld=0), dict(ld=-16), dict(t=C.c_void_p(tab8.ctypes.data + 8))):
        assert dev8(h, **{"r": 16, **kw}) == E, kw
    assert (idx == -5).all() and (d == -5).all() and (d8 == -5).all() and (sl == -5).all() and (row0 == -5).all()
    assert not tab.any() and not tab8.any()
    assert rows() == 0 and row0.tolist() == [0, 3, 10, 10]


def test_match_pairs_rows_against_numpy(dlco):
    rng = np.random.default_rng(11)
    for _ in range(20):
        n = rng.integers(0, 400, int(rng.integers(1, 12)))
        if n.sum() == 0:
            n[0] = 1
        seg = np.concatenate([[0], np.cumsum(n)])
        pairs = rng.integers(0, len(n), (int(rng.integers(1, 300)), 2))
        got = dlco.match_pairs_rows(seg, pairs)
        assert got.dtype == np.int64 and np.array_equal(got, np.concatenate([[0], np.cumsum(n[pairs[:, 0]])]))
    for seg, pairs in (([0, 3, 2], [[0, 1]]), ([0, 3], [[0, 1]]), ([1, 3], [[0, 0]]), ([0, 0], [[0, 0]])):
        try:
            dlco.match_pairs_rows(seg, pairs)
        except dlco.DlcoError as e:
            assert e.code == dlco.ERR_INVALID
        else:
            raise AssertionError((seg, pairs))


def _tool():
    subprocess.check_call(["make", "-s", "-C", CLI])
    return os.path.join(CLI, "match-pairs")


def test_usage_errors_exit_1():
    tool = _tool()
    full = ["-pairs", "p", "-out", "o", "a", "b"]
    for args, word in ((full + ["-ratio", "0"], "-ratio"), (full + ["-ratio", "1.5"], "-ratio"), (full + ["-bogus"], "Invalid -bogus option"),
                       (full + ["-device"], "Invalid -device option"), (full + ["-guided", "v"], "Invalid -guided option")):
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and USAGE in p.stdout and "ERROR" in p.stdout and word in p.stdout, (args, p.stdout)
    for args in (["-help"], ["-pairs", "p", "-out", "o"], ["-out", "o", "a", "b"], ["-pairs", "p", "a", "b"], []):
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and USAGE in p.stdout and "ERROR" not in p.stdout, (args, p.stdout)


def _write(d, tables, pairs, name="Descriptor"):
    files = []
    for k, t in enumerate(tables):
        (d / ("t%d" % k)).mkdir()
        np.save(d / ("t%d" % k) / (name + ".npy"), t)
        files.append(str(d / ("t%d" % k)))
    (d / "p").mkdir()
    np.save(d / "p" / "Pairs.npy", np.asarray(pairs, np.int32))
    return ["-pairs", str(d / "p"), "-out", str(d / "out"), "-device", "99"] + files


def test_tool_fails_before_a_device_is_opened(tmp_path):
    """bad inputs: exit 2 with a message, nothing written, and no device touched (-device 99 is one that no machine has:
    reaching it would be another message)"""
    tool = _tool()
    f = lambda n, r: np.ones((n, r), np.float32)
    nan = f(4, 8)
    nan[2, 3] = np.nan
    cases = [(([f(4, 8), f(5, 8)], [[0, 2]]), [], "names file 2 of 2"), (([f(4, 8), f(5, 8)], [[-1, 0]]), [], "names file -1 of 2"),
             (([f(4, 8), f(5, 6)], [[0, 1]]), [], "the descriptors differ in size: 8"), (([f(4, 8), nan], [[0, 1]]), [], "Descriptor contains NaN"),
             (([f(0, 8), f(0, 8)], [[0, 1]]), [], "every descriptor table is empty"), (([f(4, 8), f(5, 8)], np.zeros((0, 2), np.int32)), [], "Pairs must be"),
             (([f(4, 8), f(5, 8)], [[0, 1, 0]]), [], "Pairs must be"), (([f(4, 8), f(5, 8)], [[0, 1]]), ["-u8"], "DescriptorU8")]
    for k, ((tables, pairs), flags, word) in enumerate(cases):
        d = tmp_path / ("case%d" % k)
        d.mkdir()
        p = subprocess.run([tool] + _write(d, tables, pairs) + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.startswith("match-pairs: ") and word in p.stderr and not (d / "out").exists(), (k, p.stderr)
    # -u8: quantisers that differ in a bit
    d = tmp_path / "quant"
    d.mkdir()
    args = _write(d, [np.ones((4, 8), np.uint8)] * 3, [[0, 1], [1, 2]], "DescriptorU8")
    for k, scale in enumerate((0.5, 0.5, np.nextafter(np.float32(0.5), np.float32(1)))):
        np.save(d / ("t%d" % k) / "QuantScale.npy", np.array([scale], np.float32))
        np.save(d / ("t%d" % k) / "QuantOffset.npy", np.zeros(8, np.float32))
    p = subprocess.run([tool] + args + ["-u8"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("match-pairs: ") and "quantised differently" in p.stderr and not (d / "out").exists(), p.stderr
    # a missing file
    d = tmp_path / "missing"
    d.mkdir()
    args = _write(d, [f(4, 8), f(5, 8)], [[0, 1]])
    os.remove(d / "t1" / "Descriptor.npy")
    p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("match-pairs: ") and "Descriptor" in p.stderr and not (d / "out").exists()
    # good inputs reach the device that no machine has: the failure is the library's, and still nothing is written
    d = tmp_path / "good"
    d.mkdir()
    p = subprocess.run([tool] + _write(d, [f(4, 8), f(5, 8)], [[0, 1]]), capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("match-pairs: ") and not (d / "out").exists()
