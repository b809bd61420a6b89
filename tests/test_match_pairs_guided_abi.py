"""The guided batch (dlco_desc_match_pairs_guided and its forms, the DescContext methods) on a machine without a GPU: the C ABI
is declared, exported and bound with the stated signatures, and every argument check that needs no device returns
DLCO_ERR_INVALID with a null or never-used handle and leaves the outputs alone."""
import ctypes as C
import re
import subprocess

import numpy as np

FUNCS = ["dlco_desc_match_pairs_guided", "dlco_desc_match_pairs_guided_device", "dlco_desc_match_pairs_guided_epipolar",
         "dlco_desc_match_pairs_guided_epipolar_device"]
METHODS = ["match_pairs_guided", "match_pairs_guided_device", "match_pairs_guided_epipolar", "match_pairs_guided_epipolar_device"]
f32p, f64p, i32p, i64p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int32, C.c_int64))


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
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    host = [vp, f32p, f32p, i64p, i32, i32p, i64, i32, f64p, C.c_float, i32, i32p, f32p]
    dev = [vp, vp, i64, vp, i64, i64p, i32, i32p, i64, i32, f64p, C.c_float, i32, vp, vp]
    assert L.dlco_desc_match_pairs_guided.argtypes == host and L.dlco_desc_match_pairs_guided_epipolar.argtypes == host
    assert L.dlco_desc_match_pairs_guided_device.argtypes == dev and L.dlco_desc_match_pairs_guided_epipolar_device.argtypes == dev
    # the header states the same parameter lists
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    common = ["const int64_t *seg", "int32_t n_img", "const int32_t *pairs", "int64_t n_pairs", "int32_t r"]
    for name, mat, thr, side in (("dlco_desc_match_pairs_guided", "H", "radius", "h_side"), ("dlco_desc_match_pairs_guided_epipolar", "F", "threshold", "f_side")):
        model = ["const double *" + mat, "float " + thr, "int32_t " + side]
        assert params(name) == ["dlco_desc_ctx *ctx", "const float *table_host", "const float *xy_host"] + common + model + [
            "int32_t *idx_host", "float *sqdist_host"]
        assert params(name + "_device") == ["dlco_desc_ctx *ctx", "const float *table_dev", "int64_t ld", "const float *xy_dev", "int64_t ldxy"] + \
            common + model + ["int32_t *idx_dev", "float *sqdist_dev"]
    raw = " ".join(open(dlco.HEADER_PATH).read().split())
    assert "Out of scope: guided forms of the batch" not in raw
    for words in ("the matrix H + 9 p", "An all-zero matrix is the verification's \"no model\"", "at most 2^22 record"):
        assert words in raw, words


def test_calls_reject_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    E = dlco.ERR_INVALID
    tab, xy = np.zeros((10, 8), np.float32), np.zeros((10, 4), np.float32)
    seg, pairs = np.array([0, 3, 3, 10], np.int64), np.array([[0, 2], [2, 0], [1, 2]], np.int32)
    M = np.tile(np.eye(3).reshape(1, 9), (3, 1))
    idx, d = np.full((10, 2), -5, np.int32), np.full((10, 2), -5, np.float32)
    p = lambda a, t: a.ctypes.data_as(t)
    v = lambda a: C.c_void_p(a.ctypes.data)
    good = dict(seg=p(seg, i64p), n_img=3, pairs=p(pairs, i32p), n_pairs=3, r=8, M=p(M, f64p), t=np.float32(6.0), side=0)
    K = ("seg", "n_img", "pairs", "n_pairs", "r", "M", "t", "side")
    arg = lambda kw, keys: [{**good, **kw}[k] for k in keys]

    def host_of(fn):
        return lambda h, **kw: fn(h, *arg({"tab": p(tab, f32p), "xy": p(xy, f32p), "idx": p(idx, i32p), "d": p(d, f32p), **kw}, ("tab", "xy") + K + ("idx", "d")))

    def dev_of(fn):
        return lambda h, **kw: fn(h, *arg({"tab": v(tab), "ld": 8, "xy": v(xy), "ldxy": 4, "idx": v(idx), "d": v(d), **kw},
                                       ("tab", "ld", "xy", "ldxy") + K + ("idx", "d")))

    hosts = [host_of(L.dlco_desc_match_pairs_guided), host_of(L.dlco_desc_match_pairs_guided_epipolar)]
    devs = [dev_of(L.dlco_desc_match_pairs_guided_device), dev_of(L.dlco_desc_match_pairs_guided_epipolar_device)]
    for f in hosts + devs:
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

    def mats(pair, entry, value):
        keep.append(M.copy())
        keep[-1][pair, entry] = value
        return dict(M=p(keep[-1], f64p))

    # whatever dlco_desc_match_pairs rejects
    bad = [dict(seg=None), dict(pairs=None), dict(n_img=0), dict(n_img=-1), dict(n_pairs=0), dict(n_pairs=-3),
           segs([1, 3, 3, 10]), segs([0, 3, 2, 10]), segs([0, 0, 0, 0]), segs([0, 3, 3 + 2 ** 31, 4 + 2 ** 31]),
           prs([[0, 3], [2, 0], [1, 2]]), prs([[0, 2], [-1, 0], [1, 2]]), prs([[0, 2], [2, 0], [1, 2 ** 20]]),
           dict(tab=None), dict(idx=None), dict(d=None), dict(r=0), dict(r=1025), dict(r=-8)]
    # and what the guided forms add: null xy or matrices, a non-finite entry in ANY of the matrices (the last pair's too, and of a
    # pair whose query image is empty), a radius or threshold that is not finite or <= 0, a side other than 0 or 1
    bad += [dict(xy=None), dict(M=None), mats(0, 0, np.nan), mats(2, 8, np.inf), mats(1, 4, -np.inf), mats(2, 5, np.nan),
            dict(t=np.float32(0.0)), dict(t=np.float32(-1.0)), dict(t=np.float32(np.nan)), dict(t=np.float32(np.inf)),
            dict(side=2), dict(side=-1)]
    for kw in bad:
        for f in hosts + devs:
            assert f(h, **kw) == E, kw
    for kw in (dict(ld=4), dict(ld=9), dict(ld=10), dict(ld=0), dict(ld=-8), dict(tab=C.c_void_p(tab.ctypes.data + 4)),
               dict(ldxy=1), dict(ldxy=0), dict(ldxy=-4), dict(xy=C.c_void_p(xy.ctypes.data + 2))):
        for f in devs:
            assert f(h, **kw) == E, kw
    assert (idx == -5).all() and (d == -5).all() and not tab.any() and not xy.any()
    assert np.array_equal(M, np.tile(np.eye(3).reshape(1, 9), (3, 1)))
