"""The entry points of the verification on device-resident lists, without a GPU: dlco_desc_verify_pairs_homography_device,
dlco_desc_verify_pairs_fundamental_device and the test entry dlco_desc_verify_pairs_refit_round are declared, exported and bound
with the stated signatures, and refuse bad arguments before the handle is used and with no output touched."""
import ctypes as C
import inspect
import re
import subprocess

import numpy as np

FUNCS = ["dlco_desc_verify_pairs_homography_device", "dlco_desc_verify_pairs_fundamental_device", "dlco_desc_verify_pairs_refit_round"]
METHODS = ["verify_pairs_homography_device", "verify_pairs_fundamental_device", "verify_pairs_refit_round"]
f32p, f64p, i32p, i64p, u8p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int32, C.c_int64, C.c_uint8))


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
    vp, i64, i32, u64, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_float
    model = [vp, vp, vp, i64p, i64, f32, i32, u64, i32, f64p, vp, i64p, i32p]
    assert L.dlco_desc_verify_pairs_homography_device.argtypes == model and L.dlco_desc_verify_pairs_fundamental_device.argtypes == model
    assert L.dlco_desc_verify_pairs_refit_round.argtypes == [vp, f32p, f32p, i64p, i64, u8p, i32, f64p, u8p]
    # the header states the same parameter lists
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    common = ["dlco_desc_ctx *ctx", "const float *src_xy_dev", "const float *dst_xy_dev", "const int64_t *moff", "int64_t n_pairs", "float threshold",
              "int32_t n_hyp", "uint64_t seed", "int32_t refine"]
    tail = ["uint8_t *inlier_dev", "int64_t *n_inliers", "int32_t *best_hyp"]
    assert params("dlco_desc_verify_pairs_homography_device") == common + ["double *H_out"] + tail
    assert params("dlco_desc_verify_pairs_fundamental_device") == common + ["double *F_out"] + tail
    assert params("dlco_desc_verify_pairs_refit_round") == ["dlco_desc_ctx *ctx", "const float *src_xy_host", "const float *dst_xy_host", "const int64_t *moff",
                                                           "int64_t n_pairs", "const uint8_t *mask_host", "int32_t fundamental", "double *M_out", "uint8_t *ok"]
    for name, thr in (("verify_pairs_homography_device", 3.0), ("verify_pairs_fundamental_device", 1.0)):
        sig = inspect.signature(getattr(dlco.DescContext, name))
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("src_ptr", inspect.Parameter.empty), ("dst_ptr", inspect.Parameter.empty),
                                                                                   ("moff", inspect.Parameter.empty), ("threshold", thr), ("n_hyp", 2048),
                                                                                   ("seed", 0), ("refine", 2), ("inlier_ptr", None)]
    # the header: the device form is in scope now, and the kernel-time comment covers the new kernels
    raw = " ".join(l.strip().lstrip("*").strip() for l in open(dlco.HEADER_PATH).read().splitlines())
    raw = " ".join(raw.split())
    for words in ("In scope since: the device-memory form, dlco_desc_verify_pairs_*_device below, with its refit on the device.",
                  "the _device forms all of that and, for every round, the refit and the step kernel",
                  "a src_xy_dev or dst_xy_dev that is not 8-byte aligned is DLCO_ERR_INVALID as well"):
        assert words in raw, words
    assert "its refit runs on the host and needs the list there anyway" not in raw


def test_calls_reject_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    E = dlco.ERR_INVALID
    src, dst = np.zeros((21, 2), np.float32), np.zeros((21, 2), np.float32)          # host memory stands in: nothing is read
    assert src.ctypes.data % 8 == 0 and dst.ctypes.data % 8 == 0
    moff = np.array([0, 8, 8, 20], np.int64)
    H, n, best, ok = np.full((3, 9), -5.0), np.full(3, -5, np.int64), np.full(3, -5, np.int32), np.full(3, 7, np.uint8)
    mask = np.full(20, 9, np.uint8)
    p = lambda a, t: a.ctypes.data_as(t)
    good = dict(src=src.ctypes.data, dst=dst.ctypes.data, moff=p(moff, i64p), n_pairs=3, threshold=3.0, n_hyp=4, seed=0, refine=2, H=p(H, f64p),
                mask=mask.ctypes.data, n=p(n, i64p), best=p(best, i32p))
    MK = ("src", "dst", "moff", "n_pairs", "threshold", "n_hyp", "seed", "refine", "H", "mask", "n", "best")
    models = [lambda h, f=f, **kw: f(h, *[{**good, **kw}[k] for k in MK]) for f in (L.dlco_desc_verify_pairs_homography_device, L.dlco_desc_verify_pairs_fundamental_device)]
    rgood = dict(src=p(src, f32p), dst=p(dst, f32p), moff=p(moff, i64p), n_pairs=3, mask=p(mask, u8p), fundamental=0, H=p(H, f64p), ok=p(ok, u8p))
    RK = ("src", "dst", "moff", "n_pairs", "mask", "fundamental", "H", "ok")
    refit = lambda h, **kw: L.dlco_desc_verify_pairs_refit_round(h, *[{**rgood, **kw}[k] for k in RK])
    for f in models + [refit]:
        assert f(None) == E                                # a null handle: invalid before anything touches a device
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(src.ctypes.data)
    keep = []
    def offs(a):
        keep.append(np.array(a, np.int64))
        return dict(moff=p(keep[-1], i64p), n_pairs=len(a) - 1)
    offsets = [dict(moff=None), dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=2 ** 31), offs([1, 8, 8, 20]), offs([0, 8, 7, 20]), offs([0, -1, 8, 20]),
               offs([0, 8, 8 + 2 ** 31, 9 + 2 ** 31])]
    limits = [dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(n_hyp=0), dict(n_hyp=-1),
              dict(n_hyp=2 ** 20 + 1), dict(refine=-1), dict(refine=9)]
    misaligned = [dict(src=src.ctypes.data + 4), dict(dst=dst.ctypes.data + 4), dict(src=src.ctypes.data + 1)]
    for kw in offsets + limits + misaligned + [dict(src=None), dict(dst=None), dict(H=None), dict(n=None)]:
        for f in models:
            assert f(h, **kw) == E, kw
    for kw in offsets + [dict(src=None), dict(dst=None), dict(mask=None), dict(H=None), dict(ok=None), dict(fundamental=2), dict(fundamental=-1)]:
        assert refit(h, **kw) == E, kw
    assert (H == -5).all() and (mask == 9).all() and (n == -5).all() and (best == -5).all() and (ok == 7).all()
    assert not src.any() and not dst.any()
