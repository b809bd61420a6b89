"""The verification surface (dlco_desc_verify_homography, dlco_desc_verify_hypotheses, DescContext.verify_homography /
verify_hypotheses, the tool verify) on a machine without a GPU: the C ABI is declared, exported and bound with the stated
signatures, the argument checks that need no device, and the paths of the tool that open none."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
FUNCS = ["dlco_desc_verify_homography", "dlco_desc_verify_hypotheses"]
METHODS = ["verify_homography", "verify_hypotheses"]
USAGE = "Usage: verify query_kp_file train_kp_file match_file -out dst_h5_filename [-thresh f] [-hyp n] [-seed n] [-refine n] [-device n]"


def test_verify_functions_are_declared_exported_and_bound(dlco):
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
    f32p, f64p, u8p, i64p, i32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_uint8, C.c_int64, C.c_int32))
    assert L.dlco_desc_verify_homography.argtypes == [vp, f32p, f32p, i64, f32, i32, u64, i32, f64p, u8p, i64p, i32p]
    assert L.dlco_desc_verify_hypotheses.argtypes == [vp, f32p, f32p, i64, f32, i32, u64, f64p, i32p]
    # the header states the same parameter lists
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    assert params("dlco_desc_verify_homography") == ["dlco_desc_ctx *ctx", "const float *src_xy_host", "const float *dst_xy_host", "int64_t m", "float threshold",
                                                     "int32_t n_hyp", "uint64_t seed", "int32_t refine", "double *H_out", "uint8_t *inlier_host",
                                                     "int64_t *n_inliers", "int32_t *best_hyp"]
    assert params("dlco_desc_verify_hypotheses") == ["dlco_desc_ctx *ctx", "const float *src_xy_host", "const float *dst_xy_host", "int64_t m", "float threshold",
                                                     "int32_t n_hyp", "uint64_t seed", "double *H_all_host", "int32_t *count_host"]
    import inspect
    sig = inspect.signature(dlco.DescContext.verify_homography)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[3:]] == [("threshold", 3.0), ("n_hyp", 2048), ("seed", 0), ("refine", 2)]
    # the header says what is out of scope, and the kernel-time comment names the verify kernels
    raw = " ".join(open(dlco.HEADER_PATH).read().split())
    for words in ("a device-memory form (the match list is filtered on the host)", "a fundamental or essential matrix", "symmetric transfer error",
                  "an adaptive hypothesis count", "after a * verify call the verify kernels"):
        assert words in raw, words


def test_verify_rejects_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    f32p, f64p, u8p, i64p, i32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_uint8, C.c_int64, C.c_int32))
    src, dst = np.zeros((8, 2), np.float32), np.zeros((8, 2), np.float32)
    H, mask, n, best = np.full(9, -5.0), np.full(8, 9, np.uint8), C.c_int64(-5), C.c_int32(-5)
    H_all, count = np.full((4, 9), -5.0), np.full(4, -5, np.int32)
    S, D, Hp, Mp, HA, Cn = src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p), H.ctypes.data_as(f64p), mask.ctypes.data_as(u8p), H_all.ctypes.data_as(f64p), count.ctypes.data_as(i32p)
    E = dlco.ERR_INVALID
    good = dict(src=S, dst=D, m=8, threshold=3.0, n_hyp=4, seed=0, refine=2, H=Hp, mask=Mp, n=C.byref(n), best=C.byref(best))
    homography = lambda h, **kw: L.dlco_desc_verify_homography(h, *[{**good, **kw}[k] for k in ("src", "dst", "m", "threshold", "n_hyp", "seed", "refine", "H", "mask", "n", "best")])
    hypotheses = lambda h, **kw: L.dlco_desc_verify_hypotheses(h, *[{**good, "H": HA, "n": Cn, **kw}[k] for k in ("src", "dst", "m", "threshold", "n_hyp", "seed", "H", "n")])
    assert homography(None) == E and hypotheses(None) == E                  # a null handle: invalid before anything touches a device
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(src.ctypes.data)
    bad = [dict(src=None), dict(dst=None), dict(m=3), dict(m=0), dict(m=-1), dict(m=2 ** 31), dict(m=2 ** 40), dict(threshold=0.0), dict(threshold=-1.0),
           dict(threshold=float("nan")), dict(threshold=float("inf")), dict(n_hyp=0), dict(n_hyp=-1), dict(n_hyp=2 ** 20 + 1)]
    for kw in bad:
        assert homography(h, **kw) == E, kw
        assert hypotheses(h, **kw) == E, kw
    for kw in (dict(refine=-1), dict(refine=9), dict(H=None), dict(n=None)):
        assert homography(h, **kw) == E, kw
    for kw in (dict(H=None), dict(n=None)):
        assert hypotheses(h, **kw) == E, kw
    assert (H == -5).all() and (mask == 9).all() and (n.value, best.value) == (-5, -5) and (H_all == -5).all() and (count == -5).all()
    assert not src.any() and not dst.any()


def test_verify_usage_text_and_exit_status():
    subprocess.check_call(["make", "-s", "-C", CLI])
    tool = os.path.join(CLI, "verify")
    for args in (["-help"], [], ["q", "t", "m"], ["q", "t", "-out", "o"], ["q", "t", "m", "x", "-out", "o"], ["q", "t", "m", "-out", "o", "-hyp", "64", "-help"]):
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and USAGE in p.stdout and "ERROR" not in p.stdout, (args, p.returncode, p.stdout)
    for args, word in ((["-bogus"], "Invalid -bogus option"), (["-thresh", "0"], "-thresh"), (["-thresh", "nan"], "-thresh"), (["-hyp", "0"], "-hyp"),
                       (["-hyp", "1048577"], "-hyp"), (["-refine", "9"], "-refine"), (["-refine", "-1"], "-refine")):
        p = subprocess.run([tool, "q", "t", "m", "-out", "o"] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and USAGE in p.stdout and "ERROR" in p.stdout and word in p.stdout, (args, p.stdout)


def write_inputs(tmp_path, nq, nt, matches):
    for name, n in (("query", nq), ("train", nt)):
        (tmp_path / name).mkdir()
        np.save(tmp_path / name / "Keypoints.npy", np.arange(4 * n, dtype=np.float32).reshape(n, 4))
    (tmp_path / "matches").mkdir()
    np.save(tmp_path / "matches" / "Matches.npy", np.array(matches, np.int32).reshape(-1, 2))
    return [str(tmp_path / "query"), str(tmp_path / "train"), str(tmp_path / "matches"), "-out", str(tmp_path / "out")]


def test_verify_tool_fails_before_a_device_is_opened(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CLI])
    tool = os.path.join(CLI, "verify")
    p = subprocess.run([tool, str(tmp_path / "none"), str(tmp_path / "none"), str(tmp_path / "none"), "-out", str(tmp_path / "o")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("verify: ") and "Keypoints.npy" in p.stderr
    for k, bad in enumerate(((5, 0), (0, 7), (-1, 0), (0, -1))):
        d = tmp_path / ("case%d" % k)
        d.mkdir()
        args = write_inputs(d, 5, 7, [(0, 0), (1, 1), (2, 2), (3, 3), bad, (4, 6)])
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.startswith("verify: match 4 = (%d, %d) is outside" % bad) and not os.path.exists(d / "out"), p.stderr


def test_verify_tool_with_fewer_than_four_matches_needs_no_device(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CLI])
    tool = os.path.join(CLI, "verify")
    for m in (0, 3):
        d = tmp_path / ("m%d" % m)
        d.mkdir()
        args = write_inputs(d, 5, 7, [(i, i + 1) for i in range(m)])
        p = subprocess.run([tool] + args + ["-device", "99"], capture_output=True, text=True, timeout=60)      # a device that no machine has
        assert p.returncode == 0, p.stderr
        assert "Matches: %d\n" % m in p.stdout and "Inliers: 0 / %d\n" % m in p.stdout and "Hypothesis: -1\n" in p.stdout and "Total: " in p.stdout
        out = d / "out"
        H, bits, inl, kept, best = (np.load(out / (n + ".npy")) for n in ("Homography", "HomographyBits", "Inlier", "VerifiedMatches", "BestHypothesis"))
        assert H.dtype == np.float32 and H.shape == (3, 3) and not H.any() and bits.dtype == np.int64 and bits.shape == (9,) and not bits.any()
        assert inl.dtype == np.uint8 and inl.shape == (m,) and not inl.any() and kept.dtype == np.int32 and kept.shape == (0, 2)
        assert best.dtype == np.int32 and best.tolist() == [-1]
