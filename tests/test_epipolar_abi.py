"""The epipolar verification surface (dlco_desc_verify_fundamental, dlco_desc_verify_fundamental_hypotheses,
DescContext.verify_fundamental / verify_fundamental_hypotheses, the tool verify -model) on a machine without a GPU: the C ABI is
declared, exported and bound with the stated signatures, the argument checks that need no device, and the paths of the tool that
open none."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
FUNCS = ["dlco_desc_verify_fundamental", "dlco_desc_verify_fundamental_hypotheses"]
USAGE = "Usage: verify query_kp_file train_kp_file match_file -out dst_h5_filename [-thresh f] [-hyp n] [-seed n] [-refine n] [-device n]"
MODEL_LINE = "-model homography|fundamental"


def test_fundamental_functions_are_declared_exported_and_bound(dlco):
    declared = set(dlco.exported_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", dlco.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    L = dlco.load()
    for f in FUNCS:
        assert f in declared, f + " is not declared in include/dlco.h"
        assert f in exported, f + " is not exported by libdlco.so"
    vp, i64, i32, u64, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_float
    f32p, f64p, u8p, i64p, i32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_uint8, C.c_int64, C.c_int32))
    assert L.dlco_desc_verify_fundamental.argtypes == [vp, f32p, f32p, i64, f32, i32, u64, i32, f64p, u8p, i64p, i32p]
    assert L.dlco_desc_verify_fundamental_hypotheses.argtypes == [vp, f32p, f32p, i64, f32, i32, u64, f64p, i32p]
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    assert params("dlco_desc_verify_fundamental") == ["dlco_desc_ctx *ctx", "const float *src_xy_host", "const float *dst_xy_host", "int64_t m", "float threshold",
                                                      "int32_t n_hyp", "uint64_t seed", "int32_t refine", "double *F_out", "uint8_t *inlier_host",
                                                      "int64_t *n_inliers", "int32_t *best_hyp"]
    assert params("dlco_desc_verify_fundamental_hypotheses") == ["dlco_desc_ctx *ctx", "const float *src_xy_host", "const float *dst_xy_host", "int64_t m",
                                                                 "float threshold", "int32_t n_hyp", "uint64_t seed", "double *F_all_host", "int32_t *count_host"]
    sig = inspect.signature(dlco.DescContext.verify_fundamental)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[3:]] == [("threshold", 1.0), ("n_hyp", 2048), ("seed", 0), ("refine", 2)]
    sig = inspect.signature(dlco.DescContext.verify_fundamental_hypotheses)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[3:]] == [("threshold", 1.0), ("n_hyp", 2048), ("seed", 0)]
    # the header says what the model is, what refine = 0 returns and what stays out of scope
    raw = " ".join(open(dlco.HEADER_PATH).read().replace(" * ", " ").split())
    for words in ("It is NOT cv::findFundamentalMat", "which need not be singular", "of rank 2 up to rounding", "Degeneracy is documented and not detected",
                  "a seven-point solver", "an essential matrix", "an epipolar predicate for guided matching", "except m >= 8"):
        assert words in raw, words


def test_fundamental_rejects_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    f32p, f64p, u8p, i64p, i32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_uint8, C.c_int64, C.c_int32))
    src, dst = np.zeros((16, 2), np.float32), np.zeros((16, 2), np.float32)
    F, mask, n, best = np.full(9, -5.0), np.full(16, 9, np.uint8), C.c_int64(-5), C.c_int32(-5)
    F_all, count = np.full((4, 9), -5.0), np.full(4, -5, np.int32)
    S, D, Fp, Mp, FA, Cn = src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p), F.ctypes.data_as(f64p), mask.ctypes.data_as(u8p), F_all.ctypes.data_as(f64p), count.ctypes.data_as(i32p)
    E = dlco.ERR_INVALID
    good = dict(src=S, dst=D, m=16, threshold=1.0, n_hyp=4, seed=0, refine=2, F=Fp, mask=Mp, n=C.byref(n), best=C.byref(best))
    fundamental = lambda h, **kw: L.dlco_desc_verify_fundamental(h, *[{**good, **kw}[k] for k in ("src", "dst", "m", "threshold", "n_hyp", "seed", "refine", "F", "mask", "n", "best")])
    hypotheses = lambda h, **kw: L.dlco_desc_verify_fundamental_hypotheses(h, *[{**good, "F": FA, "n": Cn, **kw}[k] for k in ("src", "dst", "m", "threshold", "n_hyp", "seed", "F", "n")])
    assert fundamental(None) == E and hypotheses(None) == E                 # a null handle: invalid before anything touches a device
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(src.ctypes.data)
    bad = [dict(src=None), dict(dst=None), dict(m=7), dict(m=4), dict(m=0), dict(m=-1), dict(m=2 ** 31), dict(m=2 ** 40), dict(threshold=0.0), dict(threshold=-1.0),
           dict(threshold=float("nan")), dict(threshold=float("inf")), dict(n_hyp=0), dict(n_hyp=-1), dict(n_hyp=2 ** 20 + 1)]
    for kw in bad:
        assert fundamental(h, **kw) == E, kw
        assert hypotheses(h, **kw) == E, kw
    for kw in (dict(refine=-1), dict(refine=9), dict(F=None), dict(n=None)):
        assert fundamental(h, **kw) == E, kw
    for kw in (dict(F=None), dict(n=None)):
        assert hypotheses(h, **kw) == E, kw
    assert (F == -5).all() and (mask == 9).all() and (n.value, best.value) == (-5, -5) and (F_all == -5).all() and (count == -5).all()
    assert not src.any() and not dst.any()


def test_model_option_parsing_and_help_paths():
    subprocess.check_call(["make", "-s", "-C", CLI])
    tool = os.path.join(CLI, "verify")
    for model in ("fundamental", "homography"):
        for args in (["-help"], ["q", "t", "m"], ["q", "t", "m", "-out", "o", "-hyp", "64", "-help"]):
            p = subprocess.run([tool] + args + ["-model", model], capture_output=True, text=True, timeout=60)
            assert p.returncode == 1 and USAGE in p.stdout and MODEL_LINE in p.stdout and "ERROR" not in p.stdout, (args, p.returncode, p.stdout)
    for args, word in ((["-model", "essential"], "-model must be homography or fundamental"), (["-model", ""], "-model must be"), (["-model"], "Invalid -model option"),
                       (["-model", "fundamental", "-refine", "9"], "-refine"), (["-model", "fundamental", "-thresh", "0"], "-thresh")):
        p = subprocess.run([tool, "q", "t", "m", "-out", "o"] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and USAGE in p.stdout and "ERROR" in p.stdout and word in p.stdout, (args, p.stdout)
    # without the option nothing of it shows
    p = subprocess.run([tool, "-help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and USAGE in p.stdout and "-model" not in p.stdout


def write_inputs(tmp_path, nq, nt, matches):
    for name, n in (("query", nq), ("train", nt)):
        (tmp_path / name).mkdir()
        np.save(tmp_path / name / "Keypoints.npy", np.arange(4 * n, dtype=np.float32).reshape(n, 4))
    (tmp_path / "matches").mkdir()
    np.save(tmp_path / "matches" / "Matches.npy", np.array(matches, np.int32).reshape(-1, 2))
    return [str(tmp_path / "query"), str(tmp_path / "train"), str(tmp_path / "matches"), "-out", str(tmp_path / "out")]


def test_fundamental_model_with_fewer_than_eight_matches_needs_no_device(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CLI])
    tool = os.path.join(CLI, "verify")
    for m in (0, 4, 7):
        d = tmp_path / ("m%d" % m)
        d.mkdir()
        args = write_inputs(d, 9, 9, [(i, i + 1) for i in range(m)])
        p = subprocess.run([tool] + args + ["-model", "fundamental", "-device", "99"], capture_output=True, text=True, timeout=60)      # a device that no machine has
        assert p.returncode == 0, p.stderr
        assert "Matches: %d\n" % m in p.stdout and "Inliers: 0 / %d\n" % m in p.stdout and "Hypothesis: -1\n" in p.stdout and "Total: " in p.stdout
        out = d / "out"
        assert sorted(os.listdir(out)) == ["BestHypothesis.npy", "Fundamental.npy", "FundamentalBits.npy", "Inlier.npy", "VerifiedMatches.npy"]
        F, bits, inl, kept, best = (np.load(out / (n + ".npy")) for n in ("Fundamental", "FundamentalBits", "Inlier", "VerifiedMatches", "BestHypothesis"))
        assert F.dtype == np.float32 and F.shape == (3, 3) and not F.any() and bits.dtype == np.int64 and bits.shape == (9,) and not bits.any()
        assert inl.dtype == np.uint8 and inl.shape == (m,) and not inl.any() and kept.dtype == np.int32 and kept.shape == (0, 2)
        assert best.dtype == np.int32 and best.tolist() == [-1]
    # -model homography is the tool without the option: the same datasets under the same names
    d = tmp_path / "h"
    d.mkdir()
    args = write_inputs(d, 9, 9, [(0, 1), (1, 2)])
    p = subprocess.run([tool] + args + ["-model", "homography", "-device", "99"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and sorted(os.listdir(d / "out")) == ["BestHypothesis.npy", "Homography.npy", "HomographyBits.npy", "Inlier.npy", "VerifiedMatches.npy"]
