"""The batched-verification surface (dlco_desc_verify_pairs_* and the DescContext methods, the tool verify-pairs) on a machine
without a GPU: the C ABI is declared, exported and bound with the stated signatures, the argument checks that need no device,
the plan's launches against the planner's shim, and the paths of the tool that open no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_verify_batch_rules import build_shim, plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
FUNCS = ["dlco_desc_verify_pairs_homography", "dlco_desc_verify_pairs_fundamental", "dlco_desc_verify_pairs_hypotheses",
         "dlco_desc_verify_pairs_fundamental_hypotheses", "dlco_desc_verify_pairs_launches"]
METHODS = ["verify_pairs_homography", "verify_pairs_fundamental", "verify_pairs_hypotheses", "verify_pairs_fundamental_hypotheses"]
USAGE = ("Usage: verify-pairs match_pairs_out -out dst_h5_filename [-thresh f] [-hyp n] [-seed n] [-refine n] [-model homography|fundamental] [-device n] "
         "kp_file_0 kp_file_1 ...")
f32p, f64p, u8p, i64p, i32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_uint8, C.c_int64, C.c_int32))


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return build_shim(tmp_path_factory)


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
    assert callable(dlco.verify_pairs_launches)
    vp, i64, i32, u64, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_float
    model = [vp, f32p, f32p, i64p, i64, f32, i32, u64, i32, f64p, u8p, i64p, i32p]
    hyp = [vp, f32p, f32p, i64p, i64, f32, i32, u64, f64p, i32p]
    assert L.dlco_desc_verify_pairs_homography.argtypes == model and L.dlco_desc_verify_pairs_fundamental.argtypes == model
    assert L.dlco_desc_verify_pairs_hypotheses.argtypes == hyp and L.dlco_desc_verify_pairs_fundamental_hypotheses.argtypes == hyp
    assert L.dlco_desc_verify_pairs_launches.argtypes == [i64p, i64, i32, i32, i32p]
    # the header states the same parameter lists
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    common = ["dlco_desc_ctx *ctx", "const float *src_xy_host", "const float *dst_xy_host", "const int64_t *moff", "int64_t n_pairs", "float threshold",
              "int32_t n_hyp", "uint64_t seed"]
    tail = ["uint8_t *inlier_host", "int64_t *n_inliers", "int32_t *best_hyp"]
    assert params("dlco_desc_verify_pairs_homography") == common + ["int32_t refine", "double *H_out"] + tail
    assert params("dlco_desc_verify_pairs_fundamental") == common + ["int32_t refine", "double *F_out"] + tail
    assert params("dlco_desc_verify_pairs_hypotheses") == common + ["double *H_all_host", "int32_t *count_host"]
    assert params("dlco_desc_verify_pairs_fundamental_hypotheses") == common + ["double *F_all_host", "int32_t *count_host"]
    assert params("dlco_desc_verify_pairs_launches") == ["const int64_t *moff", "int64_t n_pairs", "int32_t n_hyp", "int32_t fundamental", "int32_t *launch_of_pair"]
    import inspect
    for name, thr in (("verify_pairs_homography", 3.0), ("verify_pairs_fundamental", 1.0)):
        sig = inspect.signature(getattr(dlco.DescContext, name))
        assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [("threshold", thr), ("n_hyp", 2048), ("seed", 0), ("refine", 2)]
    # the header says what is out of scope, that the batched verify no longer is, and the kernel-time comment covers the call
    raw = " ".join(open(dlco.HEADER_PATH).read().split())
    for words in ("Out of scope: a device-memory form; seeds or thresholds per pair; a choice between H and F.",
                  "In scope since: a batched verify, dlco_desc_verify_pairs_* below", "after a verify_pairs call every kernel of the call"):
        assert words in raw, words
    assert "seg / pairs in device memory; a batched verify" not in raw


def test_calls_reject_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    E = dlco.ERR_INVALID
    src, dst = np.zeros((20, 2), np.float32), np.zeros((20, 2), np.float32)
    moff = np.array([0, 8, 8, 20], np.int64)
    H, mask, n, best = np.full((3, 9), -5.0), np.full(20, 9, np.uint8), np.full(3, -5, np.int64), np.full(3, -5, np.int32)
    H_all, count, launch = np.full((3, 4, 9), -5.0), np.full((3, 4), -5, np.int32), np.full(3, -5, np.int32)
    p = lambda a, t: a.ctypes.data_as(t)
    good = dict(src=p(src, f32p), dst=p(dst, f32p), moff=p(moff, i64p), n_pairs=3, threshold=3.0, n_hyp=4, seed=0, refine=2, H=p(H, f64p), mask=p(mask, u8p),
                n=p(n, i64p), best=p(best, i32p))
    MK = ("src", "dst", "moff", "n_pairs", "threshold", "n_hyp", "seed", "refine", "H", "mask", "n", "best")
    HK = ("src", "dst", "moff", "n_pairs", "threshold", "n_hyp", "seed", "H", "n")
    models = [lambda h, f=f, **kw: f(h, *[{**good, **kw}[k] for k in MK]) for f in (L.dlco_desc_verify_pairs_homography, L.dlco_desc_verify_pairs_fundamental)]
    hyps = [lambda h, f=f, **kw: f(h, *[{**good, "H": p(H_all, f64p), "n": p(count, i32p), **kw}[k] for k in HK])
            for f in (L.dlco_desc_verify_pairs_hypotheses, L.dlco_desc_verify_pairs_fundamental_hypotheses)]
    launches = lambda **kw: L.dlco_desc_verify_pairs_launches(*[{**good, "fundamental": 0, "launch": p(launch, i32p), **kw}[k]
                                                                for k in ("moff", "n_pairs", "n_hyp", "fundamental", "launch")])
    for f in models + hyps:
        assert f(None) == E                                # a null handle: invalid before anything touches a device
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(src.ctypes.data)
    keep = []                                              # the arrays behind the pointers stay alive
    def offs(a):
        keep.append(np.array(a, np.int64))
        return dict(moff=p(keep[-1], i64p), n_pairs=len(a) - 1)
    offsets = [dict(moff=None), dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=2 ** 31), offs([1, 8, 8, 20]), offs([0, 8, 7, 20]), offs([0, -1, 8, 20]),
               offs([0, 8, 8 + 2 ** 31, 9 + 2 ** 31])]
    limits = [dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(n_hyp=0), dict(n_hyp=-1),
              dict(n_hyp=2 ** 20 + 1)]
    for kw in offsets + limits + [dict(src=None), dict(dst=None), dict(H=None), dict(n=None)]:
        for f in models + hyps:
            assert f(h, **kw) == E, kw
    for kw in (dict(refine=-1), dict(refine=9)):
        for f in models:
            assert f(h, **kw) == E, kw
    for kw in offsets + limits[4:] + [dict(launch=None), dict(fundamental=2), dict(fundamental=-1)]:
        assert launches(**kw) == E, kw
    assert (H == -5).all() and (mask == 9).all() and (n == -5).all() and (best == -5).all() and (H_all == -5).all() and (count == -5).all() and (launch == -5).all()
    assert not src.any() and not dst.any()
    assert launches() == 0 and launch.tolist() == [0, -1, 0] and launches(fundamental=1) == 0 and launch.tolist() == [0, -1, 0]
    assert launches(**offs([0, 0, 0])) == 0 and launch.tolist() == [-1, -1, 0]       # no match at all is valid: nothing launches


def test_launches_against_the_planner(dlco, rules):
    rng = np.random.default_rng(5)
    for k in range(6):
        moff = np.concatenate([[0], np.cumsum(rng.integers(0, 40, int(rng.integers(1, 300))))]).astype(np.int64)
        for fundamental in (False, True):
            for n_hyp in (1, 2048, 2 ** 15, 2 ** 20):
                assert np.array_equal(dlco.verify_pairs_launches(moff, n_hyp, fundamental), plan(rules, moff, n_hyp, fundamental)["launch"])
    many = dlco.verify_pairs_launches(np.arange(6) * 12, 2 ** 20)
    assert many.dtype == np.int32 and many.tolist() == [0, 0, 0, 0, 1]
    with pytest.raises(dlco.DlcoError):
        dlco.verify_pairs_launches([0, 5, 4], 64)


def test_usage_text_and_exit_status():
    subprocess.check_call(["make", "-s", "-C", CLI])
    tool = os.path.join(CLI, "verify-pairs")
    for args in (["-help"], [], ["m"], ["m", "-out", "o"], ["-out", "o"], ["m", "k0", "k1"], ["m", "-out", "o", "k0", "-hyp", "64", "-help"]):
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and USAGE in p.stdout and "ERROR" not in p.stdout, (args, p.returncode, p.stdout)
    for args, word in ((["-bogus"], "Invalid -bogus option"), (["-thresh", "0"], "-thresh"), (["-thresh", "nan"], "-thresh"), (["-hyp", "0"], "-hyp"),
                       (["-hyp", "1048577"], "-hyp"), (["-refine", "9"], "-refine"), (["-refine", "-1"], "-refine"), (["-model", "affine"], "-model")):
        p = subprocess.run([tool, "m", "-out", "o", "k0", "k1"] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and USAGE in p.stdout and "ERROR" in p.stdout and word in p.stdout, (args, p.stdout)


def write_inputs(d, rows, pairs, moff, matches):
    files = []
    for k, n in enumerate(rows):
        (d / ("kp%d" % k)).mkdir()
        np.save(d / ("kp%d" % k) / "Keypoints.npy", np.arange(4 * n, dtype=np.float32).reshape(n, 4))
        files.append(str(d / ("kp%d" % k)))
    (d / "matches").mkdir()
    np.save(d / "matches" / "Pairs.npy", np.array(pairs, np.int32).reshape(-1, 2))
    np.save(d / "matches" / "MatchOffsets.npy", np.array(moff, np.int64))
    np.save(d / "matches" / "Matches.npy", np.array(matches, np.int32).reshape(-1, 2))
    return [str(d / "matches"), "-out", str(d / "out")] + files


def test_tool_fails_before_a_device_is_opened(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CLI])
    tool = os.path.join(CLI, "verify-pairs")
    p = subprocess.run([tool, str(tmp_path / "none"), "-out", str(tmp_path / "o"), str(tmp_path / "none")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("verify-pairs: ") and "Keypoints.npy" in p.stderr
    good = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 6), (6, 0), (5, 4)]          # pair 0 = (file 0, file 1): 5 matches, pair 1 = (1, 0): 2
    for k, (at, bad) in enumerate(((4, (5, 0)), (2, (0, 7)), (0, (-1, 0)), (6, (0, 5)), (5, (7, 0)))):
        d = tmp_path / ("case%d" % k)
        d.mkdir()
        matches = list(good)
        matches[at] = bad
        p = subprocess.run([tool] + write_inputs(d, (5, 7), [(0, 1), (1, 0)], [0, 5, 7], matches) + ["-device", "99"], capture_output=True, text=True, timeout=60)
        where = "pair %d: match %d = (%d, %d) is outside" % ((0, at) + bad if at < 5 else (1, at - 5) + bad)
        assert p.returncode == 2 and p.stderr.startswith("verify-pairs: " + where) and not os.path.exists(d / "out"), p.stderr
    for k, (pairs, moff, word) in enumerate((([(0, 2)], [0, 7], "names file 2 of 2"), ([(0, 1), (1, 0)], [0, 5, 6], "MatchOffsets"),
                                             ([(0, 1), (1, 0)], [0, 8, 7], "MatchOffsets"), ([(0, 1)], [0, 5, 7], "MatchOffsets"))):
        d = tmp_path / ("table%d" % k)
        d.mkdir()
        p = subprocess.run([tool] + write_inputs(d, (5, 7), pairs, moff, good), capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and word in p.stderr and not os.path.exists(d / "out"), p.stderr


@pytest.mark.parametrize("model", ["homography", "fundamental"])
def test_tool_without_a_sample_in_any_pair_needs_no_device(tmp_path, model):
    subprocess.check_call(["make", "-s", "-C", CLI])
    tool = os.path.join(CLI, "verify-pairs")
    args = write_inputs(tmp_path, (5, 7), [(0, 1), (1, 0), (1, 1)], [0, 3, 3, 5], [(i, i + 1) for i in range(3)] + [(6, 4), (5, 3)])
    p = subprocess.run([tool] + args + ["-model", model, "-device", "99"], capture_output=True, text=True, timeout=60)      # a device that no machine has
    assert p.returncode == 0, p.stderr
    assert "Pairs: 3\n" in p.stdout and "Matches: 5\n" in p.stdout and "Total: " in p.stdout
    for k, m in enumerate((3, 0, 2)):
        assert "Pair %d: 0 / %d inliers, hypothesis -1\n" % (k, m) in p.stdout
    out = tmp_path / "out"
    name = "Fundamental" if model == "fundamental" else "Homography"
    ld = lambda n: np.load(out / (n + ".npy"))
    assert ld(name).dtype == np.float32 and ld(name).shape == (3, 3, 3) and not ld(name).any()
    assert ld(name + "Bits").dtype == np.int64 and ld(name + "Bits").shape == (3, 9) and not ld(name + "Bits").any()
    assert ld("Inlier").dtype == np.uint8 and ld("Inlier").shape == (5,) and not ld("Inlier").any()
    assert ld("Inliers").dtype == np.int64 and ld("Inliers").tolist() == [0, 0, 0] and ld("BestHypothesis").dtype == np.int32 and ld("BestHypothesis").tolist() == [-1] * 3
    assert ld("VerifiedOffsets").dtype == np.int64 and ld("VerifiedOffsets").tolist() == [0] * 4 and ld("VerifiedMatches").shape == (0, 2)
    assert ld("Pairs").tolist() == [[0, 1], [1, 0], [1, 1]] and ld("MatchOffsets").tolist() == [0, 3, 3, 5]
