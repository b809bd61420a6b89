"""The tool verify-pairs at the end of the chain of tools on a GPU: detect -orient, describe-image, match-pairs -ratio 0.8
-cross on three small images, one a shifted copy of another and one with three keypoints only, then verify-pairs.  Every pair's
datasets are byte-equal to a run of the tool verify on that pair's slice of the match list, for both models."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_verify_gpu import shifted_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
pytestmark = pytest.mark.gpu
PAIRS = [(0, 1), (2, 0), (1, 0), (0, 2), (1, 1)]                             # image 2 has three keypoints: its pairs have no sample


def tool(name, *args):
    q = subprocess.run([os.path.join(CLI, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, (name, q.stdout, q.stderr)
    return q.stdout


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """the keypoint files of the three images and match-pairs' output over PAIRS"""
    from test_describe_gpu import make_w
    from test_descriptors import make_filters
    subprocess.check_call(["make", "-s", "-C", CLI])
    dlco = importlib.import_module("opencv-dlco_amd")
    root = tmp_path_factory.mktemp("verify_pairs_cli")
    PR = make_filters(3 * 8, seed=3)                                         # the model of the verify tool's chain test
    w = np.array([[0.3, 0.0, 0.2]], np.float32)
    nsel = len(dlco.select_filters(PR, w[0]))
    flt, prj, pj, pairs = (root / s for s in ("filters", "prj", "pj", "pairs"))
    for d in (flt, prj, pj, pairs):
        d.mkdir()
    np.save(flt / "PRFilters.npy", PR.reshape(-1, 64, 64))
    np.save(prj / "w.npy", w)
    np.save(pj / "W.npy", make_w(10, nsel * 8, seed=5))
    np.save(pairs / "Pairs.npy", np.array(PAIRS, np.int32))
    a, b = shifted_pair()
    kps, descs = [], []
    for k, (img, most) in enumerate(((a, 300), (b, 300), (np.ascontiguousarray(a[::-1]), 3))):
        (root / ("image_%d" % k)).mkdir()
        np.save(root / ("image_%d" % k) / "Image.npy", img)
        tool("detect", root / ("image_%d" % k), "-out", root / ("kp_%d" % k), "-octaves", 2, "-threshold", 3000000, "-max", most, "-orient")
        tool("describe-image", flt, root / ("kp_%d" % k), "-prj", prj, "-id", 0, "-pj", pj, "-out", root / ("desc_%d" % k))
        kps.append(str(root / ("kp_%d" % k)))
        descs.append(str(root / ("desc_%d" % k)))
    tool("match-pairs", "-pairs", pairs, "-out", root / "matches", "-ratio", 0.8, "-cross", *descs)
    return kps, root / "matches"


@pytest.mark.parametrize("model", ["homography", "fundamental"])
def test_verify_pairs_writes_what_verify_writes_for_every_pair(chain, tmp_path, model):
    kps, matches_dir = chain
    name = "Fundamental" if model == "fundamental" else "Homography"
    out = tmp_path / "verified"
    text = tool("verify-pairs", matches_dir, "-out", out, "-hyp", 1024, "-seed", 7, "-refine", 4, "-thresh", 1.5, "-model", model, *kps)
    load = lambda d, n: np.load(os.path.join(str(d), n + ".npy"))
    pairs, moff, matches = load(matches_dir, "Pairs"), load(matches_dir, "MatchOffsets"), load(matches_dir, "Matches")
    m = np.diff(moff)
    assert m[0] >= 8 and m[2] >= 8 and m[1] < 4 and m[3] < 4, m              # the shifted pair both ways, and pairs without a sample
    P = len(PAIRS)
    M, mbits, inl, n, best, voff, kept = (load(out, x) for x in (name, name + "Bits", "Inlier", "Inliers", "BestHypothesis", "VerifiedOffsets", "VerifiedMatches"))
    assert np.array_equal(load(out, "Pairs"), pairs) and np.array_equal(load(out, "MatchOffsets"), moff) and load(out, "MatchOffsets").dtype == np.int64
    assert (M.dtype, M.shape) == (np.float32, (P, 3, 3)) and (mbits.dtype, mbits.shape) == (np.int64, (P, 9)) and (inl.dtype, inl.shape) == (np.uint8, (moff[-1],))
    assert (n.dtype, n.shape) == (np.int64, (P,)) and (best.dtype, best.shape) == (np.int32, (P,)) and (voff.dtype, voff.shape) == (np.int64, (P + 1,))
    assert kept.dtype == np.int32 and kept.shape == (voff[-1], 2) and voff[0] == 0
    for p, (a, b) in enumerate(PAIRS):
        one_m, one = tmp_path / ("matches%d" % p), tmp_path / ("pair%d" % p)
        one_m.mkdir()
        np.save(one_m / "Matches.npy", matches[moff[p]:moff[p + 1]])
        tool("verify", kps[a], kps[b], one_m, "-out", one, "-hyp", 1024, "-seed", 7, "-refine", 4, "-thresh", 1.5, "-model", model)
        for got, x in ((M[p], name), (mbits[p], name + "Bits"), (inl[moff[p]:moff[p + 1]], "Inlier"), (best[p:p + 1], "BestHypothesis"),
                       (kept[voff[p]:voff[p + 1]], "VerifiedMatches")):
            want = load(one, x)
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (p, a, b, x)
        assert n[p] == inl[moff[p]:moff[p + 1]].sum() == voff[p + 1] - voff[p]
        assert "Pair %d: %d / %d inliers, hypothesis %d\n" % (p, n[p], m[p], best[p]) in text
    assert best[0] >= 0 and best[2] >= 0 and n[0] >= 8 and best[1] == best[3] == -1 and not mbits[1].any() and not mbits[3].any()
    assert "Pairs: %d\n" % P in text and "Matches: %d\n" % moff[-1] in text and "Kernels: " in text and "Total: " in text


def test_a_bad_index_fails_before_a_device_is_opened(chain, tmp_path):
    kps, matches_dir = chain
    bad = tmp_path / "bad"
    bad.mkdir()
    matches = np.load(matches_dir / "Matches.npy")
    matches[1, 1] = 100000
    for x in ("Pairs", "MatchOffsets"):
        np.save(bad / (x + ".npy"), np.load(matches_dir / (x + ".npy")))
    np.save(bad / "Matches.npy", matches)
    q = subprocess.run([os.path.join(CLI, "verify-pairs"), str(bad), "-out", str(tmp_path / "out"), "-device", "99"] + kps, capture_output=True, text=True, timeout=60)
    assert q.returncode == 2 and q.stderr.startswith("verify-pairs: pair 0: match 1 = (") and "is outside the keypoint tables" in q.stderr
    assert not os.path.exists(tmp_path / "out")
