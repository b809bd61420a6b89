"""The tool match-pairs -guided at the end of the chain of tools on a GPU: the three small images of
tests/test_verify_pairs_cli_gpu.py (one a shifted copy of another, one with three keypoints only) go through match-pairs and
verify-pairs, then match-pairs -guided matches every pair again under its own model, with and without -ratio 0.8 -cross and
with -model fundamental.  Every pair's Nearest, NearestSqDist, Matches and MatchSqDist are byte-equal to a run of the tool
match -guided on that pair's two files and that pair's model with the same flags; a pair without a model gets -1 / +inf."""
import os
import subprocess

import numpy as np
import pytest

from test_verify_pairs_cli_gpu import CLI, PAIRS, chain, tool  # noqa: F401  (chain: the fixture of that file)

pytestmark = pytest.mark.gpu


def load(d, n):
    return np.load(os.path.join(str(d), n + ".npy"))


def chain_files(chain):
    kps, matches_dir = chain
    root = os.path.dirname(kps[0])
    return kps, [os.path.join(root, "desc_%d" % k) for k in range(len(kps))], os.path.join(root, "pairs"), matches_dir


@pytest.mark.parametrize("model", ["homography", "fundamental"])
@pytest.mark.parametrize("flags", [[], ["-ratio", "0.8", "-cross"]])
def test_match_pairs_guided_writes_what_match_guided_writes_for_every_pair(chain, tmp_path, model, flags):
    kps, descs, pairs_dir, matches_dir = chain_files(chain)
    name = "FundamentalBits" if model == "fundamental" else "HomographyBits"
    verified, out = tmp_path / "verified", tmp_path / "guided"
    tool("verify-pairs", matches_dir, "-out", verified, "-hyp", 1024, "-seed", 7, "-refine", 4, "-thresh", 1.5, "-model", model, *kps)
    text = tool("match-pairs", "-pairs", pairs_dir, "-out", out, *descs, "-guided", verified, "-kp", *kps, "-radius", 4, "-model", model, *flags)
    bits, best = load(verified, name), load(verified, "BestHypothesis")
    assert best[0] >= 0 and best[2] >= 0 and (best < 0).any()            # the shifted pair both ways has a model, a pair of image 2 has none
    pairs, row0, moff = load(out, "Pairs"), load(out, "RowOffsets"), load(out, "MatchOffsets")
    near, near_d, mat, mat_d = (load(out, n) for n in ("Nearest", "NearestSqDist", "Matches", "MatchSqDist"))
    assert pairs.dtype == np.int32 and np.array_equal(pairs, PAIRS) and row0.dtype == np.int64 and moff.dtype == np.int64
    assert row0.shape == moff.shape == (len(PAIRS) + 1,) and row0[0] == 0 and moff[0] == 0
    assert near.shape == (row0[-1], 2) and near_d.shape == (row0[-1], 2) and mat.shape == (moff[-1], 2) and mat_d.shape == (moff[-1],)
    assert near.dtype == np.int32 and mat.dtype == np.int32 and near_d.dtype == np.float32 and mat_d.dtype == np.float32
    total = 0
    for p, (a, b) in enumerate(PAIRS):
        rows = slice(row0[p], row0[p + 1])
        if best[p] < 0:                                      # "no model": the all-zero matrix admits nothing
            assert not bits[p].any() and (near[rows] == -1).all() and np.isposinf(near_d[rows]).all() and moff[p + 1] == moff[p]
            continue
        one_v, one = tmp_path / ("model%d" % p), tmp_path / ("pair%d" % p)
        one_v.mkdir()
        np.save(one_v / "BestHypothesis.npy", best[p:p + 1])
        np.save(one_v / (name + ".npy"), bits[p])
        tool("match", descs[a], descs[b], "-out", one, "-guided", one_v, "-kp", kps[a], kps[b], "-radius", 4, "-model", model, *flags)
        for got, x in ((near[rows], "Nearest"), (near_d[rows], "NearestSqDist"), (mat[moff[p]:moff[p + 1]], "Matches"),
                       (mat_d[moff[p]:moff[p + 1]], "MatchSqDist")):
            want = load(one, x)
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (p, a, b, x)
        total += moff[p + 1] - moff[p]
    assert (near[row0[0]:row0[1], 0] >= 0).any() and moff[1] > moff[0]                     # the guided pass finds matches of the shifted pair
    assert "Pairs: %d" % len(PAIRS) in text and "Guided: " in text and "Matches: %d / %d" % (total, row0[-1]) in text and "Kernels: " in text


def test_other_pairs_and_u8_are_refused_before_a_device_is_opened(chain, tmp_path):
    kps, descs, pairs_dir, matches_dir = chain_files(chain)
    verified = tmp_path / "verified"
    tool("verify-pairs", matches_dir, "-out", verified, "-hyp", 256, "-seed", 7, *kps)
    other = tmp_path / "other"
    other.mkdir()
    np.save(other / "Pairs.npy", np.array(PAIRS[::-1], np.int32))
    run = lambda *args: subprocess.run([os.path.join(CLI, "match-pairs")] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    q = run("-pairs", other, "-out", tmp_path / "out", "-device", 99, *descs, "-guided", verified, "-kp", *kps)
    assert q.returncode == 2 and q.stderr.startswith("match-pairs: ") and "its Pairs are not the pairs of" in q.stderr and not os.path.exists(tmp_path / "out")
    q = run("-pairs", pairs_dir, "-out", tmp_path / "out", "-device", 99, *descs, "-guided", verified, "-kp", *kps[:2])
    assert q.returncode == 1 and "ERROR: Invalid -guided option" in q.stdout
    q = run("-pairs", pairs_dir, "-out", tmp_path / "out", "-device", 99, "-u8", *descs, "-guided", verified, "-kp", *kps)
    assert q.returncode == 1 and "ERROR: -guided has no -u8 form." in q.stdout and not os.path.exists(tmp_path / "out")
