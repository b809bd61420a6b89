"""The tool verify at the end of the chain of tools on a GPU: detect -orient, describe-image, match -ratio 0.8 -cross, verify
on the shifted pair of tests/test_verify_gpu.py; its datasets against the binding's answer on the same gathered points."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_verify_gpu import shifted_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
pytestmark = pytest.mark.gpu


def tool(name, *args):
    q = subprocess.run([os.path.join(CLI, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, (name, q.stdout, q.stderr)
    return q.stdout


def test_the_chain_of_tools_ends_in_verified_matches(tmp_path):
    from test_describe_gpu import make_w
    from test_descriptors import make_filters
    subprocess.check_call(["make", "-s", "-C", CLI])
    dlco = importlib.import_module("opencv-dlco_amd")
    PR = make_filters(3 * 8, seed=3)                                         # the model of the detect tool's chain test
    w = np.array([[0.3, 0.0, 0.2]], np.float32)
    nsel = len(dlco.select_filters(PR, w[0]))
    flt, prj, pj = (tmp_path / s for s in ("filters", "prj", "pj"))
    for d in (flt, prj, pj):
        d.mkdir()
    np.save(flt / "PRFilters.npy", PR.reshape(-1, 64, 64))
    np.save(prj / "w.npy", w)
    np.save(pj / "W.npy", make_w(10, nsel * 8, seed=5))
    for name, img in zip("ab", shifted_pair()):
        (tmp_path / ("image_" + name)).mkdir()
        np.save(tmp_path / ("image_" + name) / "Image.npy", img)
        tool("detect", tmp_path / ("image_" + name), "-out", tmp_path / ("kp_" + name), "-octaves", 2, "-threshold", 3000000, "-max", 300, "-orient")
        tool("describe-image", flt, tmp_path / ("kp_" + name), "-prj", prj, "-id", 0, "-pj", pj, "-out", tmp_path / ("desc_" + name))
    tool("match", tmp_path / "desc_a", tmp_path / "desc_b", "-out", tmp_path / "matches", "-ratio", 0.8, "-cross")
    out = tmp_path / "verified"
    text = tool("verify", tmp_path / "kp_a", tmp_path / "kp_b", tmp_path / "matches", "-out", out, "-hyp", 1024, "-seed", 7)
    matches = np.load(tmp_path / "matches" / "Matches.npy")
    m = len(matches)
    assert m >= 8
    H, hbits, inl, kept, best = (np.load(out / (n + ".npy")) for n in ("Homography", "HomographyBits", "Inlier", "VerifiedMatches", "BestHypothesis"))
    assert (H.dtype, H.shape) == (np.float32, (3, 3)) and (hbits.dtype, hbits.shape) == (np.int64, (9,)) and (inl.dtype, inl.shape) == (np.uint8, (m,))
    assert kept.dtype == np.int32 and kept.shape == (int(inl.sum()), 2) and (best.dtype, best.shape) == (np.int32, (1,))
    ka, kb = np.load(tmp_path / "kp_a" / "Keypoints.npy"), np.load(tmp_path / "kp_b" / "Keypoints.npy")
    c = dlco.DescContext()
    wantH, want_mask, want_best = c.verify_homography(ka[matches[:, 0], :2], kb[matches[:, 1], :2], n_hyp=1024, seed=7)
    c.close()
    assert np.array_equal(hbits.view(np.float64).reshape(3, 3).view(np.uint64), wantH.view(np.uint64)) and np.array_equal(inl.astype(bool), want_mask)
    assert best[0] == want_best >= 0 and np.array_equal(H, wantH.astype(np.float32))
    assert np.array_equal(kept, matches[inl == 1]) and inl.sum() >= 8
    assert "Matches: %d\n" % m in text and "Inliers: %d / %d\n" % (inl.sum(), m) in text and "Hypothesis: %d\n" % want_best in text and "Total: " in text
