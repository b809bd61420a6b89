"""The -model fundamental form of the tool match at the end of the chain of tools on a GPU: match -ratio 0.8 -cross,
verify -model fundamental, and match again under the verified F, on the chain case of tests/test_guided_epipolar_gpu.py; its
datasets against the binding's answer on the same tables."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_guided_epipolar_gpu import chain_case
from test_verify_cli_gpu import tool
from test_verify_gpu import ratio_cross_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
pytestmark = pytest.mark.gpu


def test_the_chain_of_tools_goes_on_to_matches_guided_by_F(tmp_path):
    """keypoints and descriptors of the chain case, written as the tools detect and describe-image write them; from there on the
    tools: match, verify -model fundamental, match -guided -model fundamental"""
    subprocess.check_call(["make", "-s", "-C", CLI])
    dlco = importlib.import_module("opencv-dlco_amd")
    src, dst, Ya, Yb = chain_case()
    for name, xy, Y in (("a", src, Ya), ("b", dst, Yb)):
        kp = np.zeros((len(xy), 4), np.float32)
        kp[:, :2], kp[:, 2] = xy, 1.0
        for d, what, arr in (("kp_", "Keypoints", kp), ("desc_", "Descriptor", Y)):
            (tmp_path / (d + name)).mkdir()
            np.save(tmp_path / (d + name) / (what + ".npy"), arr)
    tool("match", tmp_path / "desc_a", tmp_path / "desc_b", "-out", tmp_path / "matches", "-ratio", 0.8, "-cross")
    tool("verify", tmp_path / "kp_a", tmp_path / "kp_b", tmp_path / "matches", "-out", tmp_path / "verified", "-model", "fundamental", "-thresh", 3,
         "-hyp", 1024, "-seed", 7)
    out = tmp_path / "guided"
    text = tool("match", tmp_path / "desc_a", tmp_path / "desc_b", "-out", out, "-guided", tmp_path / "verified", "-kp", tmp_path / "kp_a", tmp_path / "kp_b",
                "-model", "fundamental", "-radius", 3, "-ratio", 0.8, "-cross")
    F = np.load(tmp_path / "verified" / "FundamentalBits.npy").view(np.float64).reshape(3, 3)
    assert np.load(tmp_path / "verified" / "BestHypothesis.npy")[0] >= 0
    c = dlco.DescContext()
    near, d = c.match_guided_epipolar(Ya, src, Yb, dst, F, 3.0, 0)
    back, _ = c.match_guided_epipolar(Yb, dst, Ya, src, F, 3.0, 1)
    c.close()
    want = ratio_cross_ref(near, d, back, 0.8)
    got_near, got_d, got, got_md = (np.load(out / (n + ".npy")) for n in ("Nearest", "NearestSqDist", "Matches", "MatchSqDist"))
    assert np.array_equal(got_near, near) and got_d.tobytes() == d.tobytes()
    assert got.dtype == np.int32 and np.array_equal(got, want) and got_md.tobytes() == d[want[:, 0], 0].tobytes()
    first = set(map(tuple, np.load(tmp_path / "verified" / "VerifiedMatches.npy").tolist()))
    assert len(first) >= 100 and first <= set(map(tuple, got.tolist()))
    assert "Guided: fundamental, radius 3\n" in text and "Matches: %d / %d\n" % (len(got), len(Ya)) in text and "Total: " in text
