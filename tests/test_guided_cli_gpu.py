"""The -guided form of the tool match at the end of the chain of tools on a GPU: match -ratio 0.8 -cross, verify, and match again
under the verified model, on the shifted pair of tests/test_verify_gpu.py; its datasets against the binding's answer on the
same tables."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_verify_cli_gpu import tool
from test_verify_gpu import chain_model, ratio_cross_ref, shifted_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
pytestmark = pytest.mark.gpu


def test_the_chain_of_tools_goes_on_to_guided_matches(tmp_path):
    """keypoints and descriptors of the shifted pair come from the binding, written as the tools detect and describe-image
    write them (tests/test_verify_cli_gpu.py runs those two tools); from there on the tools: match, verify, match -guided"""
    subprocess.check_call(["make", "-s", "-C", CLI])
    dlco = importlib.import_module("opencv-dlco_amd")
    c = dlco.DescContext()
    chain_model(c)
    for name, img in zip("ab", shifted_pair()):
        c.set_image(img)
        kp, _, _ = c.detect_oriented(2, 3000000, 300)
        for d, what, arr in (("kp_", "Keypoints", kp), ("desc_", "Descriptor", c.describe_keypoints(kp)[0])):
            (tmp_path / (d + name)).mkdir()
            np.save(tmp_path / (d + name) / (what + ".npy"), arr)
    c.close()
    tool("match", tmp_path / "desc_a", tmp_path / "desc_b", "-out", tmp_path / "matches", "-ratio", 0.8, "-cross")
    tool("verify", tmp_path / "kp_a", tmp_path / "kp_b", tmp_path / "matches", "-out", tmp_path / "verified", "-hyp", 1024, "-seed", 7, "-thresh", 3)
    out = tmp_path / "guided"
    text = tool("match", tmp_path / "desc_a", tmp_path / "desc_b", "-out", out, "-ratio", 0.8, "-cross", "-guided", tmp_path / "verified", "-kp",
                tmp_path / "kp_a", tmp_path / "kp_b", "-radius", 6)
    Ya, Yb = np.load(tmp_path / "desc_a" / "Descriptor.npy"), np.load(tmp_path / "desc_b" / "Descriptor.npy")
    ka, kb = np.load(tmp_path / "kp_a" / "Keypoints.npy"), np.load(tmp_path / "kp_b" / "Keypoints.npy")
    H = np.load(tmp_path / "verified" / "HomographyBits.npy").view(np.float64).reshape(3, 3)
    assert np.load(tmp_path / "verified" / "BestHypothesis.npy")[0] >= 0
    c = dlco.DescContext()
    near, d = c.match_guided(Ya, ka[:, :2], Yb, kb[:, :2], H, 6.0, 0)
    back, _ = c.match_guided(Yb, kb[:, :2], Ya, ka[:, :2], H, 6.0, 1)
    c.close()
    want = ratio_cross_ref(near, d, back, 0.8)
    got_near, got_d, got, got_md = (np.load(out / (n + ".npy")) for n in ("Nearest", "NearestSqDist", "Matches", "MatchSqDist"))
    assert np.array_equal(got_near, near) and got_d.tobytes() == d.tobytes()
    assert got.dtype == np.int32 and np.array_equal(got, want) and got_md.tobytes() == d[want[:, 0], 0].tobytes()
    first = set(map(tuple, np.load(tmp_path / "verified" / "VerifiedMatches.npy").tolist()))
    assert len(first) >= 8 and first <= set(map(tuple, got.tolist()))
    assert "Guided: radius 6\n" in text and "Matches: %d / %d\n" % (len(got), len(Ya)) in text and "Total: " in text
