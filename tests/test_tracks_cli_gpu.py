"""The tool tracks behind verify-pairs on directories of .npy files: four views of one planted set of keypoints under
homographies, match lists of true and of wrong matches as match-pairs writes them, verify-pairs, then tracks.  The datasets are
byte-equal to the Python reference of tests/test_track_rules.py fed the lists the tool read; without the verified lists the tool
falls back to the match lists, and an index outside its keypoint table is an error before a device is opened."""
import os
import subprocess

import numpy as np
import pytest

from test_track_rules import reference, seg_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
pytestmark = pytest.mark.gpu
SIZES = (120, 97, 64, 3)
PAIRS = [(0, 1), (1, 0), (1, 2), (2, 0), (0, 3), (3, 3)]
HS = [np.eye(3), np.array([[0.95, -0.05, 20.0], [0.04, 1.02, -10.0], [1e-5, -2e-5, 1.0]]),
      np.array([[1.05, 0.02, -15.0], [-0.03, 0.97, 12.0], [-1e-5, 1e-5, 1.0]]), np.eye(3)]


def tool(name, *args):
    q = subprocess.run([os.path.join(CLI, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0, (name, q.stdout, q.stderr)
    return q.stdout


def load(d, n):
    return np.load(os.path.join(str(d), n + ".npy"))


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """keypoint directories of the four views and a match-pairs output: per pair the points both views hold, nine in ten of
    them, and a tenth as many wrong matches"""
    subprocess.check_call(["make", "-s", "-C", CLI])
    rng = np.random.default_rng(17)
    root = tmp_path_factory.mktemp("tracks_cli")
    base = rng.uniform(0, 640, (150, 2))
    pts, kps, tables = [], [], []
    for k, (n, H) in enumerate(zip(SIZES, HS)):
        ids = rng.permutation(150)[:n]
        p = np.c_[base[ids], np.ones(n)] @ H.T
        kp = np.c_[p[:, :2] / p[:, 2:] + rng.normal(0, 0.2, (n, 2)), np.full(n, 9.0), np.full(n, -1.0)].astype(np.float32)
        d = root / ("kp_%d" % k)
        d.mkdir()
        np.save(d / "Keypoints.npy", kp)
        pts.append(ids)
        kps.append(str(d))
        tables.append(kp)
    ms, moff = [], [0]
    for a, b in PAIRS:
        _, ia, ib = np.intersect1d(pts[a], pts[b], return_indices=True)
        sel = rng.random(len(ia)) < 0.9
        m = np.stack([ia[sel], ib[sel]], 1).reshape(-1, 2)
        nw = len(ia) // 10
        if nw:
            m = np.concatenate([m, np.stack([rng.integers(0, SIZES[a], nw), rng.integers(0, SIZES[b], nw)], 1)])
        m = m[np.argsort(m[:, 0], kind="stable")]
        ms.append(m.astype(np.int32))
        moff.append(moff[-1] + len(m))
    matches = root / "matches"
    matches.mkdir()
    np.save(matches / "Pairs.npy", np.array(PAIRS, np.int32))
    np.save(matches / "MatchOffsets.npy", np.array(moff, np.int64))
    np.save(matches / "Matches.npy", np.concatenate(ms))
    return kps, tables, matches


def check(out, tables, pairs, moff, matches, min_len, unique, text):
    seg = seg_of(SIZES)
    want = reference(seg, pairs, moff, matches, None, min_len, unique)
    image = (np.searchsorted(seg, want.obs, side="right") - 1).astype(np.int32)
    row = (want.obs - seg[image]).astype(np.int32)
    xy = np.array([tables[f][r, :2] for f, r in zip(image, row)], np.float32).reshape(-1, 2)
    for name, w in (("TrackOffsets", want.toff), ("TrackImage", image), ("TrackKeypoint", row), ("TrackXY", xy), ("TrackOf", want.track_of),
                    ("Counts", want.counts)):
        got = load(out, name)
        assert got.dtype == w.dtype and got.shape == w.shape and got.tobytes() == w.tobytes(), name
    T = len(want.toff) - 1
    assert "Tracks: %d of %d observations, longest %d; components %d, below -min %d, conflicting %d\n" % (
        T, len(want.obs), np.diff(want.toff).max() if T else 0, want.counts[0], want.counts[1], want.counts[2]) in text
    assert "Kernels: " in text and "Total: " in text
    return want


def test_tracks_behind_verify_pairs(planted, tmp_path):
    kps, tables, matches_dir = planted
    verified = tmp_path / "verified"
    tool("verify-pairs", matches_dir, "-out", verified, "-hyp", 512, "-seed", 3, "-refine", 2, "-thresh", 2.0, *kps)
    pairs, voff, kept = load(verified, "Pairs"), load(verified, "VerifiedOffsets"), load(verified, "VerifiedMatches")
    assert 0 < voff[-1] < load(matches_dir, "MatchOffsets")[-1]
    text = tool("tracks", verified, "-out", tmp_path / "tracks", *kps)
    want = check(tmp_path / "tracks", tables, pairs, voff, kept, 2, 1, text)
    assert "Matches: %d (VerifiedMatches)\n" % voff[-1] in text and "Pairs: %d\n" % len(PAIRS) in text and "Keypoints: %d\n" % sum(SIZES) in text
    assert len(want.toff) - 1 >= 20 and 2 <= int(np.diff(want.toff).max()) <= 3      # the three large views share most points
    text = tool("tracks", verified, "-out", tmp_path / "tracks3", "-min", 3, "-all", *kps)
    check(tmp_path / "tracks3", tables, pairs, voff, kept, 3, 0, text)


def test_tracks_falls_back_to_the_match_lists(planted, tmp_path):
    kps, tables, matches_dir = planted
    pairs, moff, matches = load(matches_dir, "Pairs"), load(matches_dir, "MatchOffsets"), load(matches_dir, "Matches")
    text = tool("tracks", matches_dir, "-out", tmp_path / "tracks", *kps)
    want = check(tmp_path / "tracks", tables, pairs, moff, matches, 2, 1, text)
    assert "Matches: %d (Matches)\n" % moff[-1] in text
    assert want.counts[2] >= 1                                                       # the wrong matches make conflicts
    text = tool("tracks", matches_dir, "-out", tmp_path / "all", "-all", *kps)
    check(tmp_path / "all", tables, pairs, moff, matches, 2, 0, text)


def test_a_bad_index_fails_before_a_device_is_opened(planted, tmp_path):
    kps, _, matches_dir = planted
    bad = tmp_path / "bad"
    bad.mkdir()
    matches = load(matches_dir, "Matches")
    matches[1, 1] = 100000
    for x in ("Pairs", "MatchOffsets"):
        np.save(bad / (x + ".npy"), load(matches_dir, x))
    np.save(bad / "Matches.npy", matches)
    q = subprocess.run([os.path.join(CLI, "tracks"), str(bad), "-out", str(tmp_path / "out"), "-device", "99"] + kps, capture_output=True, text=True, timeout=60)
    assert q.returncode == 2 and q.stderr.startswith("tracks: pair 0: match 1 = (") and "is outside the keypoint tables" in q.stderr
    assert not os.path.exists(tmp_path / "out")
    q = subprocess.run([os.path.join(CLI, "tracks"), str(matches_dir), "-out", str(tmp_path / "out"), "-min", "1"] + kps, capture_output=True, text=True,
                       timeout=60)
    assert q.returncode == 1 and "-min must be at least 2" in q.stdout and not os.path.exists(tmp_path / "out")
