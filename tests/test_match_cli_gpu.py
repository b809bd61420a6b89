"""The tool match on a GPU: two overlapping patch sets described into .npy directories, matched plain, with -ratio, with
-cross and with both.  "Nearest" / "NearestSqDist" are DescContext.match on the tables read back, bit for bit; "Matches" is
the Python restatement of the two rules on "Nearest"."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_describe_gpu import make_w, pair_set
from test_descriptors import make_filters

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", CLI])
    root = tmp_path_factory.mktemp("match_cli")
    wcols = 6
    PR = np.zeros((wcols * 8, 4096), np.float32)
    PR[:40] = make_filters(40, seed=3)
    w = np.array([[0.3, 0.0, 0.2, 0.1, 0.5, 0.7]], np.float32)
    dlco = importlib.import_module("opencv-dlco_amd")
    nsel = len(dlco.select_filters(PR, w[0]))
    W = make_w(20, nsel * 8, seed=5)
    patches, _ = pair_set(n_base=30, n_pairs=10, seed=6)                 # 120 patches: views of 30 points, every fourth an exact repeat
    flt, prj, pj = (root / s for s in ("filters", "prj", "pj"))
    for d in (flt, prj, pj):
        d.mkdir()
    np.save(flt / "PRFilters.npy", PR.reshape(-1, 64, 64))
    np.save(prj / "w.npy", w)
    np.save(pj / "W.npy", W)
    out = {}
    for name, rows in (("query", patches[:76]), ("train", patches[38:])):   # overlap: patches 38..75 are in both, repeats included
        img = root / (name + "_img")
        img.mkdir()
        np.save(img / "Patches.npy", rows)
        q = subprocess.run([os.path.join(CLI, "describe"), str(flt), str(img), "-prj", str(prj), "-id", "0", "-pj", str(pj), "-out", str(root / name)],
                           capture_output=True, text=True, timeout=600)
        assert q.returncode == 0, q.stderr
        out[name] = str(root / name)
    ctx = dlco.DescContext()
    yield dict(ctx=ctx, **out)
    ctx.close()


def rules(idx, d, ratio=None, back=None):
    """The two filters restated: pairs (query, train) ascending in query and their distances."""
    pairs, dist = [], []
    for i in range(len(idx)):
        j, j2 = int(idx[i, 0]), int(idx[i, 1])
        if j < 0:
            continue
        if ratio is not None and j2 != -1 and not (float(d[i, 0]) < float(np.float32(ratio)) * float(np.float32(ratio)) * float(d[i, 1])):
            continue
        if back is not None and back[j, 0] != i:
            continue
        pairs.append((i, j))
        dist.append(d[i, 0])
    return np.array(pairs, np.int32).reshape(-1, 2), np.array(dist, np.float32)


@pytest.mark.parametrize("flags", [[], ["-ratio", "0.8"], ["-cross"], ["-ratio", "0.8", "-cross"]])
def test_match_writes_the_library_answer_and_the_filtered_list(sets, tmp_path, flags):
    out = tmp_path / "m"
    q = subprocess.run([os.path.join(CLI, "match"), sets["query"], sets["train"], "-out", str(out)] + flags, capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    Q, T = np.load(os.path.join(sets["query"], "Descriptor.npy")), np.load(os.path.join(sets["train"], "Descriptor.npy"))
    assert Q.shape == (76, 20) and T.shape == (82, 20)
    idx, d = sets["ctx"].match(Q, T)
    near, near_d = np.load(out / "Nearest.npy"), np.load(out / "NearestSqDist.npy")
    assert near.dtype == np.int32 and near_d.dtype == np.float32
    assert np.array_equal(near, idx) and np.array_equal(near_d.view(np.uint32), d.view(np.uint32))
    ratio = float(flags[flags.index("-ratio") + 1]) if "-ratio" in flags else None
    back = sets["ctx"].match(T, Q)[0] if "-cross" in flags else None
    want_p, want_d = rules(idx, d, ratio, back)
    got_p, got_d = np.load(out / "Matches.npy"), np.load(out / "MatchSqDist.npy")
    assert got_p.dtype == np.int32 and got_p.shape == want_p.shape and got_d.dtype == np.float32 and got_d.shape == want_d.shape
    assert np.array_equal(got_p, want_p) and np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    m = len(want_p)
    assert "Queries: 76 x 20" in q.stdout and "Train: 82 x 20" in q.stdout and "Matches: %d / 76" % m in q.stdout and "Total: " in q.stdout
    if not flags:
        assert m == 76
        # the shared patches find themselves (query 38 + k is train k) at a distance within rounding of 0, and an exact repeat in
        # train (patches 4k+2, 4k+3 are one view twice) is decided by the index rule: the earlier copy first, the later second, tied
        shared = np.arange(38, 76)
        twin_first = (shared % 4 == 2)
        assert np.array_equal(idx[shared[twin_first], 0], shared[twin_first] - 38) and np.array_equal(idx[shared[twin_first], 1], shared[twin_first] - 37)
        twin_second = (shared % 4 == 3)
        assert np.array_equal(idx[shared[twin_second], 0], shared[twin_second] - 39) and np.array_equal(idx[shared[twin_second], 1], shared[twin_second] - 38)
        assert (d[shared[twin_first], 0] == d[shared[twin_first], 1]).all()
        plain = shared % 4 < 2
        assert np.array_equal(idx[shared[plain], 0], shared[plain] - 38)
    if flags == ["-ratio", "0.8"]:
        assert 0 < m < 76                                   # the repeats fail the ratio test (d1 == d2), the unique views pass it


def test_no_match_at_all_writes_empty_datasets(sets, tmp_path):
    """m = 0 is a valid result: every query sits half way between two train rows, which no ratio below 1 accepts."""
    q_dir, t_dir, out = tmp_path / "q", tmp_path / "t", tmp_path / "m"
    q_dir.mkdir()
    t_dir.mkdir()
    T = np.zeros((2, 8), np.float32)
    T[1, 0] = 2.0
    Q = np.zeros((3, 8), np.float32)
    Q[:, 0] = 1.0
    Q[:, 1] = (0.0, 0.5, 3.0)
    np.save(q_dir / "Descriptor.npy", Q)
    np.save(t_dir / "Descriptor.npy", T)
    q = subprocess.run([os.path.join(CLI, "match"), str(q_dir), str(t_dir), "-out", str(out), "-ratio", "0.9", "-cross"], capture_output=True, text=True,
                       timeout=600)
    assert q.returncode == 0, q.stderr
    assert "Matches: 0 / 3" in q.stdout
    near, near_d = np.load(out / "Nearest.npy"), np.load(out / "NearestSqDist.npy")
    assert near.tolist() == [[0, 1]] * 3 and near_d.tolist() == [[1.0, 1.0], [1.25, 1.25], [10.0, 10.0]]      # exact in double, ties by index
    got_p, got_d = np.load(out / "Matches.npy"), np.load(out / "MatchSqDist.npy")
    assert got_p.shape == (0, 2) and got_p.dtype == np.int32 and got_d.shape == (0,) and got_d.dtype == np.float32
