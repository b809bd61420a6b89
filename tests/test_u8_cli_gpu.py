"""The eight-bit line of the tools on a GPU: describe, quantize -fit (no GPU), describe -quant, match -u8 on .npy
directories.  "DescriptorU8" of describe -quant is the tool quantize run on describe's float output, byte for byte;
"Nearest" / "NearestSqDist" are numpy int64 on those bytes; "Matches" is the Python restatement of the two rules."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_describe_gpu import make_w, pair_set
from test_descriptors import make_filters
from test_match_gpu import top_by_key
from test_quant_rules import select_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")


def run(tool, *args):
    return subprocess.run([os.path.join(CLI, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", CLI])
    root = tmp_path_factory.mktemp("u8_cli")
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
    model = [flt, None, "-prj", prj, "-id", "0", "-pj", pj]
    out = dict(root=root)
    for name, rows in (("query", patches[:76]), ("train", patches[38:])):   # overlap: patches 38..75 are in both, repeats included
        img = root / (name + "_img")
        img.mkdir()
        np.save(img / "Patches.npy", rows)
        model[1] = img
        q = run("describe", *model, "-out", root / (name + "_f32"))
        assert q.returncode == 0, q.stderr
        if name == "query":                                               # the quantiser: fitted on the queries' float rows, no GPU
            q = run("quantize", root / "query_f32", "-out", root / "quant", "-fit", root / "query_f32")
            assert q.returncode == 0, q.stderr
        q = run("describe", *model, "-out", root / name, "-quant", root / "quant")
        assert q.returncode == 0, q.stderr
        out[name] = root / name
    return out


def test_describe_quant_writes_the_bytes_of_quantize(sets):
    root = sets["root"]
    for name in ("query", "train"):
        q = run("quantize", root / (name + "_f32"), "-out", root / (name + "_host"), "-quant", root / "quant")
        assert q.returncode == 0, q.stderr
        dev, host = np.load(sets[name] / "DescriptorU8.npy"), np.load(root / (name + "_host") / "DescriptorU8.npy")
        assert dev.dtype == np.uint8 and dev.shape == np.load(root / (name + "_f32") / "Descriptor.npy").shape
        assert np.array_equal(dev, host), name
        for ds in ("QuantScale", "QuantOffset"):
            assert np.load(sets[name] / (ds + ".npy")).tobytes() == np.load(root / "quant" / (ds + ".npy")).tobytes()
        assert not os.path.exists(sets[name] / "Descriptor.npy")        # in place of the float table
    assert np.load(sets["query"] / "DescriptorU8.npy").max() == 255      # the fit's own sample spans the range


def test_match_u8_writes_the_reference_answer_and_the_filtered_list(sets, tmp_path):
    out = tmp_path / "m"
    q = run("match", sets["query"], sets["train"], "-out", out, "-u8", "-ratio", "0.8", "-cross")
    assert q.returncode == 0, q.stderr
    Q, T = np.load(sets["query"] / "DescriptorU8.npy"), np.load(sets["train"] / "DescriptorU8.npy")
    assert Q.shape == (76, 20) and T.shape == (82, 20)
    D = ((Q.astype(np.int64)[:, None, :] - T.astype(np.int64)[None, :, :]) ** 2).sum(2)
    o = top_by_key(D, 2)
    near, near_d = np.load(out / "Nearest.npy"), np.load(out / "NearestSqDist.npy")
    assert near.dtype == np.int32 and near_d.dtype == np.int32
    assert np.array_equal(near, o) and np.array_equal(near_d, D[np.arange(76)[:, None], o])
    back = top_by_key(D.T.copy(), 2)
    want_p, want_d = select_ref(near, near_d, 0.8, back)
    got_p, got_d = np.load(out / "Matches.npy"), np.load(out / "MatchSqDist.npy")
    assert got_p.dtype == np.int32 and got_d.dtype == np.int32 and got_p.shape == want_p.shape and got_d.shape == want_d.shape
    assert np.array_equal(got_p, want_p) and np.array_equal(got_d, want_d)
    m = len(want_p)
    assert 0 < m < 76 and "Queries: 76 x 20" in q.stdout and "Matches: %d / 76" % m in q.stdout
    # the shared patches find themselves at distance 0: query 38 + k is train k
    plain = np.arange(38, 76)[np.arange(38, 76) % 4 < 2]
    assert np.array_equal(near[plain, 0], plain - 38) and (near_d[plain, 0] == 0).all()


def test_match_u8_refuses_differently_quantised_tables(sets, tmp_path):
    other = tmp_path / "other"
    other.mkdir()
    for ds in ("DescriptorU8", "QuantOffset"):
        np.save(other / (ds + ".npy"), np.load(sets["train"] / (ds + ".npy")))
    s = np.load(sets["train"] / "QuantScale.npy")
    np.save(other / "QuantScale.npy", np.nextafter(s, np.float32(np.inf)))      # one bit
    q = run("match", sets["query"], other, "-out", tmp_path / "m", "-u8")
    assert q.returncode != 0 and q.stderr.startswith("match: ") and "quantised differently" in q.stderr
    assert not os.path.exists(tmp_path / "m")
    # a table without a quantiser is taken as it is
    bare = tmp_path / "bare"
    bare.mkdir()
    np.save(bare / "DescriptorU8.npy", np.load(sets["train"] / "DescriptorU8.npy"))
    q = run("match", sets["query"], bare, "-out", tmp_path / "m2", "-u8")
    assert q.returncode == 0, q.stderr
    # and without -u8 the tool still wants "Descriptor"
    q = run("match", sets["query"], sets["train"], "-out", tmp_path / "m3")
    assert q.returncode == 2
