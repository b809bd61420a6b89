"""The tools describe and eval-patches on a GPU: the files they read are comp-uprjdists' plus pj-learn's W, "Descriptor"
is DescContext.describe bit for bit, and the "Stat:" line is eval-fpr95's grammar with pair_stats' numbers."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from test_describe_gpu import make_w, pair_set
from test_descriptors import make_filters

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
STAT = re.compile(r"^Stat: Dim \[(\d+)\] AUC: (\d\.\d{6}) \((\d\.\d{6})\) FPR95: (\d+\.\d{2}) \((\d+\.\d{2})\)$")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """A filter bank with a repeat and all-zero rows, two rows of "w", a W for the first, and a pair set: .npy directories."""
    subprocess.check_call(["make", "-s", "-C", CLI])
    root = tmp_path_factory.mktemp("describe_cli")
    wcols = 6
    PR = np.zeros((wcols * 8, 4096), np.float32)
    PR[:40] = make_filters(40, seed=3)
    PR[5] = PR[4]
    w = np.array([[0.3, 0.0, 0.2, 0.1, 0.5, 0.7], [0, 0, 0, 0, 1.0, 0]], np.float32)
    patches, pairs = pair_set(n_base=30, n_pairs=1500, seed=6)
    dlco = importlib.import_module("opencv-dlco_amd")
    sPR = dlco.select_filters(PR, w[0])
    assert len(sPR) == 31
    W = make_w(20, 248, seed=5)
    W[3] = 0
    flt, img, prj, pj, bad = (root / s for s in ("filters", "images", "prj", "pj", "pj_bad"))
    for d in (flt, img, prj, pj, bad):
        d.mkdir()
    np.save(flt / "PRFilters.npy", PR.reshape(-1, 64, 64))
    np.save(img / "Indices.npy", pairs)
    np.save(img / "Patches.npy", patches)
    np.save(prj / "w.npy", w)
    np.save(pj / "W.npy", W)
    np.save(bad / "W.npy", make_w(20, 240, seed=5))
    ctx = dlco.DescContext()
    ctx.set_filters(sPR)
    ctx.set_projection(W)
    return dict(root=root, flt=str(flt), img=str(img), prj=str(prj), pj=str(pj), bad=str(bad), ctx=ctx, patches=patches, pairs=pairs)


def test_describe_writes_the_library_descriptors(model, tmp_path):
    out = tmp_path / "desc"
    q = subprocess.run([os.path.join(CLI, "describe"), model["flt"], model["img"], "-prj", model["prj"], "-id", "0", "-pj", model["pj"], "-out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    assert "PRFilters: 31 x 4096" in q.stdout and "Descriptor size: 248" in q.stdout and "Projection: 20 x 248" in q.stdout and "Done." in q.stdout
    Y = np.load(out / "Descriptor.npy")
    want = model["ctx"].describe(model["patches"])
    assert Y.dtype == np.float32 and Y.shape == (len(model["patches"]), 20) and np.array_equal(Y, want)
    assert (Y[:, 3] == 0).all() and (Y[:, 4] != 0).any()                 # W's rows as given
    # "Indices" is not needed
    only = tmp_path / "patches_only"
    only.mkdir()
    np.save(only / "Patches.npy", model["patches"][:7])
    q = subprocess.run([os.path.join(CLI, "describe"), model["flt"], str(only), "-prj", model["prj"], "-id", "0", "-pj", model["pj"], "-out", str(tmp_path / "d7")],
                       capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    assert np.array_equal(np.load(tmp_path / "d7" / "Descriptor.npy"), want[:7])


def test_eval_patches_prints_pair_stats(model):
    q = subprocess.run([os.path.join(CLI, "eval-patches"), model["flt"], model["img"], "-prj", model["prj"], "-id", "0", "-pj", model["pj"]],
                       capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    stat = [l for l in q.stdout.splitlines() if l.startswith("Stat:")]
    assert len(stat) == 1 and STAT.match(stat[0]), q.stdout
    dim, f95, auc = model["ctx"].pair_stats(model["patches"], model["pairs"])
    assert dim == 19
    assert stat[0] == "Stat: Dim [%i] AUC: %.6f (%.6f) FPR95: %.2f (%.2f)" % (dim, auc, auc, f95 * 100, f95 * 100)


@pytest.mark.parametrize("tool", ["describe", "eval-patches"])
def test_a_projection_of_the_wrong_width_exits_2(model, tool, tmp_path):
    args = [os.path.join(CLI, tool), model["flt"], model["img"], "-prj", model["prj"], "-id", "0", "-pj", model["bad"]]
    if tool == "describe":
        args += ["-out", str(tmp_path / "never")]
    q = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert q.returncode == 2 and q.stderr.startswith(tool + ": W has 240 columns") and "248" in q.stderr
    assert not (tmp_path / "never").exists()
    # row 1 of "w" selects 8 filters: the W of row 0 does not fit them either
    args[args.index(model["bad"])] = model["pj"]
    args[args.index("-id") + 1] = "1"
    q = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert q.returncode == 2 and "W has 248 columns" in q.stderr
