"""A grid of pr-learn settings in one launch (dlco_pr_grid_*, PrGrid, pr-learn-grid) on the MI355X.

Every setting of a grid is one independent pr-learn chain on the same sampled row pairs, so everything the grid
reports must equal, BIT FOR BIT, what a PrContext with that (mu, gamma, seed) reports after the same iterations:
w, dfAvg, the validation objective, the statistics, and the pr-learn log (up to the Ttime / Vtime fields)."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_pr_learn import pr_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")

MUS = [0.025, 0.01, 0.04]
GAMMAS = [0.10, 0.35]
ZERO_MU = 50.0                       # mu far above every |dfAvg|: w = max(-(sqrt(t+1)/gamma)(dfAvg + mu), 0) stays 0


def grid_settings():
    mus = [m for m in MUS for _ in GAMMAS] + [ZERO_MU]
    gammas = [g for _ in MUS for g in GAMMAS] + [0.10]
    return np.array(mus, np.float32), np.array(gammas, np.float32)


def solo(dlco, D, L, mu, gamma, seed=2215):
    c = dlco.PrContext(D.shape[1], D.shape[0], mu=float(mu), gamma=float(gamma), seed=seed)
    c.set_data(D, L)
    return c


@pytest.mark.parametrize("F", [64, 640, 5120, 8192])
def test_grid_is_bit_identical_to_solo_runs(dlco, F):
    N = 1600
    D, L = pr_data(N, F, 100 + F, nsig=min(F // 4, 40))
    mus, gammas = grid_settings()
    assert any(m == np.float32(0.025) and ga == np.float32(0.10) for m, ga in zip(mus, gammas))
    src = solo(dlco, D, L, 0.025, 0.10)
    groups = (1, 2, 4) if F <= 5120 else (1, 2)
    grids = []
    for c in groups:
        g = dlco.PrGrid(src, mus, gammas)
        g.set_group(c)
        assert g.group() == c
        grids.append(g)
    solos = [solo(dlco, D, L, m, ga) for m, ga in zip(mus, gammas)]
    done = 0
    for n in (1, 999, 4000):
        for g in grids:
            g.steps(n)
        for s in solos:
            s.steps(n)
        done += n
        for g in grids:
            st = g.state()
            assert st["t"] == done and st["w"].shape == (len(mus), F)
            for k, s in enumerate(solos):
                want = s.state()
                assert np.array_equal(st["w"][k], want["w"]), (F, g.group(), k, done)
                assert np.array_equal(st["dfavg"][k], want["dfavg"]), (F, g.group(), k, done)
    st = grids[0].state()
    assert not st["w"][-1].any() and st["dfavg"][-1].any()             # the all-zero setting
    assert sum(int((st["w"][k] != 0).any()) for k in range(len(mus) - 1)) >= 3
    assert src.state()["t"] == 0                                       # the source context never moved
    for g in grids:
        g.close()
    for s in solos + [src]:
        s.close()


def test_ragged_and_large_grids(dlco):
    N, F = 1200, 640
    D, L = pr_data(N, F, 7, nsig=30)
    src = solo(dlco, D, L, 0.025, 0.10)
    G = 261
    mus = np.linspace(0.005, 0.06, G).astype(np.float32)
    gammas = np.tile(np.array([0.1, 0.2, 0.5], np.float32), G // 3)
    want = {}
    for k in (0, 130, 260):
        s = solo(dlco, D, L, mus[k], gammas[k])
        s.steps(700)
        s.steps(1300)
        want[k] = s.state()
        s.close()
    for c in (0, 1, 2, 4):
        g = dlco.PrGrid(src, mus, gammas)
        g.set_group(c)
        g.steps(700)
        g.steps(1300)
        st = g.state()
        for k, w in want.items():
            assert np.array_equal(st["w"][k], w["w"]) and np.array_equal(st["dfavg"][k], w["dfavg"]), (c, g.group(), k)
        g.close()
    # G = 1 is a solo run
    g = dlco.PrGrid(src, [0.03], [0.25])
    s = solo(dlco, D, L, 0.03, 0.25)
    for n in (1, 2, 500):
        g.steps(n)
        s.steps(n)
    a, b = g.state(), s.state()
    assert a["t"] == b["t"] == 503
    assert np.array_equal(a["w"][0], b["w"]) and np.array_equal(a["dfavg"][0], b["dfavg"])
    g.close(); s.close(); src.close()


def test_grid_against_the_oracle(dlco, ref):
    N, F = 2000, 5120
    D, L = pr_data(N, F, 11, nsig=40)
    src = solo(dlco, D, L, 0.035, 0.25)
    settings = [(0.035, 0.25), (0.01, 0.10)]
    g = dlco.PrGrid(src, [m for m, _ in settings], [ga for _, ga in settings])
    trs = [ref.PrTrainer(D, L, mu=m, gamma=ga) for m, ga in settings]
    for n in (1, 120, 279):
        g.steps(n)
        for tr in trs:
            tr.steps(n)
    st = g.state()
    for k, tr in enumerate(trs):
        a = tr.state()
        assert a["t"] == st["t"] == 400
        assert np.array_equal(a["w"], st["w"][k]) and np.array_equal(a["dfavg"], st["dfavg"][k]), k
        tr.close()
    g.close(); src.close()


@pytest.mark.parametrize("F", [640, 5120])
def test_grid_validation_and_statistics_equal_solo(dlco, F):
    N = 4000
    D, L = pr_data(N, F, 31 + F, nsig=40)
    mus, gammas = grid_settings()
    src = solo(dlco, D, L, 0.025, 0.10)
    g = dlco.PrGrid(src, mus, gammas)
    solos = [solo(dlco, D, L, m, ga) for m, ga in zip(mus, gammas)]
    g.steps(6000)
    for s in solos:
        s.steps(6000)
    v = g.validate()
    for k, s in enumerate(solos):
        lo, rg, nz = s.validate()
        assert (v["loss"][k], v["regul"][k], v["nnz"][k]) == (np.float32(lo), np.float32(rg), nz), k
    rng = np.random.default_rng(5)
    P = rng.integers(0, 5, (8 * F, 3)).astype(np.float32)
    P[8 * 5 + 1] = P[8 * 9 + 2]
    dims = [s.stats(P, max_dim=0)["dim"] for s in solos]
    assert len(set(dims)) > 1
    max_dim = sorted(set(dims))[-2]                            # some settings above it, the others not
    configs = [3, 0, 6, 3, 5, 1, 4, 2]
    for md in (-1, max_dim):
        out = g.stats(P, configs=configs, max_dim=md)
        early = 0
        for i, k in enumerate(configs):
            want = solos[k].stats(P, max_dim=md)
            got = dict(nPR=out["nPR"][i], dim=out["dim"][i], nzdim=out["nzdim"][i], fpr95=out["fpr95"][i], auc=out["auc"][i])
            assert got["nPR"] == want["nPR"] and got["dim"] == want["dim"] and got["nzdim"] == want["nzdim"], (md, i, k)
            assert np.float32(got["fpr95"]) == np.float32(want["fpr95"]) and got["auc"] == want["auc"], (md, i, k, got, want)
            early += want["fpr95"] == -1.0
        assert (early > 0) == (md != -1)
    # explicit weight vectors instead of the current ones
    W = np.stack([solos[k].state()["w"] for k in (2, 4)]) * np.float32(0.5)
    out = g.stats(P, configs=[2, 4], w=W)
    for i, k in enumerate((2, 4)):
        want = solos[k].stats(P, w=W[i])
        assert (out["nPR"][i], out["dim"][i], out["nzdim"][i]) == (want["nPR"], want["dim"], want["nzdim"])
        assert np.float32(out["fpr95"][i]) == np.float32(want["fpr95"]) and out["auc"][i] == want["auc"]
    with pytest.raises(dlco.DlcoError):
        g.stats(P, configs=[0, len(mus)])
    for s in solos + [g, src]:
        s.close()


def test_grid_rejects_invalid_settings(dlco):
    N, F = 400, 64
    D, L = pr_data(N, F, 3, nsig=8)
    empty = dlco.PrContext(F, N)
    with pytest.raises(dlco.DlcoError):
        dlco.PrGrid(empty, [0.025], [0.1])                     # src without data
    src = solo(dlco, D, L, 0.025, 0.10)
    with pytest.raises(dlco.DlcoError):
        dlco.PrGrid(src, [], [])
    with pytest.raises(dlco.DlcoError):
        dlco.PrGrid(src, [0.025, 0.03], [0.1, 0.0])
    with pytest.raises(dlco.DlcoError):
        dlco.PrGrid(src, [0.025], [-1.0])
    L1 = np.zeros(N, np.uint8)
    L1[0] = 1                                                   # one positive: its training or its validation split is empty
    thin = solo(dlco, D, L1, 0.025, 0.10)
    ix = thin.index()
    assert ix["n_pos"] == 1 and ix["n_pos_trn"] in (0, 1)
    with pytest.raises(dlco.DlcoError):
        dlco.PrGrid(thin, [0.025], [0.1])
    g = dlco.PrGrid(src, [0.025], [0.1])
    with pytest.raises(dlco.DlcoError):
        g.set_group(3)
    for c in (empty, thin, g, src):
        c.close()


def test_grid_leaves_its_source_context_alone(dlco):
    N, F = 1500, 256
    D, L = pr_data(N, F, 17, nsig=20)
    plain = solo(dlco, D, L, 0.02, 0.2)
    src = solo(dlco, D, L, 0.02, 0.2)
    plain.steps(321)
    src.steps(321)
    g = dlco.PrGrid(src, [0.02, 0.03], [0.2, 0.2])
    g.steps(1000)
    g.validate()
    g.stats(np.ones((8 * F, 2), np.float32))
    src.steps(679)
    plain.steps(679)
    g.steps(10)
    a, b = src.state(), plain.state()
    assert a["t"] == b["t"] == 1000
    assert np.array_equal(a["w"], b["w"]) and np.array_equal(a["dfavg"], b["dfavg"])
    assert src.validate() == plain.validate()
    # and the grid's own setting 0 started from zero with a fresh sampler, not from src's state
    fresh = solo(dlco, D, L, 0.02, 0.2)
    fresh.steps(1010)
    assert np.array_equal(g.state()["w"][0], fresh.state()["w"])
    for c in (plain, src, g, fresh):
        c.close()


MASK = re.compile(r"Ttime: \d+\.\d{4} Vtime: \d+\.\d{4}")


def _cli_inputs(tmp_path, N=3000, F=256):
    rng = np.random.default_rng(4)
    L = (np.arange(N) % 2 == 0).astype(np.uint8)
    D = rng.random((N, F)).astype(np.float32)
    D[:, :24] *= np.where(L[:, None] == 1, 0.25, 1.0).astype(np.float32)
    P = rng.integers(0, 6, (8 * F, 3)).astype(np.float32)
    flt, src = tmp_path / "filters", tmp_path / "liberty"
    flt.mkdir(); src.mkdir()
    np.save(flt / "PRParams.npy", P)
    np.save(flt / "RingParams.npy", np.zeros((5, 3), np.float32))
    np.save(src / "Distance.npy", D)
    np.save(src / "Label.npy", L.reshape(-1, 1))
    return flt, src


def test_pr_learn_grid_logs_equal_pr_learn(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CLI])
    pr, grid = os.path.join(CLI, "pr-learn"), os.path.join(CLI, "pr-learn-grid")
    flt, src = _cli_inputs(tmp_path)
    mus, gammas = ["0.03", "0.005"], ["0.25", "0.1"]
    common = ["-iters", "12000", "-logstep", "3000", "-maxdim", "100000"]
    forms = [True] + ([False] if os.path.exists("/opt/conda/lib/libhdf5.so") else [])
    for npy in forms:
        out = tmp_path / ("grid_npy" if npy else "grid_h5")
        q = subprocess.run([grid, str(flt), str(src), str(out), "-mus", ",".join(mus), "-gammas", ",".join(gammas)] + common + (["-npy"] if npy else []),
                           capture_output=True, text=True, timeout=600)
        assert q.returncode == 0, q.stdout + q.stderr
        nsaved_total = 0
        for m in mus:
            for ga in gammas:
                stem = "liberty-%.3f-%.3f-pr" % (float(m), float(ga))
                dst = tmp_path / ("solo_%s_%s_%s" % (m, ga, "npy" if npy else "h5"))
                dst = str(dst) if npy else str(dst) + ".h5"
                p = subprocess.run([pr, str(flt), str(src), dst, "-mu", m, "-gamma", ga] + common, capture_output=True, text=True, timeout=600)
                assert p.returncode == 0, p.stderr
                log = (out / (stem + ".log")).read_text()
                assert MASK.sub("T", log) == MASK.sub("T", p.stdout), stem
                nsaved = log.count("[saved]")
                nsaved_total += nsaved
                if npy:
                    got = out / stem / "w.npy"
                    if nsaved:
                        assert np.array_equal(np.load(got), np.load(os.path.join(dst, "w.npy"))), stem
                    else:
                        assert not got.exists()
                else:
                    assert (out / (stem + ".h5")).exists() == (nsaved > 0)
                    if nsaved:
                        assert os.path.getsize(out / (stem + ".h5")) > 0
        assert nsaved_total >= 2
        assert "Stat: " in log and "Best: 3000" in log
    # a name collision: exit 1 with the usage text, nothing trained
    q = subprocess.run([grid, str(flt), str(src), str(tmp_path / "clash"), "-mus", "0.0301,0.0299", "-gammas", "0.25", "-npy"],
                       capture_output=True, text=True, timeout=60)
    assert q.returncode == 1 and "Usage: pr-learn-grid" in q.stdout and not (tmp_path / "clash").exists()
