"""GPU parity tests: the HIP path (through the C ABI of libdlco.so) against the CPU oracle
on the same seeded inputs, plus the committed golden vectors.  Integer work (pair
indexing, violation counts, FPR95 rank position) must be bit-exact; fp32 work carries the
tolerance written next to each assert.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from util import golden, relmax, synth

pytestmark = pytest.mark.gpu

# fp32 tolerances (relative to the largest magnitude of the reference quantity)
TOL_DIST = 2e-5      # per-pair squared distances: K = F fmaf chain vs OpenBLAS sgemm order
TOL_GRAD = 5e-6      # dfAvg after one fused SYRK + dual average, vs fp64 accumulation
TOL_A = 1e-4         # PSD-projected A: SURVEY 8(d) gate (tracker eig_tol = 2e-4 on the weighted residual; measured ~1e-5)
TOL_LOSS = 1e-5      # validation hinge loss

_MEASURED = {}       # largest error seen per check, printed (pytest -s) and written out by the last test of this module


def _check_A(tag, got, want):
    """PSD-projected A against the oracle's ssyevr result, SURVEY 8(d): <= 1e-4 of the largest entry."""
    e = relmax(got, want)
    _MEASURED[tag] = max(_MEASURED.get(tag, 0.0), e)
    assert e <= TOL_A, (tag, e)
    return e


@pytest.fixture(scope="module")
def small(dlco):
    N, F, B = 3000, 64, 40
    D, L = synth(N, F, k=12, seed=77)
    ctx = dlco.Context(F, N, B=B, mu=0.005, gamma=0.5)
    ctx.set_data(D, L)
    yield ctx, D, L
    ctx.close()


def test_device_is_gfx950(small):
    name, _, _ = small[0].device_name()
    assert "gfx950" in name


@pytest.mark.parametrize("mode,N", [("alternate", 5000), ("ragged", 4097), ("alternate", 2), ("ragged", 333)])
def test_pair_index_bit_exact(dlco, ref, mode, N):
    F = 8
    D, L = synth(N, F, k=2, seed=N, label_mode=mode)
    ctx = dlco.Context(F, N, B=4)
    ctx.set_data(D, L)
    got = ctx.index()
    pos, neg = ref.build_index(L)
    assert np.array_equal(got["pos"], pos) and np.array_equal(got["neg"], neg)
    assert got["n_pos_trn"] == ref.split(pos.size) and got["n_neg_trn"] == ref.split(neg.size)
    ctx.close()


def test_pair_index_golden_500k(dlco):
    z = golden("oracle_rng.npz")
    N, F = 500000, 4
    L = (np.arange(N) % 2 == 0).astype(np.uint8)
    ctx = dlco.Context(F, N, B=4)
    ctx.set_data(np.zeros((N, F), np.float32), L)
    got = ctx.index()
    assert np.array_equal(got["pos"][:8], z["idx500k_pos_head"]) and np.array_equal(got["pos"][-8:], z["idx500k_pos_tail"])
    assert np.array_equal(got["neg"][:8], z["idx500k_neg_head"]) and np.array_equal(got["neg"][-8:], z["idx500k_neg_tail"])
    w = np.arange(got["pos"].size) % 977
    assert int((got["pos"].astype(np.int64) * w).sum()) == int(z["idx500k_pos_sum"])
    assert int((got["neg"].astype(np.int64) * w).sum()) == int(z["idx500k_neg_sum"])
    assert got["n_pos_trn"] == 200000 and got["n_neg_trn"] == 200000
    ctx.close()


def test_sampler_bit_exact(dlco, ref):
    N, F, B = 2000, 32, 25
    D, L = synth(N, F, k=6, seed=5)
    ctx = dlco.Context(F, N, B=B, mu=0.01)
    ctx.set_data(D, L)
    tr = ref.Trainer(D, L, B=B, mu=0.01, gamma=0.5, grad_order=1)
    for _ in range(12):
        ctx.step()
        tr.step()
        b = ctx.batch()
        pr, nr = tr.batch_ids()
        assert np.array_equal(b["pos_rows"], pr) and np.array_equal(b["neg_rows"], nr)
    ctx.close()
    tr.close()


@pytest.mark.parametrize("r,n", [(1, 7), (12, 80), (37, 400), (64, 5000), (0, 16)])
def test_project_sqdist(small, ref, r, n):
    ctx, D, _ = small
    rng = np.random.default_rng(r * 1000 + n)
    W = (rng.standard_normal((r, ctx.F)) * 0.3).astype(np.float32)
    ids = rng.integers(0, ctx.N, n).astype(np.int32)
    got = ctx.project_sqdist(ids, W)
    want = ref.project_sqdist_ids(W, D, ids) if r else np.zeros(n, np.float32)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= TOL_DIST * max(want.max(), 1e-30)


def test_project_linearity_property(small):
    ctx, D, _ = small
    rng = np.random.default_rng(3)
    W = rng.standard_normal((20, ctx.F)).astype(np.float32)
    ids = rng.integers(0, ctx.N, 300).astype(np.int32)
    d1 = ctx.project_sqdist(ids, W)
    d2 = ctx.project_sqdist(ids, 2.0 * W)       # scaling by 2 is exact in binary floating point
    assert np.array_equal(d2, 4.0 * d1)
    assert (d1 >= 0).all()


@pytest.mark.parametrize("B", [1, 8, 200, 777])
def test_viol_counts_exact(small, ref, B):
    ctx = small[0]
    rng = np.random.default_rng(B)
    pd = rng.random(B).astype(np.float32) * 3
    nd = rng.random(B).astype(np.float32) * 4
    if B >= 8:   # exact ties on the strict threshold pd + 1 > nd
        nd[:4] = pd[:4] + np.float32(1.0)
        nd[4] = np.nextafter(pd[4] + np.float32(1.0), np.float32(-10))
    rho, kap = ctx.viol_counts(pd, nd)
    r2, k2 = ref.viol_counts(pd, nd)
    assert np.array_equal(rho, r2) and np.array_equal(kap, k2)
    assert rho.sum() == kap.sum()


@pytest.mark.parametrize("B,zero_frac", [(40, 0.0), (40, 0.6), (17, 1.0)])
def test_grad_rda(small, ref, B, zero_frac):
    ctx, D, _ = small
    rng = np.random.default_rng(B + int(zero_frac * 10))
    pr = rng.integers(0, ctx.N, B).astype(np.int32)
    nr = rng.integers(0, ctx.N, B).astype(np.int32)
    rho = rng.integers(0, B + 1, B).astype(np.int32)
    kap = rng.integers(0, B + 1, B).astype(np.int32)
    rho[rng.random(B) < zero_frac] = 0
    kap[rng.random(B) < zero_frac] = 0
    df0 = rng.standard_normal((ctx.F, ctx.F)).astype(np.float32)
    df0 = (df0 + df0.T) * np.float32(0.5)
    alpha, beta = np.float32(1.0 / (B * B * 7)), np.float32(6.0 / 7.0)
    got = ctx.grad_rda(pr, nr, rho, kap, float(alpha), float(beta), df0)
    g64 = ref.grad_reform(D[pr], D[nr], rho, kap, f64=True)
    want = np.float64(beta) * df0 + np.float64(alpha) * g64
    assert relmax(got, want) <= TOL_GRAD
    assert np.array_equal(got, got.T)            # upper triangle mirrored: exactly symmetric


@pytest.mark.parametrize("F,B,zero_frac", [(128, 8, 0.0), (256, 200, 0.3), (384, 33, 0.9), (256, 16, 1.0)])
def test_grad_rda_fused_kernel(dlco, ref, F, B, zero_frac):
    """F a multiple of 128 takes the fused symmetric SYRK + dual-average kernel (kernels_syrk.hip)."""
    N = 1500
    D, L = synth(N, F, k=10, seed=F + B)
    ctx = dlco.Context(F, N, B=B)
    ctx.set_data(D, L)
    rng = np.random.default_rng(F * 7 + B)
    pr = rng.integers(0, N, B).astype(np.int32)
    nr = rng.integers(0, N, B).astype(np.int32)
    rho = rng.integers(0, B + 1, B).astype(np.int32)
    kap = rng.integers(0, B + 1, B).astype(np.int32)
    rho[rng.random(B) < zero_frac] = 0
    kap[rng.random(B) < zero_frac] = 0
    df0 = rng.standard_normal((F, F)).astype(np.float32)
    df0 = (df0 + df0.T) * np.float32(0.5)
    alpha, beta = np.float32(1.0 / (B * B * 3)), np.float32(2.0 / 3.0)
    got = ctx.grad_rda(pr, nr, rho, kap, float(alpha), float(beta), df0)
    want = np.float64(beta) * df0 + np.float64(alpha) * ref.grad_reform(D[pr], D[nr], rho, kap, f64=True)
    assert relmax(got, want) <= TOL_GRAD
    assert np.array_equal(got, got.T)
    # beta = 0 must not read the (possibly uninitialised) previous contents
    got0 = ctx.grad_rda(pr, nr, rho, kap, 1.0, 0.0, None)
    assert relmax(got0, ref.grad_reform(D[pr], D[nr], rho, kap, f64=True)) <= TOL_GRAD
    ctx.close()


@pytest.mark.parametrize("F,rows", [(256, 7), (512, 96), (1024, 128), (384, 40), (4096, 96), (2560, 33)])
def test_tracker_product_kernels(dlco, F, rows):
    """The product kernels of the eigen tracker against fp64: the generic fp32 MFMA GEMM (mode 0), two-way split-bf16 MFMA
    (Chebyshev filter only; stated error budget 3e-5 of |X||G|) and three-way split-bf16 MFMA
    (Rayleigh-Ritz product; same budget as the fp32 kernel)."""
    rng = np.random.default_rng(F + rows)
    G = rng.standard_normal((F, F)).astype(np.float32)
    G = ((G + G.T) * 0.5).astype(np.float32)
    X = rng.standard_normal((rows, F)).astype(np.float32)
    X[0, :] = 0.0
    X[-1, 3] = 1e-3
    want = X.astype(np.float64) @ G.astype(np.float64)
    scale = np.abs(X).astype(np.float64) @ np.abs(G).astype(np.float64)      # sum of |terms| per output
    ctx = dlco.Context(F, 16, B=4)
    got32 = ctx.sym_product(X, G, mode=0)
    assert (np.abs(got32 - want) <= 2e-6 * scale + 1e-30).all()
    if F % 512 == 0:
        got16 = ctx.sym_product(X, G, mode=1)
        assert (np.abs(got16 - want) <= 3e-5 * scale + 1e-30).all()
        assert np.abs(got16 - want).max() > 0                                  # it really is the approximate path
        got24 = ctx.sym_product(X, G, mode=2)                                  # three-way split: fp32-level accuracy
        assert (np.abs(got24 - want) <= 2e-6 * scale + 1e-30).all()
        assert np.abs(got24 - want).max() <= 0.2 * np.abs(got16 - want).max()    # what is left is the fp32 accumulation
    ctx.close()


def test_symmetric_product_on_packed_tiles_and_layout_round_trip(dlco):
    """F = 8192, single rank: the dual average lives as its packed upper 128 x 128 tiles and the tracker's products fetch
    every tile once (two workgroups per tile, paired on one XCD and in one step).  The symmetric kernel against float64,
    row counts that exercise every tile count per block (1..5 x 32 rows), against the full-matrix kernel (same arithmetic,
    another summation grouping), and using ONLY the upper triangle; then dlco_set_state -> dlco_get_dfavg through the
    packed layout, and one fused SYRK + dual average on it against float64."""
    F = 8192
    rng = np.random.default_rng(5)
    G = rng.standard_normal((F, F)).astype(np.float32)
    G = np.triu(G) + np.triu(G, 1).T                                          # exactly symmetric
    ctx = dlco.Context(F, 64, B=8)
    Glow = np.triu(G) + np.tril(rng.standard_normal((F, F)).astype(np.float32), -1)   # garbage below the diagonal
    for rows, mode in ((96, 3), (33, 3), (160, 3), (128, 3), (7, 3), (96, 4), (64, 4), (20, 4)):
        X = rng.standard_normal((rows, F)).astype(np.float32)
        want = X.astype(np.float64) @ G.astype(np.float64)
        scale = np.abs(X).astype(np.float64) @ np.abs(G).astype(np.float64)
        got = ctx.sym_product(X, Glow, mode=mode)
        tol = 3e-5 if mode == 3 else 2e-6
        assert (np.abs(got - want) <= tol * scale + 1e-30).all(), (rows, mode, float((np.abs(got - want) / scale).max()))
        if rows <= 128:
            full = ctx.sym_product(X, G, mode=mode - 2)
            assert (np.abs(got - full) <= 2 * tol * scale + 1e-30).all()
    del Glow
    # layout round trip: what goes in through set_state comes back bit for bit (the lower triangle is the mirror)
    ctx.set_state(3, G, None)
    assert np.array_equal(ctx.dfavg(), G)
    # one fused SYRK + dual average on the packed tiles
    D, L = synth(64, F, k=8, seed=2)
    ctx.set_data(D, L)
    B = 8
    pr, nr = np.arange(0, 16, 2, dtype=np.int32), np.arange(1, 17, 2, dtype=np.int32)
    rho, kap = rng.integers(0, 9, B).astype(np.int32), rng.integers(0, 9, B).astype(np.int32)
    got = ctx.grad_rda(pr, nr, rho, kap, 0.25, 0.5, G)
    want = 0.25 * ((D[pr].astype(np.float64).T * rho) @ D[pr].astype(np.float64) - (D[nr].astype(np.float64).T * kap) @ D[nr].astype(np.float64)) + 0.5 * G
    assert relmax(got, want) <= TOL_GRAD and np.array_equal(got, got.T)
    ctx.close()


def test_hinge_sum(small, ref):
    ctx = small[0]
    rng = np.random.default_rng(11)
    for npos, nneg in ((1, 1), (257, 3000), (5000, 5000), (64, 0)):
        p = (rng.random(npos) * 2).astype(np.float32)
        n = (rng.random(nneg) * 3).astype(np.float32)
        got = ctx.hinge_sum(p, n)
        want = ref.hinge_sum(p, n)
        # per-row fp32 sums follow the reference kernel's order exactly; rows are added in double
        assert abs(got - want) <= 1e-12 * max(abs(want), 1.0)


def test_roc_stats(small, ref):
    ctx = small[0]
    rng = np.random.default_rng(13)
    for n in (2, 999, 50000):
        lab = (rng.random(n) < 0.5).astype(np.uint8)
        lab[0], lab[1] = 1, 0
        d = (rng.random(n) + 0.8 * (lab == 0)).astype(np.float32)
        d[rng.integers(0, n, n // 10)] = np.float32(0.5)      # ties
        if n > 100:
            lab[rng.integers(0, n, 5)] = 3                        # labels that count for neither class
        f, a = ctx.roc_stats(d, lab)
        f2, a2 = ref.roc_stats(d, lab)
        assert f == f2
        assert abs(a - a2) <= 1e-12


def _psd_case(ref, F, seed, t, mu, gamma, rank_hint):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((F, F)))[0]
    ev = np.concatenate([-rng.random(rank_hint) * 0.5 - 0.02, rng.random(F - rank_hint) * 0.2 - 0.001])
    G = ((Q * ev) @ Q.T).astype(np.float32)
    G = (G + G.T) * np.float32(0.5)
    A = ref.dual_to_primal(G, mu, gamma, t)
    Ap, W, _ = ref.psd_project(A)
    return G, Ap, W


# F <= 160 is the dense case (the block is the whole space: the m x m solver alone decides the result): the widths walk
# the block-Jacobi kernel's three column lengths (32 / 96 / 160), a column count that is not a multiple of 8 and an odd
# number of 8-column blocks; F = 176 takes the wide seat kernel, F = 256 the tracker proper
@pytest.mark.parametrize("F,rank_hint", [(64, 9), (256, 40), (24, 5), (96, 30), (100, 17), (128, 50), (160, 41), (176, 20)])
def test_psd_project(dlco, ref, F, rank_hint):
    mu, gamma, t = 0.004, 0.5, 17
    G, Ap, Wref = _psd_case(ref, F, F + rank_hint, t, mu, gamma, rank_hint)
    ctx = dlco.Context(F, 16, B=4, mu=mu, gamma=gamma)
    W, A = ctx.psd_project(G, t)
    assert abs(W.shape[0] - Wref.shape[0]) <= 1          # eigenvalues within fp32 noise of mu may flip
    _check_A("psd_project F=%d" % F, A, Ap)
    # rows ascending in eigenvalue (LAPACK order), mutually orthogonal
    n2 = (W.astype(np.float64) ** 2).sum(1)
    assert (np.diff(n2) >= -1e-6 * n2.max()).all()
    Gm = W.astype(np.float64) @ W.T.astype(np.float64)
    assert np.abs(Gm - np.diag(np.diag(Gm))).max() <= 1e-4 * n2.max()
    ctx.close()


@pytest.mark.parametrize("fname", ["oracle_step_F32_B8.npz", "oracle_step_F64_B40.npz"])
def test_teacher_forced_steps_golden(dlco, ref, fname):
    """Each recorded oracle step is replayed from the oracle's own state."""
    z = golden(fname)
    N, F, B, mu, gamma, nstep = z["cfg"]
    N, F, B, nstep = int(N), int(F), int(B), int(nstep)
    ctx = dlco.Context(F, N, B=B, mu=float(mu), gamma=float(gamma))
    ctx.set_data(z["D"], z["L"])
    checked = 0
    for s in range(nstep):
        W_in = z["s%d_W_in" % s]
        if s == 0:
            W_in = W_in[:0]                      # the reference starts from W = zeros(F,F): distances are 0
        ctx.set_state(s, z["s%d_dfavg_in" % s], W_in)
        ctx.step()
        b = ctx.batch()
        # the sampler state is sequential: identical because every earlier step was also run here
        assert np.array_equal(b["pos_rows"], z["s%d_pos_rows" % s]) and np.array_equal(b["neg_rows"], z["s%d_neg_rows" % s])
        pd, nd = z["s%d_pd" % s], z["s%d_nd" % s]
        scale = max(pd.max(), nd.max(), 1e-30)
        assert np.abs(b["pd"] - pd).max() <= TOL_DIST * scale and np.abs(b["nd"] - nd).max() <= TOL_DIST * scale
        rho, kap = ref.viol_counts(b["pd"], b["nd"])             # counts are exact given the GPU's own distances
        assert np.array_equal(b["rho"], rho) and np.array_equal(b["kappa"], kap)
        if np.array_equal(rho, z["s%d_rho" % s]) and np.array_equal(kap, z["s%d_kappa" % s]):
            assert relmax(ctx.dfavg(), z["s%d_dfavg" % s]) <= TOL_GRAD * 4
            _check_A("teacher-forced golden " + fname, ctx.A(), z["s%d_A" % s])
            checked += 1
    # a distance within an ulp of a margin may flip one count in one step; more than that is a regression, not rounding
    assert checked >= nstep - 1, (checked, nstep)
    ctx.close()


def test_teacher_forced_live(dlco, ref):
    """Same idea on a longer live trajectory with the reference's B = 200."""
    N, F, B = 4000, 128, 200
    D, L = synth(N, F, k=20, seed=9)
    mu, gamma = 0.004, 0.5
    tr = ref.Trainer(D, L, B=B, mu=mu, gamma=gamma, grad_order=1)
    ctx = dlco.Context(F, N, B=B, mu=mu, gamma=gamma)
    ctx.set_data(D, L)
    checked = 0
    for s in range(30):
        before = tr.state()
        tr.step()
        after = tr.state()
        ctx.set_state(s, before["dfavg"], before["W"] if s else None)
        ctx.step()
        b = ctx.batch()
        pr, nr = tr.batch_ids()
        assert np.array_equal(b["pos_rows"], pr) and np.array_equal(b["neg_rows"], nr)
        pd, nd = tr.batch_dists()
        scale = max(pd.max(), nd.max(), 1e-30)
        assert np.abs(b["pd"] - pd).max() <= TOL_DIST * scale and np.abs(b["nd"] - nd).max() <= TOL_DIST * scale
        rho, kap = ref.viol_counts(pd, nd)
        if np.array_equal(b["rho"], rho) and np.array_equal(b["kappa"], kap):
            assert relmax(ctx.dfavg(), after["dfavg"]) <= TOL_GRAD * 4
            _check_A("teacher-forced live F=128 B=200", ctx.A(), after["A"])
            checked += 1
    assert checked >= 20
    ctx.close()
    tr.close()


@pytest.mark.parametrize("F,mu", [(256, 0.004), (544, 0.002)])
def test_free_run_each_step_against_ssyevr(dlco, ref, F, mu):
    """A live chain of steps (no state hand-over: the tracker carries its block, and its first filter term comes from the
    step's own rank update, kernels_rankupd.hip): after every step the GPU's A+ is compared with the oracle's ssyevr
    projection of the GPU's OWN dual average (src/pj-learn.cpp:434-490)."""
    N, B, gamma = 4000, 200, 0.5
    D, L = synth(N, F, k=20, seed=9)
    ctx = dlco.Context(F, N, B=B, mu=mu, gamma=gamma)
    ctx.set_data(D, L)
    nstep, eligible = 40, 0
    for s in range(nstep):
        eligible += 1 if 0 < ctx.eig_stats()["block_rows"] <= 160 else 0      # the shortcut's kernels take up to 160 rows
        ctx.step()
        A = ref.dual_to_primal(ctx.dfavg(), mu, gamma, s)
        Ap, _, _ = ref.psd_project(A)
        _check_A("free run F=%d step by step" % F, ctx.A(), Ap)
    cn = ctx.counters()
    assert cn["nonconverged"] == 0
    # every step that starts from a carried block of at most 160 rows takes the shortcut (not the first ones: no block
    # yet, or one of several hundred rows - and there the locking of converged pairs is at work instead)
    assert eligible >= 20 and cn["rank_update_passes"] >= eligible - 2, (eligible, cn)
    assert cn["locked_passes"] >= 1, cn
    ctx.close()


def test_validation_and_stats(dlco, ref):
    N, F, B = 6000, 64, 50
    D, L = synth(N, F, k=10, seed=21, sp=0.7, noise=0.2)
    mu, gamma = 0.004, 0.5
    tr = ref.Trainer(D, L, B=B, mu=mu, gamma=gamma, grad_order=1)
    ctx = dlco.Context(F, N, B=B, mu=mu, gamma=gamma)
    ctx.set_data(D, L)
    for _ in range(25):
        tr.step()
    st = tr.state()
    ctx.set_state(st["t"] - 1, st["dfavg"], None)
    # re-derive W on the GPU from the oracle's dual average (teacher forcing), then compare objectives
    W, _ = ctx.psd_project(st["dfavg"], st["t"] - 1, want_A=False)
    ctx.set_state(st["t"], st["dfavg"], W)
    lo_ref, rg_ref = tr.validate()
    dim_ref, f95_ref, auc_ref = tr.stats()
    # T1/H1/H2 on the SAME model: the oracle's W in the GPU context (set_state takes trace(A) = |W|_F^2)
    ctx.set_state(st["t"], st["dfavg"], st["W"])
    lo_same, rg_same, rk_same = ctx.validate()
    assert rk_same == st["W"].shape[0]
    assert abs(lo_same - lo_ref) <= TOL_LOSS * max(lo_ref, 1e-12)        # 50k^2-term hinge sum, same W: 1e-5 relative
    assert abs(rg_same - rg_ref) <= 1e-5 * max(rg_ref, 1e-12)            # mu * trace(A)
    # and on the GPU's own re-derived W (tracker tolerance on A+ carries over to the objective)
    ctx.set_state(st["t"], st["dfavg"], W)
    lo_gpu, rg_gpu, _ = ctx.validate()
    assert abs(lo_gpu - lo_ref) <= 1e-3 * max(lo_ref, 1e-12) and abs(rg_gpu - rg_ref) <= 1e-3 * max(rg_ref, 1e-12)
    dim, f95, auc = ctx.stats(W)
    assert abs(dim - dim_ref) <= 1
    assert abs(f95 - f95_ref) <= 1e-3          # +-0.1 % absolute, the metric's stated band
    assert abs(auc - auc_ref) <= 1e-3
    d_all = ctx.project_sqdist(np.arange(N, dtype=np.int32), W)
    f95b, aucb = ref.roc_stats(d_all, L)         # same distances -> identical ranking statistics
    assert f95 == f95b and abs(auc - aucb) <= 1e-12
    ctx.close()
    tr.close()


def test_end_to_end_trajectory_band(dlco, ref):
    """Free-running GPU and oracle trainers: the trajectories are chaotic in the hinge mask, so
    they are compared as the metric asks: objective, rank and FPR95 bands after the same steps."""
    N, F, B = 6000, 64, 50
    D, L = synth(N, F, k=10, seed=31, sp=0.7, noise=0.2)
    mu, gamma = 0.004, 0.5
    tr = ref.Trainer(D, L, B=B, mu=mu, gamma=gamma, grad_order=1)
    ctx = dlco.Context(F, N, B=B, mu=mu, gamma=gamma)
    ctx.set_data(D, L)
    for _ in range(300):
        tr.step()
    ctx.steps(300)
    lo, rg, rank = ctx.validate()
    lo_r, rg_r = tr.validate()
    _, f95, auc = ctx.stats()
    dim_r, f95_r, auc_r = tr.stats()
    assert abs(lo - lo_r) <= 0.05 * max(lo_r, 1e-6) + 1e-4
    assert abs(rg - rg_r) <= 0.05 * max(rg_r, 1e-6) + 1e-4
    assert abs(rank - dim_r) <= 2
    # two equally valid final models: band of three standard errors of an FPR95 estimate on this
    # many negatives (the +-0.1 % statement for ONE model is test_validation_and_stats)
    n_neg = int((L == 0).sum())
    se = float(np.sqrt(max(f95_r * (1.0 - f95_r), 1e-6) / n_neg))
    assert abs(f95 - f95_r) <= max(1e-3, 3.0 * se) and abs(auc - auc_r) <= 3e-3
    e = ctx.log_step()
    assert e.is_best == 1 and e.saved == 1 and e.t == 299
    Ws, As = ctx.saved()
    assert relmax(Ws.T.astype(np.float64) @ Ws.astype(np.float64), As) <= 1e-5
    ctx.close()
    tr.close()


def test_full_width_properties(dlco):
    """BASELINE shape in the feature dimension (F = 8192, B = 200) on a small row count:
    size-independent invariants only (the oracle needs ~40 s per step at this width)."""
    N, F, B = 4096, 8192, 200
    ctx = dlco.Context(F, N, B=B, mu=0.002, gamma=0.5)
    rng = np.random.default_rng(1)
    U = np.linalg.qr(rng.standard_normal((F, 48)))[0].T.astype(np.float32)
    ctx.synth_data(U, 99, 0.45, 1.0, 0.03)
    ctx.steps(3)
    b = ctx.batch()
    assert (b["pd"] >= 0).all() and (b["nd"] >= 0).all() and b["rho"].sum() == b["kappa"].sum()
    W = ctx.W()
    assert 1 <= W.shape[0] < F
    G = W.astype(np.float64) @ W.T.astype(np.float64)
    n2 = np.diag(G)
    assert np.abs(G - np.diag(n2)).max() <= 1e-4 * n2.max()       # rows orthogonal
    assert (np.diff(n2) >= -1e-6 * n2.max()).all()                 # ascending eigenvalue order
    df = ctx.dfavg()
    assert np.array_equal(df, df.T)
    rows = ctx.get_rows(0, 8)
    assert np.abs(rows).max() <= 1.0
    d = ctx.project_sqdist(np.arange(8, dtype=np.int32), W)
    want = ((rows.astype(np.float64) @ W.T.astype(np.float64)) ** 2).sum(1)
    assert np.abs(d - want).max() <= 1e-4 * want.max()
    ctx.close()


def _pair_case(N, F, P, seed):
    """Per-patch descriptors + the reference's [N,4] Indices table (patchID1, 3DpointID1,
    patchID2, 3DpointID2; src/comp-uprjdists.cpp:268-269,308-314) and the matrix of
    differences that comp-uprjdists would have written for it."""
    rng = np.random.default_rng(seed)
    point = rng.integers(0, P // 3, P).astype(np.int32)              # 3-D point of each patch
    centre = rng.standard_normal((P // 3, F)).astype(np.float32) * 0.3
    desc = np.clip(centre[point] + 0.12 * rng.standard_normal((P, F)).astype(np.float32), -1, 1).astype(np.float32)
    a = rng.integers(0, P, N).astype(np.int32)
    b = rng.integers(0, P, N).astype(np.int32)
    # make about half of the pairs matches
    same = rng.random(N) < 0.5
    by_point = [np.flatnonzero(point == q) for q in range(P // 3)]
    for i in np.flatnonzero(same):
        cand = by_point[point[a[i]]]
        b[i] = cand[rng.integers(0, cand.size)]
    pairs = np.stack([a, point[a], b, point[b]], axis=1).astype(np.int32)
    D = (desc[a] - desc[b]).astype(np.float32)                        # Dist = Desc1 - Desc2, :327
    L = (pairs[:, 1] == pairs[:, 3]).astype(np.uint8)
    return desc, pairs, D, L


@pytest.mark.parametrize("F,B", [(256, 40), (96, 24)])               # fused SYRK path / generic GEMM path
def test_pair_mode_bit_identical_to_row_mode(dlco, F, B):
    """dlco_set_pairs (descriptors + Indices, differences formed inside the kernels) against
    dlco_set_data on the pre-differenced matrix: every output must be the same bits."""
    N, P = 3000, 900
    desc, pairs, D, L = _pair_case(N, F, P, seed=5)
    mu, gamma = 0.004, 0.5
    row = dlco.Context(F, N, B=B, mu=mu, gamma=gamma)
    row.set_data(D, L)
    par = dlco.Context(F, N, B=B, mu=mu, gamma=gamma)
    par.set_pairs(desc, pairs)
    assert np.array_equal(par.get_rows(17, 40), D[17:57])
    ia, ib = row.index(), par.index()
    assert np.array_equal(ia["pos"], ib["pos"]) and np.array_equal(ia["neg"], ib["neg"])
    for _ in range(12):
        row.step()
        par.step()
        ba, bb = row.batch(), par.batch()
        for k in ("pos_rows", "neg_rows", "pd", "nd", "rho", "kappa"):
            assert np.array_equal(ba[k], bb[k]), k
    assert np.array_equal(row.dfavg(), par.dfavg())
    # (the tracker's rank-update first term reads the gradient's planes, which pair mode forms from two descriptor rows)
    ca, cb = row.counters(), par.counters()
    assert ca["rank_update_passes"] == cb["rank_update_passes"] and (F % 128 != 0 or ca["rank_update_passes"] >= 6), (ca, cb)
    Wa, Wb = row.W(), par.W()
    assert Wa.shape == Wb.shape and np.array_equal(Wa, Wb)
    assert row.validate() == par.validate()
    assert row.stats() == par.stats()
    ids = np.arange(0, N, 7, dtype=np.int32)
    assert np.array_equal(row.project_sqdist(ids, Wa), par.project_sqdist(ids, Wa))
    row.close()
    par.close()


def test_pair_mode_against_oracle(dlco, ref):
    """Pair mode teacher-forced against the oracle run on the materialised differences."""
    N, F, B, P = 3000, 128, 32, 900
    desc, pairs, D, L = _pair_case(N, F, P, seed=9)
    mu, gamma = 0.004, 0.5
    tr = ref.Trainer(D, L, B=B, mu=mu, gamma=gamma, grad_order=1)
    ctx = dlco.Context(F, N, B=B, mu=mu, gamma=gamma)
    ctx.set_pairs(desc, pairs)
    checked = 0
    for s in range(8):
        before = tr.state()
        tr.step()
        after = tr.state()
        ctx.set_state(s, before["dfavg"], before["W"] if s else None)
        ctx.step()
        b = ctx.batch()
        pr, nr = tr.batch_ids()
        assert np.array_equal(b["pos_rows"], pr) and np.array_equal(b["neg_rows"], nr)
        pd, nd = tr.batch_dists()
        scale = max(pd.max(), nd.max(), 1e-30)
        assert np.abs(b["pd"] - pd).max() <= TOL_DIST * scale and np.abs(b["nd"] - nd).max() <= TOL_DIST * scale
        rho, kap = ref.viol_counts(pd, nd)
        if np.array_equal(b["rho"], rho) and np.array_equal(b["kappa"], kap):
            assert relmax(ctx.dfavg(), after["dfavg"]) <= TOL_GRAD * 4
            _check_A("teacher-forced pair mode", ctx.A(), after["A"])
            checked += 1
    assert checked >= 5
    ctx.close()
    tr.close()


def test_config0_trajectory_band(dlco, ref):
    """BASELINE configs[0] shape — 5 000 pair-rows, PR-dim 512, the reference's batch of 200+200,
    mu chosen so that the learned rank settles near 32 — free-running for 300 steps on both sides.
    The trajectories are chaotic in the hinge mask: the two final models are compared in a band
    that the sample size justifies, and the +-0.1 % FPR@95 statement is checked where it is
    meaningful — the same model (the oracle's final W) scored by both sides."""
    N, F, B = 5000, 512, 200
    D, L = synth(N, F, k=40, seed=2215, sp=0.8, noise=0.25)        # hard enough that FPR95 is a few per cent
    mu, gamma = 0.004, 0.5
    tr = ref.Trainer(D, L, B=B, mu=mu, gamma=gamma, grad_order=1)
    ctx = dlco.Context(F, N, B=B, mu=mu, gamma=gamma)
    ctx.set_data(D, L)
    for _ in range(300):
        tr.step()
    ctx.steps(300)
    lo, rg, rank = ctx.validate()
    lo_r, rg_r = tr.validate()
    _, f95, auc = ctx.stats()
    dim_r, f95_r, auc_r = tr.stats()
    assert 8 <= dim_r <= 128 and 0.01 <= f95_r <= 0.2               # low-rank regime, non-trivial operating point
    assert abs(rank - dim_r) <= 2
    # the same model scored by both sides: the oracle's final W through the GPU's S1-S4 pipeline
    W_ref = tr.state()["W"]
    dim_g, f95_g, auc_g = ctx.stats(W_ref)
    assert dim_g == dim_r and abs(f95_g - f95_r) <= 1e-3 and abs(auc_g - auc_r) <= 1e-4     # +-0.1 % absolute
    # two free-running trajectories end in different (equally valid) models: with 2 500 negatives
    # one FPR95 estimate has a standard error of sqrt(p(1-p)/n) ~ 0.4 %, so the band for the two
    # models is three standard errors, not the 0.1 % that holds for one model (and for 250 000
    # negatives of the real sets)
    n_neg = int((L == 0).sum())
    se = float(np.sqrt(max(f95_r * (1.0 - f95_r), 1e-6) / n_neg))
    assert abs(f95 - f95_r) <= max(1e-3, 3.0 * se) and abs(auc - auc_r) <= 3e-3
    assert abs(lo - lo_r) <= 0.05 * max(lo_r, 1e-6) + 1e-4
    assert abs(rg - rg_r) <= 0.05 * max(rg_r, 1e-6) + 1e-4
    assert ctx.counters()["nonconverged"] == 0
    ctx.close()
    tr.close()


def test_log_step_branches_best_step_saved(dlco, ref):
    """The model-selection block, src/pj-learn.cpp:527-580: "Best:" iff Loss+Regul improves,
    "[saved]" iff additionally AUC_Best <= AUC and FPR95_Best >= FPR95, else "Step:".  A scripted
    sequence of models visits every branch; the flags must follow the rule applied to the entry's
    own numbers and the saved W / A must be those of the last saved entry."""
    N, F, B = 6000, 64, 50
    D, L = synth(N, F, k=10, seed=21, sp=0.7, noise=0.2)
    mu, gamma = 0.004, 0.5
    ctx = dlco.Context(F, N, B=B, mu=mu, gamma=gamma)
    ctx.set_data(D, L)
    ctx.steps(60)
    W = ctx.W()
    df = ctx.dfavg()
    assert W.shape[0] >= 4
    inflated = (4.0 * W).astype(np.float32)          # same ranking (x16 distances, exact), 16x the regulariser
    fewer = W[:-1].copy()                               # without the top direction: worse ROC, objective below `inflated`
    script = [("inflated", inflated), ("fewer", fewer), ("inflated again", inflated), ("full", W)]
    obj_best, auc_best, f_best = np.inf, 0.0, np.inf
    seen, last_saved = [], None
    for i, (name, Wi) in enumerate(script):
        ctx.set_state(61 + i, df, Wi)
        e = ctx.log_step()
        assert e.t == 60 + i and e.rank == Wi.shape[0]
        assert abs(e.obj - (e.loss_val + e.regul)) <= 1e-6 * max(e.obj, 1.0)
        is_best = bool(e.obj < obj_best)
        assert bool(e.is_best) == is_best, name
        if is_best:
            obj_best = e.obj
            assert e.dim == Wi.shape[0]
            saved = auc_best <= e.auc and f_best >= e.fpr95
            assert bool(e.saved) == saved, name
            if saved:
                auc_best, f_best = e.auc, e.fpr95
                last_saved = Wi
        else:
            assert e.saved == 0
        assert e.obj_best == np.float32(obj_best) and e.auc_best == auc_best and e.fpr95_best == np.float32(f_best)
        seen.append((int(e.is_best), int(e.saved)))
    # every branch was visited: Best+saved, Best without [saved], Step
    assert (1, 1) in seen and (1, 0) in seen and (0, 0) in seen, seen
    Ws, As = ctx.saved()
    assert np.array_equal(Ws, last_saved)
    assert relmax(Ws.T.astype(np.float64) @ Ws.astype(np.float64), As) <= 1e-5
    ctx.close()


def test_strict_conv_surfaces_a_missed_tolerance(dlco):
    """cfg.strict_conv: a step whose tracker stops at its iteration cap returns DLCO_ERR_NOCONV
    (the default only counts it: counters()['nonconverged'], log entry .nonconv)."""
    N, F, B = 3000, 256, 40
    D, L = synth(N, F, k=60, seed=5, sp=0.9, noise=0.3)
    # an unreachable tolerance with a single filter + Rayleigh-Ritz pass per step
    lax = dlco.Context(F, N, B=B, mu=0.0005, gamma=0.5, eig_tol=1e-9, eig_max_iter=1)
    lax.set_data(D, L)
    lax.steps(12)
    n_missed = lax.counters()["nonconverged"]
    e = lax.log_step()
    assert n_missed > 0 and e.nonconv == n_missed
    assert lax.log_step().nonconv == 0                     # the window restarts at every log step
    lax.close()
    strict = dlco.Context(F, N, B=B, mu=0.0005, gamma=0.5, eig_tol=1e-9, eig_max_iter=1, strict_conv=1)
    strict.set_data(D, L)
    with pytest.raises(dlco.DlcoError) as err:
        strict.steps(12)
    assert err.value.code == dlco.ERR_NOCONV
    assert strict.t() >= 1                                  # the step itself was applied
    strict.close()


def test_grad_rda_bf16_variant(dlco, ref):
    """cfg.grad_bf16 (BASELINE configs[4]): the SYRK's operands are rounded to bf16 (8 significant bits)
    when the MFMA fragments are read, accumulation stays fp32.  Error budget vs fp64: each product carries
    ~2^-8 relative error of random sign, so the sum over K rows stays within 1e-2 of the largest entry;
    the exact fp32 path is 5e-6.  Symmetry (mirrored store) is exact in both."""
    F, N, B = 256, 1500, 200
    D, L = synth(N, F, k=10, seed=3)
    rng = np.random.default_rng(1)
    pr, nr = rng.integers(0, N, B).astype(np.int32), rng.integers(0, N, B).astype(np.int32)
    rho, kap = rng.integers(0, 40, B).astype(np.int32), rng.integers(0, 40, B).astype(np.int32)
    want = ref.grad_reform(D[pr], D[nr], rho, kap, f64=True)
    got = {}
    for mode in (0, 1):
        ctx = dlco.Context(F, N, B=B, grad_bf16=mode)
        ctx.set_data(D, L)
        got[mode] = ctx.grad_rda(pr, nr, rho, kap, 1.0, 0.0, None)
        ctx.close()
        assert np.array_equal(got[mode], got[mode].T)
    assert relmax(got[0], want) <= TOL_GRAD
    e16 = relmax(got[1], want)
    assert 1e-6 < e16 <= 1e-2, e16                       # really the bf16 path, and inside its budget


def test_bf16_variant_keeps_the_fpr95_band(dlco):
    """The gate of the bf16 variant is the metric's, not the fp32 tolerances: two free-running
    trainers (exact fp32 / bf16 gradient) on BASELINE configs[0]'s shape end at the same operating point
    within three standard errors of an FPR@95 estimate and the same rank +-3."""
    N, F, B = 5000, 512, 200
    D, L = synth(N, F, k=40, seed=2215, sp=0.8, noise=0.25)
    out = []
    for mode in (0, 1):
        ctx = dlco.Context(F, N, B=B, mu=0.004, gamma=0.5, grad_bf16=mode)
        ctx.set_data(D, L)
        ctx.steps(300)
        lo, rg, rank = ctx.validate()
        _, f95, auc = ctx.stats()
        out.append((lo, rg, rank, f95, auc))
        assert ctx.counters()["nonconverged"] == 0
        ctx.close()
    (lo0, rg0, r0, f0, a0), (lo1, rg1, r1, f1, a1) = out
    se = float(np.sqrt(max(f0 * (1.0 - f0), 1e-6) / int((L == 0).sum())))
    assert 0.01 <= f0 <= 0.2
    assert abs(f1 - f0) <= max(1e-3, 3.0 * se) and abs(a1 - a0) <= 3e-3 and abs(r1 - r0) <= 3
    assert abs(lo1 - lo0) <= 0.05 * lo0 + 1e-4 and abs(rg1 - rg0) <= 0.05 * rg0 + 1e-4


def test_uploaded_dual_average_is_symmetrised_from_its_upper_triangle(dlco):
    """The fused SYRK keeps dfAvg exactly symmetric and relies on that for its mirrored stores; a dual average
    that comes from outside (a reference checkpoint is symmetric only up to rounding) is taken from its upper
    triangle, as the epilogue of the kernel has always done for its own output."""
    F, N, B = 256, 1200, 48
    D, L = synth(N, F, k=10, seed=77)
    rng = np.random.default_rng(5)
    df = rng.standard_normal((F, F)).astype(np.float32) * np.float32(1e-3)
    df = (df + df.T) * np.float32(0.5)
    noisy = df + np.tril(rng.standard_normal((F, F)).astype(np.float32) * np.float32(1e-9), -1)
    assert not np.array_equal(noisy, noisy.T)
    outs = []
    for start in (df, noisy):
        ctx = dlco.Context(F, N, B=B, seed=9)
        ctx.set_data(D, L)
        ctx.set_state(40, start, None)
        ctx.step()
        outs.append(ctx.dfavg())
        ctx.close()
    assert np.array_equal(outs[0], outs[0].T)
    assert np.array_equal(outs[0], outs[1])


def test_tracker_block_above_1024_rows_and_the_batch_cap(dlco, ref):
    """A global batch of 1300 + 1300 rows: at t = 0 (W = 0) every pair violates, the positive eigenspace of -dfAvg is
    spanned by the ~1200 distinct negative rows of the batch, and the tracker's block outgrows 1024 rows (the global-memory Jacobi).  One
    teacher-forced step against the oracle's ssyevr.  A batch whose block could outgrow the 4096-row solver is refused
    at dlco_ctx_create with a message, not in the middle of a run."""
    N, F, B = 20000, 2048, 1300                       # 8 000 training negatives: ~1 200 distinct rows among 1 300 draws
    D, L = synth(N, F, k=40, seed=77)
    mu, gamma = 0.0005, 0.5
    ctx = dlco.Context(F, N, B=B, mu=mu, gamma=gamma)
    ctx.set_data(D, L)
    tr = ref.Trainer(D, L, B=B, mu=mu, gamma=gamma, grad_order=1)
    before = tr.state()
    tr.step()
    after = tr.state()
    ctx.set_state(0, before["dfavg"], None)
    ctx.step()
    b = ctx.batch()
    pr, nr = tr.batch_ids()
    assert np.array_equal(b["pos_rows"], pr) and np.array_equal(b["neg_rows"], nr)
    assert relmax(ctx.dfavg(), after["dfavg"]) <= 5e-6
    W = ctx.W()
    r = W.shape[0]
    block = ctx.eig_stats()["block_rows"]
    assert r > 1000 and block >= 1024, (r, block)        # the trimmed block; during the step it held r + 32 or more rows
    nz = int((np.abs(W).max(axis=1) > 0).sum())
    assert nz == r
    assert abs(r - after["r"]) <= 2
    err_a = _check_A("B=1300 first step F=2048", ctx.A(), after["A"])
    print("B=1300 first step: rank %d (oracle %d), err_A %.2e" % (r, after["r"], err_a))
    assert ctx.counters()["nonconverged"] == 0
    ctx.close()
    tr.close()
    with pytest.raises(dlco.DlcoError) as e:
        dlco.Context(8192, N, B=2100)
    assert "4096" in str(e.value)


def test_zz_report_measured_errors():
    """Not a check: prints the largest A+ error each test above measured against its 1e-4 gate (and leaves the
    numbers in gpurun_out/ when that directory exists, for profiles/)."""
    import json
    import os
    line = json.dumps({"TOL_A": TOL_A, "max_err_A": _MEASURED}, sort_keys=True)
    print(line)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, "parity_err_A.json"), "w") as f:
            f.write(line + "\n")
    assert all(v <= TOL_A for v in _MEASURED.values())
