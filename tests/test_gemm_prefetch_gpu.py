"""The generic fp32 GEMM with several K tiles of loads in flight (gemm_kernel's DEPTH, kernels_gemm.hip) against the
single-tile schedule and against float64, through dlco_gemm_probe.

Every case runs twice, depth 0 (the library's choice: the ring wherever the tiles are 64 wide and the operands plain) and
depth 1 (one tile in flight, the loader of before), and asks for
  * the same bits: C (and C2) np.array_equal between the two, and
  * the fp32 chain bound of test_tracker_product_kernels against float64 for both,
    |got - want| <= 2e-6 * (|A| |B| + |epilogue terms|) + 1e-30 elementwise,
    which catches the two schedules being wrong together.
The shapes are the smallest at which the ring can go wrong: K around the depth, ragged last tiles, row / column tails, a
single live row, every orientation, gathered and differenced rows, a device-side K limit inside a tile, the twin product.
Rows of zeros and one isolated small entry as in that test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.Context(128, 16, B=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def D(ctx):
    """The depth the library chose for 64 x 64 tiles of plain operands."""
    one = np.ones((16, 16), np.float32)
    d = ctx.gemm_probe(one, one, 16, 16, 16)["depth"]
    assert d in (2, 4, 8)
    return d


def _mem(X, kmajor, pad, rng):
    """Logical operand X [T, K] as it lies in memory: [T, K + pad] or, k-major, [K, T + pad]; the pad holds garbage."""
    L = X.T if kmajor else X
    out = rng.standard_normal((L.shape[0], L.shape[1] + pad)).astype(np.float32) * 100.0
    out[:, :L.shape[1]] = L
    return out


def _operands(M, N, K, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)).astype(np.float32)
    Bt = rng.standard_normal((N, K)).astype(np.float32)      # B^T: row j = column j of B
    A[0, :] = 0.0
    A[-1, 3] = 1e-3
    Bt[N // 2, :] = 0.0
    return rng, A, Bt


def _check(ctx, A, Bt, probe_kw, want_depth=None, Bt2=None, k_lim=None, epi=None):
    """A [M,K], Bt [N,K] (and Bt2) are the logical operands in float32; probe_kw holds their memory images and the launch
    options.  epi = (beta, C_in, b1, E1, b2, E2).  Returns the depth-0 result."""
    M, K = A.shape
    N = Bt.shape[0]
    k = K if k_lim is None else k_lim
    A64, add, addabs = A.astype(np.float64)[:, :k], 0.0, 0.0
    if epi is not None:
        beta, C_in, b1, E1, b2, E2 = epi
        add = beta * C_in.astype(np.float64) + b1 * E1.astype(np.float64) + b2 * E2.astype(np.float64)
        addabs = np.abs(beta * C_in.astype(np.float64)) + np.abs(b1 * E1.astype(np.float64)) + np.abs(b2 * E2.astype(np.float64))
        probe_kw = dict(probe_kw, beta=beta, C_in=C_in, b1=b1, E1=E1, b2=b2, E2=E2)
    r0 = ctx.gemm_probe(M=M, N=N, K=K, depth=0, **probe_kw)
    r1 = ctx.gemm_probe(M=M, N=N, K=K, depth=1, **probe_kw)
    assert r1["depth"] == 1
    if want_depth is not None:
        assert r0["depth"] == want_depth, "the case was meant to run the ring"
    for key, T in (("C", Bt), ("C2", Bt2)):
        if T is None:
            assert r0[key] is None
            continue
        B64 = T.astype(np.float64)[:, :k].T
        want = A64 @ B64 + add
        bound = 2e-6 * (np.abs(A64) @ np.abs(B64) + addabs) + 1e-30
        assert np.array_equal(r0[key], r1[key]), (key, float(np.abs(r0[key] - r1[key]).max()))
        for r in (r0, r1):
            assert (np.abs(r[key] - want) <= bound).all(), (key, r["depth"], float((np.abs(r[key] - want) / bound).max()))
    return r0


@pytest.mark.parametrize("M,N,b_kmajor", [(96, 96, True), (70, 33, False), (1, 130, False), (64, 64, True)])
def test_k_around_the_depth_and_tile_tails(ctx, D, M, N, b_kmajor):
    """K = 16 j for j in {1, D-1, D, D+1, 2D+1}, and 40 and 200 for a ragged last tile, unsplit and in three K slices, on
    64-wide tiles with row and column tails and on a workgroup with a single live row."""
    for K in sorted({16 * j for j in (1, D - 1, D, D + 1, 2 * D + 1)} | {40, 200}):
        rng, A, Bt = _operands(M, N, K, 1000 * M + K)
        kw = dict(A=_mem(A, False, 0, rng), B=_mem(Bt, b_kmajor, 4 if b_kmajor else 8, rng), b_kmajor=b_kmajor)
        for split in (1, 3):
            _check(ctx, A, Bt, dict(kw, split_k=split), want_depth=D)


@pytest.mark.parametrize("a_km", [False, True])
@pytest.mark.parametrize("b_km", [False, True])
def test_every_orientation_of_both_operands(ctx, D, a_km, b_km):
    """M = 70, N = 130, K = 112 (a k-major operand of such an extent is not plain: one tile in flight), the same with an odd
    pitch of either operand (no 16-byte rows at all), and M = 72, N = 132, where every orientation runs the ring."""
    K = 112
    for M, N, odd_a, odd_b in ((70, 130, False, False), (70, 130, True, False), (70, 130, False, True), (72, 132, False, False)):
        rng, A, Bt = _operands(M, N, K, 7 + M + 2 * a_km + b_km)

        def pad(extent, odd):                                 # pitch = the next multiple of 4 plus 4, or that plus 1
            return (-extent) % 4 + 4 + odd

        kw = dict(A=_mem(A, a_km, pad(M if a_km else K, odd_a), rng), a_kmajor=a_km,
                  B=_mem(Bt, b_km, pad(N if b_km else K, odd_b), rng), b_kmajor=b_km)
        ring = not (odd_a or odd_b) and (M % 4 == 0 or not a_km) and (N % 4 == 0 or not b_km)
        _check(ctx, A, Bt, kw, want_depth=D if ring else 1)


def test_gathered_and_differenced_rows(ctx, D):
    """M = 100, N = 96, K = 176 in two K slices; A's rows gathered from a 300-row source with repeated ids, alone and as
    differences of two rows, B k-major with and without a row scale; then the gather along K of a k-major A."""
    M, N, K = 100, 96, 176
    rng = np.random.default_rng(42)
    S = rng.standard_normal((300, K)).astype(np.float32)
    S[17, :] = 0.0
    ids = rng.integers(0, 300, M).astype(np.int32)
    ids[:6] = (17, 5, 5, 299, 0, 5)
    ids2 = rng.integers(0, 300, M).astype(np.int32)
    ids2[1] = 5                                               # a row minus itself
    Bt = rng.standard_normal((N, K)).astype(np.float32)
    Bt[9, :] = 0.0
    scale = rng.standard_normal(K).astype(np.float32)
    scale[11] = 0.0
    Bmem = _mem(Bt, True, 0, rng)
    for use2, sc in ((False, None), (False, scale), (True, scale), (True, None)):
        A = S[ids] - S[ids2] if use2 else S[ids]             # one fp32 rounding, as in the kernel
        T = Bt if sc is None else Bt * sc[None, :]            # likewise
        kw = dict(A=S, a_ids=ids, a_ids2=ids2 if use2 else None, B=Bmem, b_kmajor=True, b_scale=sc, split_k=2)
        _check(ctx, A, T, kw, want_depth=D if (not use2 and sc is None) else 1)
    idk = rng.integers(0, 300, K).astype(np.int32)
    idk[:3] = (4, 4, 17)
    Sk = rng.standard_normal((300, M)).astype(np.float32)    # k-major source: memory row = a k, M elements long
    A = (Sk[idk] * scale[:, None]).T.copy()
    _check(ctx, A, Bt, dict(A=Sk, a_kmajor=True, a_ids=idk, a_scale=scale, B=Bmem, b_kmajor=True, split_k=2), want_depth=1)


@pytest.mark.parametrize("k_dev", [0, 1, 16, 17, 95, 160])
def test_device_side_k_limit(ctx, D, k_dev):
    """K = 160 cut by a limit in device memory: at 0 the accumulator contributes nothing, C = beta C + b1 E1 + b2 E2; 1, 17
    and 95 cut a tile in the middle."""
    M, N, K = 70, 96, 160
    rng, A, Bt = _operands(M, N, K, 300 + k_dev)
    C_in, E1, E2 = (rng.standard_normal((M, N)).astype(np.float32) for _ in range(3))
    epi = (0.75, C_in, -1.5, E1, 0.25, E2)
    for b_km in (True, False):
        kw = dict(A=_mem(A, False, 0, rng), B=_mem(Bt, b_km, 0, rng), b_kmajor=b_km, k_dev=k_dev)
        r = _check(ctx, A, Bt, kw, want_depth=D, k_lim=k_dev, epi=epi)
        if k_dev == 0:                                        # no product term at all, not even a rounding of one
            f = np.float32
            lo = f(0.75) * C_in + f(-1.5) * E1
            assert np.abs(r["C"] - (lo + f(0.25) * E2)).max() <= 4 * np.finfo(f).eps * (np.abs(lo) + np.abs(E2)).max()


def test_twin_product_and_the_rectangular_small_tiles(ctx, D):
    """M = K = 96 with a twin operand on 64-row tiles: N = 640, and N = 8192, from where on gemm_f32 keeps the 128 columns
    of <1,2> (below, too few workgroups would be left and it takes <1,1>); the same without a twin; and a product tall
    enough to keep 128-row tiles beside 64 columns (<2,1>)."""
    K = 96
    for M, N in ((96, 640), (96, 8192)):
        rng, A, Bt = _operands(M, N, K, 77 + N)
        Bt2 = rng.standard_normal((N, K)).astype(np.float32)
        kw = dict(A=_mem(A, False, 0, rng), B=_mem(Bt, True, 0, rng), b_kmajor=True)
        _check(ctx, A, Bt, dict(kw, B2=_mem(Bt2, True, 0, rng), small_m_tiles=True), want_depth=D, Bt2=Bt2)
        _check(ctx, A, Bt, kw, want_depth=D)
    M, N, K = 32768 + 5, 40, 48
    rng, A, Bt = _operands(M, N, K, 78)
    _check(ctx, A, Bt, dict(A=_mem(A, False, 0, rng), B=_mem(Bt, False, 0, rng)), want_depth=D)


def test_full_width_tiles_keep_one_tile_in_flight(ctx):
    """128 x 128 tiles (<2,2>) got no deeper schedule: the library's choice there is depth 1."""
    M = N = 2048
    rng, A, Bt = _operands(M, N, 32, 79)
    _check(ctx, A, Bt, dict(A=_mem(A, False, 0, rng), B=_mem(Bt, False, 0, rng)), want_depth=1)
