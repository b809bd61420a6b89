"""Guided matching under a fundamental matrix on a GPU: dlco_desc_match_guided_epipolar / match_guided_epipolar_device /
cross_sqdists_guided_epipolar.

Every comparison is with equality, distances through view(np.uint32).  The reference is the GPU's own cross_sqdists(Q, T),
which tests/test_match_gpu.py holds against float64, masked by the numpy restatement of the predicate (epi_mask of
tests/test_guided_epipolar_rules.py, which the CPU tests hold against the header): the guided matrix is that matrix with +inf
where the predicate fails, and the guided answer is the top two of its finite entries under the (distance, index) key.  No
tolerance is involved anywhere.

The coordinates are those of guided_case, the model is case_F (an epipole well outside the frame) and the threshold is 2: a
band of train points for every query.  Every case with 100 train rows or more first asserts, from the numpy predicate alone
and before the library's answer is read, that at least 90 % of its queries admit two or more; smaller cases that the mask is
not empty.  The single pair of the 1 x 1 case is not admitted at threshold 2, so that case runs a second time at 2^20, where it
is: the empty and the full mask.  Planted where nq >= 100: query 2 with a NaN coordinate, which admits nothing on either side,
and the tied descriptor rows of make_tables."""
import functools

import numpy as np
import pytest

from test_describe_gpu import make_w, pair_set
from test_descriptors import make_filters
from test_epipolar_rules import planted_case
from test_guided_epipolar_rules import BOUNDARY_F, THRESHOLD, boundary_pairs, contraction_pairs, epi_mask, epipolar_case
from test_guided_rules import INF, RADIUS, guided_case, top2_of_masked
from test_match_gpu import make_tables
from test_verify_gpu import ratio_cross_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=8)
def geometry(nq, nt, f_side, threshold=THRESHOLD):
    """(qxy, txy, F, mask) of a shared case, computed once and left unchanged; asserts the condition on the input"""
    qxy, txy, F = epipolar_case(nq, nt)
    mask = epi_mask(F, qxy, txy, threshold, f_side)
    per_row = mask.sum(1)
    if nt >= 100:
        assert (per_row >= 2).mean() >= 0.9, "the case is unfit: %.3f of its queries admit two or more" % (per_row >= 2).mean()
        assert not mask.all()
    elif (nq, nt) != (1, 1):
        assert mask.any() and not mask.all()
    if nq >= 100:
        assert per_row[2] == 0                                               # the planted NaN query
    return qxy, txy, F, mask


def same_top2(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(u32(got[1]), u32(want[1]))


# ---- 1. the guided matrix is the plain matrix with +inf where the predicate fails ----------------------------------------------
@pytest.mark.parametrize("f_side", [0, 1])
@pytest.mark.parametrize("nq,nt,r", [(300, 500, r) for r in (1, 3, 64, 67, 128, 129, 200)] + [(37, 2, 64), (129, 17, 64), (1, 1, 64)])
def test_cross_sqdists_guided_epipolar_is_the_masked_cross_matrix(ctx, nq, nt, r, f_side):
    Q, T = make_tables(nq, nt, r)
    X = ctx.cross_sqdists(Q, T)
    seen = False
    for threshold in (THRESHOLD, 2.0 ** 20) if (nq, nt) == (1, 1) else (THRESHOLD,):
        qxy, txy, F, mask = geometry(nq, nt, f_side, threshold)
        seen = seen or bool(mask.any())
        G = ctx.cross_sqdists_guided_epipolar(Q, qxy, T, txy, F, threshold, f_side)
        assert G.shape == (nq, nt) and G.dtype == np.float32 and np.isfinite(X).all()
        want = np.where(mask, X, INF)
        print("cross_sqdists_guided_epipolar %d x %d r %d f_side %d threshold %g: %d of %d entries admitted, %d differ"
              % (nq, nt, r, f_side, threshold, mask.sum(), mask.size, (u32(G) != u32(want)).sum()))
        assert np.array_equal(u32(G), u32(want))
    assert seen


# ---- 2. the guided answer is the top two of that matrix --------------------------------------------------------------------------
SHAPES = ([(3000, 5000, r, 0) for r in (1, 48, 64, 67, 128, 200)] + [(4100, 4100, 128, 0), (3, 40000, 64, 0), (20000, 300, 48, 0), (130, 129, 200, 0),
                                                                     (3000, 5000, 64, 1), (3, 40000, 64, 1)])


@pytest.mark.parametrize("nq,nt,r,f_side", SHAPES)
def test_match_guided_epipolar_is_the_top_two_of_the_masked_matrix(ctx, nq, nt, r, f_side):
    qxy, txy, F, mask = geometry(nq, nt, f_side)
    Q, T = make_tables(nq, nt, r)
    want = top2_of_masked(np.where(mask, ctx.cross_sqdists(Q, T), INF))
    idx, d = ctx.match_guided_epipolar(Q, qxy, T, txy, F, THRESHOLD, f_side)
    assert idx.shape == (nq, 2) and idx.dtype == np.int32 and d.shape == (nq, 2) and d.dtype == np.float32
    print("match_guided_epipolar %d x %d r %d f_side %d: %d index and %d distance mismatches; %d queries with none, %d with one admitted"
          % (nq, nt, r, f_side, (idx != want[0]).sum(), (u32(d) != u32(want[1])).sum(), (want[0][:, 0] < 0).sum(), ((want[0][:, 0] >= 0) & (want[0][:, 1] < 0)).sum()))
    assert same_top2((idx, d), want)
    assert ((idx >= -1) & (idx < nt)).all() and (d[idx < 0] == INF).all() and np.isfinite(d[idx >= 0]).all()
    per_row = mask.sum(1)
    assert ((idx[:, 0] == -1) == (per_row == 0)).all() and ((idx[:, 1] == -1) == (per_row <= 1)).all()
    assert ctx.last_kernel_ms() > 0


# ---- 3. f_side = 1 with the tables swapped sees the transpose of the same admissible set -----------------------------------------
@pytest.mark.parametrize("nq,nt,r", [(3000, 5000, 64), (130, 129, 200)])
def test_swapped_tables_with_f_side_1_see_the_transposed_mask(ctx, nq, nt, r):
    qxy, txy, F, mask = geometry(nq, nt, 0)
    assert np.array_equal(epi_mask(F, txy, qxy, THRESHOLD, 1), mask.T)
    Q, T = make_tables(nq, nt, r)
    want = top2_of_masked(np.where(mask.T, ctx.cross_sqdists(T, Q), INF))
    back = ctx.match_guided_epipolar(T, txy, Q, qxy, F, THRESHOLD, 1)
    assert same_top2(back, want)
    fwd = ctx.match_guided_epipolar(Q, qxy, T, txy, F, THRESHOLD, 0)
    mutual = [(i, j) for i, j in enumerate(fwd[0][:, 0].tolist()) if j >= 0 and back[0][j, 0] == i]
    assert len(mutual) > 0 and all(mask[i, j] for i, j in mutual)


# ---- 4. a predicate that admits everything gives the plain answer, one that admits nothing an empty one ---------------------------
def test_everything_admitted_equals_the_plain_match_and_the_zero_model_admits_nothing(ctx):
    nq, nt, r = 3000, 5000, 64
    Q, T = make_tables(nq, nt, r)
    rng = np.random.default_rng(3)
    qxy, txy = ((rng.random((n, 2)) * (2.0 ** 20 - 1)).astype(np.float32) for n in (nq, nt))
    assert qxy.max() < 2.0 ** 20 and txy.max() < 2.0 ** 20
    huge = 2.0 ** 22                                                         # S = 4 and |e| < 2^22: e e < t2 S for every pair
    plain = ctx.match(Q, T)
    for f_side in (0, 1):
        got = ctx.match_guided_epipolar(Q, qxy, T, txy, BOUNDARY_F, huge, f_side)
        assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes(), f_side
    # the same after an earlier, larger call that admitted little: stale records and partials would show
    n2, t2 = 4100, 12000
    q2, x2, F2 = epipolar_case(n2, t2)
    Q2, T2 = make_tables(n2, t2, r)
    for f_side in (0, 1):
        ctx.match_guided_epipolar(Q2, q2, T2, x2, F2, THRESHOLD, f_side)
        small = ctx.match_guided_epipolar(Q[:300], qxy[:300], T[:2000], txy[:2000], BOUNDARY_F, huge, f_side)
        want = ctx.match(Q[:300], T[:2000])
        assert small[0].tobytes() == want[0].tobytes() and small[1].tobytes() == want[1].tobytes(), f_side
        idx, d = ctx.match_guided_epipolar(Q[:300], qxy[:300], T[:2000], txy[:2000], np.zeros((3, 3)), huge, f_side)
        assert (idx == -1).all() and (d == INF).all(), f_side
        assert (ctx.cross_sqdists_guided_epipolar(Q[:300], qxy[:300], T[:200], txy[:200], np.zeros((3, 3)), huge, f_side) == INF).all()


# ---- 5. independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f_side", [0, 1])
def test_match_guided_epipolar_does_not_depend_on_nq_or_on_the_run(ctx, f_side):
    nq, nt, r = 3000, 5000, 64
    qxy, txy, F, _ = geometry(nq, nt, f_side)
    Q, T = make_tables(nq, nt, r)
    idx, d = ctx.match_guided_epipolar(Q, qxy, T, txy, F, THRESHOLD, f_side)
    for n in (1, 15, 16, 17, 127, 128, 129):
        i_n, d_n = ctx.match_guided_epipolar(Q[:n], qxy[:n], T, txy, F, THRESHOLD, f_side)
        assert np.array_equal(i_n, idx[:n]) and np.array_equal(u32(d_n), u32(d[:n])), n
    i2, d2 = ctx.match_guided_epipolar(Q, qxy, T, txy, F, THRESHOLD, f_side)
    assert idx.tobytes() == i2.tobytes() and d.tobytes() == d2.tobytes()


# ---- 6. the two loops of the host path carry the coordinates with the rows -----------------------------------------------------------
BLOCK, BASE = 2 ** 20, 1009                                # queries per launch; a prime period of repeated queries (and coordinates)
CHUNK_BYTES, WIDE = 2 ** 28, 1021                          # the documented chunk size of the uploads; rows whose host and device pitch differ
CHUNK = CHUNK_BYTES // ((4 * WIDE + 15) // 16 * 16)


def loop_case(ctx, nq, nt, r, f_side, first, marks):
    """the construction of tests/test_guided_gpu.py: nq queries that repeat a base of BASE rows, coordinates included; row i
    carries the answer of row i mod BASE of the base's own guided match, which is held against the masked matrix first.  `first`
    is the row at which the loop under test starts its second round; BASE does not divide it, so records formed from coordinates
    that stayed behind at offset 0 would belong to other rows."""
    qxy, txy, F, mask = geometry(BASE, nt, f_side)
    Qb, T = make_tables(BASE, nt, r)
    bi, bd = ctx.match_guided_epipolar(Qb, qxy, T, txy, F, THRESHOLD, f_side)
    assert same_top2((bi, bd), top2_of_masked(np.where(mask, ctx.cross_sqdists(Qb, T), INF)))
    assert first % BASE != 0 and (bi != np.roll(bi, -(first % BASE), 0)).any(1).mean() > 0.5
    rep = np.arange(nq) % BASE
    idx, d = ctx.match_guided_epipolar(Qb[rep], qxy[rep], T, txy, F, THRESHOLD, f_side)
    bad = np.nonzero((idx != bi[rep]).any(1) | (u32(d) != u32(bd[rep])).any(1))[0]
    print("match_guided_epipolar %d x %d r %d f_side %d: %d rows differ from the base's" % (nq, nt, r, f_side, len(bad)))
    assert len(bad) == 0, "rows %s differ; %s" % (bad[:8].tolist(), "; ".join(
        "row %d: got %s / %s, want %s / %s" % (i, idx[i].tolist(), d[i].tolist(), bi[i % BASE].tolist(), bd[i % BASE].tolist()) for i in marks))


@pytest.mark.parametrize("f_side", [0, 1])
def test_match_guided_epipolar_over_the_query_block_loop(ctx, f_side):
    loop_case(ctx, BLOCK + 77, 700, 4, f_side, BLOCK, (BLOCK - 1, BLOCK, BLOCK + 76))


@pytest.mark.parametrize("f_side", [0, 1])
def test_match_guided_epipolar_over_the_query_chunk_loop(ctx, f_side):
    assert CHUNK == 65536
    loop_case(ctx, CHUNK + 37, 40, WIDE, f_side, CHUNK, (CHUNK - 1, CHUNK, CHUNK + 36))


# ---- 7. the device form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,ld,f_side", [(48, 52, 0), (67, 68, 1)])
def test_match_guided_epipolar_device_on_tables_written_by_describe_device(dlco, r, ld, f_side):
    import torch
    nsel = 60
    patches, _ = pair_set(n_base=30, n_pairs=10, seed=11)
    pq, pt = patches[:70], patches[40:]
    nq, nt = len(pq), len(pt)
    assert (nq, nt) == (70, 80)
    qxy, txy, F, mask = geometry(nq, nt, f_side)
    c = dlco.DescContext()
    c.set_filters(make_filters(nsel, seed=nsel))
    c.set_projection(make_w(r, nsel * 8, seed=r))
    Yq, Yt = c.describe(pq), c.describe(pt)
    want_i, want_d = c.match_guided_epipolar(Yq, qxy, Yt, txy, F, THRESHOLD, f_side)
    assert same_top2((want_i, want_d), top2_of_masked(np.where(mask, c.cross_sqdists(Yq, Yt), INF)))
    assert not np.array_equal(want_i, c.match(Yq, Yt)[0])
    # keypoint rows [n][4] = (x, y, scale, angle) as detect_device writes them: pitch 4, the last two never read
    kq, kt = np.full((nq, 4), np.nan, np.float32), np.full((nt, 4), -3.5, np.float32)
    kq[:, :2], kt[:, :2] = qxy, txy
    dq, dt = torch.from_numpy(kq).to("cuda:0"), torch.from_numpy(kt).to("cuda:0")
    sq, st = -7.25, float("nan")                                          # the columns beyond r: never read into a distance, never written
    bq = torch.full((nq, ld), sq, dtype=torch.float32, device="cuda:0")
    bt = torch.full((nt, ld), st, dtype=torch.float32, device="cuda:0")
    oi = torch.full((nq, 2), -5, dtype=torch.int32, device="cuda:0")
    od = torch.full((nq, 2), -5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    c.describe_device(pq, bq.data_ptr(), ld=ld)
    c.describe_device(pt, bt.data_ptr(), ld=ld)
    args = (bq.data_ptr(), dq.data_ptr(), nq, bt.data_ptr(), dt.data_ptr(), nt, r, F, oi.data_ptr(), od.data_ptr())
    c.match_guided_epipolar_device(*args, threshold=THRESHOLD, f_side=f_side, ldq=ld, ldt=ld, ldxy_q=4, ldxy_t=4)
    torch.cuda.synchronize()
    assert c.last_kernel_ms() > 0
    gq, gt = bq.cpu().numpy(), bt.cpu().numpy()
    assert np.array_equal(gq[:, :r], Yq) and np.array_equal(gt[:, :r], Yt)
    assert (gq[:, r:] == np.float32(sq)).all() and np.isnan(gt[:, r:]).all()
    assert dq.cpu().numpy().tobytes() == kq.tobytes() and dt.cpu().numpy().tobytes() == kt.tobytes()
    assert np.array_equal(oi.cpu().numpy(), want_i) and np.array_equal(u32(od.cpu().numpy()), u32(want_d))
    for bad in (dict(ldxy_q=1), dict(ldxy_t=1), dict(ldxy_q=0), dict(ldxy_t=-4), dict(ldq=ld + 1), dict(ldt=ld + 2), dict(ldq=r - 4), dict(ldt=4)):
        with pytest.raises(dlco.DlcoError) as ei:
            c.match_guided_epipolar_device(*args, **{**dict(threshold=THRESHOLD, f_side=f_side, ldq=ld, ldt=ld, ldxy_q=4, ldxy_t=4), **bad})
        assert ei.value.code == dlco.ERR_INVALID, bad
    assert np.array_equal(oi.cpu().numpy(), want_i) and np.array_equal(u32(od.cpu().numpy()), u32(want_d))
    c.close()


# ---- 8. the boundary and the pairs on which a fused multiply-add would show, through the kernel --------------------------------------
@pytest.mark.parametrize("r", [4, 200])
def test_boundary_and_contraction_pairs_through_the_kernel(ctx, r):
    Q, T = np.full((1, r), 0.5, np.float32), np.full((1, r), 0.25, np.float32)

    def verdicts(F, src, dst, threshold):
        """the entry of the 1 x 1 guided matrix, both ways round: finite or +inf"""
        a = ctx.cross_sqdists_guided_epipolar(Q, src, T, dst, F, threshold, 0)
        b = ctx.cross_sqdists_guided_epipolar(T, dst, Q, src, F, threshold, 1)
        assert a.shape == b.shape == (1, 1) and all(np.isfinite(x[0, 0]) or x[0, 0] == INF for x in (a, b))
        assert np.isfinite(a[0, 0]) == np.isfinite(b[0, 0])
        return bool(np.isfinite(a[0, 0]))

    pairs = contraction_pairs()
    assert len(pairs) == 8
    for F, src, dst, t in pairs:
        assert verdicts(F, src, dst, t), "a product was fused with its sum: %s" % F.tolist()
    for src, dst, k in boundary_pairs():
        t_in = np.float32(k)
        assert verdicts(BOUNDARY_F, src, dst, t_in) and not verdicts(BOUNDARY_F, src, dst, np.nextafter(t_in, np.float32(0))), k


# ---- 9. the chain: match, verify against F, match again under F -------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def chain_case():
    """(src, dst [300,2], Ya, Yb [300,64]): the keypoints of a two-camera scene with 30 % of the dst rows elsewhere, and a
    descriptor row per point: random for src, the src row plus noise of a tenth of the row scale for the dst point of a planted
    pair, random for the others"""
    src, dst, planted = planted_case(300, 0.3, 7, 0.3)
    rng = np.random.default_rng(64)
    scale = 0.25
    Ya = rng.standard_normal((300, 64)) * scale
    Yb = rng.standard_normal((300, 64)) * scale
    Yb[planted] = Ya[planted] + rng.standard_normal((int(planted.sum()), 64)) * (0.1 * scale)
    return src, dst, Ya.astype(np.float32), Yb.astype(np.float32)


def test_guided_matching_under_F_keeps_every_verified_match(ctx):
    src, dst, Ya, Yb = chain_case()
    nearest, sqdist = ctx.match(Ya, Yb)
    back, _ = ctx.match(Yb, Ya)
    matches = ratio_cross_ref(nearest, sqdist, back, 0.8)
    F, inl, best = ctx.verify_fundamental(src[matches[:, 0]], dst[matches[:, 1]], threshold=3.0)
    assert best >= 0 and inl.sum() >= 100
    verified = set(map(tuple, matches[inl].tolist()))
    g_near, g_d = ctx.match_guided_epipolar(Ya, src, Yb, dst, F, 3.0, 0)
    g_back, _ = ctx.match_guided_epipolar(Yb, dst, Ya, src, F, 3.0, 1)
    guided = ratio_cross_ref(g_near, g_d, g_back, 0.8)
    print("chain: %d matches, %d verified; guided: %d matches" % (len(matches), len(verified), len(guided)))
    assert verified <= set(map(tuple, guided.tolist()))
    assert all(epi_mask(F, src[i:i + 1], dst[j:j + 1], 3.0)[0, 0] for i, j in guided.tolist())


# ---- 10. the existing surface is untouched -------------------------------------------------------------------------------------------
def test_an_epipolar_guided_call_leaves_the_other_calls_alone(dlco):
    patches, pairs = pair_set(n_base=12, n_pairs=200, seed=2)
    c = dlco.DescContext()
    c.set_filters(make_filters(60, seed=60))
    c.set_projection(make_w(48, 480, seed=1))
    Y = c.describe(patches)
    Yr = Y[::-1].copy()
    qxy, txy, H = guided_case(len(Y), len(Y))
    F = epipolar_case(len(Y), len(Y))[2]

    def others():
        out = [c.describe(patches), c.cross_sqdists(Y[:20], Y)]
        out += list(c.match(Y, Yr)) + list(c.pair_sqdists(patches, pairs))
        for h_side in (0, 1):
            out += list(c.match_guided(Y, qxy, Yr, txy, H, RADIUS, h_side)) + [c.cross_sqdists_guided(Y[:20], qxy[:20], Y, txy, H, RADIUS, h_side)]
        return out

    before = others()
    for f_side in (0, 1):
        idx, d = c.match_guided_epipolar(Y, qxy, Yr, txy, F, THRESHOLD, f_side)
        G = c.cross_sqdists_guided_epipolar(Y[:20], qxy[:20], Y, txy, F, THRESHOLD, f_side)
        assert idx.shape == (len(Y), 2) and G.shape == (20, len(Y)) and np.isinf(G).any() and np.isfinite(G).any()
    after = others()
    assert len(before) == len(after) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(before, after))
    c.close()
