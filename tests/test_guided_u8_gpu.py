"""Guided matching on byte tables on a GPU: dlco_desc_match_guided_u8 / _epipolar_u8, their device forms and matrices.

Every comparison is equality of integers.  The reference is the exact integer matrix (ref_matrix of
tests/test_match_u8_tiles_gpu.py, ref_u8 of tests/test_match_u8_gpu.py) masked by the numpy restatements of the two predicates
(pair_mask of tests/test_guided_rules.py, epi_mask of tests/test_guided_epipolar_rules.py, which the CPU tests hold against the
headers): the guided matrix is that matrix with INT32_MAX where the predicate fails, the guided answer the top two of its
entries below INT32_MAX under the (distance, index) order.  No tolerance is involved anywhere.

Coordinates and models are those of guided_case / epipolar_case.  Every case with 100 train rows or more first asserts, from
the numpy mask alone and before the library's answer is read, that at least 90 % of its queries admit two or more rows.
Planted where nq >= 100: query 1 with W < 0 (under the homography), query 2 with a NaN coordinate."""
import functools

import numpy as np
import pytest

from test_describe_gpu import make_w, pair_set
from test_descriptors import make_filters
from test_guided_epipolar_rules import BOUNDARY_F, THRESHOLD, epi_mask, epipolar_case
from test_guided_epipolar_rules import boundary_pairs as epi_boundary_pairs, contraction_pairs as epi_contraction_pairs
from test_guided_rules import RADIUS, boundary_pairs, contraction_pairs, guided_case, pair_mask
from test_match_slices import slices, tiles_per_slice
from test_match_u8_gpu import byte_tables, ref_u8
from test_match_u8_tiles_gpu import ref_matrix
from test_verify_gpu import chain_model, ratio_cross_ref, shifted_pair

pytestmark = pytest.mark.gpu

I32MAX = 2 ** 31 - 1
TILE = 128
MODELS = ("H", "F")
SIDES = (0, 1)


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def bound(kind):
    return RADIUS if kind == "H" else THRESHOLD


def mask_of(kind, M, qxy, txy, t, side):
    return pair_mask(M, qxy, txy, t, side) if kind == "H" else epi_mask(M, qxy, txy, t, side)


def fit(mask, tag=""):
    """the condition on the input: at least 90 % of the queries admit two or more rows (nt >= 100)"""
    if mask.shape[1] >= 100:
        share = (mask.sum(1) >= 2).mean()
        assert share >= 0.9, "%s: the case is unfit: %.3f of its queries admit two or more" % (tag, share)
        assert not mask.all()


@functools.lru_cache(maxsize=16)
def geometry(kind, nq, nt, side):
    """(qxy, txy, M, mask) of a shared case, computed once and left unchanged; asserts the condition on the input"""
    qxy, txy, M = guided_case(nq, nt) if kind == "H" else epipolar_case(nq, nt)
    mask = mask_of(kind, M, qxy, txy, bound(kind), side)
    fit(mask, "%s %d x %d side %d" % (kind, nq, nt, side))
    if nq >= 100:
        assert not mask[2].any() and (kind == "F" or side == 1 or not mask[1].any())          # the planted rows: NaN, W < 0
    for a in (qxy, txy, M, mask):
        a.setflags(write=False)
    return qxy, txy, M, mask


@functools.lru_cache(maxsize=4)
def tables(nq, nt, r, hi=256):
    """(Q, T, D): byte tables and their exact integer matrix (every entry is below 2^27), computed once and left unchanged"""
    Q, T = byte_tables(nq, nt, r, hi)
    D = (ref_matrix(Q, T) if nq * nt > 2 ** 16 else ref_u8(Q, T)).astype(np.int32)
    for a in (Q, T, D):
        a.setflags(write=False)
    return Q, T, D


def masked(D, mask):
    return np.where(mask, D, I32MAX).astype(np.int32)


def top2_of_masked(D, mask):
    """(idx [nq,2] int32, d [nq,2] int32): the first two admitted entries of every row under (distance, index); -1 / INT32_MAX
    where a row has fewer.  The keys D * nt + index are unique among the admitted."""
    nq, nt = D.shape
    big = np.int64(I32MAX) * nt
    K = np.where(mask, D.astype(np.int64) * nt + np.arange(nt, dtype=np.int64), big)
    if nt == 1:
        K = np.concatenate([K, np.full((nq, 1), big)], 1)
    two = np.sort(np.partition(K, 1, axis=1)[:, :2], axis=1)
    none = two >= big
    return np.where(none, -1, two % nt).astype(np.int32), np.where(none, I32MAX, two // nt).astype(np.int32)


def call(ctx, kind, Q, qxy, T, txy, M, side, t=None):
    t = bound(kind) if t is None else t
    return (ctx.match_guided_u8 if kind == "H" else ctx.match_guided_epipolar_u8)(Q, qxy, T, txy, M, t, side)


def cross(ctx, kind, Q, qxy, T, txy, M, side, t=None):
    t = bound(kind) if t is None else t
    return (ctx.cross_sqdists_guided_u8 if kind == "H" else ctx.cross_sqdists_guided_epipolar_u8)(Q, qxy, T, txy, M, t, side)


def report(tag, got, want):
    bad = np.nonzero((got[0] != want[0]).any(1) | (got[1] != want[1]).any(1))[0]
    msg = "%s: %d of %d rows differ, the first at %s" % (tag, len(bad), len(want[0]), bad[:8].tolist())
    for i in bad[:3]:
        msg += "\n    row %d: got %s / %s, want %s / %s" % (i, got[0][i].tolist(), got[1][i].tolist(), want[0][i].tolist(), want[1][i].tolist())
    return msg


def same(got, want):
    return got[0].dtype == np.int32 and got[1].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def check_top2(ctx, kind, nq, nt, r, side, hi=256):
    qxy, txy, M, mask = geometry(kind, nq, nt, side)
    Q, T, D = tables(nq, nt, r, hi)
    want = top2_of_masked(D, mask)
    got = call(ctx, kind, Q, qxy, T, txy, M, side)
    tag = "match_guided%s_u8 %d x %d r %d side %d" % ("" if kind == "H" else "_epipolar", nq, nt, r, side)
    print("%s: %d index and %d distance mismatches; %d queries with none, %d with one admitted"
          % (tag, (got[0] != want[0]).sum(), (got[1] != want[1]).sum(), (want[0][:, 0] < 0).sum(), ((want[0][:, 0] >= 0) & (want[0][:, 1] < 0)).sum()))
    assert got[0].shape == (nq, 2) and got[1].shape == (nq, 2)
    assert same(got, want), report(tag, got, want)
    assert ((got[0] >= -1) & (got[0] < nt)).all() and (got[1][got[0] < 0] == I32MAX).all() and (got[1][got[0] >= 0] < I32MAX).all()
    assert ctx.last_kernel_ms() > 0
    return got


# ---- 1. the guided matrix is the plain matrix with INT32_MAX where the predicate fails ------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", MODELS)
@pytest.mark.parametrize("nq,nt,r", [(300, 500, r) for r in (1, 16, 64, 67, 128, 129, 200)] + [(37, 2, 64), (1, 1, 64), (129, 17, 64)])
def test_the_guided_matrix_is_the_masked_plain_matrix(ctx, nq, nt, r, kind, side):
    qxy, txy, M, mask = geometry(kind, nq, nt, side)
    Q, T, D = tables(nq, nt, r)
    X = ctx.cross_sqdists_u8(Q, T)
    assert np.array_equal(X, D)
    seen = False
    for t in (bound(kind), 2.0 ** 20) if (nq, nt) == (1, 1) else (bound(kind),):           # 1 x 1: the empty and the full mask
        if t != bound(kind):
            mask = mask_of(kind, M, qxy, txy, t, side)
        seen = seen or bool(mask.any())
        G = cross(ctx, kind, Q, qxy, T, txy, M, side, t)
        want = masked(D, mask)
        print("cross_sqdists_guided_u8 %s %d x %d r %d side %d bound %g: %d of %d entries admitted, %d differ"
              % (kind, nq, nt, r, side, t, mask.sum(), mask.size, (G != want).sum()))
        assert G.shape == (nq, nt) and G.dtype == np.int32 and np.array_equal(G, want)
        got = call(ctx, kind, Q, qxy, T, txy, M, side, t)
        assert same(got, top2_of_masked(D, mask)), report("top two of the matrix", got, top2_of_masked(D, mask))
    assert seen


# ---- 2. the top two, one tile per slice and a merge ------------------------------------------------------------------------------
SHAPES = ([(3000, 5000, r, 0) for r in (16, 64, 128, 200)] + [(130, 129, 200, 0), (3, 40000, 64, 0), (20000, 300, 48, 0), (3000, 5000, 64, 1), (3, 40000, 64, 1)])


@pytest.mark.parametrize("kind", MODELS)
@pytest.mark.parametrize("nq,nt,r,side", SHAPES)
def test_the_guided_answer_is_the_top_two_of_the_masked_matrix(ctx, n_cu, nq, nt, r, side, kind):
    if (nq, nt) == (3000, 5000):
        tps = tiles_per_slice(nq, nt, n_cu, "u8")
        print("3000 x 5000 at %d CUs: %d tiles per slice, %d slices" % (n_cu, tps, slices(nt, tps, "u8")))
        assert slices(nt, tps, "u8") > 1, "the case is unfit: no merge"
    got = check_top2(ctx, kind, nq, nt, r, side)
    mask = geometry(kind, nq, nt, side)[3]
    per_row = mask.sum(1)
    assert ((got[0][:, 0] == -1) == (per_row == 0)).all() and ((got[0][:, 1] == -1) == (per_row <= 1)).all()


# ---- 3. several tiles per slice: both LDS buffers of the staged geometry are in use ---------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", MODELS)
@pytest.mark.parametrize("r", [64, 200])
def test_several_tiles_per_slice(ctx, n_cu, r, kind, side):
    nq, nt = 16384, 2600
    tps = tiles_per_slice(nq, nt, n_cu, "u8")
    s = slices(nt, tps, "u8")
    print("%d x %d at %d CUs: %d tiles per slice, %d slices" % (nq, nt, n_cu, tps, s))
    assert tps >= 3 and s >= 2, "the case is unfit: %d tiles per slice, %d slices at %d CUs" % (tps, s, n_cu)
    check_top2(ctx, kind, nq, nt, r, side)


# ---- 4. ties: the lower-indexed of two equal candidates is not admitted --------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", MODELS)
def test_ties_where_the_lower_index_is_not_admitted(ctx, n_cu, kind, side):
    """Bytes below 4: ties are the rule.  Exact copies of one train row in two lane groups of one MFMA, in another 16-row block,
    in the next tile, in the next slice and in the last row of the table, and a query equal to them: distance 0 six times.  The
    copies take the coordinates of a train point the query admits, or of one it does not, in several patterns: the answer
    names the first two admitted copies.  A mask applied after the compare would name a lower, rejected one or lose the second."""
    nq, nt, r = 8192, 2600, 64
    tps = tiles_per_slice(nq, nt, n_cu, "u8")
    assert tps >= 2 and slices(nt, tps, "u8") >= 3, "the case is unfit: %d tiles per slice at %d CUs" % (tps, n_cu)
    qxy, txy, M, mask0 = geometry(kind, nq, nt, side)
    Q, T = (a.copy() for a in byte_tables(nq, nt, r, 4))
    rng = np.random.default_rng(9400)
    row = rng.integers(0, 4, r, dtype=np.uint8)
    clash = (T == row).all(1)
    T[clash, 0] = (T[clash, 0] + 1) % 4
    j = tps * TILE + 3                                     # the first tile of the second slice
    planted = [j, j + 4, j + 16, j + TILE, j + tps * TILE, nt - 1]
    assert planted == sorted(set(planted)) and (j + TILE) // (tps * TILE) == j // (tps * TILE) != (j + tps * TILE) // (tps * TILE)
    T[planted] = row
    qi = nq - 5
    Q[qi] = row
    free = np.setdiff1d(np.arange(nt), planted)
    yes, no = free[mask0[qi, free]][0], free[~mask0[qi, free]][0]
    D = ref_matrix(Q, T).astype(np.int32)
    assert (D[qi, planted] == 0).all() and (np.delete(D[qi], planted) > 0).all()
    s3 = np.sort(np.partition(D, 2, axis=1)[:, :3], axis=1)
    assert ((s3[:, 0] == s3[:, 1]) | (s3[:, 1] == s3[:, 2])).mean() >= 0.05, "the case is unfit: ties are rare"
    for pattern in ("010101", "001010", "000011", "100100"):
        xy = txy.copy()
        for p, bit in zip(planted, pattern):
            xy[p] = txy[yes if bit == "1" else no]
        mask = mask0.copy()                                # a column of the mask depends on its own train point alone
        mask[:, planted] = mask_of(kind, M, qxy, xy[planted], bound(kind), side)
        fit(mask, "ties " + pattern)
        admitted = [p for p, bit in zip(planted, pattern) if bit == "1"]
        assert [p for p in planted if mask[qi, p]] == admitted
        want = top2_of_masked(D, mask)
        assert want[0][qi].tolist()[:len(admitted)] == admitted[:2] and want[1][qi, 0] == 0
        got = call(ctx, kind, Q, qxy, T, xy, M, side)
        print("ties %s side %d pattern %s: %d index and %d distance mismatches" % (kind, side, pattern, (got[0] != want[0]).sum(), (got[1] != want[1]).sum()))
        assert same(got, want), report("pattern " + pattern, got, want)


# ---- 5. planted rows: W < 0, NaN, and a point at an epipole ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MODELS)
def test_planted_rows_admit_nothing(ctx, kind):
    nq, nt, r = 300, 500, 64
    qxy, txy, M, mask = geometry(kind, nq, nt, 0)
    Q, T, D = tables(nq, nt, r)
    assert not mask[2].any() and (kind == "F" or not mask[1].any())
    idx, d = call(ctx, kind, Q, qxy, T, txy, M, 0)
    for i in (2,) if kind == "F" else (1, 2):
        assert (idx[i] == -1).all() and (d[i] == I32MAX).all()
    G = cross(ctx, kind, Q, qxy, T, txy, M, 0)
    assert (G[2] == I32MAX).all() and (G < I32MAX).any()


@pytest.mark.parametrize("side", SIDES)
def test_a_point_at_an_epipole_admits_everything(ctx, side):
    """F = [t]x with t = (100, 50, 1): F t = 0 exactly, so the query at (100, 50) has l = 0 (side 0) or m = 0 (side 1), e = 0, and
    admits every train point that is not at the epipole itself"""
    nq, nt, r = 300, 500, 64
    Q, T, D = tables(nq, nt, r)
    F = np.array([[0.0, -1.0, 50.0], [1.0, 0.0, -100.0], [-50.0, 100.0, 0.0]])
    rng = np.random.default_rng(77)
    qxy, txy = ((rng.random((n, 2)) * 200.0).astype(np.float32) for n in (nq, nt))
    qxy[7] = (100.0, 50.0)
    qxy[2, 0] = np.nan
    mask = epi_mask(F, qxy, txy, THRESHOLD, side)
    fit(mask, "epipole side %d" % side)
    assert mask[7].all() and not mask[2].any()
    got = call(ctx, "F", Q, qxy, T, txy, F, side)
    want = top2_of_masked(D, mask)
    assert same(got, want), report("epipole", got, want)
    plain = ctx.match_u8(Q, T)
    assert np.array_equal(got[0][7], plain[0][7]) and np.array_equal(got[1][7], plain[1][7])
    assert np.array_equal(cross(ctx, "F", Q, qxy, T, txy, F, side), masked(D, mask))


# ---- 6. a predicate that admits everything gives the plain answer ------------------------------------------------------------------
@pytest.mark.parametrize("kind", MODELS)
def test_everything_admitted_equals_the_plain_byte_match(ctx, kind):
    nq, nt, r = 3000, 5000, 64
    Q, T, _ = tables(nq, nt, r)
    rng = np.random.default_rng(3)
    qxy, txy = ((rng.random((n, 2)) * (2.0 ** 20 - 1)).astype(np.float32) for n in (nq, nt))
    M, huge = (np.eye(3), 2.0 ** 21) if kind == "H" else (BOUNDARY_F, 2.0 ** 22)            # S = 4 and |e| < 2^22
    plain = ctx.match_u8(Q, T)
    for side in SIDES:
        got = call(ctx, kind, Q, qxy, T, txy, M, side, huge)
        assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes(), side
    # the same after an earlier, larger guided call that admitted little: stale records and partials would show
    n2, t2 = 4100, 12000
    q2, x2, M2 = guided_case(n2, t2) if kind == "H" else epipolar_case(n2, t2)
    Q2, T2 = byte_tables(n2, t2, r)
    want = ctx.match_u8(Q[:300], T[:2000])
    for side in SIDES:
        call(ctx, kind, Q2, q2, T2, x2, M2, side)
        small = call(ctx, kind, Q[:300], qxy[:300], T[:2000], txy[:2000], M, side, huge)
        assert small[0].tobytes() == want[0].tobytes() and small[1].tobytes() == want[1].tobytes(), side
    if kind == "F":                                        # the zero model admits nothing
        idx, d = call(ctx, kind, Q[:300], qxy[:300], T[:2000], txy[:2000], np.zeros((3, 3)), 0, huge)
        assert (idx == -1).all() and (d == I32MAX).all()


# ---- 7. the boundary and the pairs on which a fused multiply-add would show, through the kernel ---------------------------------------
@pytest.mark.parametrize("r", [4, 200])
def test_boundary_and_contraction_pairs_through_the_kernel(ctx, r):
    Q, T = np.full((1, r), 7, np.uint8), np.full((1, r), 9, np.uint8)

    def verdicts(kind, M, a_xy, b_xy, t):
        """the entry of the 1 x 1 guided matrix, both ways round: the distance or INT32_MAX"""
        a = cross(ctx, kind, Q, a_xy, T, b_xy, M, 0, t)
        b = cross(ctx, kind, T, b_xy, Q, a_xy, M, 1, t)
        assert a.shape == b.shape == (1, 1) and all(x[0, 0] in (4 * r, I32MAX) for x in (a, b)) and a[0, 0] == b[0, 0]
        for (idx, d), side, args in ((call(ctx, kind, Q, a_xy, T, b_xy, M, 0, t), 0, a), (call(ctx, kind, T, b_xy, Q, a_xy, M, 1, t), 1, b)):
            assert idx.tolist() == [[0 if args[0, 0] < I32MAX else -1, -1]] and d.tolist() == [[int(args[0, 0]), I32MAX]], (kind, side)
        return bool(a[0, 0] < I32MAX)

    for H, qxy, txy, rho in contraction_pairs():
        assert verdicts("H", H, qxy, txy, rho), "a product was fused with the sum: %s" % H.tolist()
    for qxy, txy, k in boundary_pairs():
        r_in = np.float32(5 * k)
        assert verdicts("H", np.eye(3), qxy, txy, r_in) and not verdicts("H", np.eye(3), qxy, txy, np.nextafter(r_in, np.float32(0))), k
    pairs = epi_contraction_pairs()
    assert len(pairs) == 8
    for F, src, dst, t in pairs:
        assert verdicts("F", F, src, dst, t), "a product was fused with its sum: %s" % F.tolist()
    for src, dst, k in epi_boundary_pairs():
        t_in = np.float32(k)
        assert verdicts("F", BOUNDARY_F, src, dst, t_in) and not verdicts("F", BOUNDARY_F, src, dst, np.nextafter(t_in, np.float32(0))), k


# ---- 8. independence of nq and of the run ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", MODELS)
def test_the_answer_does_not_depend_on_nq_or_on_the_run(ctx, kind, side):
    nq, nt, r = 3000, 5000, 64
    qxy, txy, M, _ = geometry(kind, nq, nt, side)
    Q, T, _ = tables(nq, nt, r)
    idx, d = call(ctx, kind, Q, qxy, T, txy, M, side)
    for n in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257):
        i_n, d_n = call(ctx, kind, Q[:n], qxy[:n], T, txy, M, side)
        assert np.array_equal(i_n, idx[:n]) and np.array_equal(d_n, d[:n]), n
    i2, d2 = call(ctx, kind, Q, qxy, T, txy, M, side)
    assert idx.tobytes() == i2.tobytes() and d.tobytes() == d2.tobytes()


# ---- 9. the two loops of the host path carry the coordinates with the rows -----------------------------------------------------------
BLOCK, BASE = 2 ** 20, 1009                                # queries per launch; a prime period of repeated queries (and coordinates)
CHUNK_BYTES, WIDE = 2 ** 28, 1021                          # the documented chunk size of the uploads; rows whose host and device pitch differ
CHUNK = CHUNK_BYTES // ((WIDE + 15) // 16 * 16)            # the byte line's chunk: 262 144 rows


def loop_case(ctx, kind, nq, nt, r, side, first, marks):
    """the construction of tests/test_guided_gpu.py: nq queries that repeat a base of BASE rows, coordinates included; row i
    carries the answer of row i mod BASE of the base's own guided match, which is held against the masked matrix first."""
    qxy, txy, M, mask = geometry(kind, BASE, nt, side)
    Qb, T, D = tables(BASE, nt, r)
    bi, bd = call(ctx, kind, Qb, qxy, T, txy, M, side)
    assert same((bi, bd), top2_of_masked(D, mask))
    # the answers of rows `first` mod BASE apart differ: results or coordinates that stayed behind at offset 0 would show
    assert first % BASE != 0 and (bi != np.roll(bi, -(first % BASE), 0)).any(1).mean() > 0.5
    rep = np.arange(nq) % BASE
    idx, d = call(ctx, kind, Qb[rep], qxy[rep], T, txy, M, side)
    bad = np.nonzero((idx != bi[rep]).any(1) | (d != bd[rep]).any(1))[0]
    print("match_guided_u8 %s %d x %d r %d side %d: %d rows differ from the base's" % (kind, nq, nt, r, side, len(bad)))
    assert len(bad) == 0, "rows %s differ; %s" % (bad[:8].tolist(), "; ".join(
        "row %d: got %s / %s, want %s / %s" % (i, idx[i].tolist(), d[i].tolist(), bi[i % BASE].tolist(), bd[i % BASE].tolist()) for i in marks))


@pytest.mark.parametrize("kind,side", [("H", 0), ("H", 1), ("F", 0), ("F", 1)])
def test_over_the_query_block_loop(ctx, kind, side):
    loop_case(ctx, kind, BLOCK + 77, 700, 4, side, BLOCK, (BLOCK - 1, BLOCK, BLOCK + 76))


@pytest.mark.parametrize("kind,side", [("H", 0), ("H", 1), ("F", 0), ("F", 1)])
def test_over_the_query_chunk_loop(ctx, kind, side):
    assert CHUNK == 262144
    loop_case(ctx, kind, CHUNK + 37, 40, WIDE, side, CHUNK, (CHUNK - 1, CHUNK, CHUNK + 36))


# ---- 10. the device forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MODELS)
@pytest.mark.parametrize("r,ld,side", [(48, 64, 0), (67, 96, 1)])
def test_device_forms_on_tables_written_by_describe_u8_device(dlco, kind, r, ld, side):
    import torch
    nsel = 60
    patches, _ = pair_set(n_base=30, n_pairs=10, seed=11)
    pq, pt = patches[:70], patches[40:]
    nq, nt = len(pq), len(pt)
    assert (nq, nt) == (70, 80)
    qxy, txy, M, mask = geometry(kind, nq, nt, side)
    assert mask.any() and not mask.all()
    c = dlco.DescContext()
    c.set_filters(make_filters(nsel, seed=nsel))
    c.set_projection(make_w(r, nsel * 8, seed=r))
    scale, off = dlco.quant_fit(c.describe(patches))
    c.set_quantizer(scale, off)
    Yq, Yt = c.describe_u8(pq), c.describe_u8(pt)
    want = call(c, kind, Yq, qxy, Yt, txy, M, side)
    assert same(want, top2_of_masked(ref_u8(Yq, Yt), mask)) and not np.array_equal(want[0], c.match_u8(Yq, Yt)[0])
    # keypoint rows [n][4] = (x, y, scale, angle) as detect_device writes them: pitch 4, the last two never read
    kq, kt = np.full((nq, 4), np.nan, np.float32), np.full((nt, 4), np.nan, np.float32)
    kq[:, :2], kt[:, :2] = qxy, txy
    dq, dt = torch.from_numpy(kq).to("cuda:0"), torch.from_numpy(kt).to("cuda:0")
    bq = torch.full((nq, ld), 0xA5, dtype=torch.uint8, device="cuda:0")                    # the bytes beyond r: garbage, never read into a distance
    bt = torch.full((nt, ld), 0x3C, dtype=torch.uint8, device="cuda:0")
    oi = torch.full((nq, 2), -5, dtype=torch.int32, device="cuda:0")
    od = torch.full((nq, 2), -5, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    c.describe_u8_device(pq, bq.data_ptr(), ld=ld)
    c.describe_u8_device(pt, bt.data_ptr(), ld=ld)
    torch.cuda.synchronize()
    gq, gt = bq.cpu().numpy().copy(), bt.cpu().numpy().copy()
    assert np.array_equal(gq[:, :r], Yq) and np.array_equal(gt[:, :r], Yt) and (gq[:, r:] == 0xA5).all() and (gt[:, r:] == 0x3C).all()
    args = (bq.data_ptr(), dq.data_ptr(), nq, bt.data_ptr(), dt.data_ptr(), nt, r, M, oi.data_ptr(), od.data_ptr())
    fn = c.match_guided_u8_device if kind == "H" else c.match_guided_epipolar_u8_device
    good = dict(ldq=ld, ldt=ld, ldxy_q=4, ldxy_t=4)
    fn(*args, bound(kind), side, **good)
    torch.cuda.synchronize()
    assert c.last_kernel_ms() > 0
    assert np.array_equal(bq.cpu().numpy(), gq) and np.array_equal(bt.cpu().numpy(), gt)                   # the inputs are only read
    assert dq.cpu().numpy().tobytes() == kq.tobytes() and dt.cpu().numpy().tobytes() == kt.tobytes()
    assert np.array_equal(oi.cpu().numpy(), want[0]) and np.array_equal(od.cpu().numpy(), want[1])
    oi.fill_(-5)
    od.fill_(-5)
    torch.cuda.synchronize()
    for bad in (dict(ldxy_q=1), dict(ldxy_t=1), dict(ldxy_q=0), dict(ldxy_t=-4), dict(ldq=ld + 8), dict(ldt=ld + 4), dict(ldq=r // 16 * 16 - 16 or 0),
                dict(ldt=16)):
        with pytest.raises(dlco.DlcoError) as ei:
            fn(*args, bound(kind), side, **{**good, **bad})
        assert ei.value.code == dlco.ERR_INVALID, bad
    torch.cuda.synchronize()
    assert (oi.cpu().numpy() == -5).all() and (od.cpu().numpy() == -5).all()                # outputs untouched
    c.close()


# ---- 12. the quantised chain: match, verify, match again under the model, verify again ---------------------------------------------
def test_the_quantised_chain_keeps_every_verified_match(dlco, ctx):
    a, b = shifted_pair()
    chain_model(ctx)
    kps, floats = [], []
    for img in (a, b):
        ctx.set_image(img)
        kp, _, _ = ctx.detect_oriented(2, 3000000, 300)
        kps.append(kp)
        floats.append(ctx.describe_keypoints(kp)[0])
    scale, off = dlco.quant_fit(np.concatenate(floats))
    ctx.set_quantizer(scale, off)
    Ys = []
    for img, kp in zip((a, b), kps):
        ctx.set_image(img)
        Ys.append(ctx.describe_keypoints_u8(kp)[0])
    nearest, sqdist = ctx.match_u8(Ys[0], Ys[1])
    back, _ = ctx.match_u8(Ys[1], Ys[0])
    matches = ratio_cross_ref(nearest, sqdist, back, 0.8)
    H, inl, best = ctx.verify_homography(kps[0][matches[:, 0], :2], kps[1][matches[:, 1], :2], threshold=3.0)
    assert best >= 0 and inl.sum() >= 8
    verified = set(map(tuple, matches[inl].tolist()))
    xy0, xy1 = kps[0][:, :2], kps[1][:, :2]
    g_near, g_d = ctx.match_guided_u8(Ys[0], xy0, Ys[1], xy1, H, 6.0, 0)
    g_back, _ = ctx.match_guided_u8(Ys[1], xy1, Ys[0], xy0, H, 6.0, 1)
    guided = ratio_cross_ref(g_near, g_d, g_back, 0.8)
    print("quantised chain: %d matches, %d verified; guided: %d matches" % (len(matches), len(verified), len(guided)))
    assert verified <= set(map(tuple, guided.tolist()))
    assert all(pair_mask(H, xy0[i:i + 1], xy1[j:j + 1], 6.0)[0, 0] for i, j in guided.tolist())
    H2, inl2, best2 = ctx.verify_homography(xy0[guided[:, 0]], xy1[guided[:, 1]], threshold=3.0)
    assert best2 >= 0 and inl2.sum() >= inl.sum()


# ---- 13. the neighbours are untouched ----------------------------------------------------------------------------------------------
def test_byte_guided_calls_leave_the_other_calls_alone(dlco):
    c = dlco.DescContext()
    nq, nt, r = 300, 500, 64
    Q, T, _ = tables(nq, nt, r)
    rng = np.random.default_rng(5)
    Qf, Tf = rng.standard_normal((nq, r)).astype(np.float32), rng.standard_normal((nt, r)).astype(np.float32)
    qxy, txy, H, _ = geometry("H", nq, nt, 0)
    F = geometry("F", nq, nt, 0)[2]
    snapshot = lambda: (c.match_u8(Q, T), (c.cross_sqdists_u8(Q[:20], T),), c.match_pairs_u8([Q, T], [(0, 1), (1, 0)])[0],
                        c.match_guided(Qf, qxy, Tf, txy, H, RADIUS, 0), c.match_guided_epipolar(Qf, qxy, Tf, txy, F, THRESHOLD, 1),
                        (c.cross_sqdists_guided(Qf[:20], qxy[:20], Tf, txy, H, RADIUS, 1),), c.match(Qf, Tf))
    before = snapshot()
    for kind in MODELS:
        for side in SIDES:
            M = H if kind == "H" else F
            idx, d = call(c, kind, Q, qxy, T, txy, M, side)
            G = cross(c, kind, Q[:20], qxy[:20], T, txy, M, side)
            assert idx.shape == (nq, 2) and G.shape == (20, nt) and (G == I32MAX).any() and (G < I32MAX).any()
    after = snapshot()
    assert all(x.tobytes() == y.tobytes() for bs, as_ in zip(before, after) for x, y in zip(bs, as_))
    c.close()
