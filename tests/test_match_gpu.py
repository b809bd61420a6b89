"""dlco_desc_match / match_device / cross_sqdists on the GPU against float64 numpy on the same float32 tables, the direct
form ((q - t)^2).sum().

The bound is derived, not tuned.  The library forms d = max(0, |q|^2 + |t|^2 - 2 q.t) in double and rounds to float once.
Products of two floats are exact in double, so the value differs from the exact distance by one float rounding, 2^-24 d,
plus r + 2 double roundings of terms bounded by |q|^2 + |t|^2 + 2 sum|q_k t_k| <= 2 (|q|^2 + |t|^2).  The gate used here,
    2^-23 d + 4 (r + 2) 2^-53 (|q|^2 + |t|^2),
leaves a factor two on the float term (the reference's own rounding of d is 2^-53 relative and vanishes beside it).

Indices are compared with the reference's (distance, index) order for every query except those the reference itself calls
ambiguous: two neighbouring distances that differ, but by no more than the sum of their gates.  At most 0.2 % of a case's
queries may be so; the count comes from the reference alone and is asserted before the GPU's answer is looked at.  Exact
ties of the reference are not excluded: the smaller index wins, and the planted rows check it."""
import functools

import numpy as np
import pytest

from test_describe_gpu import make_w, pair_set
from test_descriptors import make_filters

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


def make_tables(nq, nt, r):
    """T = 0.25 N(0,1); half of the queries are noisy views of train rows, the rest fresh; planted exact ties.  Drawn in
    float64 in the order T, Q, src, noise."""
    rng = np.random.default_rng(1000 * r + nt)
    T = (rng.standard_normal((nt, r)) * 0.25).astype(np.float32)
    Q = (rng.standard_normal((nq, r)) * 0.25).astype(np.float32)
    k = nq // 2
    src = rng.integers(0, nt, k)
    Q[:k] = (T[src].astype(np.float64) + rng.standard_normal((k, r)) * 0.02).astype(np.float32)
    if nt >= 8:
        T[nt - 1] = T[3]
        T[nt // 2] = T[3]
        Q[nq - 1] = T[3]
        Q[nq - 2] = T[5]
    return Q, T


def ref_dists(Q, T):
    Q64, T64 = Q.astype(np.float64), T.astype(np.float64)
    D = np.empty((len(Q), len(T)))
    step = max(1, (1 << 24) // (T64.size))
    for i0 in range(0, len(Q), step):
        d = Q64[i0:i0 + step, None, :] - T64[None, :, :]
        D[i0:i0 + step] = (d * d).sum(2)
    return D


def gate(Q, T, D):
    r = Q.shape[1]
    nq2, nt2 = (Q.astype(np.float64) ** 2).sum(1), (T.astype(np.float64) ** 2).sum(1)
    return 2.0 ** -23 * D + 4 * (r + 2) * 2.0 ** -53 * (nq2[:, None] + nt2[None, :])


def top_by_key(D, k):
    """The first k columns of every row under the (distance, index) order."""
    nt = D.shape[1]
    return np.lexsort((np.broadcast_to(np.arange(nt), D.shape), D), axis=1)[:, :k]


@functools.lru_cache(maxsize=2)
def case(nq, nt, r):
    Q, T = make_tables(nq, nt, r)
    D = ref_dists(Q, T)
    return Q, T, D, gate(Q, T, D)


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()                                # no filters, no projection: matching needs neither
    yield c
    c.close()


# ---- 1. distances -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nt,r", [(300, 500, r) for r in (1, 3, 48, 64, 67, 128, 129, 200, 544, 1024)] + [(37, 2, 64), (1, 1, 64), (129, 17, 64)])
def test_cross_sqdists_within_the_derived_bound(ctx, nq, nt, r):
    Q, T = make_tables(nq, nt, r)
    D = ref_dists(Q, T)
    G = gate(Q, T, D)
    X = ctx.cross_sqdists(Q, T)
    assert X.shape == (nq, nt) and X.dtype == np.float32
    err = np.abs(X.astype(np.float64) - D)
    print("cross_sqdists %d x %d r %d: max |err| %.3e, max err/gate %.3f, min %.3e" % (nq, nt, r, err.max(), (err / G).max(), X.min()))
    assert (X >= 0).all()
    assert (err <= G).all(), float((err / G).max())


# ---- 2. the top two are the top two of that matrix, exactly -------------------------------------------------------------
@pytest.mark.parametrize("nq,nt,r", [(3000, 5000, r) for r in (1, 48, 64, 67, 128, 200)] + [(37, 2, 64), (5, 1, 64), (4100, 4100, 128)])
def test_match_is_the_top_two_of_the_cross_matrix(ctx, nq, nt, r):
    Q, T = make_tables(nq, nt, r)
    X = ctx.cross_sqdists(Q, T)
    idx, d = ctx.match(Q, T)
    assert idx.shape == (nq, 2) and idx.dtype == np.int32 and d.shape == (nq, 2) and d.dtype == np.float32
    order = top_by_key(X, 2)
    rows = np.arange(nq)[:, None]
    want_i, want_d = order.astype(np.int32), X[rows, order]
    if nt == 1:
        want_i = np.concatenate([want_i, np.full((nq, 1), -1, np.int32)], 1)
        want_d = np.concatenate([want_d, np.full((nq, 1), INF, np.float32)], 1)
    print("match %d x %d r %d: %d index and %d distance mismatches against the GPU's own matrix"
          % (nq, nt, r, (idx != want_i).sum(), (d.view(np.uint32) != want_d.view(np.uint32)).sum()))
    assert np.array_equal(idx, want_i)
    assert np.array_equal(d.view(np.uint32), want_d.view(np.uint32))


# ---- 3. against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nt,r", [(3000, 5000, r) for r in (1, 48, 64, 67, 128)] + [(1000, 20000, 64), (4100, 4100, 128)])
def test_match_against_the_float64_reference(ctx, nq, nt, r):
    check_against_the_reference(ctx, *case(nq, nt, r))


def check_against_the_reference(ctx, Q, T, D, G):
    """match(Q, T) against the reference's distances D and gates G; returns the library's (idx, d)."""
    nq, nt, r = len(Q), len(T), Q.shape[1]
    o3 = top_by_key(D, 3)
    rows = np.arange(nq)[:, None]
    d3, g3 = D[rows, o3], G[rows, o3]
    amb1 = (d3[:, 1] - d3[:, 0] <= g3[:, 0] + g3[:, 1]) & (d3[:, 1] != d3[:, 0])
    amb2 = (d3[:, 2] - d3[:, 1] <= g3[:, 1] + g3[:, 2]) & (d3[:, 2] != d3[:, 1])
    n_amb = int((amb1 | amb2).sum())
    print("match vs reference %d x %d r %d: ambiguous first %d, second %d (%d of %d queries)" % (nq, nt, r, amb1.sum(), amb2.sum(), n_amb, nq))
    assert n_amb <= 0.002 * nq, "the reference calls %d of %d queries ambiguous: the case is unfit" % (n_amb, nq)
    # only now the GPU's answer
    idx, d = ctx.match(Q, T)
    err = np.abs(d.astype(np.float64) - d3[:, :2])
    print("    max err/gate of the two distances %.3f; index mismatches: first %d, second %d"
          % ((err / g3[:, :2]).max(), (idx[:, 0] != o3[:, 0]).sum(), (idx[:, 1] != o3[:, 1]).sum()))
    assert (err <= g3[:, :2]).all()
    ok1, ok2 = ~amb1, ~amb2
    assert np.array_equal(idx[ok1, 0], o3[ok1, 0])
    assert np.array_equal(idx[ok2, 1], o3[ok2, 1])
    # the planted rows: Q[nq-1] = T[3] = T[nt//2] = T[nt-1], the third copy loses on index; Q[nq-2] = T[5]
    assert not amb1[nq - 1] and not amb2[nq - 1] and not amb1[nq - 2]
    assert tuple(idx[nq - 1]) == (3, nt // 2) and d[nq - 1, 0] == d[nq - 1, 1]
    assert idx[nq - 2, 0] == 5
    return idx, d


# ---- 4. independence ----------------------------------------------------------------------------------------------------
def test_match_does_not_depend_on_nq_on_the_order_of_train_or_on_the_run(ctx):
    nq, nt, r = 3000, 5000, 64
    Q, T = make_tables(nq, nt, r)
    idx, d = ctx.match(Q, T)
    for n in (1, 15, 16, 17, 127, 128, 129, 3000):
        i_n, d_n = ctx.match(Q[:n], T)
        assert np.array_equal(i_n, idx[:n]) and np.array_equal(d_n.view(np.uint32), d[:n].view(np.uint32)), n
    # two calls: identical bytes
    i2, d2 = ctx.match(Q, T)
    assert idx.tobytes() == i2.tobytes() and d.tobytes() == d2.tobytes()
    # rows of T permuted: the distances are the same bits; the indices map through the permutation wherever the three
    # smallest returned distances are distinct (ties go to the smaller NEW index)
    perm = np.random.default_rng(7).permutation(nt)        # row p of the new table is row perm[p] of T
    i_p, d_p = ctx.match(Q, T[perm])
    assert np.array_equal(d_p.view(np.uint32), d.view(np.uint32))
    X = ctx.cross_sqdists(Q, T)
    s3 = np.sort(X, axis=1)[:, :3]
    distinct = (s3[:, 0] != s3[:, 1]) & (s3[:, 1] != s3[:, 2])
    assert distinct.sum() >= nq - 2 - 0.002 * nq           # all but the planted queries, give or take a float tie
    assert np.array_equal(perm[i_p[distinct]], idx[distinct])
    # the planted copies: Q[nq-1] equals three train rows, the two smallest new positions win, in order
    inv = np.argsort(perm)
    assert i_p[nq - 1].tolist() == sorted(inv[[3, nt // 2, nt - 1]].tolist())[:2]
    # identical train rows give identical distances to every query wherever they sit
    assert np.array_equal(X[:, 3].view(np.uint32), X[:, nt // 2].view(np.uint32)) and np.array_equal(X[:, 3].view(np.uint32), X[:, nt - 1].view(np.uint32))


def test_match_with_more_queries_than_one_slice_rule(ctx):
    """Few queries against many train rows (many slices, merged) and many queries against few (one slice, direct store)
    are the top two of the same matrix."""
    for nq, nt, r in ((3, 40000, 64), (20000, 300, 48), (130, 129, 200)):
        Q, T = make_tables(nq, nt, r)
        X = ctx.cross_sqdists(Q, T)
        idx, d = ctx.match(Q, T)
        order = top_by_key(X, 2)
        assert np.array_equal(idx, order.astype(np.int32)), (nq, nt, r)
        assert np.array_equal(d.view(np.uint32), X[np.arange(nq)[:, None], order].view(np.uint32)), (nq, nt, r)


# ---- 4b. the loop over blocks of 2^20 queries -------------------------------------------------------------------------------
BLOCK, BASE = 2 ** 20, 1009                                # queries per launch of the host loop; a prime period of repeated queries


def test_match_over_the_query_block_loop(ctx):
    """2^20 + 77 queries are two launches (the first: one slice that holds all six tiles of train, no merge; the second:
    one-tile slices, merged), their results at an offset of 2^20 rows.  The queries repeat a base of 1009 rows: a row's
    answer depends on the row alone (the test above), so row i carries the bits of row i mod 1009 of the base's own match,
    and the base is held against the float64 reference like every other case."""
    nq, nt, r = BLOCK + 77, 700, 4
    Qb, T = make_tables(BASE, nt, r)
    D = ref_dists(Qb, T)
    bi, bd = check_against_the_reference(ctx, Qb, T, D, gate(Qb, T, D))
    rep = np.arange(nq) % BASE
    idx, d = ctx.match(Qb[rep], T)
    bad = np.nonzero((idx != bi[rep]).any(1) | (d.view(np.uint32) != bd[rep].view(np.uint32)).any(1))[0]
    print("match %d x %d r %d: %d rows differ from the base's" % (nq, nt, r, len(bad)))
    assert len(bad) == 0, "rows %s differ; %s" % (bad[:8].tolist(), "; ".join(
        "row %d: got %s / %s, want %s / %s" % (i, idx[i].tolist(), d[i].tolist(), bi[i % BASE].tolist(), bd[i % BASE].tolist())
        for i in (BLOCK - 1, BLOCK, BLOCK + 76)))


def test_cross_sqdists_over_the_query_block_loop(ctx):
    nq, nt, r = BLOCK + 77, 40, 4
    Qb, T = make_tables(BASE, nt, r)
    D = ref_dists(Qb, T)
    Xb = ctx.cross_sqdists(Qb, T)
    assert (np.abs(Xb.astype(np.float64) - D) <= gate(Qb, T, D)).all() and (Xb >= 0).all()
    rep = np.arange(nq) % BASE
    X = ctx.cross_sqdists(Qb[rep], T)
    want = Xb[rep]
    bad = np.nonzero((X.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    print("cross_sqdists %d x %d r %d: %d rows differ from the base's" % (nq, nt, r, len(bad)))
    assert len(bad) == 0, "rows %s differ; rows 2^20 - 1, 2^20, 2^20 + 76 equal: %s" % (
        bad[:8].tolist(), [bool((X[i].view(np.uint32) == want[i].view(np.uint32)).all()) for i in (BLOCK - 1, BLOCK, BLOCK + 76)])


# ---- 4c. the loop over chunks of queries of the host forms ------------------------------------------------------------------
CHUNK_BYTES = 2 ** 28                                      # the library's documented chunk size: query rows, padded to 16 bytes, per upload
WIDE = 1021                                                # the widest rows whose host pitch (1021 floats) and device pitch (1024) differ
CHUNK = CHUNK_BYTES // ((4 * WIDE + 15) // 16 * 16)        # 65 536 rows


def test_match_over_the_query_chunk_loop(ctx):
    """65 536 + 37 queries of 1021 floats are two uploads of the host form, the second read at row 65 536 of the caller's
    table (pitch 1021) into rows of pitch 1024, its results written at an offset of 65 536 rows.  The queries repeat the
    base as in the block-loop test, and the base is held against the float64 reference, planted ties included."""
    nq, nt, r = CHUNK + 37, 40, WIDE
    assert CHUNK == 65536
    Qb, T, D, G = case(BASE, nt, r)
    bi, bd = check_against_the_reference(ctx, Qb, T, D, G)
    rep = np.arange(nq) % BASE
    idx, d = ctx.match(Qb[rep], T)
    bad = np.nonzero((idx != bi[rep]).any(1) | (d.view(np.uint32) != bd[rep].view(np.uint32)).any(1))[0]
    print("match %d x %d r %d: %d rows differ from the base's" % (nq, nt, r, len(bad)))
    assert len(bad) == 0, "rows %s differ; %s" % (bad[:8].tolist(), "; ".join(
        "row %d: got %s / %s, want %s / %s" % (i, idx[i].tolist(), d[i].tolist(), bi[i % BASE].tolist(), bd[i % BASE].tolist())
        for i in (CHUNK - 1, CHUNK, CHUNK + 36)))


def test_cross_sqdists_over_the_query_chunk_loop(ctx):
    nq, nt, r = CHUNK + 37, 40, WIDE
    Qb, T, D, G = case(BASE, nt, r)
    Xb = ctx.cross_sqdists(Qb, T)
    assert (np.abs(Xb.astype(np.float64) - D) <= G).all() and (Xb >= 0).all()
    rep = np.arange(nq) % BASE
    X = ctx.cross_sqdists(Qb[rep], T)
    want = Xb[rep]
    bad = np.nonzero((X.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    print("cross_sqdists %d x %d r %d: %d rows differ from the base's" % (nq, nt, r, len(bad)))
    assert len(bad) == 0, "rows %s differ; rows 65535, 65536, 65572 equal: %s" % (
        bad[:8].tolist(), [bool((X[i].view(np.uint32) == want[i].view(np.uint32)).all()) for i in (CHUNK - 1, CHUNK, CHUNK + 36)])


def test_non_finite_inputs_keep_the_indices_in_range(ctx):
    Q, T = make_tables(200, 300, 64)
    Q[5, 7], Q[9, :] = np.nan, np.inf
    T[17, 3], T[40, :], T[41, 0] = np.nan, -np.inf, 3.0e38
    idx, d = ctx.match(Q, T)
    assert ((idx >= -1) & (idx < 300)).all()
    clean = np.ones(200, bool)
    clean[[5, 9]] = False
    assert (idx[clean] >= 0).all()


# ---- 5. the device form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,ld", [(48, 52), (67, 68)])
def test_match_device_on_tables_written_by_describe_device(dlco, r, ld):
    import torch
    nsel = 60
    patches, _ = pair_set(n_base=30, n_pairs=10, seed=11)                # 120 patches, every fourth an exact repeat
    pq, pt = patches[:70], patches[40:]
    c = dlco.DescContext()
    c.set_filters(make_filters(nsel, seed=nsel))
    c.set_projection(make_w(r, nsel * 8, seed=r))
    Yq, Yt = c.describe(pq), c.describe(pt)
    want_i, want_d = c.match(Yq, Yt)
    sq, st = -7.25, float("nan")                                          # the columns beyond r: never read into a distance, never written
    bq = torch.full((len(pq), ld), sq, dtype=torch.float32, device="cuda:0")
    bt = torch.full((len(pt), ld), st, dtype=torch.float32, device="cuda:0")
    oi = torch.full((len(pq), 2), -5, dtype=torch.int32, device="cuda:0")
    od = torch.full((len(pq), 2), -5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    c.describe_device(pq, bq.data_ptr(), ld=ld)
    c.describe_device(pt, bt.data_ptr(), ld=ld)
    c.match_device(bq.data_ptr(), len(pq), bt.data_ptr(), len(pt), r, oi.data_ptr(), od.data_ptr(), ldq=ld, ldt=ld)
    torch.cuda.synchronize()
    assert c.last_kernel_ms() > 0
    gq, gt = bq.cpu().numpy(), bt.cpu().numpy()
    assert np.array_equal(gq[:, :r], Yq) and np.array_equal(gt[:, :r], Yt)
    assert (gq[:, r:] == np.float32(sq)).all() and np.isnan(gt[:, r:]).all()
    assert np.array_equal(oi.cpu().numpy(), want_i) and np.array_equal(od.cpu().numpy().view(np.uint32), want_d.view(np.uint32))
    assert (want_i[:, 0] >= 0).all() and np.isfinite(want_d).all()
    for bad_q, bad_t in ((ld + 1, ld), (ld, ld + 2), (r - 4, ld), (ld, 4)):
        with pytest.raises(dlco.DlcoError) as ei:
            c.match_device(bq.data_ptr(), len(pq), bt.data_ptr(), len(pt), r, oi.data_ptr(), od.data_ptr(), ldq=bad_q, ldt=bad_t)
        assert ei.value.code == dlco.ERR_INVALID
    c.close()


# ---- 6. the existing surface is untouched -------------------------------------------------------------------------------------
def test_a_match_call_leaves_the_other_calls_alone(dlco):
    patches, pairs = pair_set(n_base=12, n_pairs=200, seed=2)
    c = dlco.DescContext()
    c.set_filters(make_filters(60, seed=60))
    c.set_projection(make_w(48, 480, seed=1))
    before = (c.describe(patches), c.pair_sqdists(patches, pairs), c.compute(patches))
    Y = before[0]
    idx, d = c.match(Y, Y[::-1].copy())
    X = c.cross_sqdists(Y[:20], Y)
    assert idx.shape == (len(Y), 2) and X.shape == (20, len(Y))
    after = (c.describe(patches), c.pair_sqdists(patches, pairs), c.compute(patches))
    assert before[0].tobytes() == after[0].tobytes() and before[2].tobytes() == after[2].tobytes()
    assert before[1][0].tobytes() == after[1][0].tobytes() and before[1][1].tobytes() == after[1][1].tobytes()
    # and the other way round: the same match after them
    i2, d2 = c.match(Y, Y[::-1].copy())
    assert idx.tobytes() == i2.tobytes() and d.tobytes() == d2.tobytes()
    c.close()
