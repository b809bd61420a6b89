"""The byte matcher where it was written to work: slices of several tiles (both LDS buffers, the hand-over between them, a
train-row decode with tile > 0, a ragged last tile behind whole ones: cases b and d), the chunks of r > 128 interleaved with those tiles,
every level of the merge under ties, one slice that holds all tiles, and the host loops over blocks of 2^20 queries and
over the chunks in which the queries go up.  The
small shapes of test_match_u8_gpu.py never leave one tile per slice (tests/test_match_slices.py pins that).

Which regime a shape reaches depends on the device's CU count, so the shapes are picked with the restated rule of
test_match_slices.py from a short fixed list, and a case whose regime no candidate reaches FAILS: a skip would hide it.

Reference.  All distances are integers <= 1024 * 255^2 < 2^27, so |q|^2 + |t|^2 - 2 Q T' in float64 is exact (every
partial sum is an integer below 2^53); on 64 sampled query rows it is compared with the direct form ((q - t)^2).sum() in
int64 before anything touches the GPU.  The top two under (distance, index) are the two smallest keys D * nt + index,
which are unique.  Every comparison with the GPU is equality: no tolerance, no ambiguous set, nothing excluded."""
import numpy as np
import pytest

from test_match_slices import slices, tiles_per_slice

pytestmark = pytest.mark.gpu

TILE = 128
BLOCK = 2 ** 20                                               # queries per launch of the host loop
BASE = 1009                                                   # prime: the period of the repeated queries aligns with no block, wave or tile


# ---- the reference ------------------------------------------------------------------------------------------------------
def ref_matrix(Q, T):
    """[nq, nt] int64 of the exact squared distances, checked against the direct form on 64 sampled query rows."""
    Q64, T64 = Q.astype(np.float64), T.astype(np.float64)
    D = ((Q64 * Q64).sum(1)[:, None] + (T64 * T64).sum(1)[None, :] - 2.0 * (Q64 @ T64.T)).astype(np.int64)
    rows = np.unique(np.linspace(0, len(Q) - 1, 64).astype(np.int64))
    T_i = T.astype(np.int64)
    for i in rows:                                        # a row at a time: the difference of all 64 at once is 0.6 GB at r = 200
        d = T_i - Q[i].astype(np.int64)[None, :]
        assert np.array_equal(D[i], (d * d).sum(1)), "the float64 reference differs from the direct form in query row %d" % i
    return D


def ref_top2(D):
    """(idx [nq, 2] int32, dist [nq, 2] int32) under the (distance, index) order; nt >= 2."""
    nt = D.shape[1]
    assert nt >= 2 and int(D.max()) * nt + nt < 2 ** 58
    K = D * nt + np.arange(nt, dtype=np.int64)
    two = np.partition(K, 1, axis=1)[:, :2]
    return (two % nt).astype(np.int32), (two // nt).astype(np.int32)


def report(tag, got_i, got_d, want_i, want_d, rows=()):
    bad = np.nonzero((got_i != want_i).any(1) | (got_d != want_d).any(1))[0]
    msg = "%s: %d of %d rows differ, the first at %s" % (tag, len(bad), len(want_i), bad[:8].tolist())
    for i in list(bad[:3]) + list(rows):
        msg += "\n    row %d: got %s / %s, want %s / %s" % (i, got_i[i].tolist(), got_d[i].tolist(), want_i[i].tolist(), want_d[i].tolist())
    return msg


# ---- shapes by regime ---------------------------------------------------------------------------------------------------
# nq in {2048, 4096, 8192, 16384}, nt = 128 k + 60 (a ragged last tile of 60 rows).  Where the test forms the matrix,
# nq * nt <= 2^26; where it runs match_u8 alone on repeated queries (case b), the reference is BASE x nt.
MATRIX_SHAPES = [(4096, 6204), (8192, 6204), (2048, 6204), (8192, 8124), (16384, 4028), (2048, 16444)]
DEEP_SHAPES = [(16384, 8252), (16384, 16444), (8192, 8252), (8192, 16444)]


DEVICE = 0                                                    # the context's device, and the one whose CU count picks the shapes


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(DEVICE).multi_processor_count     # hipDeviceProp_t::multiProcessorCount, what the library reads


def pick(candidates, n_cu, min_tps, tag, min_last=1):
    """The first candidate whose slices hold at least min_tps tiles and are merged (more than one slice), and whose last
    slice holds at least min_last tiles: at 2 or more the ragged tile of 60 rows comes behind a whole one in its slice."""
    assert all(nt % TILE == 60 for _, nt in candidates)
    for nq, nt in candidates:
        tps = tiles_per_slice(nq, nt, n_cu, "u8")
        s = slices(nt, tps, "u8")
        last = (nt + TILE - 1) // TILE - (s - 1) * tps
        if tps >= min_tps and s > 1 and last >= min_last:
            print("%s: %d CUs, %d x %d: %d tiles per slice, %d slices, %d in the last" % (tag, n_cu, nq, nt, tps, s, last))
            return nq, nt, tps, s
    pytest.fail("the case is unfit: no candidate shape gives %d tiles per slice, a merge and %d tiles in the last slice at %d CUs (%s)"
                % (min_tps, min_last, n_cu, tag))


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext(device=DEVICE)                   # no filters, no projection: matching needs neither
    yield c
    c.close()


# ---- a. the matrix and the top two at two or more tiles per slice, merged ---------------------------------------------------
@pytest.mark.parametrize("r", [1, 64, 128, 129, 200])
def test_several_tiles_per_slice_and_a_merge(ctx, n_cu, r):
    """r <= 128: one chunk per tile; 129 and 200: two chunks interleaved with the tiles of a slice."""
    nq, nt, tps, _ = pick(MATRIX_SHAPES, n_cu, 2, "tiles a, r %d" % r)
    assert nq * nt <= 2 ** 26
    rng = np.random.default_rng(9000 + r)
    Q = rng.integers(0, 256, (nq, r), dtype=np.uint8)
    T = rng.integers(0, 256, (nt, r), dtype=np.uint8)
    j255 = tps * TILE + TILE + 37                         # in the second tile of the second slice
    assert j255 < nt and (j255 // TILE) % tps == 1
    Q[nq // 2], T[j255] = 0, 255
    D = ref_matrix(Q, T)
    assert D[nq // 2, j255] == r * 255 * 255              # the largest possible distance is met there
    want_i, want_d = ref_top2(D)
    X = ctx.cross_sqdists_u8(Q, T)
    assert X.shape == (nq, nt) and X.dtype == np.int32
    bad = np.argwhere(X != D)
    print("    cross_sqdists_u8: %d of %d entries differ" % (len(bad), X.size))
    assert np.array_equal(X, D), "entries (query, train) %s differ; train tiles %s" % (bad[:8].tolist(), np.unique(bad[:, 1] // TILE)[:16].tolist())
    idx, d = ctx.match_u8(Q, T)
    assert idx.dtype == np.int32 and d.dtype == np.int32
    print("    match_u8: %d index and %d distance mismatches" % ((idx != want_i).sum(), (d != want_d).sum()))
    assert np.array_equal(idx, want_i) and np.array_equal(d, want_d), report("match_u8", idx, d, want_i, want_d)


# ---- b. four or more tiles per slice ------------------------------------------------------------------------------------------
def test_four_or_more_tiles_per_slice(ctx, n_cu):
    """match_u8 alone (the matrix would be 135 M entries); the queries repeat a base of BASE distinct rows."""
    r = 64
    nq, nt, tps, _ = pick(DEEP_SHAPES, n_cu, 4, "tiles b", min_last=2)    # the ragged tile is not the first of its slice
    rng = np.random.default_rng(9100)
    base = rng.integers(0, 256, (BASE, r), dtype=np.uint8)
    T = rng.integers(0, 256, (nt, r), dtype=np.uint8)
    base[BASE // 2], T[(tps - 1) * TILE + 77] = 0, 255    # the last tile of the first slice
    D = ref_matrix(base, T)
    assert D[BASE // 2, (tps - 1) * TILE + 77] == r * 255 * 255
    bi, bd = ref_top2(D)
    rep = np.arange(nq) % BASE
    idx, d = ctx.match_u8(base[rep], T)
    print("    match_u8: %d index and %d distance mismatches" % ((idx != bi[rep]).sum(), (d != bd[rep]).sum()))
    assert np.array_equal(idx, bi[rep]) and np.array_equal(d, bd[rep]), report("match_u8", idx, d, bi[rep], bd[rep])


# ---- c. ties across every level of the merge ----------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [3, 64])
def test_ties_across_every_merge_level(ctx, n_cu, r):
    """Bytes below 4: ties are the rule.  Then exact copies of one train row in two lane groups of one MFMA, in another
    16-row block, in the next tile of the slice, in the next slice and in the last row of the table, and a query equal to it:
    distance 0 twice at the two smallest positions; the smallest copy is removed in turn so that every level decides once."""
    nq, nt, tps, _ = pick(MATRIX_SHAPES, n_cu, 2, "tiles c, r %d" % r)
    rng = np.random.default_rng(9200 + r)
    Q = rng.integers(0, 4, (nq, r), dtype=np.uint8)
    T = rng.integers(0, 4, (nt, r), dtype=np.uint8)
    row = rng.integers(0, 4, r, dtype=np.uint8)
    clash = (T == row).all(1)
    T[clash, 0] = (T[clash, 0] + 1) % 4                   # no train row equals the planted one by chance (at r = 3 many would)
    j = tps * TILE + 3                                    # the first tile of the second slice
    planted = [j, j + 4, j + 16, j + TILE, j + tps * TILE, nt - 1]
    assert planted == sorted(set(planted)) and (j + TILE) // (tps * TILE) == j // (tps * TILE) != (j + tps * TILE) // (tps * TILE)
    original = T[planted].copy()
    T[planted] = row
    qi = nq - 5
    Q[qi] = row
    D = ref_matrix(Q, T)
    s3 = np.partition(D, 2, axis=1)[:, :3]
    s3.sort(axis=1)
    tied = ((s3[:, 0] == s3[:, 1]) | (s3[:, 1] == s3[:, 2])).mean()
    print("    %.3f of the queries have an exact tie among their first three distances" % tied)
    assert tied >= 0.05, "the case is unfit: ties are rare"
    for level in range(len(planted) - 1):
        want_i, want_d = ref_top2(D)
        assert want_i[qi].tolist() == planted[level:level + 2] and want_d[qi].tolist() == [0, 0]
        idx, d = ctx.match_u8(Q, T)
        print("    copies at %s: %d index and %d distance mismatches" % (planted[level:], (idx != want_i).sum(), (d != want_d).sum()))
        assert np.array_equal(idx, want_i) and np.array_equal(d, want_d), report("copies at %s" % planted[level:], idx, d, want_i, want_d, [qi])
        if level == 0:
            assert np.array_equal(ctx.cross_sqdists_u8(Q, T), D)
        # the smallest copy gets its own row back: one column of the reference changes
        p = planted[level]
        T[p] = original[level]
        dq = Q.astype(np.int64) - T[p].astype(np.int64)[None, :]
        D[:, p] = (dq * dq).sum(1)


# ---- d. one slice that holds all tiles, and the loop over blocks of 2^20 queries --------------------------------------------
def block_case(nt, r=16):
    rng = np.random.default_rng(9300 + nt)
    base = rng.integers(0, 256, (BASE, r), dtype=np.uint8)
    T = rng.integers(0, 256, (nt, r), dtype=np.uint8)
    base[BASE // 2], T[nt - 3] = 0, 255
    D = ref_matrix(base, T)
    assert D[BASE // 2, nt - 3] == r * 255 * 255
    return base, T, D


def test_one_slice_of_all_tiles_and_the_query_block_loop(ctx, n_cu):
    nq, nt = BLOCK + 77, 700
    tps = tiles_per_slice(BLOCK, nt, n_cu, "u8")
    s = slices(nt, tps, "u8")
    tps2 = tiles_per_slice(nq - BLOCK, nt, n_cu, "u8")
    print("tiles d: %d CUs, %d x %d: first launch %d tiles per slice, %d slice; second launch of %d queries %d tiles per slice, %d slices"
          % (n_cu, nq, nt, tps, s, nq - BLOCK, tps2, slices(nt, tps2, "u8")))
    if (tps, s) != (6, 1):
        pytest.fail("the case is unfit: 2^20 queries against %d rows are not one slice of six tiles at %d CUs" % (nt, n_cu))
    base, T, D = block_case(nt)
    bi, bd = ref_top2(D)
    rep = np.arange(nq) % BASE
    idx, d = ctx.match_u8(base[rep], T)
    print("    match_u8: %d index and %d distance mismatches" % ((idx != bi[rep]).sum(), (d != bd[rep]).sum()))
    assert np.array_equal(idx, bi[rep]) and np.array_equal(d, bd[rep]), report("match_u8", idx, d, bi[rep], bd[rep], [BLOCK - 1, BLOCK, BLOCK + 76])


def test_cross_sqdists_u8_over_the_query_block_loop(ctx):
    nq, nt = BLOCK + 77, 40
    base, T, D = block_case(nt)
    rep = np.arange(nq) % BASE
    X = ctx.cross_sqdists_u8(base[rep], T)
    want = D.astype(np.int32)[rep]
    bad = np.nonzero((X != want).any(1))[0]
    print("cross_sqdists_u8 %d x %d: %d rows differ" % (nq, nt, len(bad)))
    assert np.array_equal(X, want), "rows %s differ; row 2^20 - 1: %s, row 2^20: %s, row 2^20 + 76: %s" % (
        bad[:8].tolist(), (X[BLOCK - 1] == want[BLOCK - 1]).all(), (X[BLOCK] == want[BLOCK]).all(), (X[BLOCK + 76] == want[BLOCK + 76]).all())


# ---- e. the loop over chunks of queries of the host forms -----------------------------------------------------------------
CHUNK_BYTES = 2 ** 28                                         # the library's documented chunk size: query rows, padded to 16 bytes, per upload
WIDE = 1021                                                   # the widest rows whose host pitch (1021 bytes) and device pitch (1024) differ
CHUNK = CHUNK_BYTES // ((WIDE + 15) // 16 * 16)               # 262 144 rows


def test_match_u8_over_the_query_chunk_loop(ctx):
    """262 144 + 37 queries of 1021 bytes are two uploads: the second is read at row 262 144 of the caller's table (pitch
    1021) into rows of pitch 1024, and its results land at an offset of 262 144 rows.  Three tiles of train, the last ragged."""
    nq, nt = CHUNK + 37, 300
    assert CHUNK == 262144
    base, T, D = block_case(nt, WIDE)
    bi, bd = ref_top2(D)
    rep = np.arange(nq) % BASE
    idx, d = ctx.match_u8(base[rep], T)
    print("    match_u8: %d index and %d distance mismatches" % ((idx != bi[rep]).sum(), (d != bd[rep]).sum()))
    assert np.array_equal(idx, bi[rep]) and np.array_equal(d, bd[rep]), report("match_u8", idx, d, bi[rep], bd[rep], [CHUNK - 1, CHUNK, CHUNK + 36])


def test_cross_sqdists_u8_over_the_query_chunk_loop(ctx):
    nq, nt = CHUNK + 37, 40
    base, T, D = block_case(nt, WIDE)
    rep = np.arange(nq) % BASE
    X = ctx.cross_sqdists_u8(base[rep], T)
    want = D.astype(np.int32)[rep]
    bad = np.nonzero((X != want).any(1))[0]
    print("cross_sqdists_u8 %d x %d: %d rows differ" % (nq, nt, len(bad)))
    assert np.array_equal(X, want), "rows %s differ; row 262143: %s, row 262144: %s, row 262180: %s" % (
        bad[:8].tolist(), (X[CHUNK - 1] == want[CHUNK - 1]).all(), (X[CHUNK] == want[CHUNK]).all(), (X[CHUNK + 36] == want[CHUNK + 36]).all())
