"""GPU tests of the guided batch on byte tables (dlco_desc_match_pairs_guided_u8*, _epipolar_u8*), in the structure of
tests/test_match_pairs_guided_gpu.py: many (query image, train image) pairs over one segmented byte table in one call, every
pair under a matrix of its own.  Every comparison is byte equality against a Python loop of ctx.match_guided_u8 /
ctx.match_guided_epipolar_u8 over the pairs, the calls that tests/test_guided_u8_gpu.py holds against the masked integer matrix.

Geometry: that of the float file (coords, model_of): image s of n rows has keypoints uniform in [0, 8 sqrt(n))^2 and the matrix
of a pair maps the square of one image onto that of the other.  Side 0 runs at radius 12 / threshold 2.  Side 1 measures the
radius in the query image, where the train keypoints of the pair (a, b) arrive at one per 64 n_a / n_b px^2: among the images of
100 rows or more (127 .. 300) that is down to 0.42 of the density of side 0, so side 1 runs at radius 20 and threshold 4, which
gives back (20 / 12)^2 = 2.8 in area and 2 in band width.  Every case asserts, from the numpy predicates alone and before the
library's answer is read, that in every pair whose two images both have 100 rows or more at least 90 % of the queries admit two
or more rows."""
import numpy as np
import pytest

from test_guided_epipolar_rules import epi_mask
from test_guided_rules import pair_mask
from test_match_pairs_gpu import images, same
from test_match_pairs_guided_gpu import coords, model_of, models_of
from test_match_u8_gpu import byte_tables

pytestmark = pytest.mark.gpu

I32MAX = 2 ** 31 - 1
MODELS = ("H", "F")
SIZES = (1, 15, 16, 17, 127, 128, 129, 257, 300)
BLOCK, BASE = 2 ** 20, 1009
BOUND = {("H", 0): 12.0, ("F", 0): 2.0, ("H", 1): 20.0, ("F", 1): 4.0}


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


def mask_of(kind, M, qxy, txy, side):
    return pair_mask(M, qxy, txy, BOUND[kind, side], side) if kind == "H" else epi_mask(M, qxy, txy, BOUND[kind, side], side)


def assert_condition(kind, tabs, xys, pairs, Ms, side, tag):
    """at least 90 % of the queries of every pair of two images of >= 100 rows admit two or more rows, by numpy alone"""
    seen, low = set(), 1.0
    for (a, b), M in zip(pairs, Ms):
        key = (a, b, M.tobytes())
        if key in seen or len(tabs[a]) < 100 or len(tabs[b]) < 100 or not M.any():
            continue
        seen.add(key)
        share = (mask_of(kind, M, xys[a], xys[b], side).sum(1) >= 2).mean()
        low = min(low, share)
        assert share >= 0.9, "%s: the case is unfit: %.3f of the queries of pair (%d, %d) admit two or more" % (tag, share, a, b)
    print("%s: %d pairs of two images of >= 100 rows, lowest share of queries that admit two or more %.3f" % (tag, len(seen), low))


def single(ctx, kind, Q, qxy, T, txy, M, side):
    """what the single byte guided call returns for one pair; an empty train image: the documented fill"""
    if len(Q) == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32)
    if len(T) == 0:
        return np.full((len(Q), 2), -1, np.int32), np.full((len(Q), 2), I32MAX, np.int32)
    return (ctx.match_guided_u8 if kind == "H" else ctx.match_guided_epipolar_u8)(Q, qxy, T, txy, M, BOUND[kind, side], side)


def batch(ctx, kind, tabs, xys, pairs, Ms, side):
    return (ctx.match_pairs_guided_u8 if kind == "H" else ctx.match_pairs_guided_epipolar_u8)(tabs, xys, pairs, Ms, BOUND[kind, side], side)


def check(ctx, kind, tabs, xys, pairs, Ms, side, got, tag, cache=None):
    cache = {} if cache is None else cache
    bad = []
    for p, (a, b) in enumerate(pairs):
        key = (a, b, Ms[p].tobytes())
        if key not in cache:
            cache[key] = single(ctx, kind, tabs[a], xys[a], tabs[b], xys[b], Ms[p], side)
        if not same(got[p], cache[key]):
            bad.append((p, a, b, int((got[p][0] != cache[key][0]).any(1).sum()) if got[p][0].shape == cache[key][0].shape else -1))
    print("%s: %d pairs, %d differ from the single byte guided call" % (tag, len(pairs), len(bad)))
    assert not bad, "%s: (pair, a, b, rows with another index) %s" % (tag, bad[:8])
    return cache


# ---- 1. boundaries: every ordered pair of images of 1 .. 300 rows ------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("kind", MODELS)
@pytest.mark.parametrize("r", [64, 129])
def test_all_ordered_pairs_of_small_images(ctx, r, kind, side):
    tabs, xys = images("u8", SIZES, r, nt=SIZES[-1]), coords(SIZES)
    pairs = [(a, b) for a in range(len(SIZES)) for b in range(len(SIZES))]
    Ms = models_of(kind, tabs, pairs, side)
    tag = "%s side %d r %d all pairs" % (kind, side, r)
    assert_condition(kind, tabs, xys, pairs, Ms, side, tag)
    got = batch(ctx, kind, tabs, xys, pairs, Ms, side)
    assert len(got) == 81 and ctx.last_kernel_ms() > 0
    check(ctx, kind, tabs, xys, pairs, Ms, side, got, tag)
    for p, (a, b) in enumerate(pairs):
        if SIZES[b] == 1:                                  # one train row: no second neighbour
            assert (got[p][0][:, 1] == -1).all() and (got[p][1][:, 1] == I32MAX).all()
        assert got[p][0].shape == (SIZES[a], 2) and got[p][0].min() >= -1 and got[p][0].max() < SIZES[b]
        m = mask_of(kind, Ms[p], xys[a], xys[b], side).sum(1)
        assert ((got[p][0][:, 0] == -1) == (m == 0)).all() and ((got[p][0][:, 1] == -1) == (m <= 1)).all()
    assert any((g[0][:, 1] >= 0).mean() >= 0.9 for g in got)       # the models admit: the answers are not all "none"


# ---- 2. entries with one slice and with several in one launch ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", MODELS)
@pytest.mark.parametrize("r", [64, 200])
def test_slices_of_different_counts_mixed_in_one_launch(ctx, kind, r):
    side = 0
    tabs = images("u8", (300, 5000, 17), r, nt=5000)       # A, B, C
    xys = coords([len(t) for t in tabs], seed=11)
    seg = np.concatenate([[0], np.cumsum([len(t) for t in tabs])])
    four = [(0, 1), (1, 0), (0, 2), (2, 1)]
    sl = ctx.match_pairs_slices(seg, four, u8=True)
    print("%s r %d: slices of the four pairs %s" % (kind, r, sl.tolist()))
    assert (sl == 1).any() and (sl > 1).any() and len(set(sl.tolist())) >= 3, "the case is unfit: the plan does not mix slice counts"
    Ms = models_of(kind, tabs, four, side)
    assert_condition(kind, tabs, xys, four, Ms, side, "%s four pairs" % kind)
    got = batch(ctx, kind, tabs, xys, four, Ms, side)
    check(ctx, kind, tabs, xys, four, Ms, side, got, "%s r %d four pairs" % (kind, r))


# ---- 3. "no model" and empty images; a pair's rows do not move when the other pairs change -----------------------------------------
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("kind", MODELS)
def test_no_model_and_empty_images_between_modelled_pairs(ctx, kind, side):
    r = 64
    sizes = (129, 0, 300, 0, 17)
    tabs, xys = images("u8", sizes, r), coords(sizes)
    pairs = [(0, 2), (1, 2), (2, 0), (0, 1), (2, 2), (3, 1), (4, 3), (2, 4), (0, 2), (1, 0), (4, 2)]
    Ms = models_of(kind, tabs, pairs, side)
    zero = (2, 4, 8)                                       # "no model" between modelled pairs; pair 8 repeats pair 0 without a model
    Ms[list(zero)] = 0.0
    assert_condition(kind, tabs, xys, pairs, Ms, side, "%s side %d no model" % (kind, side))
    got = batch(ctx, kind, tabs, xys, pairs, Ms, side)
    for p, (a, b) in enumerate(pairs):
        assert got[p][0].shape == (sizes[a], 2) and got[p][1].dtype == np.int32
        if sizes[b] == 0 or p in zero:
            assert (got[p][0] == -1).all() and (got[p][1] == I32MAX).all()
    assert (got[0][0][:, 0] >= 0).any()
    check(ctx, kind, tabs, xys, pairs, Ms, side, got, "%s side %d no model and empty images" % (kind, side))
    # the other pairs' bytes do not move when those pairs leave the batch, when the order changes, or on a second run
    keep = [p for p, (a, b) in enumerate(pairs) if sizes[a] and sizes[b] and p not in zero]
    got2 = batch(ctx, kind, tabs, xys, [pairs[p] for p in keep], Ms[keep], side)
    for k, p in enumerate(keep):
        assert same(got2[k], got[p])
    order = np.random.default_rng(5).permutation(len(pairs))
    shuffled = batch(ctx, kind, tabs, xys, [pairs[k] for k in order], Ms[order], side)
    assert all(same(shuffled[j], got[k]) for j, k in enumerate(order))
    # a batch in which every pair is "no model" launches no tile loop and still fills
    got3 = batch(ctx, kind, tabs, xys, [(0, 2), (1, 2), (2, 0)], np.zeros((3, 9)), side)
    assert got3[1][0].shape == (0, 2) and all((g[0] == -1).all() and (g[1] == I32MAX).all() for g in got3)
    assert got3[0][0].shape == (sizes[0], 2) and got3[2][0].shape == (300, 2)


# ---- 4. the same image under another matrix in the same batch -------------------------------------------------------------------
@pytest.mark.parametrize("kind", MODELS)
def test_a_pair_depends_on_its_own_matrix(ctx, kind):
    r, side = 67, 0
    sizes = (300, 129, 2000)
    tabs, xys = images("u8", sizes, r, nt=2000), coords(sizes, seed=13)
    pairs = [(0, 2), (1, 2), (2, 0), (0, 2)]
    Ms = models_of(kind, tabs, pairs, side)
    # the last pair repeats (0, 2) under ANOTHER matrix: records kept per image would serve one of the two wrongly
    Ms[-1] = np.array([[1.0, 0.0, 20.0], [0.0, 1.0, -20.0], [0.0, 0.0, 1.0]]) @ Ms[-1] if kind == "H" else model_of("F", 300, 2000, 0).T
    assert_condition(kind, tabs, xys, pairs[:-1], Ms[:-1], side, "%s own matrix" % kind)
    got = batch(ctx, kind, tabs, xys, pairs, Ms, side)
    check(ctx, kind, tabs, xys, pairs, Ms, side, got, "%s own matrix" % kind)
    assert not same(got[-1], got[0]), "the two matrices of (0, 2) give the same answer: the case shows nothing"
    assert same(batch(ctx, kind, tabs, xys, [pairs[3]], Ms[3:4], side)[0], got[3])          # a batch of one pair after a larger one


# ---- 5. a predicate that admits everything gives the plain byte batch -----------------------------------------------------------
def test_identity_and_a_huge_radius_equal_the_plain_byte_batch(ctx):
    r = 64
    sizes = (300, 129, 17, 1)
    tabs = images("u8", sizes, r)
    rng = np.random.default_rng(3)
    xys = [(rng.random((n, 2)) * (2.0 ** 20 - 1)).astype(np.float32) for n in sizes]
    pairs = [(a, b) for a in range(4) for b in range(4)]
    plain = ctx.match_pairs_u8(tabs, pairs)
    for side in (0, 1):
        got = ctx.match_pairs_guided_u8(tabs, xys, pairs, np.tile(np.eye(3).reshape(1, 9), (len(pairs), 1)), 2.0 ** 21, side)
        assert all(same(x, y) for x, y in zip(got, plain)), side


# ---- 6. the device forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MODELS)
@pytest.mark.parametrize("r,side", [(67, 0), (128, 1)])
def test_device_forms_with_pitches_and_garbage(ctx, dlco, kind, r, side):
    """ld > r with garbage between r and ld, ldxy = 4 with NaN in columns 2 and 3, garbage rows between the images"""
    import torch
    sizes = (300, 333, 17)
    tabs, xys = images("u8", sizes, r, nt=333), coords(sizes, seed=19)
    rng = np.random.default_rng(r)
    ld = (r + 15) // 16 * 16 + 16
    junk = lambda n: rng.integers(0, 256, (n, ld), dtype=np.uint8)
    blocks, kps, seg = [], [], [0]
    for t, x in zip(tabs, xys):                            # image, 5 rows of garbage, image, ...
        g, k = junk(len(t)), np.full((len(t), 4), np.nan, np.float32)
        g[:, :r], k[:, :2] = t, x
        blocks += [g, junk(5)]
        kps += [k, np.full((5, 4), np.nan, np.float32)]
        seg += [seg[-1] + len(t), seg[-1] + len(t) + 5]
    table, kp = np.ascontiguousarray(np.concatenate(blocks)), np.ascontiguousarray(np.concatenate(kps))
    pairs = [(0, 2), (2, 0), (4, 2), (2, 2), (0, 4)]       # images 1, 3, 5 are the garbage
    real = {0: 0, 2: 1, 4: 2}
    rp = [(real[a], real[b]) for a, b in pairs]
    Ms = models_of(kind, tabs, rp, side)
    assert_condition(kind, tabs, xys, rp, Ms, side, "%s side %d device" % (kind, side))
    want = [single(ctx, kind, tabs[a], xys[a], tabs[b], xys[b], M, side) for (a, b), M in zip(rp, Ms)]
    row0 = dlco.match_pairs_rows(seg, pairs)
    dev, dkp = torch.from_numpy(table).to("cuda:0"), torch.from_numpy(kp).to("cuda:0")
    oi = torch.full((int(row0[-1]) + 3, 2), -5, dtype=torch.int32, device="cuda:0")
    od = torch.full((int(row0[-1]) + 3, 2), -5, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    call = ctx.match_pairs_guided_u8_device if kind == "H" else ctx.match_pairs_guided_epipolar_u8_device
    t = BOUND[kind, side]
    call(dev.data_ptr(), dkp.data_ptr(), seg, pairs, r, Ms, oi.data_ptr(), od.data_ptr(), t, side, ld=ld, ldxy=4)
    torch.cuda.synchronize()
    assert ctx.last_kernel_ms() > 0
    gi, gd = oi.cpu().numpy(), od.cpu().numpy()
    for p in range(len(pairs)):
        assert same((gi[row0[p]:row0[p + 1]], gd[row0[p]:row0[p + 1]]), want[p]), (kind, r, pairs[p])
    assert (gi[row0[-1]:] == -5).all() and (gd[row0[-1]:] == -5).all()              # nothing written behind the last pair
    assert np.array_equal(dev.cpu().numpy(), table) and dkp.cpu().numpy().tobytes() == kp.tobytes()      # only read
    for bad in (dict(ld=ld + 8), dict(ld=r // 16 * 16 - 16), dict(ld=-16), dict(ldxy=1), dict(ldxy=0), dict(ldxy=-4)):
        with pytest.raises(dlco.DlcoError) as ei:
            call(dev.data_ptr(), dkp.data_ptr(), seg, pairs, r, Ms, oi.data_ptr(), od.data_ptr(), t, side, **{**dict(ld=ld, ldxy=4), **bad})
        assert ei.value.code == dlco.ERR_INVALID, bad
    assert np.array_equal(oi.cpu().numpy(), gi) and np.array_equal(od.cpu().numpy(), gd)


# ---- 7. a pair of more than 2^20 query rows is cut: the record offsets of its ranges -------------------------------------------
@pytest.mark.parametrize("kind", MODELS)
def test_a_pair_of_more_than_a_launch_of_queries_between_two_small_pairs(ctx, kind):
    """2^20 + 77 queries against 40 train rows, r = 16.  Descriptors and coordinates repeat a base of 1009 rows: a row's answer
    depends on the row alone, so row i carries the answer of row i mod 1009 of one single call on the base."""
    nq, nt, r, side = BLOCK + 77, 40, 16, 0
    base, T = byte_tables(BASE, nt, r)
    bxy, txy = coords((BASE, nt), seed=23)
    rep = np.arange(nq) % BASE
    tabs, xys = [base[:50], base[rep], T], [bxy[:50], bxy[rep], txy]
    pairs = [(0, 2), (1, 2), (2, 0)]
    M = model_of(kind, BASE, nt, side)                     # the base's square onto train's
    Ms = np.stack([M, M, model_of(kind, nt, BASE, side)])
    assert mask_of(kind, M, bxy, txy, side).any(1).mean() > 0.5
    bi, bd = single(ctx, kind, base, bxy, T, txy, M, side)
    got = batch(ctx, kind, tabs, xys, pairs, Ms, side)
    assert same(got[0], (bi[:50], bd[:50])) and same(got[2], single(ctx, kind, T, txy, base[:50], bxy[:50], Ms[2], side))
    idx, d = got[1]
    bad = np.nonzero((idx != bi[rep]).any(1) | (d != bd[rep]).any(1))[0]
    print("match_pairs_guided_u8 %s %d x %d r %d: %d rows differ from the base's" % (kind, nq, nt, r, len(bad)))
    assert idx.shape == (nq, 2) and len(bad) == 0, "rows %s differ" % bad[:8].tolist()


# ---- 8. the kernel time ------------------------------------------------------------------------------------------------------
def test_last_kernel_ms_covers_the_call(ctx):
    sizes = (300, 17, 0)
    tabs, xys = images("u8", sizes, 64), coords(sizes)
    pairs = [(0, 1), (1, 0), (0, 2)]
    for kind in MODELS:
        for side in (0, 1):
            batch(ctx, kind, tabs, xys, pairs, models_of(kind, tabs, pairs, side), side)
            assert ctx.last_kernel_ms() > 0
