"""GPU tests of the guided batch (dlco_desc_match_pairs_guided*, _epipolar*; the plan: opencv-dlco_amd/csrc/match_batch.hpp):
many (query image, train image) pairs over one segmented table in one call, every pair under a matrix of its own.  Every
comparison is byte equality against a Python loop of ctx.match_guided / ctx.match_guided_epipolar over the pairs, the calls
that tests/test_guided_gpu.py and tests/test_guided_epipolar_gpu.py hold against the masked distance matrix.  No tolerance is
used anywhere.

Geometry: image s of n rows has keypoints uniform in [0, 8 sqrt(n))^2, one per 64 px^2.  For the pair (a, b) and side 0 the
model is case_model(n_b)[0] @ diag(s, s, 1) (or case_F(n_b) @ diag(s, s, 1)) with s = sqrt(n_b / n_a): it maps the square of
image a onto that of image b; for side 1 it is built in the other direction.  Radius 12, threshold 2.  Every case asserts,
from the numpy predicates (pair_mask, epi_mask) alone and before the library's answer is read, that in every pair whose two
images both have 100 rows or more at least 90 % of the queries admit two or more rows.

Side 1 needs sizes of its own.  The radius is measured in the image the model maps TO, which for side 1 is the query image: the
train keypoints arrive there at one per 64 n_a / n_b px^2, so a pair whose train image is much smaller than its query image
admits too few whatever the seed (257 against 127 rows: 0.85 of the queries).  The side-1 cases therefore keep the small sizes
and take their images of 100 rows or more within 10 % of each other, around the same tile and block edges (255, 256, 257)."""
import math

import numpy as np
import pytest

from test_guided_epipolar_rules import THRESHOLD, case_F, epi_mask
from test_guided_rules import RADIUS, case_model, pair_mask
from test_match_gpu import make_tables
from test_match_pairs_gpu import images, same
from test_match_slices import NUMBERS, ceil_div

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
MODELS = ("H", "F")
SIZES = (1, 15, 16, 17, 127, 128, 129, 257, 300)
SIZES_1 = (1, 15, 16, 17, 255, 256, 257, 270, 280)        # side 1 (see above)
BLOCK, BASE = 2 ** 20, 1009


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def coords(sizes, seed=7):
    """the keypoints of every image of a set: uniform in [0, 8 sqrt(n))^2"""
    rng = np.random.default_rng(seed)
    return [(rng.random((n, 2)) * 8.0 * math.sqrt(max(n, 1))).astype(np.float32) for n in sizes]


def model_of(kind, na, nb, side):
    """the matrix of the pair (image of na rows, image of nb rows): side 0 maps a's square onto b's, side 1 b's onto a's"""
    src, dst = (na, nb) if side == 0 else (nb, na)
    if src == 0 or dst == 0:
        return np.eye(3)                                   # an empty image: the matrix is never consulted
    s = math.sqrt(dst / src)
    M = case_model(dst)[0] if kind == "H" else case_F(dst)
    return M @ np.diag([s, s, 1.0])


def models_of(kind, tabs, pairs, side):
    return np.stack([model_of(kind, len(tabs[a]), len(tabs[b]), side) for a, b in pairs])


def mask_of(kind, M, qxy, txy, side):
    return pair_mask(M, qxy, txy, RADIUS, side) if kind == "H" else epi_mask(M, qxy, txy, THRESHOLD, side)


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
    """what the single guided call returns for one pair; an empty train image: the documented fill"""
    if len(Q) == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32)
    if len(T) == 0:
        return np.full((len(Q), 2), -1, np.int32), np.full((len(Q), 2), INF)
    if kind == "H":
        return ctx.match_guided(Q, qxy, T, txy, M, RADIUS, side)
    return ctx.match_guided_epipolar(Q, qxy, T, txy, M, THRESHOLD, side)


def batch(ctx, kind, tabs, xys, pairs, Ms, side):
    if kind == "H":
        return ctx.match_pairs_guided(tabs, xys, pairs, Ms, RADIUS, side)
    return ctx.match_pairs_guided_epipolar(tabs, xys, pairs, Ms, THRESHOLD, side)


def check(ctx, kind, tabs, xys, pairs, Ms, side, got, tag, cache=None):
    cache = {} if cache is None else cache
    bad = []
    for p, (a, b) in enumerate(pairs):
        key = (a, b, Ms[p].tobytes())
        if key not in cache:
            cache[key] = single(ctx, kind, tabs[a], xys[a], tabs[b], xys[b], Ms[p], side)
        if not same(got[p], cache[key]):
            bad.append((p, a, b, int((got[p][0] != cache[key][0]).any(1).sum()) if got[p][0].shape == cache[key][0].shape else -1))
    print("%s: %d pairs, %d differ from the single guided call" % (tag, len(pairs), len(bad)))
    assert not bad, "%s: (pair, a, b, rows with another index) %s" % (tag, bad[:8])
    return cache


# ---- 1. boundaries: every ordered pair of images of 1 .. 300 rows ------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("kind", MODELS)
@pytest.mark.parametrize("r", [3, 64, 129])
def test_all_ordered_pairs_of_small_images(ctx, r, kind, side):
    sizes = SIZES if side == 0 else SIZES_1
    tabs, xys = images("float", sizes, r, nt=sizes[-1]), coords(sizes)
    pairs = [(a, b) for a in range(len(sizes)) for b in range(len(sizes))]
    Ms = models_of(kind, tabs, pairs, side)
    tag = "%s side %d r %d all pairs" % (kind, side, r)
    assert_condition(kind, tabs, xys, pairs, Ms, side, tag)
    got = batch(ctx, kind, tabs, xys, pairs, Ms, side)
    assert len(got) == 81 and ctx.last_kernel_ms() > 0
    check(ctx, kind, tabs, xys, pairs, Ms, side, got, tag)
    for p, (a, b) in enumerate(pairs):
        if sizes[b] == 1:                                  # one train row: no second neighbour
            assert (got[p][0][:, 1] == -1).all() and (got[p][1][:, 1] == INF).all()
        assert got[p][0].shape == (sizes[a], 2) and got[p][0].min() >= -1 and got[p][0].max() < sizes[b]
    assert any((g[0][:, 1] >= 0).mean() >= 0.9 for g in got)       # the models admit: the answers are not all "none"


# ---- 2. entries with one slice and with several in one launch; enough pairs make every entry one slice ---------------------------
@pytest.mark.parametrize("kind", MODELS)
def test_slices_mixed_in_one_launch_and_one_slice_once_the_launch_is_large(ctx, n_cu, kind):
    r, side = 64, 0
    qb, _, _, per_cu = NUMBERS["float"]
    tabs = images("float", (300, 5000, 17), r, nt=5000)    # A, B, C
    seg = np.concatenate([[0], np.cumsum([len(t) for t in tabs])])
    four = [(0, 1), (1, 0), (0, 2), (2, 1)]
    sl = ctx.match_pairs_slices(seg, four)
    print("%s r %d: slices of the four pairs alone %s" % (kind, r, sl.tolist()))
    assert (sl == 1).any() and (sl > 1).any(), "the case is unfit: the plan of the four pairs does not mix one slice and several"
    big = images("float", (1000, 999, 998), r, nt=5000)
    tabs2 = tabs + big
    xys2 = coords([len(t) for t in tabs2], seed=11)
    M4 = models_of(kind, tabs2, four, side)
    assert_condition(kind, tabs2, xys2, four, M4, side, "%s four pairs" % kind)
    alone = batch(ctx, kind, tabs, xys2[:3], four, M4, side)
    cache = check(ctx, kind, tabs, xys2[:3], four, M4, side, alone, "%s r %d four pairs" % (kind, r))
    n_fill = max(300, ceil_div(per_cu * n_cu, ceil_div(998, qb)))     # enough 1000-row pairs that the launch has per_cu * n_cu query blocks
    fillers = [(3 + k % 3, 3 + (k // 3) % 3) for k in range(n_fill)]
    seg2 = np.concatenate([[0], np.cumsum([len(t) for t in tabs2])])
    sl2 = ctx.match_pairs_slices(seg2, fillers + four)
    print("    behind %d pairs of 1000-row images: slices %s" % (n_fill, np.unique(sl2).tolist()))
    assert (sl2 == 1).all()
    Ms = models_of(kind, tabs2, fillers + four, side)
    assert_condition(kind, tabs2, xys2, fillers[:9], Ms[:9], side, "%s fillers" % kind)
    got = batch(ctx, kind, tabs2, xys2, fillers + four, Ms, side)
    check(ctx, kind, tabs2, xys2, four, M4, side, got[n_fill:], "%s r %d four pairs behind %d" % (kind, r, n_fill), cache)
    for p in range(4):
        assert same(got[n_fill + p], alone[p])
    check(ctx, kind, tabs2, xys2, fillers[:9], Ms[:9], side, got[:9], "%s r %d the first fillers" % (kind, r))


# ---- 3. "no model" and empty images ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("kind", MODELS)
def test_no_model_and_empty_images_between_modelled_pairs(ctx, kind, side):
    r = 64
    sizes = (129, 0, 300, 0, 17) if side == 0 else (280, 0, 300, 0, 17)
    tabs, xys = images("float", sizes, r), coords(sizes)
    pairs = [(0, 2), (1, 2), (2, 0), (0, 1), (2, 2), (3, 1), (4, 3), (2, 4), (0, 2), (1, 0), (4, 2)]
    Ms = models_of(kind, tabs, pairs, side)
    zero = (2, 4, 8)                                       # "no model" between modelled pairs; pair 8 repeats pair 0 without a model
    Ms[list(zero)] = 0.0
    assert_condition(kind, tabs, xys, pairs, Ms, side, "%s side %d no model" % (kind, side))
    got = batch(ctx, kind, tabs, xys, pairs, Ms, side)
    for p, (a, b) in enumerate(pairs):
        assert got[p][0].shape == (sizes[a], 2)
        if sizes[b] == 0 or p in zero:
            assert (got[p][0] == -1).all() and (got[p][1] == INF).all()
    assert (got[0][0][:, 0] >= 0).any()
    check(ctx, kind, tabs, xys, pairs, Ms, side, got, "%s side %d no model and empty images" % (kind, side))
    # the other pairs' bytes do not move when those pairs leave the batch
    keep = [p for p, (a, b) in enumerate(pairs) if sizes[a] and sizes[b] and p not in zero]
    got2 = batch(ctx, kind, tabs, xys, [pairs[p] for p in keep], Ms[keep], side)
    for k, p in enumerate(keep):
        assert same(got2[k], got[p])
    # a batch in which every pair is "no model" launches no tile loop and still fills
    got3 = batch(ctx, kind, tabs, xys, [(0, 2), (1, 2), (2, 0)], np.zeros((3, 9)), side)
    assert got3[1][0].shape == (0, 2) and all((g[0] == -1).all() and (g[1] == INF).all() for g in got3)
    assert got3[0][0].shape == (sizes[0], 2) and got3[2][0].shape == (300, 2)


# ---- 4. independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("kind", MODELS)
def test_a_pair_depends_on_nothing_but_its_two_images_and_its_matrix(ctx, kind, side):
    r = 67
    sizes = (300, 129, 2000, 17, 700) if side == 0 else (1900, 1850, 2000, 17, 1950)
    tabs, xys = images("float", sizes, r, nt=2000), coords(sizes, seed=13)
    rng = np.random.default_rng(5)
    pairs = [(a, b) for a in range(5) for b in range(5)] + [(2, 2), (0, 2)]
    Ms = models_of(kind, tabs, pairs, side)
    # the last pair repeats (0, 2) under ANOTHER matrix, 20 px to the side: records kept per image would serve one of the two wrongly
    Ms[-1] = np.array([[1.0, 0.0, 20.0], [0.0, 1.0, -20.0], [0.0, 0.0, 1.0]]) @ Ms[-1] if kind == "H" else case_F(sizes[2] if side == 0 else sizes[0]).T
    assert_condition(kind, tabs, xys, pairs[:-1], Ms[:-1], side, "%s side %d independence" % (kind, side))
    got = batch(ctx, kind, tabs, xys, pairs, Ms, side)
    cache = check(ctx, kind, tabs, xys, pairs, Ms, side, got, "%s side %d independence" % (kind, side))
    assert not same(got[-1], got[2]), "the two matrices of (0, 2) give the same answer: the case shows nothing"
    again = batch(ctx, kind, tabs, xys, pairs, Ms, side)
    assert all(same(x, y) for x, y in zip(got, again))                            # the run
    order = rng.permutation(len(pairs))
    shuffled = batch(ctx, kind, tabs, xys, [pairs[k] for k in order], Ms[order], side)
    assert all(same(shuffled[j], got[k]) for j, k in enumerate(order))            # the order
    sub = [pairs[k] for k in order[:5]]
    assert all(same(x, got[k]) for x, k in zip(batch(ctx, kind, tabs, xys, sub, Ms[order[:5]], side), order[:5]))     # the other pairs
    # a batch of one pair is the single call; a small batch after a large one meets no stale plan, partials or records
    for p in (25, 26, 19):
        assert same(batch(ctx, kind, tabs, xys, [pairs[p]], Ms[p:p + 1], side)[0], got[p])
    assert same(batch(ctx, kind, tabs[:2], xys[:2], [(1, 0)], Ms[5:6], side)[0], cache[(1, 0, Ms[5].tobytes())])


# ---- 5. planted rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MODELS)
def test_planted_rows_in_a_300_row_image(ctx, kind):
    """a query with W < 0 (under the homography; a far point under F), a NaN coordinate, and the tied descriptor rows of make_tables"""
    r, side = 64, 0
    sizes = (300, 257, 129)
    tabs, xys = images("float", sizes, r), coords(sizes, seed=17)
    S = 8.0 * math.sqrt(300)
    xys[0][1] = (-60.0 * S, 0.0)
    xys[0][2, 1] = np.nan
    xys[0][150], xys[0][299] = xys[0][3] + np.float32([1.0, 0.0]), xys[0][3] + np.float32([0.0, 1.0])   # the tied rows 3, 150, 299: neighbours
    pairs = [(0, 1), (1, 0), (0, 0), (2, 0), (0, 2)]
    Ms = models_of(kind, tabs, pairs, side)
    assert_condition(kind, tabs, xys, pairs, Ms, side, "%s planted" % kind)
    m = mask_of(kind, Ms[0], xys[0], xys[1], side)
    assert not m[2].any() and (kind == "F" or not m[1].any())
    Q, T = make_tables(300, 300, r)
    assert np.array_equal(tabs[0], T) and len(np.unique(T, axis=0)) < len(T), "the image of 300 rows has no tied descriptor rows"
    got = batch(ctx, kind, tabs, xys, pairs, Ms, side)
    assert (got[0][0][2] == -1).all() and (got[0][1][2] == INF).all()
    check(ctx, kind, tabs, xys, pairs, Ms, side, got, "%s planted rows" % kind)


# ---- 6. a predicate that admits everything gives the plain batch ---------------------------------------------------------------
def test_identity_and_a_huge_radius_equal_the_plain_batch(ctx):
    r = 64
    sizes = (300, 129, 17, 1)
    tabs = images("float", sizes, r)
    rng = np.random.default_rng(3)
    xys = [(rng.random((n, 2)) * (2.0 ** 20 - 1)).astype(np.float32) for n in sizes]
    assert all(x.max() < 2.0 ** 20 for x in xys)
    pairs = [(a, b) for a in range(4) for b in range(4)]
    plain = ctx.match_pairs(tabs, pairs)
    for side in (0, 1):
        got = ctx.match_pairs_guided(tabs, xys, pairs, np.tile(np.eye(3).reshape(1, 9), (len(pairs), 1)), 2.0 ** 21, side)
        assert all(same(x, y) for x, y in zip(got, plain)), side


# ---- 7. the device forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MODELS)
@pytest.mark.parametrize("r,side", [(67, 0), (128, 1)])
def test_device_forms_with_pitches_and_garbage(ctx, dlco, kind, r, side):
    """ld > r with garbage between r and ld, ldxy = 4 with garbage in columns 2 and 3, garbage rows between the images"""
    import torch
    sizes = (150, 333, 17) if side == 0 else (310, 333, 17)
    tabs, xys = images("float", sizes, r, nt=333), coords(sizes, seed=19)
    rng = np.random.default_rng(r)
    ld = (r + 3) // 4 * 4 + 4
    junk = lambda n, w: (rng.standard_normal((n, w)) * 100).astype(np.float32)
    blocks, kps, seg = [], [], [0]
    for t, x in zip(tabs, xys):                            # image, 5 rows of garbage, image, ...
        g, k = junk(len(t), ld), junk(len(t), 4)
        g[:, :r], k[:, :2] = t, x
        blocks += [g, junk(5, ld)]
        kps += [k, junk(5, 4)]
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
    od = torch.full((int(row0[-1]) + 3, 2), -5, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    call = ctx.match_pairs_guided_device if kind == "H" else ctx.match_pairs_guided_epipolar_device
    t = RADIUS if kind == "H" else THRESHOLD
    call(dev.data_ptr(), dkp.data_ptr(), seg, pairs, r, Ms, oi.data_ptr(), od.data_ptr(), t, side, ld=ld, ldxy=4)
    torch.cuda.synchronize()
    assert ctx.last_kernel_ms() > 0
    gi, gd = oi.cpu().numpy(), od.cpu().numpy()
    for p in range(len(pairs)):
        assert same((gi[row0[p]:row0[p + 1]], gd[row0[p]:row0[p + 1]]), want[p]), (kind, r, pairs[p])
    assert (gi[row0[-1]:] == -5).all() and (gd[row0[-1]:] == -5).all()              # nothing written behind the last pair
    assert np.array_equal(dev.cpu().numpy(), table) and dkp.cpu().numpy().tobytes() == kp.tobytes()      # only read
    for bad in (dict(ld=ld + 2), dict(ld=r // 4 * 4 - 4), dict(ld=-4), dict(ldxy=1), dict(ldxy=0), dict(ldxy=-4)):
        with pytest.raises(dlco.DlcoError) as ei:
            call(dev.data_ptr(), dkp.data_ptr(), seg, pairs, r, Ms, oi.data_ptr(), od.data_ptr(), t, side, **{**dict(ld=ld, ldxy=4), **bad})
        assert ei.value.code == dlco.ERR_INVALID, bad
    assert np.array_equal(oi.cpu().numpy(), gi)


# ---- 8. a pair of more than 2^20 query rows is cut: the record offsets of its ranges -------------------------------------------
@pytest.mark.parametrize("kind", MODELS)
def test_a_pair_of_more_than_a_launch_of_queries_between_two_small_pairs(ctx, kind):
    """2^20 + 77 queries against 40 train rows, r = 16.  Descriptors and coordinates repeat a base of 1009 rows: a row's answer
    depends on the row alone, so row i carries the bits of row i mod 1009 of one single call on the base."""
    nq, nt, r, side = BLOCK + 77, 40, 16, 0
    base, T = make_tables(BASE, nt, r)
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
    bad = np.nonzero((idx != bi[rep]).any(1) | (d.view(np.uint32) != bd[rep].view(np.uint32)).any(1))[0]
    print("match_pairs_guided %s %d x %d r %d: %d rows differ from the base's" % (kind, nq, nt, r, len(bad)))
    assert idx.shape == (nq, 2) and len(bad) == 0, "rows %s differ" % bad[:8].tolist()


# ---- 9. the kernel time ------------------------------------------------------------------------------------------------------
def test_last_kernel_ms_covers_the_call(ctx):
    sizes = (300, 17, 0)
    tabs, xys = images("float", sizes, 64), coords(sizes)
    pairs = [(0, 1), (1, 0), (0, 2)]
    for kind in MODELS:
        for side in (0, 1):
            batch(ctx, kind, tabs, xys, pairs, models_of(kind, tabs, pairs, side), side)
            assert ctx.last_kernel_ms() > 0
