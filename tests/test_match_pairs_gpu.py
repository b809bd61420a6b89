"""GPU tests of the batched matcher (dlco_desc_match_pairs*, the plan: opencv-dlco_amd/csrc/match_batch.hpp): many (query
image, train image) pairs over one segmented table in one call.  Every comparison is byte equality against a Python loop of
ctx.match(Q_a, T_b) / ctx.match_u8 over the pairs, the calls that tests/test_match_gpu.py and tests/test_match_u8*_gpu.py hold
against float64 and the integer reference.  No tolerance is used anywhere."""
import numpy as np
import pytest

from test_match_gpu import make_tables
from test_match_slices import NUMBERS, ceil_div
from test_match_u8_gpu import byte_tables

pytestmark = pytest.mark.gpu

INF, I32MAX = np.float32(np.inf), np.int32(2 ** 31 - 1)
LINES = ("float", "u8")
SIZES = (1, 15, 16, 17, 127, 128, 129, 257, 300)
BLOCK, BASE = 2 ** 20, 1009


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()                                # no filters, no projection: matching needs neither
    yield c
    c.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def images(line, sizes, r, nt=300):
    """Images that share structure, so that planted ties and near neighbours fall inside images and across them: the image
    of nt rows is the train table of make_tables / byte_tables, every other one the query table drawn against it (half of
    its rows noisy views of train rows, planted copies; bytes below 4 at small r, where ties are the rule)."""
    out = []
    for n in sizes:
        if n == 0:
            out.append(np.zeros((0, r), np.float32 if line == "float" else np.uint8))
        elif line == "float":
            Q, T = make_tables(max(n, 2), nt, r)
            out.append(T if n == nt else Q[:n])
        else:
            Q, T = byte_tables(max(n, 2), nt, r, 4 if r in (1, 3, 64) else 256)
            out.append(T if n == nt else Q[:n])
    return out


def single(ctx, line, Q, T):
    """what the plain call returns for one pair; an empty train image: the documented fill"""
    if len(Q) == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32 if line == "float" else np.int32)
    if len(T) == 0:
        return np.full((len(Q), 2), -1, np.int32), np.full((len(Q), 2), INF if line == "float" else I32MAX)
    return ctx.match(Q, T) if line == "float" else ctx.match_u8(Q, T)


def batch(ctx, line, tabs, pairs):
    return ctx.match_pairs(tabs, pairs) if line == "float" else ctx.match_pairs_u8(tabs, pairs)


def same(got, want):
    return got[0].dtype == want[0].dtype and got[1].dtype == want[1].dtype and got[0].shape == want[0].shape and \
        got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def check(ctx, line, tabs, pairs, got, tag, cache=None):
    cache = {} if cache is None else cache
    bad = []
    for p, (a, b) in enumerate(pairs):
        if (a, b) not in cache:
            cache[(a, b)] = single(ctx, line, tabs[a], tabs[b])
        if not same(got[p], cache[(a, b)]):
            bad.append((p, a, b, int((got[p][0] != cache[(a, b)][0]).any(1).sum()) if got[p][0].shape == cache[(a, b)][0].shape else -1))
    print("%s: %d pairs, %d differ from the plain call" % (tag, len(pairs), len(bad)))
    assert not bad, "%s: (pair, a, b, rows with another index) %s" % (tag, bad[:8])
    return cache


# ---- 1. boundaries: every ordered pair of images of 1 .. 300 rows ------------------------------------------------------------
@pytest.mark.parametrize("line", LINES)
@pytest.mark.parametrize("r", [1, 3, 64, 67, 128, 129, 200])
def test_all_ordered_pairs_of_small_images(ctx, dlco, line, r):
    tabs = images(line, SIZES, r)
    pairs = [(a, b) for a in range(len(SIZES)) for b in range(len(SIZES))]
    got = batch(ctx, line, tabs, pairs)
    assert len(got) == 81 and ctx.last_kernel_ms() > 0
    seg = np.concatenate([[0], np.cumsum(SIZES)])
    assert np.array_equal(dlco.match_pairs_rows(seg, pairs), np.concatenate([[0], np.cumsum([SIZES[a] for a, _ in pairs])]))
    check(ctx, line, tabs, pairs, got, "%s r %d all pairs" % (line, r))
    for p, (a, b) in enumerate(pairs):
        if SIZES[b] == 1:                                  # one train row: no second neighbour
            assert (got[p][0][:, 1] == -1).all() and (got[p][1][:, 1] == (INF if line == "float" else I32MAX)).all()
        assert got[p][0].min() >= -1 and got[p][0].max() < SIZES[b]


# ---- 2. entries with one slice and with several in one launch; enough pairs make every entry one slice ---------------------------
@pytest.mark.parametrize("line", LINES)
@pytest.mark.parametrize("r", [64, 200])
def test_slices_mixed_in_one_launch_and_one_slice_once_the_launch_is_large(ctx, n_cu, line, r):
    qb, _, _, per_cu = NUMBERS[line]
    tabs = images(line, (300, 5000, 17), r, nt=5000)       # A, B, C
    seg = np.concatenate([[0], np.cumsum([len(t) for t in tabs])])
    four = [(0, 1), (1, 0), (0, 2), (2, 1)]
    sl = ctx.match_pairs_slices(seg, four, u8=(line == "u8"))
    print("%s r %d at %d CUs: slices of the four pairs alone %s" % (line, r, n_cu, sl.tolist()))
    assert (sl == 1).any() and (sl > 1).any(), "the case is unfit: the plan of the four pairs does not mix one slice and several"
    alone = batch(ctx, line, tabs, four)
    cache = check(ctx, line, tabs, four, alone, "%s r %d four pairs" % (line, r))
    # the same four pairs behind enough pairs of 1000-row images that the launch has per_cu * n_cu query blocks: about 300 on the
    # float line at 256 CUs, more on the byte line, whose workgroups take 256 queries and of which a CU wants 16
    big = images(line, (1000, 999, 998), r, nt=5000)
    n_fill = max(300, ceil_div(per_cu * n_cu, ceil_div(998, qb)))
    tabs2 = tabs + big
    fillers = [(3 + k % 3, 3 + (k // 3) % 3) for k in range(n_fill)]
    seg2 = np.concatenate([[0], np.cumsum([len(t) for t in tabs2])])
    sl2 = ctx.match_pairs_slices(seg2, fillers + four, u8=(line == "u8"))
    print("    behind %d pairs of 1000-row images: slices %s" % (n_fill, np.unique(sl2).tolist()))
    assert (sl2 == 1).all()
    got = batch(ctx, line, tabs2, fillers + four)
    check(ctx, line, tabs2, four, got[n_fill:], "%s r %d four pairs behind %d" % (line, r, n_fill), cache)
    for p in range(4):
        assert same(got[n_fill + p], alone[p])
    check(ctx, line, tabs2, fillers[:9], got[:9], "%s r %d the first fillers" % (line, r))


# ---- 3. empty images ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line", LINES)
def test_empty_images_as_query_as_train_and_as_both(ctx, line):
    r = 64
    tabs = images(line, (129, 0, 300, 0, 17), r)
    pairs = [(0, 2), (1, 2), (2, 0), (0, 1), (3, 1), (4, 3), (2, 4), (1, 0), (4, 2)]
    got = batch(ctx, line, tabs, pairs)
    none = INF if line == "float" else I32MAX
    for p, (a, b) in enumerate(pairs):
        assert got[p][0].shape == (len(tabs[a]), 2)
        if len(tabs[b]) == 0:
            assert (got[p][0] == -1).all() and (got[p][1] == none).all()
    check(ctx, line, tabs, pairs, got, "%s empty images" % line)
    # the other rows do not move when the empty images leave the batch
    keep = [p for p, (a, b) in enumerate(pairs) if len(tabs[a]) and len(tabs[b])]
    got2 = batch(ctx, line, tabs, [pairs[p] for p in keep])
    for k, p in enumerate(keep):
        assert same(got2[k], got[p])
    # a batch in which nothing is launched at all
    got3 = batch(ctx, line, tabs, [(1, 3), (0, 1), (3, 0)])
    assert got3[0][0].shape == (0, 2) and got3[2][0].shape == (0, 2) and (got3[1][0] == -1).all() and (got3[1][1] == none).all()


# ---- 4. independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line", LINES)
def test_a_pair_depends_on_nothing_but_its_two_images(ctx, line):
    r = 67
    tabs = images(line, (300, 129, 2000, 17, 700), r, nt=2000)
    rng = np.random.default_rng(5)
    pairs = [(a, b) for a in range(5) for b in range(5)] + [(2, 2), (0, 2)]        # self pairs and repeated pairs
    got = batch(ctx, line, tabs, pairs)
    cache = check(ctx, line, tabs, pairs, got, "%s independence" % line)
    again = batch(ctx, line, tabs, pairs)
    assert all(same(x, y) for x, y in zip(got, again))                            # the run
    order = rng.permutation(len(pairs))
    shuffled = batch(ctx, line, tabs, [pairs[k] for k in order])
    assert all(same(shuffled[j], got[k]) for j, k in enumerate(order))            # the order
    sub = [pairs[k] for k in order[:5]]
    assert all(same(x, got[k]) for x, k in zip(batch(ctx, line, tabs, sub), order[:5]))     # the other pairs
    # a batch of one pair is the plain call; a small batch after a large one meets no stale plan or partials
    for a, b in ((2, 2), (0, 2), (3, 4)):
        assert same(batch(ctx, line, tabs, [(a, b)])[0], cache[(a, b)])
    assert same(batch(ctx, line, tabs[:2], [(1, 0)])[0], cache[(1, 0)])


# ---- 5. the device forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line", LINES)
@pytest.mark.parametrize("r", [67, 128])
def test_device_forms_with_a_pitch_and_garbage(ctx, dlco, line, r):
    """ld > r with garbage between r and ld, and garbage rows behind the last row of each image (images that no pair names)"""
    import torch
    tabs = images(line, (150, 333, 17), r, nt=333)
    rng = np.random.default_rng(r)
    unit = 4 if line == "float" else 16
    ld = (r + unit - 1) // unit * unit + unit
    dt = np.float32 if line == "float" else np.uint8
    junk = lambda n, w: (rng.standard_normal((n, w)) * 100).astype(np.float32) if line == "float" else rng.integers(0, 256, (n, w), dtype=np.uint8)
    blocks, seg = [], [0]
    for t in tabs:                                         # image, 5 rows of garbage, image, ...
        g = junk(len(t), ld)
        g[:, :r] = t
        blocks += [g, junk(5, ld)]
        seg += [seg[-1] + len(t), seg[-1] + len(t) + 5]
    table = np.ascontiguousarray(np.concatenate(blocks).astype(dt))
    pairs = [(0, 2), (2, 0), (4, 2), (2, 2), (0, 4)]       # images 1, 3, 5 are the garbage
    real = {0: 0, 2: 1, 4: 2}
    want = [single(ctx, line, tabs[real[a]], tabs[real[b]]) for a, b in pairs]
    row0 = dlco.match_pairs_rows(seg, pairs)
    dev = torch.from_numpy(table).to("cuda:0")
    oi = torch.full((int(row0[-1]) + 3, 2), -5, dtype=torch.int32, device="cuda:0")
    od = torch.full((int(row0[-1]) + 3, 2), -5, dtype=torch.float32 if line == "float" else torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    call = ctx.match_pairs_device if line == "float" else ctx.match_pairs_u8_device
    call(dev.data_ptr(), seg, pairs, r, oi.data_ptr(), od.data_ptr(), ld=ld)
    torch.cuda.synchronize()
    assert ctx.last_kernel_ms() > 0
    gi, gd = oi.cpu().numpy(), od.cpu().numpy()
    for p in range(len(pairs)):
        assert same((gi[row0[p]:row0[p + 1]], gd[row0[p]:row0[p + 1]]), want[p]), (line, r, pairs[p])
    assert (gi[row0[-1]:] == -5).all() and (gd[row0[-1]:] == -5).all()              # nothing written behind the last pair
    assert np.array_equal(dev.cpu().numpy(), table)                               # the table is only read
    for bad in (ld + unit // 2, r // unit * unit - unit, 0):
        with pytest.raises(dlco.DlcoError) as ei:
            call(dev.data_ptr(), seg, pairs, r, oi.data_ptr(), od.data_ptr(), ld=bad or -unit)
        assert ei.value.code == dlco.ERR_INVALID


# ---- 6. a pair of more than 2^20 query rows is cut into launches ----------------------------------------------------------------
@pytest.mark.parametrize("line", LINES)
def test_a_pair_of_more_than_a_launch_of_queries_between_two_small_pairs(ctx, line):
    """2^20 + 77 queries against 40 train rows, r = 16.  The queries repeat a base of 1009 rows, as the block-loop tests of the
    plain matchers build theirs: a row's answer depends on the row alone, so row i carries the bits of row i mod 1009."""
    nq, nt, r = BLOCK + 77, 40, 16
    if line == "float":
        base, T = make_tables(BASE, nt, r)
    else:
        rng = np.random.default_rng(9300 + nt)
        base, T = rng.integers(0, 256, (BASE, r), dtype=np.uint8), rng.integers(0, 256, (nt, r), dtype=np.uint8)
        base[BASE // 2], T[nt - 3] = 0, 255
    rep = np.arange(nq) % BASE
    small = base[:50]
    tabs = [small, base[rep], T]
    pairs = [(0, 2), (1, 2), (2, 0)]
    bi, bd = single(ctx, line, base, T)
    got = batch(ctx, line, tabs, pairs)
    assert same(got[0], single(ctx, line, small, T)) and same(got[2], single(ctx, line, T, small))
    idx, d = got[1]
    bad = np.nonzero((idx != bi[rep]).any(1) | (d.view(np.uint32) != bd[rep].view(np.uint32)).any(1))[0]
    print("match_pairs %s %d x %d r %d: %d rows differ from the base's" % (line, nq, nt, r, len(bad)))
    assert idx.shape == (nq, 2) and len(bad) == 0, "rows %s differ" % bad[:8].tolist()


# ---- 7. the kernel time ------------------------------------------------------------------------------------------------------
def test_last_kernel_ms_covers_the_call(ctx):
    tabs = images("float", (300, 17, 0), 64)
    ctx.match_pairs(tabs, [(0, 1), (1, 0), (0, 2)])
    assert ctx.last_kernel_ms() > 0
    ctx.match_pairs_u8(images("u8", (300, 17), 64), [(0, 1)])
    assert ctx.last_kernel_ms() > 0
