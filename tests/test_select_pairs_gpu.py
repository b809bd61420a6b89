"""GPU tests of match selection (dlco_desc_select_pairs*, the rule: opencv-dlco_amd/csrc/select_rules.hpp): from the answer of a
batched match to the segmented match list of a batched verification.  The reference is the numpy restatement of the rule in
tests/test_select_rules.py, never the call itself.  Every comparison is byte equality with dtype and shape, and the entries of
the lists beyond M must still hold the poison they were filled with.  Nothing here holds an index outside its train image:
that is tested on the CPU."""
import ctypes as C

import numpy as np
import pytest

from test_select_rules import COUNTS, DIST, I32MAX, INF, LINES, NONE, PAIRS, REVERSE, SETTINGS, SIZES, coordinates, reference, row0_of, synthetic

pytestmark = pytest.mark.gpu

f32p, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
POISON = -7


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()                                # no filters, no projection: selection needs neither
    yield c
    c.close()


@pytest.fixture(scope="module")
def synth():
    s = {line: synthetic(line) for line in LINES}
    for line in LINES:
        for a in s[line]:
            a[0].setflags(write=False)
            a[1].setflags(write=False)
    return s


@pytest.fixture(scope="module")
def constants(dlco):
    """kBlockRows and kScanChunk as csrc/select_rules.hpp states them"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(dlco.LIB_PATH), "csrc", "select_rules.hpp")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) for name in ("kBlockRows", "kScanChunk"))


def seg_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def stacked(answers, line):
    """the answers of all pairs as the two tables of the C call, with a row of padding so that an empty table has an address"""
    idx = np.ascontiguousarray(np.concatenate([a[0] for a in answers] + [np.zeros((1, 2), np.int32)]))
    d = np.ascontiguousarray(np.concatenate([a[1] for a in answers] + [np.zeros((1, 2), DIST[line])]))
    return idx, d


def p_(a, t):
    return None if a is None else a.ctypes.data_as(t)


def trimmed(moff, lists):
    M = int(moff[-1])
    for a in lists:
        assert (a[M:] == POISON).all(), "entries beyond M were written"
    return [moff] + [a[:M] for a in lists]


def host_call(dlco, ctx, line, sizes, pairs, idx, d, ratio=None, back_idx=None, back_row0=None, n_back=0, xy=None):
    """the host form of the C call; idx / d [R + 1, 2]; back_idx True: idx itself"""
    seg, q = seg_of(sizes), np.ascontiguousarray(pairs, np.int32)
    R, dp = len(idx) - 1, f32p if line == "float" else i32p
    moff, m, dd = np.full(len(q) + 1, POISON, np.int64), np.full((R + 1, 2), POISON, np.int32), np.full(R + 1, POISON, DIST[line])
    src = dst = None
    if xy is not None:
        src, dst = np.full((R + 1, 2), POISON, np.float32), np.full((R + 1, 2), POISON, np.float32)
    call = dlco.load().dlco_desc_select_pairs if line == "float" else dlco.load().dlco_desc_select_pairs_u8
    rc = call(ctx.h, p_(seg, i64p), len(sizes), p_(q, i32p), len(q), p_(idx, i32p), p_(d, dp), 0.0 if ratio is None else ratio,
              p_(idx if back_idx is True else back_idx, i32p), p_(back_row0, i64p), n_back, p_(xy, f32p), p_(moff, i64p), p_(m, i32p), p_(dd, dp),
              p_(src, f32p), p_(dst, f32p))
    assert rc == 0, rc
    return trimmed(moff, [m, dd] + ([] if xy is None else [src, dst]))


def device_call(ctx, line, sizes, pairs, idx, d, ratio=None, back_idx=None, back_row0=None, n_back=0, xy=None, ldxy=2):
    """the device form through the DescContext method, torch tensors for the device pointers"""
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    full = lambda shape, t: torch.full(shape, POISON, dtype=t, device="cuda:0")
    R, td = len(idx) - 1, torch.float32 if line == "float" else torch.int32
    ti, tdist = dev(idx), dev(d)
    tb = None if back_idx is None else ti if back_idx is True else dev(back_idx)
    m, dd = full((R + 1, 2), torch.int32), full((R + 1,), td)
    txy = src = dst = None
    if xy is not None:
        txy, src, dst = dev(xy), full((R + 1, 2), torch.float32), full((R + 1, 2), torch.float32)
    torch.cuda.synchronize()
    call = ctx.select_pairs_device if line == "float" else ctx.select_pairs_u8_device
    ptr = lambda t: None if t is None else t.data_ptr()
    moff = call(ti.data_ptr(), tdist.data_ptr(), seg_of(sizes), pairs, m.data_ptr(), dd.data_ptr(), ratio=ratio, back_idx_ptr=ptr(tb), back_row0=back_row0,
                n_back_rows=n_back, xy_ptr=ptr(txy), ldxy=ldxy, src_ptr=ptr(src), dst_ptr=ptr(dst))
    torch.cuda.synchronize()
    return trimmed(moff, [t.cpu().numpy() for t in ([m, dd] + ([] if xy is None else [src, dst]))])


def same(got, want, tag=""):
    assert len(got) == len(want), tag
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (tag, k)


def pitched(xy2, ld):
    xy = np.full((len(xy2), ld), -3, np.float32)
    xy[:, :2] = xy2
    return xy


@pytest.mark.parametrize("line", LINES)
def test_synthetic_set(dlco, ctx, synth, line):
    ans = synth[line]
    R = sum(SIZES[a] for a, _ in PAIRS)
    idx, d = stacked(ans, line)
    xys = coordinates(SIZES)
    xy2 = np.ascontiguousarray(np.concatenate(xys + [np.zeros((1, 2), np.float32)]))
    row0 = row0_of(SIZES, PAIRS)
    backs = [ans[q][0] for q in REVERSE]
    second = np.ascontiguousarray(np.concatenate(backs + [np.zeros((1, 2), np.int32)]))
    second_row0 = np.concatenate([[0], np.cumsum([len(b) for b in backs])])[:-1].astype(np.int64)
    select = ctx.select_pairs if line == "float" else ctx.select_pairs_u8
    for ratio, mutual in SETTINGS:
        want = reference(ans, ratio, backs if mutual else None, xys, PAIRS)
        M = int(want[0][-1])
        print("%s ratio %s mutual %s: M = %d of R = %d" % (line, ratio, mutual, M, R))
        assert M == COUNTS[ratio][1 if mutual else 0] and 0 < M < R
        forms = [(True, row0[REVERSE], R), (second, second_row0, len(second) - 1)] if mutual else [(None, None, 0)]
        for bidx, brow0, nback in forms:
            tag = (line, ratio, mutual, bidx is True)
            same(host_call(dlco, ctx, line, SIZES, PAIRS, idx, d, ratio, bidx, brow0, nback, xy2), want, tag + ("host", 2))
            same(host_call(dlco, ctx, line, SIZES, PAIRS, idx, d, ratio, bidx, brow0, nback), want[:3], tag + ("host", None))
            same(device_call(ctx, line, SIZES, PAIRS, idx, d, ratio, bidx, brow0, nback, xy2, 2), want, tag + ("device", 2))
            same(device_call(ctx, line, SIZES, PAIRS, idx, d, ratio, bidx, brow0, nback, pitched(xy2, 4), 4), want, tag + ("device", 4))
            same(device_call(ctx, line, SIZES, PAIRS, idx, d, ratio, bidx, brow0, nback), want[:3], tag + ("device", None))
        # the DescContext methods on the lists match_pairs returns: back as pair indices of the same batch, or as a second list
        moff = want[0]
        for back in ([REVERSE, [(b, None) for b in backs]] if mutual else [None]):
            sel, lists = select(ans, SIZES, PAIRS, ratio, back, xys)
            assert len(sel) == len(lists) == len(PAIRS)
            for p in range(len(PAIRS)):
                same(list(sel[p]) + list(lists[p]), [w[moff[p]:moff[p + 1]] for w in want[1:]], (line, ratio, mutual, p))
            sel = select(ans, seg_of(SIZES), PAIRS, ratio, back)
            assert all(len(s) == 2 for s in sel) and sum(len(s[0]) for s in sel) == M
    assert ctx.last_kernel_ms() > 0


def planted(line, n, nt, keep):
    """the answer of one pair of n rows against nt train rows that keeps exactly the rows of the mask `keep` under ratio 0.8"""
    i = np.arange(n)
    idx = np.stack([np.where(keep, i % nt, -1), np.where(keep, (i + 1) % nt if nt > 1 else -1, -1)], 1).astype(np.int32)
    d = np.stack([np.where(keep, 1 + i % 5, float(NONE[line])), np.where(keep, 100 + i % 7, float(NONE[line]))], 1).astype(DIST[line])
    return idx, d


PATTERNS = {"all": lambda i: i >= 0, "none": lambda i: i < 0, "alternate": lambda i: i % 2 == 0, "lane 63": lambda i: i % 64 == 63,
            "row 0": lambda i: i == 0, "last row": lambda i: i == i[-1]}


@pytest.mark.parametrize("line", LINES)
def test_planted_patterns(dlco, ctx, constants, line):
    block = constants[0]
    assert block == 256
    for n in (1, 63, 64, 65, 255, 256, 257, 2 * block + 1):
        sizes, pairs = (n, 7), [(0, 1)]
        xys = coordinates(sizes, seed=n)
        xy2 = np.ascontiguousarray(np.concatenate(xys))
        for name in ("all", "none", "alternate", "lane 63", "row 0"):
            keep = PATTERNS[name](np.arange(n))
            ans = [planted(line, n, 7, keep)]
            want = reference(ans, 0.8, None, xys, pairs)
            assert want[0][-1] == keep.sum() and np.array_equal(want[1][:, 0], np.flatnonzero(keep))
            idx, d = stacked(ans, line)
            same(host_call(dlco, ctx, line, sizes, pairs, idx, d, 0.8, xy=xy2), want, (line, n, name, "host"))
            same(device_call(ctx, line, sizes, pairs, idx, d, 0.8, xy=pitched(xy2, 4), ldxy=4), want, (line, n, name, "device"))
    # a batch whose first, middle and last pairs are empty: moff repeats values at both ends
    sizes = (0, 70, 0, 300)
    pairs = [(0, 1), (2, 3), (1, 3), (0, 0), (2, 1), (3, 1), (1, 0), (0, 3), (2, 2)]
    ans = [planted(line, sizes[a], max(sizes[b], 1), (np.arange(sizes[a]) % 3 != 1) & (sizes[b] > 0)) for a, b in pairs]
    want = reference(ans, 0.8)
    assert want[0].tolist() == [0, 0, 0, 47, 47, 47, 247, 247, 247, 247]
    idx, d = stacked(ans, line)
    same(host_call(dlco, ctx, line, sizes, pairs, idx, d, 0.8), want, (line, "empty pairs", "host"))
    same(device_call(ctx, line, sizes, pairs, idx, d, 0.8), want, (line, "empty pairs", "device"))
    # every query image empty: no row at all, and nothing is launched
    moff = host_call(dlco, ctx, line, (0, 5), [(0, 1), (0, 0)], *stacked([planted(line, 0, 5, np.zeros(0, bool))] * 2, line), 0.8)[0]
    assert moff.tolist() == [0, 0, 0]


@pytest.mark.parametrize("line", LINES)
def test_rows_beyond_one_chunk_of_the_scan(dlco, ctx, constants, line):
    block, chunk = constants
    R = 3 * chunk * block + 1
    n0 = R // 4 + 1000
    sizes, pairs = (n0, R - 3 * n0), [(0, 1), (0, 0), (1, 0), (0, 1)]
    assert sum(sizes[a] for a, _ in pairs) == R and min(sizes) > 0
    xys = coordinates(sizes, seed=5)
    xy2 = np.ascontiguousarray(np.concatenate(xys))
    g0 = row0_of(sizes, pairs)
    for name in ("alternate", "last row"):
        g = np.arange(R)
        keep = PATTERNS[name](g)
        ans = [planted(line, sizes[a], sizes[b], keep[g0[p]:g0[p + 1]]) for p, (a, b) in enumerate(pairs)]
        want = reference(ans, 0.8, None, xys, pairs)
        assert want[0][-1] == keep.sum() and 0 < want[0][-1] < R
        idx, d = stacked(ans, line)
        if name == "alternate":
            same(device_call(ctx, line, sizes, pairs, idx, d, 0.8, xy=xy2), want, (line, name))
        else:
            same(host_call(dlco, ctx, line, sizes, pairs, idx, d, 0.8, xy=xy2), want, (line, name))


def test_ratio_boundary_on_the_device(dlco, ctx):
    """the rows of test_match_rules.py::test_ratio_rule_at_the_boundary: what a float product in place of the double one, or a
    comparison that is not strict, would get wrong"""
    f32 = np.float32
    f = f32(0.8)
    lim = float(f) * float(f) * 3.0
    below, above = f32(lim), np.nextafter(f32(lim), f32(10))
    if float(below) >= lim:
        below = np.nextafter(below, f32(0))
    cases = {0.5: ([(0.25, 1.0, 1), (np.nextafter(f32(0.25), f32(0)), 1.0, 1), (np.nextafter(f32(0.25), f32(1)), 1.0, 1), (5.0, INF, -1), (0.0, 0.0, -1),
                    (0.0, 0.0, 1)], [0, 1, 0, 1, 1, 0]),
             float(f): ([(below, 3.0, 1), (above, 3.0, 1), (0.0, 0.0, 1), (np.nextafter(below, f32(0)), 3.0, 1)], [1, 0, 0, 1]),
             1.0: ([(1.0, 1.0, 1), (1.0, np.nextafter(f32(1), f32(2)), 1), (0.0, 0.0, 1)], [0, 1, 0])}
    for ratio, (rows, kept) in cases.items():
        n = len(rows)
        ans = [(np.array([[0, r[2]] for r in rows], np.int32), np.array([[r[0], r[1]] for r in rows], np.float32))]
        want = reference(ans, ratio)
        assert want[1][:, 0].tolist() == [i for i in range(n) if kept[i]]
        idx, d = stacked(ans, "float")
        same(host_call(dlco, ctx, "float", (n, 2), [(0, 1)], idx, d, ratio), want, ("float", ratio, "host"))
        same(device_call(ctx, "float", (n, 2), [(0, 1)], idx, d, ratio), want, ("float", ratio, "device"))
    big = 2 ** 31 - 1
    edge = int(np.floor(float(f) * float(f) * big))
    cases = {0.5: ([(1, 4, 1), (0, 4, 1), (2, 4, 1), (0, 0, 1), (0, 0, -1), (5, int(I32MAX), -1)], [0, 1, 0, 0, 1, 1]),
             float(f): ([(edge, big, 1), (edge + 1, big, 1), (0, 0, 1)], [1, 0, 0]),
             1.0: ([(1, 1, 1), (1, 2, 1), (0, 0, 1)], [0, 1, 0])}
    for ratio, (rows, kept) in cases.items():
        n = len(rows)
        ans = [(np.array([[0, r[2]] for r in rows], np.int32), np.array([[r[0], r[1]] for r in rows], np.int32))]
        want = reference(ans, ratio)
        assert want[1][:, 0].tolist() == [i for i in range(n) if kept[i]]
        idx, d = stacked(ans, "u8")
        same(host_call(dlco, ctx, "u8", (n, 2), [(0, 1)], idx, d, ratio), want, ("u8", ratio, "host"))
        same(device_call(ctx, "u8", (n, 2), [(0, 1)], idx, d, ratio), want, ("u8", ratio, "device"))


@pytest.mark.parametrize("line", LINES)
@pytest.mark.parametrize("r", (3, 64))
def test_on_real_answers(ctx, line, r):
    """the answers of match_pairs / match_pairs_u8 on the images of tests/test_match_pairs_gpu.py, all 81 ordered pairs: ratio 0.8
    and the mutual check through the DescContext methods against the reference on the same answers; on the float line the
    selected lists then give verify_pairs_homography what the reference's lists give it, byte for byte"""
    from test_match_pairs_gpu import SIZES as REAL, images
    tabs = images(line, REAL, r)
    pairs = [(a, b) for a in range(len(REAL)) for b in range(len(REAL))]
    reverse = [b * len(REAL) + a for a, b in pairs]
    ans = ctx.match_pairs(tabs, pairs) if line == "float" else ctx.match_pairs_u8(tabs, pairs)
    xys = coordinates(REAL, seed=r)
    want = reference(ans, 0.8, [ans[q][0] for q in reverse], xys, pairs)
    moff, R = want[0], sum(REAL[a] for a, _ in pairs)
    print("%s r = %d: M = %d of R = %d" % (line, r, moff[-1], R))
    assert 0 < moff[-1] < R
    sel, lists = (ctx.select_pairs if line == "float" else ctx.select_pairs_u8)(ans, REAL, pairs, 0.8, reverse, xys)
    assert ctx.last_kernel_ms() > 0
    for p in range(len(pairs)):
        same(list(sel[p]) + list(lists[p]), [w[moff[p]:moff[p + 1]] for w in want[1:]], (line, r, p))
    if line == "float":
        ref_lists = [(want[3][moff[p]:moff[p + 1]], want[4][moff[p]:moff[p + 1]]) for p in range(len(pairs))]
        got, exp = ctx.verify_pairs_homography(lists, n_hyp=256), ctx.verify_pairs_homography(ref_lists, n_hyp=256)
        for (H, mask, best), (H2, mask2, best2) in zip(got, exp):
            assert H.tobytes() == H2.tobytes() and mask.tobytes() == mask2.tobytes() and best == best2
