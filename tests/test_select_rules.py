"""CPU tests of the rule that turns a batched match answer into match lists (opencv-dlco_amd/csrc/select_rules.hpp, through
tests/shim/select_rules_shim.cpp): Lowe's ratio test, the mutual check, the compaction and its offsets.  The reference is the
numpy restatement below; the GPU tests (tests/test_select_pairs_gpu.py) import it and the synthetic answers.  Nothing here needs
a GPU or libdlco.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim")
f32p, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
INF, I32MAX = np.float32(np.inf), np.int32(2 ** 31 - 1)
LINES = ("float", "u8")
DIST = {"float": np.float32, "u8": np.int32}
NONE = {"float": INF, "u8": I32MAX}

# the synthetic set: nine images, all 81 ordered pairs, R = 11 349 rows
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 300)
PAIRS = [(a, b) for a in range(len(SIZES)) for b in range(len(SIZES))]
REVERSE = [b * len(SIZES) + a for a, b in PAIRS]          # the pair of the same batch that reverses pair p
RATIOS = (None, 0.5, 0.8, 1.0)
COUNTS = {None: (9098, 3520), 0.5: (2682, 688), 0.8: (5832, 2115), 1.0: (7529, 2848)}     # M without / with the mutual check
SETTINGS = [(r, m) for r in RATIOS for m in (False, True)]


def synthetic(line):
    """Answers that need no matcher, one (idx [na, 2] int32, d [na, 2]) per pair of PAIRS: integer distances d1 = m k and
    d2 = 4 k with m in 0 .. 4 (times 0.125 on the float line, still exact), so that d1 = d2 / 4 and d1 = d2 occur exactly; a
    train image of one row has no second neighbour; a tenth of the rows have no candidate, as guided answers have; an empty
    train image gives none at all.  Then every second row's nearest row is made to agree with the reverse pair."""
    rng = np.random.default_rng(7)
    idx, d = [], []
    for a, b in PAIRS:
        na, nb = SIZES[a], SIZES[b]
        if nb == 0:
            idx.append(np.full((na, 2), -1, np.int32))
            d.append(np.full((na, 2), NONE[line], DIST[line]))
            continue
        j, k, m = rng.integers(0, nb, na), rng.integers(1, 1000, na), rng.integers(0, 5, na)
        d1, d2 = (m * k).astype(np.float64), (4 * k).astype(np.float64)
        if line == "float":
            d1, d2 = d1 * 0.125, d2 * 0.125
        if nb == 1:
            j2, d2 = np.full(na, -1), np.full(na, float(NONE[line]))
        else:
            j2 = (j + 1 + rng.integers(0, nb - 1, na)) % nb
        gone = rng.random(na) < 0.1
        j, j2 = np.where(gone, -1, j), np.where(gone, -1, j2)
        d1, d2 = np.where(gone, float(NONE[line]), d1), np.where(gone, float(NONE[line]), d2)
        idx.append(np.stack([j, j2], 1).astype(np.int32))
        d.append(np.stack([d1, d2], 1).astype(DIST[line]))
    for p, (a, b) in enumerate(PAIRS):
        back = idx[REVERSE[p]]
        for i in range(0, SIZES[a], 2):
            j = idx[p][i, 0]
            if j >= 0 and back[j, 0] >= 0:
                back[j, 0] = i
    return list(zip(idx, d))


def coordinates(sizes, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0, 640, (n, 2)).astype(np.float32) for n in sizes]


def reference(answers, ratio=None, backs=None, xys=None, pairs=None):
    """The rule in numpy, pair by pair.  backs[p]: the reverse answer's idx [nb, 2] or None.  Returns moff, matches, dist and,
    with xys and pairs, src and dst, all concatenated over the pairs."""
    ms, ds, ss, ts, moff = [], [], [], [], [0]
    for p, (idx, d) in enumerate(answers):
        n = len(idx)
        keep = idx[:, 0] >= 0
        if ratio is not None:
            f = float(np.float32(ratio))
            keep &= (idx[:, 1] == -1) | (d[:, 0].astype(np.float64) < f * f * d[:, 1].astype(np.float64))
        if backs is not None and backs[p] is not None:
            back = backs[p]
            keep &= (back[np.maximum(idx[:, 0], 0), 0] == np.arange(n)) if len(back) else False
        i = np.flatnonzero(keep)
        ms.append(np.stack([i, idx[i, 0]], 1).astype(np.int32))
        ds.append(d[i, 0])
        if xys is not None:
            ss.append(xys[pairs[p][0]][i])
            ts.append(xys[pairs[p][1]][idx[i, 0]])
        moff.append(moff[-1] + len(i))
    out = [np.array(moff, np.int64), np.concatenate(ms), np.concatenate(ds)]
    if xys is not None:
        out += [np.concatenate(ss).astype(np.float32), np.concatenate(ts).astype(np.float32)]
    return out


@pytest.fixture(scope="module")
def synth():
    s = {line: synthetic(line) for line in LINES}
    for line in LINES:
        for a in s[line]:
            a[0].setflags(write=False)
            a[1].setflags(write=False)
    return s


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libselectshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), os.path.join(SHIM, "select_rules_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_select_ratio_keep.argtypes = [C.c_float, C.c_float, C.c_int32, C.c_float]
    L.shim_select_ratio_keep_i32.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_float]
    L.shim_select_ratio_ok.argtypes = [C.c_float]
    L.shim_select_keep.argtypes = [C.c_int32, C.c_int64, i32p, f32p, C.c_float, i32p]
    L.shim_select_keep_i32.argtypes = [C.c_int32, C.c_int64, i32p, i32p, C.c_float, i32p]
    L.shim_select_back_rows_ok.argtypes = [i64p, i32p, C.c_int64, i64p, C.c_int64]
    L.shim_select_pair_of_row.argtypes = [i64p, i32p, C.c_int64, C.c_int64]
    L.shim_select_pair_of_row.restype = C.c_int64
    for name, dp in (("shim_select_pairs", f32p), ("shim_select_pairs_i32", i32p)):
        getattr(L, name).argtypes = [i64p, i32p, C.c_int64, i32p, dp, C.c_float, i32p, i64p, f32p, C.c_int64, i64p, i32p, dp, f32p, f32p]
        getattr(L, name).restype = C.c_int64
    return L


def p_(a, t):
    return None if a is None else a.ctypes.data_as(t)


def host_select(L, line, sizes, pairs, answers, ratio, back_idx, back_row0, xy, ldxy):
    """select_rules::select_host over the whole batch; the lists are poisoned beyond what the call writes"""
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    q = np.ascontiguousarray(pairs, np.int32)
    idx = np.ascontiguousarray(np.concatenate([a[0] for a in answers] + [np.zeros((1, 2), np.int32)]))
    d = np.ascontiguousarray(np.concatenate([a[1] for a in answers] + [np.zeros((1, 2), DIST[line])]))
    R = len(idx) - 1
    moff, m, dd = np.full(len(q) + 1, -7, np.int64), np.full((R + 1, 2), -7, np.int32), np.full(R + 1, -7, DIST[line])
    src = dst = None
    if xy is not None:
        src, dst = np.full((R + 1, 2), -7, np.float32), np.full((R + 1, 2), -7, np.float32)
    bidx = idx if back_idx is True else back_idx
    call, dp = (L.shim_select_pairs, f32p) if line == "float" else (L.shim_select_pairs_i32, i32p)
    got_R = call(p_(seg, i64p), p_(q, i32p), len(q), p_(idx, i32p), p_(d, dp), 0.0 if ratio is None else ratio, p_(bidx, i32p), p_(back_row0, i64p),
                 p_(xy, f32p), ldxy, p_(moff, i64p), p_(m, i32p), p_(dd, dp), p_(src, f32p), p_(dst, f32p))
    assert got_R == R
    M = int(moff[-1])
    assert (m[M:] == -7).all() and (dd[M:] == -7).all() and (src is None or ((src[M:] == -7).all() and (dst[M:] == -7).all()))
    return [moff, m[:M], dd[:M]] + ([] if xy is None else [src[:M], dst[:M]])


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def row0_of(sizes, pairs):
    return np.concatenate([[0], np.cumsum([sizes[a] for a, _ in pairs])]).astype(np.int64)


def test_constants_are_readable(rules):
    assert rules.shim_select_block_rows() == 256
    chunk = rules.shim_select_scan_chunk()
    assert chunk >= 64 and chunk % 64 == 0


def test_reference_counts_of_the_synthetic_set(synth):
    """what the comparisons below rest on: no setting keeps everything or nothing, and a ratio empties whole pairs"""
    R = sum(SIZES[a] for a, _ in PAIRS)
    assert R == 11349
    for line in LINES:
        ans = synth[line]
        backs = [ans[q][0] for q in REVERSE]
        for ratio, mutual in SETTINGS:
            moff = reference(ans, ratio, backs if mutual else None)[0]
            assert moff[-1] == COUNTS[ratio][1 if mutual else 0] and 0 < moff[-1] < R
        m = np.diff(reference(ans, 0.5)[0])
        emptied = [p for p, (a, b) in enumerate(PAIRS) if SIZES[a] > 0 and SIZES[b] > 0 and m[p] == 0]
        assert len(emptied) >= 1


@pytest.mark.parametrize("line", LINES)
def test_rule_against_numpy_on_the_synthetic_set(rules, synth, line):
    ans = synth[line]
    xys = coordinates(SIZES)
    xy2 = np.ascontiguousarray(np.concatenate(xys + [np.zeros((1, 2), np.float32)]))
    xy4 = np.full((len(xy2), 4), -3, np.float32)
    xy4[:, :2] = xy2
    row0 = row0_of(SIZES, PAIRS)
    same_batch = row0[REVERSE]
    backs = [ans[q][0] for q in REVERSE]
    second = np.ascontiguousarray(np.concatenate(backs + [np.zeros((1, 2), np.int32)]))
    second_row0 = np.concatenate([[0], np.cumsum([len(b) for b in backs])])[:-1].astype(np.int64)
    for ratio, mutual in SETTINGS:
        want = reference(ans, ratio, backs if mutual else None, xys, PAIRS)
        forms = [(True, same_batch), (second, second_row0)] if mutual else [(None, None)]
        for bidx, brow0 in forms:
            same(host_select(rules, line, SIZES, PAIRS, ans, ratio, bidx, brow0, xy2, 2), want)
            same(host_select(rules, line, SIZES, PAIRS, ans, ratio, bidx, brow0, xy4, 4), want)
            same(host_select(rules, line, SIZES, PAIRS, ans, ratio, bidx, brow0, None, 2), want[:3])
    # -1 in back_row0 switches the check off pair by pair
    off = same_batch.copy()
    off[::2] = -1
    want = reference(ans, 0.8, [None if p % 2 == 0 else b for p, b in enumerate(backs)])
    same(host_select(rules, line, SIZES, PAIRS, ans, 0.8, True, off, None, 2), want)


def test_ratio_rule_at_the_boundary(rules):
    """the cases of test_match_rules.py::test_ratio_rule_at_the_boundary, and their integer kin"""
    keep, keep_i = rules.shim_select_ratio_keep, rules.shim_select_ratio_keep_i32
    assert keep(0.25, 1.0, 7, 0.5) == 0
    assert keep(float(np.nextafter(np.float32(0.25), np.float32(0))), 1.0, 7, 0.5) == 1
    assert keep(float(np.nextafter(np.float32(0.25), np.float32(1))), 1.0, 7, 0.5) == 0
    f = np.float32(0.8)
    lim = float(f) * float(f) * 3.0
    below, above = np.float32(lim), np.nextafter(np.float32(lim), np.float32(10))
    if float(below) >= lim:
        below = np.nextafter(below, np.float32(0))
    assert keep(float(below), 3.0, 1, float(f)) == 1 and keep(float(above), 3.0, 1, float(f)) == 0
    assert keep(5.0, float("inf"), -1, 0.5) == 1 and keep(0.0, 0.0, -1, 0.5) == 1
    assert keep(0.0, 0.0, 3, 0.8) == 0 and keep(0.0, 0.0, 3, 1.0) == 0
    assert keep(1.0, 1.0, 3, 1.0) == 0 and keep(1.0, float(np.nextafter(np.float32(1), np.float32(2))), 3, 1.0) == 1
    # int32 distances: 1 < 0.25 * 4 is false, 0 < 0 is false, and the comparison is in double on the float f
    assert keep_i(1, 4, 7, 0.5) == 0 and keep_i(0, 4, 7, 0.5) == 1 and keep_i(2, 4, 7, 0.5) == 0
    assert keep_i(0, 0, 3, 0.8) == 0 and keep_i(0, 0, 3, 1.0) == 0 and keep_i(0, 0, -1, 0.5) == 1
    assert keep_i(5, int(I32MAX), -1, 0.5) == 1 and keep_i(1, 1, 3, 1.0) == 0 and keep_i(1, 2, 3, 1.0) == 1
    big = 2 ** 31 - 1
    lim = float(f) * float(f) * big
    assert keep_i(int(np.floor(lim)), big, 1, float(f)) == 1 and keep_i(int(np.floor(lim)) + 1, big, 1, float(f)) == 0
    # the ratio itself: 0 (none) and (0, 1]
    ok = rules.shim_select_ratio_ok
    assert ok(0.0) == 1 and ok(0.5) == 1 and ok(1.0) == 1
    assert ok(float("nan")) == 0 and ok(-0.5) == 0 and ok(float(np.nextafter(np.float32(1), np.float32(2)))) == 0 and ok(float("inf")) == 0


def test_an_index_outside_the_train_image_is_dropped_without_a_read(rules):
    """the reverse table of nt_b rows lies inside a larger poisoned array: every value around it says "mutual", so a read
    outside would keep the row"""
    nt, i = 5, 3
    big = np.full((4096 + nt + 4096, 2), i, np.int32)
    back = big[4096:4096 + nt]
    back[:] = -9
    back[2, 0] = i
    d, d8 = np.array([1.0, 100.0], np.float32), np.array([1, 100], np.int32)
    for call, dist, dp in ((rules.shim_select_keep, d, f32p), (rules.shim_select_keep_i32, d8, i32p)):
        run = lambda j, b, f=0.8: call(nt, i, p_(np.array([j, 0], np.int32), i32p), p_(dist, dp), f, None if b is None else p_(b, i32p))
        assert run(2, back) == 1 and run(1, back) == 0
        for j in (-1, -2, -4096, -2 ** 31, nt, nt + 1, 4000, 2 ** 31 - 1):
            assert run(j, back) == 0 and run(j, None) == 0 and run(j, None, 0.0) == 0, j
        assert run(nt - 1, None) == 1 and run(0, None, 0.0) == 1
    # the bound check of the reverse table: back_row0[p] is -1 or the first of nt_b rows inside [0, n_back_rows)
    seg, pairs = np.array([0, 3, 3, 10], np.int64), np.array([[0, 2], [2, 0], [1, 2]], np.int32)
    ok = lambda b, n: rules.shim_select_back_rows_ok(p_(seg, i64p), p_(pairs, i32p), 3, None if b is None else p_(np.array(b, np.int64), i64p), n)
    assert ok([3, 0, -1], 10) == 1 and ok([-1, -1, -1], 0) == 1 and ok([0, 7, 3], 10) == 1
    assert ok([4, 0, -1], 10) == 0 and ok([3, 8, -1], 10) == 0 and ok([3, 0, -2], 10) == 0 and ok([3, 0, 4], 10) == 0
    assert ok(None, 10) == 0 and ok([3, 0, -1], -1) == 0 and ok([3, 0, -1], 9) == 0 and ok([2 ** 62, 0, -1], 10) == 0


def test_rows_find_their_pair_across_empty_pairs(rules):
    sizes = (0, 2, 0, 3)
    pairs = [(0, 1), (1, 0), (2, 3), (0, 0), (3, 1), (2, 2), (0, 3)]
    seg, q = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), np.array(pairs, np.int32)
    row0 = row0_of(sizes, pairs)
    assert row0.tolist() == [0, 0, 2, 2, 2, 5, 5, 5]
    got = [rules.shim_select_pair_of_row(p_(seg, i64p), p_(q, i32p), len(q), g) for g in range(5)]
    assert got == [1, 1, 4, 4, 4]
    # a batch of empty pairs at both ends: moff repeats values there
    ans = [(np.zeros((sizes[a], 2), np.int32), np.ones((sizes[a], 2), np.float32)) for a, _ in pairs]
    moff = host_select(rules, "float", sizes, pairs, ans, None, None, None, None, 2)[0]
    assert moff.tolist() == [0, 0, 0, 0, 0, 3, 3, 3]       # pair (1, 0): an empty train image keeps nothing


def test_select_under_address_and_undefined_sanitizers(tmp_path):
    """the stand-alone program walks the host-side index arithmetic of the call with its own checks"""
    exe = tmp_path / "select_rules_asan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(SHIM, "select_rules_asan_main.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "select_rules_asan: ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
