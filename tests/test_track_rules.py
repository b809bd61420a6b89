"""CPU tests of the rule that turns the verified matches of many image pairs into multi-view tracks
(opencv-dlco_amd/csrc/track_rules.hpp, through tests/shim/track_rules_shim.cpp): nodes, edges, labels, tracks, counts and order.
The reference is the plain Python union-find below; the GPU tests (tests/test_tracks_gpu.py, tests/test_tracks_cli_gpu.py)
import it, the synthetic set and the special graphs.  Nothing here needs a GPU or libdlco.so."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim")
i32p, i64p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
STRAY = (-1, None, 2 ** 31 - 1)                            # None stands for n, the rows of the image

# the synthetic set: nine images, the 72 ordered pairs of different images, N = 1261 nodes, M = 2043 matches
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 300)
# (min_len, unique, mask used) -> (tracks, observations, counts)
SETTINGS = collections.OrderedDict([
    ((2, 1, True), (287, 918, [321, 0, 34])),
    ((2, 1, False), (187, 573, [239, 0, 52])),
    ((2, 0, True), (321, 1194, [321, 0, 0])),
    ((2, 0, False), (239, 1220, [239, 0, 0])),
    ((3, 1, True), (207, 758, [321, 80, 34])),
    ((3, 1, False), (126, 451, [239, 61, 52])),
    ((5, 0, False), (58, 681, [239, 181, 0])),
])


def synthetic(seed=11, P=400):
    rng = np.random.default_rng(seed)
    pts = [rng.permutation(P)[:n] for n in SIZES]
    pairs = [(a, b) for a in range(9) for b in range(9) if a != b]
    moff, ms, ks = [0], [], []
    for a, b in pairs:
        common, ia, ib = np.intersect1d(pts[a], pts[b], return_indices=True)
        sel = rng.random(len(common)) < 0.6
        m = np.stack([ia[sel], ib[sel]], 1).reshape(-1, 2)
        k = rng.random(len(m)) < 0.9
        nw = len(common) // 20
        if nw:
            w = np.stack([rng.integers(0, SIZES[a], nw), rng.integers(0, SIZES[b], nw)], 1)
            m = np.concatenate([m, w]); k = np.concatenate([k, rng.random(nw) < 0.3])
        o = rng.permutation(len(m)); m, k = m[o], k[o]
        ms.append(m.astype(np.int32)); ks.append(k.astype(np.uint8)); moff.append(moff[-1] + len(m))
    return np.array(pairs, np.int32), np.array(moff, np.int64), np.concatenate(ms), np.concatenate(ks)


def seg_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


Ref = collections.namedtuple("Ref", "toff obs track_of label counts")


def reference(seg, pairs, moff, matches, keep=None, min_len=2, unique=1):
    """The rule in plain Python: a union-find with path compression over dictionaries-free lists, then the components in
    ascending order of their smallest node.  Returns Ref(toff, obs, track_of, label, counts) with the dtypes of the call."""
    seg = [int(s) for s in seg]
    N = seg[-1]
    parent = list(range(N))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for p, (a, b) in enumerate(np.asarray(pairs).tolist()):
        na, nb = seg[a + 1] - seg[a], seg[b + 1] - seg[b]
        for m in range(int(moff[p]), int(moff[p + 1])):
            i, j = int(matches[m][0]), int(matches[m][1])
            if (keep is not None and keep[m] == 0) or not (0 <= i < na) or not (0 <= j < nb):
                continue
            u, v = find(seg[a] + i), find(seg[b] + j)
            if u != v:
                parent[max(u, v)] = min(u, v)
    label = [find(g) for g in range(N)]
    image = np.searchsorted(np.array(seg, np.int64), np.arange(N), side="right") - 1
    members = collections.OrderedDict()
    for g in range(N):                                     # ascending g: a component is first met at its smallest node, its label
        members.setdefault(label[g], []).append(g)
    counts, toff, obs, track_of = [0, 0, 0], [0], [], [-1] * N
    for l, nodes in members.items():
        if len(nodes) < 2:
            continue
        counts[0] += 1
        conflict = len(set(int(image[g]) for g in nodes)) < len(nodes)
        if len(nodes) < min_len:
            counts[1] += 1
            continue
        if unique and conflict:
            counts[2] += 1
            continue
        for g in nodes:
            track_of[g] = len(toff) - 1
        obs += nodes
        toff.append(len(obs))
    return Ref(np.array(toff, np.int64), np.array(obs, np.int32).reshape(-1), np.array(track_of, np.int32).reshape(-1),
               np.array(label, np.int32).reshape(-1), np.array(counts, np.int64))


def reorder(moff, matches, keep, rng):
    """the same batch with every pair's matches in another order"""
    o = np.concatenate([moff[p] + rng.permutation(int(moff[p + 1] - moff[p])) for p in range(len(moff) - 1)] + [np.zeros(0, np.int64)]).astype(np.int64)
    return np.ascontiguousarray(matches[o]), None if keep is None else np.ascontiguousarray(keep[o])


# ---- special graphs, shared with the GPU tests: (sizes, pairs, moff, matches) ----
def chain(n=64):
    """n images of one row, matches (k, k + 1) listed in descending k: one track of n, the deepest parent walk"""
    pairs = np.array([(k, k + 1) for k in range(n - 2, -1, -1)], np.int32)
    return (1,) * n, pairs, np.arange(n, dtype=np.int64), np.zeros((n - 1, 2), np.int32)


def star(n=301):
    """n images of one row, pairs (0, k): n - 1 hooks on one root"""
    pairs = np.array([(0, k) for k in range(1, n)], np.int32)
    return (1,) * n, pairs, np.arange(n, dtype=np.int64), np.zeros((n - 1, 2), np.int32)


def cycle(n=256):
    """two images of n rows, matches (i, i) and (i, (i + 1) % n): one component of 2 n nodes"""
    i = np.arange(n)
    m = np.concatenate([np.stack([i, i], 1), np.stack([i, (i + 1) % n], 1)]).astype(np.int32)
    return (n, n), np.array([(0, 1)], np.int32), np.array([0, 2 * n], np.int64), m


def stray_batch():
    """matches whose i or j is -1, n or 2^31 - 1 among good ones: three images of 5, 0 and 7 rows"""
    sizes = (5, 0, 7)
    pairs = np.array([(0, 2), (2, 0), (0, 1), (1, 2), (2, 2)], np.int32)
    ms, moff = [], [0]
    for a, b in pairs.tolist():
        na, nb = sizes[a], sizes[b]
        m = [(i, j) for i in ([0, na - 1] if na else [0]) for j in [s if s is not None else nb for s in STRAY]]
        m += [(i, j) for j in ([1, nb - 1] if nb else [0]) for i in [s if s is not None else na for s in STRAY]]
        m += [(s if s is not None else na, t if t is not None else nb) for s in STRAY for t in STRAY]
        if na and nb:
            m += [(1, 2), (na - 1, nb - 1)]
        ms += m
        moff.append(len(ms))
    return sizes, pairs, np.array(moff, np.int64), np.array(ms, np.int64).astype(np.int32)


@pytest.fixture(scope="module")
def synth():
    s = synthetic()
    for a in s:
        a.setflags(write=False)
    return s


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libtrackshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), os.path.join(SHIM, "track_rules_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_track_edge.argtypes = [C.c_int32] * 6 + [i32p]
    L.shim_track_image_of.argtypes = [i64p, C.c_int32, C.c_int64]
    L.shim_track_moff_ok.argtypes = [i64p, C.c_int64]
    L.shim_track_settings_ok.argtypes = [C.c_int32, C.c_int32]
    L.shim_track_pair_of_match.argtypes = [i64p, i32p, C.c_int64, i64p, C.c_int64]
    L.shim_track_pair_of_match.restype = C.c_int64
    L.shim_track_labels.argtypes = [i64p, C.c_int32, i32p, C.c_int64, i64p, i32p, u8p, i64p, i32p]
    L.shim_track_labels.restype = None
    L.shim_track_build.argtypes = [i64p, C.c_int32, i32p, C.c_int64, i64p, i32p, u8p, C.c_int32, C.c_int32, i64p, i32p, i32p, i32p, i64p]
    L.shim_track_build.restype = C.c_int64
    return L


def p_(a, t):
    return None if a is None else a.ctypes.data_as(t)


def padded(a, dtype, shape_tail=()):
    """a contiguous copy with one entry of padding: an empty list still has an address"""
    a = np.asarray(a, dtype).reshape((-1,) + shape_tail)
    return np.ascontiguousarray(np.concatenate([a, np.zeros((1,) + shape_tail, dtype)]))


def host_tracks(L, seg, pairs, moff, matches, keep, min_len, unique, want_label=True):
    """track_rules::tracks_host; the outputs are poisoned beyond what the call writes"""
    seg, q, o = np.ascontiguousarray(seg, np.int64), np.ascontiguousarray(pairs, np.int32), np.ascontiguousarray(moff, np.int64)
    N = int(seg[-1])
    m, k = padded(matches, np.int32, (2,)), None if keep is None else padded(keep, np.uint8)
    toff, obs = np.full(N // 2 + 1, -7, np.int64), np.full(N + 1, -7, np.int32)
    track_of, label, counts = np.full(N + 1, -7, np.int32), np.full(N + 1, -7, np.int32), np.full(3, -7, np.int64)
    T = L.shim_track_build(p_(seg, i64p), seg.size - 1, p_(q, i32p), len(q), p_(o, i64p), p_(m, i32p), p_(k, u8p), min_len, unique, p_(toff, i64p),
                           p_(obs, i32p), p_(track_of, i32p), p_(label, i32p) if want_label else None, p_(counts, i64p))
    K = int(toff[T])
    assert (toff[T + 1:] == -7).all() and (obs[K:] == -7).all() and track_of[N] == -7 and label[N] == -7
    assert want_label or (label == -7).all()
    return Ref(toff[:T + 1], obs[:K], track_of[:N], label[:N], counts)


def host_labels(L, seg, pairs, moff, matches, keep, order):
    seg, q, o = np.ascontiguousarray(seg, np.int64), np.ascontiguousarray(pairs, np.int32), np.ascontiguousarray(moff, np.int64)
    N = int(seg[-1])
    m, k = padded(matches, np.int32, (2,)), None if keep is None else padded(keep, np.uint8)
    order = None if order is None else padded(order, np.int64)
    label = np.full(N + 1, -7, np.int32)
    L.shim_track_labels(p_(seg, i64p), seg.size - 1, p_(q, i32p), len(q), p_(o, i64p), p_(m, i32p), p_(k, u8p), p_(order, i64p), p_(label, i32p))
    assert label[N] == -7
    return label[:N]


def same(got, want, label=True):
    for name in Ref._fields:
        if name == "label" and not label:
            continue
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name


def test_constants_are_readable(rules):
    assert rules.shim_track_block_nodes() == 256
    chunk = rules.shim_track_scan_chunk()
    assert chunk >= 64 and chunk % 64 == 0
    assert rules.shim_track_counted() == 5


def test_reference_figures_of_the_synthetic_set(synth):
    """what the comparisons rest on: the figures of the reference at every setting, and that neither branch is idle"""
    pairs, moff, matches, keep = synth
    seg = seg_of(SIZES)
    assert seg[-1] == 1261 and moff[-1] == 2043 and len(matches) == 2043 and int(keep.sum()) == 1759 and len(pairs) == 72
    for (min_len, unique, masked), (tracks, n_obs, counts) in SETTINGS.items():
        r = reference(seg, pairs, moff, matches, keep if masked else None, min_len, unique)
        assert (len(r.toff) - 1, len(r.obs), r.counts.tolist()) == (tracks, n_obs, counts), (min_len, unique, masked)
        assert r.counts[0] - r.counts[1] - r.counts[2] == tracks and (r.track_of >= 0).sum() == n_obs
    r = reference(seg, pairs, moff, matches, None, 2, 0)
    assert int(np.diff(r.toff).max()) == 61
    for masked in (True, False):
        c = reference(seg, pairs, moff, matches, keep if masked else None, 2, 1).counts
        assert 0.10 <= c[2] / c[0] <= 0.22


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_host_rule_against_the_reference_on_the_synthetic_set(rules, synth, setting):
    min_len, unique, masked = setting
    pairs, moff, matches, keep = synth
    seg = seg_of(SIZES)
    want = reference(seg, pairs, moff, matches, keep if masked else None, min_len, unique)
    same(host_tracks(rules, seg, pairs, moff, matches, keep if masked else None, min_len, unique), want)
    same(host_tracks(rules, seg, pairs, moff, matches, keep if masked else None, min_len, unique, want_label=False), want, label=False)
    m2, k2 = reorder(moff, matches, keep if masked else None, np.random.default_rng(5))
    same(host_tracks(rules, seg, pairs, moff, m2, k2, min_len, unique), want)


@pytest.mark.parametrize("masked", (True, False))
def test_hook_step_gives_the_same_labels_in_every_order(rules, synth, masked):
    """the header's hook step, the function the kernel runs, over the edges in ascending, reversed and three shuffled orders"""
    pairs, moff, matches, keep = synth
    seg, M = seg_of(SIZES), int(moff[-1])
    k = keep if masked else None
    want = reference(seg, pairs, moff, matches, k).label
    rng = np.random.default_rng(23)
    orders = [None, np.arange(M - 1, -1, -1)] + [rng.permutation(M) for _ in range(3)]
    for order in orders:
        got = host_labels(rules, seg, pairs, moff, matches, k, order)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    # a label is the smallest node of its component
    assert (want <= np.arange(len(want))).all() and (want[want] == want).all()


def test_special_graphs(rules):
    for sizes, pairs, moff, m in (chain(), star()):
        n = len(sizes)
        r = host_tracks(rules, seg_of(sizes), pairs, moff, m, None, 2, 1)
        same(r, reference(seg_of(sizes), pairs, moff, m))
        assert r.toff.tolist() == [0, n] and r.obs.tolist() == list(range(n)) and r.counts.tolist() == [1, 0, 0] and not r.label.any()
    sizes, pairs, moff, m = cycle()
    r = host_tracks(rules, seg_of(sizes), pairs, moff, m, None, 2, 1)
    same(r, reference(seg_of(sizes), pairs, moff, m, None, 2, 1))
    assert r.toff.tolist() == [0] and r.counts.tolist() == [1, 0, 1] and (r.track_of == -1).all()
    r = host_tracks(rules, seg_of(sizes), pairs, moff, m, None, 2, 0)
    same(r, reference(seg_of(sizes), pairs, moff, m, None, 2, 0))
    assert r.toff.tolist() == [0, 512] and r.counts.tolist() == [1, 0, 0]


def test_out_of_range_matches_are_skipped(rules):
    uv = np.full(2, -7, np.int32)
    for n in (1, 5, 300):
        for s in STRAY:
            bad = n if s is None else s
            assert rules.shim_track_edge(10, n, 1000, 7, bad, 3, p_(uv, i32p)) == 0
            assert rules.shim_track_edge(10, 7, 1000, n, 3, bad, p_(uv, i32p)) == 0
            assert rules.shim_track_edge(10, n, 1000, n, bad, bad, p_(uv, i32p)) == 0
        assert (uv == -7).all()
        assert rules.shim_track_edge(10, n, 1000, n, n - 1, 0, p_(uv, i32p)) == 1 and uv.tolist() == [10 + n - 1, 1000]
        uv[:] = -7
    assert rules.shim_track_edge(10, 0, 1000, 7, 0, 3, p_(uv, i32p)) == 0 and rules.shim_track_edge(10, 7, 1000, 0, 3, 0, p_(uv, i32p)) == 0
    sizes, pairs, moff, m = stray_batch()
    seg = seg_of(sizes)
    want = reference(seg, pairs, moff, m)
    same(host_tracks(rules, seg, pairs, moff, m, None, 2, 1), want)
    # only the good matches count: (0, 2): 5 rows against 7; (2, 0); (2, 2) joins nodes of one image
    good = [(a, b, i, j) for p, (a, b) in enumerate(pairs.tolist()) for i, j in m[moff[p]:moff[p + 1]].tolist() if 0 <= i < sizes[a] and 0 <= j < sizes[b]]
    assert len(good) == 6 and want.counts[0] >= 1


def test_images_pairs_and_argument_checks(rules):
    seg = np.array([0, 0, 3, 3, 3, 10, 10], np.int64)
    got = [rules.shim_track_image_of(p_(seg, i64p), 6, g) for g in range(10)]
    assert got == [1, 1, 1, 4, 4, 4, 4, 4, 4, 4]
    pairs, moff = np.array([[1, 4], [0, 1], [4, 1], [2, 3], [4, 4]], np.int32), np.array([0, 0, 0, 4, 4, 6], np.int64)
    assert [rules.shim_track_pair_of_match(p_(seg, i64p), p_(pairs, i32p), 5, p_(moff, i64p), m) for m in range(6)] == [2, 2, 2, 2, 4, 4]
    ok = lambda a: rules.shim_track_moff_ok(p_(np.array(a, np.int64), i64p), len(a) - 1)
    assert ok([0, 0, 5]) == 1 and ok([0, 2 ** 31 - 1]) == 1 and ok([0, 0]) == 1
    assert ok([1, 2]) == 0 and ok([0, 5, 4]) == 0 and ok([0, 2 ** 31]) == 0 and ok([0, -1]) == 0
    s = rules.shim_track_settings_ok
    assert s(2, 0) == 1 and s(2, 1) == 1 and s(64, 1) == 1
    assert s(1, 1) == 0 and s(0, 0) == 0 and s(-3, 1) == 0 and s(2, 2) == 0 and s(2, -1) == 0
    # empty batches: no match, no node
    for sizes in ((0, 0, 0), (4, 0, 2)):
        sg = seg_of(sizes)
        q, o = np.array([[0, 2], [2, 1]], np.int32), np.zeros(3, np.int64)
        r = host_tracks(rules, sg, q, o, np.zeros((0, 2), np.int32), None, 2, 1)
        assert r.toff.tolist() == [0] and len(r.obs) == 0 and (r.track_of == -1).all() and r.counts.tolist() == [0, 0, 0]
        assert r.label.tolist() == list(range(int(sg[-1])))


def write_cases(path, cases):
    """the cases of the stand-alone sanitizer program as a stream of int64: inputs and the reference's answers"""
    out = [len(cases)]
    for seg, pairs, moff, m, keep, min_len, unique in cases:
        r = reference(seg, pairs, moff, m, keep, min_len, unique)
        out += [len(seg) - 1, *seg.tolist(), len(pairs), *np.asarray(pairs).reshape(-1).tolist(), *moff.tolist(), *np.asarray(m).reshape(-1).tolist()]
        out += [0] if keep is None else [1, *keep.tolist()]
        out += [min_len, unique, len(r.toff) - 1, *r.toff.tolist(), *r.obs.tolist(), *r.track_of.tolist(), *r.label.tolist(), *r.counts.tolist()]
    np.array(out, np.int64).tofile(str(path))


def test_rule_under_address_and_undefined_sanitizers(tmp_path, synth):
    """the stand-alone program runs the host rule on the cases of this file, on buffers of exactly the sizes used"""
    pairs, moff, matches, keep = synth
    cases = [(seg_of(SIZES), pairs, moff, matches, keep if masked else None, min_len, unique) for (min_len, unique, masked) in SETTINGS]
    for g in (chain(), star(), cycle(), stray_batch()):
        for unique in (0, 1):
            cases.append((seg_of(g[0]), g[1], g[2], g[3], None, 2, unique))
    cases.append((seg_of((0, 0)), np.array([[0, 1]], np.int32), np.zeros(2, np.int64), np.zeros((0, 2), np.int32), None, 2, 1))
    cases.append((seg_of(SIZES), pairs, moff, matches, np.zeros(len(matches), np.uint8), 2, 1))
    write_cases(tmp_path / "cases.i64", cases)
    exe = tmp_path / "track_rules_asan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(SHIM, "track_rules_asan_main.cpp")])
    p = subprocess.run([str(exe), str(tmp_path / "cases.i64")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stderr == "" and ("track_rules_asan: ok (%d cases of the file" % len(cases)) in p.stdout
