"""CPU tests of the plan of a batched match (opencv-dlco_amd/csrc/match_batch.hpp, through tests/shim/match_batch_shim.cpp):
how dlco_desc_match_pairs cuts a list of (query image, train image) pairs over one segmented table into launches, entries,
slices, partials and fills.  Every property the kernels rely on is checked on seeded sets; the slicing rule itself is held
against the restatement of tests/test_match_slices.py.  Nothing here needs a GPU or libdlco.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_match_slices import KINDS, NUMBERS, ceil_div, slices, tiles_per_slice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim")
i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
SIZES = (0, 1, 15, 16, 17, 127, 128, 129, 257, 5000)
CUS = (1, 64, 256, 304)
LAUNCH_ROWS = 2 ** 20
E_FIELDS = ("q0", "t0", "out0", "part0", "nq", "nt", "tps", "slices", "wg0", "mwg0", "qblocks", "pair")
L_FIELDS = ("e0", "n", "rows", "qblocks", "wgs", "merge_wgs", "parts")
F_FIELDS = ("out0", "n", "first", "pair")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libmatchbatchshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), os.path.join(SHIM, "match_batch_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_tiles_per_slice.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int]
    L.shim_tiles_per_slice_of.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int]
    L.shim_slices.argtypes = [C.c_int64, C.c_int, C.c_int]
    L.shim_launch_rows.restype = C.c_int64
    L.shim_batch_row_offsets.argtypes, L.shim_batch_row_offsets.restype = [i64p, i32p, C.c_int64, i64p], None
    L.shim_batch_plan.argtypes, L.shim_batch_plan.restype = [C.c_int, i64p, i32p, C.c_int64, C.c_int], C.c_void_p
    L.shim_batch_free.argtypes, L.shim_batch_free.restype = [C.c_void_p], None
    L.shim_batch_count.argtypes, L.shim_batch_count.restype = [C.c_void_p, C.c_int], C.c_int64
    for name in ("entries", "launches", "fills", "row0"):
        f = getattr(L, "shim_batch_" + name)
        f.argtypes, f.restype = [C.c_void_p, i64p], None
    L.shim_batch_slices.argtypes, L.shim_batch_slices.restype = [C.c_void_p, i32p], None
    return L


def plan(L, kind, seg, pairs, n_cu):
    """the plan as dicts of int64 columns: entries, launches, fills; row0, slices; fill_rows, max_parts"""
    seg, pairs = np.ascontiguousarray(seg, np.int64), np.ascontiguousarray(pairs, np.int32)
    h = L.shim_batch_plan(KINDS.index(kind), seg.ctypes.data_as(i64p), pairs.ctypes.data_as(i32p), len(pairs), n_cu)
    try:
        def table(what, fn, fields):
            a = np.zeros((L.shim_batch_count(h, what), len(fields)), np.int64)
            fn(h, a.ctypes.data_as(i64p))
            return {f: a[:, k] for k, f in enumerate(fields)}
        row0, sl = np.zeros(len(pairs) + 1, np.int64), np.zeros(len(pairs), np.int32)
        L.shim_batch_row0(h, row0.ctypes.data_as(i64p))
        L.shim_batch_slices(h, sl.ctypes.data_as(i32p))
        return dict(e=table(0, L.shim_batch_entries, E_FIELDS), l=table(1, L.shim_batch_launches, L_FIELDS), f=table(2, L.shim_batch_fills, F_FIELDS),
                    row0=row0, slices=sl, fill_rows=L.shim_batch_count(h, 3), max_parts=L.shim_batch_count(h, 4))
    finally:
        L.shim_batch_free(h)


def seeded_sets():
    """(seg, pairs): image sizes from SIZES and random, 1 to 2000 pairs, and sets with one image of 2^20 + 77 rows as a query"""
    rng = np.random.default_rng(20240611)
    out = []
    for k in range(8):
        n_img = int(rng.integers(2, 16))
        sizes = [int(rng.choice(SIZES)) if rng.integers(2) else int(rng.integers(0, 3000)) for _ in range(n_img)]
        if k == 0:
            sizes = list(SIZES)
        if sum(sizes) == 0:
            sizes[0] = 1
        P = 1 if k == 1 else int(rng.integers(1, 2001))
        pairs = rng.integers(0, len(sizes), (P, 2)).astype(np.int32)
        if k in (2, 5):                                    # one pair of 2^20 + 77 query rows, between other pairs
            sizes.append(LAUNCH_ROWS + 77)
            pairs = pairs[(pairs != len(sizes) - 1).all(axis=1)]
            pairs = np.concatenate([pairs[:3], [[len(sizes) - 1, 1]], pairs[3:]]).astype(np.int32)
        out.append((np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), pairs))
    return out


SETS = seeded_sets()


def test_the_sets_hold_what_they_should():
    assert any((np.diff(s) == LAUNCH_ROWS + 77).any() for s, _ in SETS) and any(len(p) == 1 for _, p in SETS) and any(len(p) > 1000 for _, p in SETS)
    assert set(SIZES) <= set(int(x) for s, _ in SETS for x in np.diff(s))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_cu", CUS)
def test_plan_properties(rules, kind, n_cu):
    assert rules.shim_launch_rows() == LAUNCH_ROWS
    qb, tile, fill_cu, per_cu = NUMBERS[kind]
    for seg, pairs in SETS:
        pl = plan(rules, kind, seg, pairs, n_cu)
        e, l, f = pl["e"], pl["l"], pl["f"]
        n = np.diff(seg)
        nq_p, nt_p = n[pairs[:, 0]], n[pairs[:, 1]]
        # row0 is the numpy cumulative sum, through the plan and through the function the API calls
        want_row0 = np.concatenate([[0], np.cumsum(nq_p)])
        assert np.array_equal(pl["row0"], want_row0)
        row0 = np.zeros(len(pairs) + 1, np.int64)
        rules.shim_batch_row_offsets(seg.ctypes.data_as(i64p), pairs.ctypes.data_as(i32p), len(pairs), row0.ctypes.data_as(i64p))
        assert np.array_equal(row0, want_row0)
        # every output row is covered by exactly one entry or fill: per pair, the ranges tile [row0[p], row0[p + 1]) in order
        starts = np.concatenate([e["out0"], f["out0"]])
        lens = np.concatenate([e["nq"], f["n"]])
        owner = np.concatenate([e["pair"], f["pair"]])
        order = np.lexsort((starts, owner))
        starts, lens, owner = starts[order], lens[order], owner[order]
        assert (lens >= 1).all()
        first_of_pair = np.concatenate([[True], owner[1:] != owner[:-1]])
        assert np.array_equal(starts[first_of_pair], want_row0[owner[first_of_pair]])
        same = owner[1:] == owner[:-1]
        assert np.array_equal((starts + lens)[:-1][same], starts[1:][same])
        last_of_pair = np.concatenate([first_of_pair[1:], [True]])
        assert np.array_equal((starts + lens)[last_of_pair], want_row0[owner[last_of_pair] + 1])
        # empty-query pairs have no entry and are on no list; empty-train pairs are on the fill list and have no entry
        has_entry, has_fill = np.isin(np.arange(len(pairs)), e["pair"]), np.isin(np.arange(len(pairs)), f["pair"])
        assert np.array_equal(has_entry, (nq_p > 0) & (nt_p > 0)) and np.array_equal(has_fill, (nq_p > 0) & (nt_p == 0))
        assert np.array_equal(f["n"], nq_p[f["pair"]]) and np.array_equal(f["first"], np.concatenate([[0], np.cumsum(f["n"])])[:-1])
        assert pl["fill_rows"] == f["n"].sum()
        # an entry's rows are rows of its pair's images
        a, b = pairs[e["pair"], 0], pairs[e["pair"], 1]
        assert np.array_equal(e["t0"], seg[b]) and np.array_equal(e["nt"], n[b])
        assert (e["q0"] >= seg[a]).all() and (e["q0"] + e["nq"] <= seg[a + 1]).all()
        assert np.array_equal(e["out0"] - want_row0[e["pair"]], e["q0"] - seg[a])
        assert np.array_equal(e["qblocks"], -(-e["nq"] // qb))
        # no slice is empty, and the slices cover the tiles
        tiles = -(-e["nt"] // tile)
        assert (e["tps"] >= 1).all() and (e["slices"] >= 1).all()
        assert ((e["slices"] - 1) * e["tps"] < tiles).all() and (e["slices"] * e["tps"] >= tiles).all()
        # launches: consecutive entries, at most 2^20 query rows, consistent and disjoint workgroup prefixes and partial offsets
        assert np.array_equal(l["e0"], np.concatenate([[0], np.cumsum(l["n"])])[:-1]) and l["n"].sum() == len(e["nq"])
        for k in range(len(l["e0"])):
            s_ = slice(int(l["e0"][k]), int(l["e0"][k] + l["n"][k]))
            nq, sl, qbl = e["nq"][s_], e["slices"][s_], e["qblocks"][s_]
            assert nq.sum() == l["rows"][k] <= LAUNCH_ROWS and qbl.sum() == l["qblocks"][k]
            wgs = qbl * sl
            assert np.array_equal(e["wg0"][s_], np.concatenate([[0], np.cumsum(wgs)])[:-1]) and wgs.sum() == l["wgs"][k] < 2 ** 31
            mw = np.where(sl > 1, -(-nq // 256), 0)
            assert np.array_equal(e["mwg0"][s_], np.concatenate([[0], np.cumsum(mw)])[:-1]) and mw.sum() == l["merge_wgs"][k]
            parts = np.where(sl > 1, sl * nq, 0)
            assert np.array_equal(e["part0"][s_], np.concatenate([[0], np.cumsum(parts)])[:-1]) and parts.sum() == l["parts"][k] <= pl["max_parts"]
            # the slices are the single call's rule with the launch's query blocks
            for j in range(s_.start, s_.stop, max(1, (s_.stop - s_.start) // 50)):
                tps = rules.shim_tiles_per_slice_of(int(l["qblocks"][k]), int(e["nt"][j]), n_cu, KINDS.index(kind))
                assert (tps, slices(int(e["nt"][j]), tps, kind)) == (e["tps"][j], e["slices"][j])
            # a launch with per_cu * n_cu query blocks merges nothing
            if l["qblocks"][k] >= per_cu * n_cu:
                assert (sl == 1).all() and l["merge_wgs"][k] == 0 and l["parts"][k] == 0
        # the figure dlco_desc_match_pairs_slices reports: the most slices of a pair's ranges, 0 for a pair without an entry
        want = np.zeros(len(pairs), np.int64)
        np.maximum.at(want, e["pair"], e["slices"])
        assert np.array_equal(pl["slices"], want)


def test_a_pair_of_more_than_a_launch_is_cut_into_row_ranges(rules):
    seg = np.array([0, 40, 40 + LAUNCH_ROWS + 77, 40 + LAUNCH_ROWS + 77 + 9], np.int64)
    pairs = np.array([[2, 0], [1, 0], [0, 2]], np.int32)
    for kind in KINDS:
        pl = plan(rules, kind, seg, pairs, 256)
        e, l = pl["e"], pl["l"]
        assert e["pair"].tolist() == [0, 1, 1, 2] and e["nq"].tolist() == [9, LAUNCH_ROWS, 77, 40]
        assert e["q0"].tolist() == [seg[2], 40, 40 + LAUNCH_ROWS, 0] and e["out0"].tolist() == [0, 9, 9 + LAUNCH_ROWS, 9 + LAUNCH_ROWS + 77]
        assert l["n"].tolist() == [1, 1, 2] and l["rows"].tolist() == [9, LAUNCH_ROWS, 117]


def test_one_pair_is_the_single_calls_rule(rules):
    """a batch of one pair slices train as dlco_desc_match does: the launch's query blocks are the call's"""
    for kind in KINDS:
        for nq, nt in ((2048, 2048), (300, 5000), (17, 5000), (5000, 300), (1, 1)):
            for n_cu in CUS:
                pl = plan(rules, kind, np.array([0, nq, nq + nt], np.int64), np.array([[0, 1]], np.int32), n_cu)
                tps = tiles_per_slice(nq, nt, n_cu, kind)
                assert (pl["e"]["tps"][0], pl["e"]["slices"][0], pl["slices"][0]) == (tps, slices(nt, tps, kind), slices(nt, tps, kind))


def test_the_single_call_rule_has_not_moved(rules):
    """the shapes tests/test_match_slices.py quotes, through the function that now calls the new one"""
    tps = rules.shim_tiles_per_slice(100000, 100000, 256, 1)
    assert (tps, rules.shim_slices(100000, tps, 1)) == (72, 11)
    tps = rules.shim_tiles_per_slice(100000, 100000, 256, 0)
    assert rules.shim_slices(100000, tps, 0) == 3
    assert rules.shim_tiles_per_slice(3000, 5000, 256, 0) == 4 and rules.shim_slices(5000, 4, 0) == 10
    assert (rules.shim_tiles_per_slice(4096, 6204, 256, 1), rules.shim_slices(6204, 2, 1)) == (2, 25)
    assert (rules.shim_tiles_per_slice(16384, 8252, 256, 1), rules.shim_slices(8252, 5, 1)) == (5, 13)
    assert rules.shim_tiles_per_slice(2048, 2048, 256, 0) == 1 and rules.shim_slices(2048, 1, 0) == 16
    for nq in (1, 255, 256, 257, 4096, 2 ** 20):
        for nt in (1, 127, 128, 129, 700, 6204, 100000, 2 ** 31 - 1):
            for n_cu in (1, 32, 64, 256, 304):
                for k, kind in enumerate(KINDS):
                    want = tiles_per_slice(nq, nt, n_cu, kind)
                    assert rules.shim_tiles_per_slice(nq, nt, n_cu, k) == want
                    assert rules.shim_tiles_per_slice_of(ceil_div(nq, NUMBERS[kind][0]), nt, n_cu, k) == want


def test_planner_under_address_and_undefined_sanitizers(tmp_path):
    """the stand-alone program walks the planner over seeded sets of the same kind with its own checks"""
    exe = tmp_path / "match_batch_asan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(SHIM, "match_batch_asan_main.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "match_batch_asan: ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
