"""CPU tests of the guided arguments of the batch plan (opencv-dlco_amd/csrc/match_batch.hpp, through
tests/shim/match_batch_guided_shim.cpp, which this file builds): how dlco_desc_match_pairs_guided* lays out the records of a
launch, closes a launch at a record limit and routes a pair without a model to the fill list.  Without a Guide the plan is
today's, field for field.  Nothing here needs a GPU or libdlco.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_match_batch_rules import E_FIELDS, F_FIELDS, KINDS, L_FIELDS, LAUNCH_ROWS, SETS, plan as plain_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim")
i64p, i32p, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
GL_FIELDS = L_FIELDS + ("rec_rows",)
O_FIELDS = ("rec0", "nqrec", "ntrec")
FORMS = ((False, 0), (False, 1), (True, 0), (True, 1))      # (records on both sides, the homography's side)


@pytest.fixture(scope="module")
def plain_rules(tmp_path_factory):
    """the shim of tests/test_match_batch_rules.py, for plan() of that file: today's plan"""
    out = tmp_path_factory.mktemp("shim") / "libmatchbatchshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), os.path.join(SHIM, "match_batch_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_batch_plan.argtypes, L.shim_batch_plan.restype = [C.c_int, i64p, i32p, C.c_int64, C.c_int], C.c_void_p
    L.shim_batch_free.argtypes, L.shim_batch_free.restype = [C.c_void_p], None
    L.shim_batch_count.argtypes, L.shim_batch_count.restype = [C.c_void_p, C.c_int], C.c_int64
    for name in ("entries", "launches", "fills", "row0"):
        f = getattr(L, "shim_batch_" + name)
        f.argtypes, f.restype = [C.c_void_p, i64p], None
    L.shim_batch_slices.argtypes, L.shim_batch_slices.restype = [C.c_void_p, i32p], None
    return L


@pytest.fixture(scope="module")
def guided(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libmatchbatchguidedshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), os.path.join(SHIM, "match_batch_guided_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_record_rows.restype = C.c_int64
    L.shim_guided_plan.argtypes = [C.c_int, i64p, i32p, C.c_int64, C.c_int, C.c_int, u8p, C.c_int, C.c_int, C.c_int64, C.c_int64]
    L.shim_guided_plan.restype = C.c_void_p
    L.shim_guided_free.argtypes, L.shim_guided_free.restype = [C.c_void_p], None
    L.shim_guided_count.argtypes, L.shim_guided_count.restype = [C.c_void_p, C.c_int], C.c_int64
    for name in ("entries", "launches", "fills", "offsets", "row0"):
        f = getattr(L, "shim_guided_" + name)
        f.argtypes, f.restype = [C.c_void_p, i64p], None
    L.shim_guided_slices.argtypes, L.shim_guided_slices.restype = [C.c_void_p, i32p], None
    return L


def gplan(L, kind, seg, pairs, n_cu, guide=None):
    """the plan as dicts of int64 columns; guide: None (plan() as the plain batch calls it) or a dict of no_model [n_pairs] or
    None, both, side, rec_limit, launch_rows (0: the library's)"""
    seg, pairs = np.ascontiguousarray(seg, np.int64), np.ascontiguousarray(pairs, np.int32)
    g = guide or {}
    nm = None if g.get("no_model") is None else np.ascontiguousarray(g["no_model"], np.uint8)
    h = L.shim_guided_plan(KINDS.index(kind), seg.ctypes.data_as(i64p), pairs.ctypes.data_as(i32p), len(pairs), n_cu, 0 if guide is None else 1,
                           None if nm is None else nm.ctypes.data_as(u8p), int(g.get("both", False)), g.get("side", 0), g.get("rec_limit", 0),
                           g.get("launch_rows", 0))
    try:
        def table(what, fn, fields):
            a = np.zeros((L.shim_guided_count(h, what), len(fields)), np.int64)
            fn(h, a.ctypes.data_as(i64p))
            return {f: a[:, k] for k, f in enumerate(fields)}
        row0, sl = np.zeros(len(pairs) + 1, np.int64), np.zeros(len(pairs), np.int32)
        L.shim_guided_row0(h, row0.ctypes.data_as(i64p))
        L.shim_guided_slices(h, sl.ctypes.data_as(i32p))
        return dict(e=table(0, L.shim_guided_entries, E_FIELDS), l=table(1, L.shim_guided_launches, GL_FIELDS), f=table(2, L.shim_guided_fills, F_FIELDS),
                    o=table(5, L.shim_guided_offsets, O_FIELDS), row0=row0, slices=sl, fill_rows=L.shim_guided_count(h, 3),
                    max_parts=L.shim_guided_count(h, 4), max_rec_rows=L.shim_guided_count(h, 6))
    finally:
        L.shim_guided_free(h)


def same_plan(a, b, launch_fields=L_FIELDS):
    return all(np.array_equal(a["e"][f], b["e"][f]) for f in E_FIELDS) and all(np.array_equal(a["l"][f], b["l"][f]) for f in launch_fields) and \
        all(np.array_equal(a["f"][f], b["f"][f]) for f in F_FIELDS) and np.array_equal(a["row0"], b["row0"]) and np.array_equal(a["slices"], b["slices"]) and \
        a["fill_rows"] == b["fill_rows"] and a["max_parts"] == b["max_parts"]


def random_sets(n, seed=20241020):
    """a few hundred small segment tables: 2 to 9 images of 0 to 700 rows, 1 to 60 pairs"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        sizes = [int(rng.choice((0, 1, 15, 16, 17, 127, 128, 129, 257, 700))) if rng.integers(2) else int(rng.integers(0, 400)) for _ in range(int(rng.integers(2, 10)))]
        if sum(sizes) == 0:
            sizes[0] = 1
        P = 1 if k == 0 else int(rng.integers(1, 61))
        out.append((np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), rng.integers(0, len(sizes), (P, 2)).astype(np.int32)))
    return out


def test_without_the_guide_the_plan_is_todays(guided, plain_rules):
    """field for field what tests/shim/match_batch_shim.cpp returns, on the sets of tests/test_match_batch_rules.py; and a Guide
    that flags nothing under the library's limits moves nothing but the record layout it adds"""
    assert guided.shim_record_rows() == 2 ** 22
    for kind in KINDS:
        for n_cu in (1, 256):
            for seg, pairs in SETS:
                want = plain_plan(plain_rules, kind, seg, pairs, n_cu)
                got = gplan(guided, kind, seg, pairs, n_cu)
                assert same_plan(got, want)
                assert len(got["o"]["rec0"]) == 0 and got["max_rec_rows"] == 0 and (got["l"]["rec_rows"] == 0).all()
    for seg, pairs in random_sets(40):
        want = gplan(guided, "float", seg, pairs, 256)
        for both, side in FORMS:
            got = gplan(guided, "float", seg, pairs, 256, dict(both=both, side=side, no_model=np.zeros(len(pairs), np.uint8)))
            assert same_plan(got, want)                    # 2^22 record rows are never reached here


@pytest.mark.parametrize("both,side", FORMS)
def test_record_layout_limits_and_fills_under_shrunken_limits(guided, both, side):
    REC, ROWS = 64, 256
    rng = np.random.default_rng(7 + 2 * both + side)
    lone = cut = closed_by_records = 0
    for seg, pairs in random_sets(300):
        n = np.diff(seg)
        flags = (rng.random(len(pairs)) < 0.2).astype(np.uint8)
        pl = gplan(guided, "float", seg, pairs, 256, dict(both=both, side=side, no_model=flags, rec_limit=REC, launch_rows=ROWS))
        e, l, f, o = pl["e"], pl["l"], pl["f"], pl["o"]
        nq_p, nt_p = n[pairs[:, 0]], n[pairs[:, 1]]
        # flagged pairs land in fills and nowhere else; the other pairs are where the plain plan puts them
        has_entry, has_fill = np.isin(np.arange(len(pairs)), e["pair"]), np.isin(np.arange(len(pairs)), f["pair"])
        assert np.array_equal(has_fill, (nq_p > 0) & ((nt_p == 0) | (flags != 0)))
        assert np.array_equal(has_entry, (nq_p > 0) & (nt_p > 0) & (flags == 0))
        assert np.array_equal(f["n"], nq_p[f["pair"]]) and np.array_equal(f["out0"], pl["row0"][f["pair"]]) and pl["fill_rows"] == f["n"].sum()
        assert np.array_equal(f["first"], np.concatenate([[0], np.cumsum(f["n"])])[:-1])
        # every output row of a pair with an entry is covered once, in order
        for p in np.nonzero(has_entry)[0]:
            k = np.nonzero(e["pair"] == p)[0]
            assert np.array_equal(e["out0"][k], pl["row0"][p] + np.concatenate([[0], np.cumsum(e["nq"][k])])[:-1]) and e["nq"][k].sum() == nq_p[p]
            assert np.array_equal(e["q0"][k] - seg[pairs[p, 0]], e["out0"][k] - pl["row0"][p]) and (e["t0"][k] == seg[pairs[p, 1]]).all()
            if len(k) > 1:                                 # a cut pair: full ranges, then the rest; each range has the train records again
                cut += 1
                assert (e["nq"][k][:-1] == ROWS).all() and (o["ntrec"][k] == (nt_p[p] if both or side else 0)).all()
        # the record layout: the guide offsets are indexed like the entries
        assert len(o["rec0"]) == len(e["nq"])
        assert np.array_equal(o["nqrec"], e["nq"] if both or side == 0 else 0 * e["nq"])
        assert np.array_equal(o["ntrec"], e["nt"] if both or side == 1 else 0 * e["nt"])
        rows = o["nqrec"] + o["ntrec"]
        assert (rows >= 1).all()
        assert np.array_equal(l["e0"], np.concatenate([[0], np.cumsum(l["n"])])[:-1]) and l["n"].sum() == len(e["nq"]) and (l["n"] >= 1).all()
        for k in range(len(l["e0"])):
            s_ = slice(int(l["e0"][k]), int(l["e0"][k] + l["n"][k]))
            # the ranges of a launch's entries are disjoint, in order, and fill the launch's buffer exactly
            assert np.array_equal(o["rec0"][s_], np.concatenate([[0], np.cumsum(rows[s_])])[:-1]) and rows[s_].sum() == l["rec_rows"][k] <= pl["max_rec_rows"]
            # both limits are respected, the record limit except by a lone entry
            assert e["nq"][s_].sum() == l["rows"][k] <= ROWS
            assert l["rec_rows"][k] <= REC or l["n"][k] == 1
            lone += l["rec_rows"][k] > REC
            # a launch is closed only when the next entry would not fit
            if k + 1 < len(l["e0"]):
                nxt = int(l["e0"][k + 1])
                by_rows, by_rec = l["rows"][k] + e["nq"][nxt] > ROWS, l["rec_rows"][k] + rows[nxt] > REC
                assert by_rows or by_rec
                closed_by_records += by_rec and not by_rows
            # workgroups, merge workgroups and partials are prefixes within the launch, the slices those of the launch's query blocks
            wgs = e["qblocks"][s_] * e["slices"][s_]
            assert np.array_equal(e["wg0"][s_], np.concatenate([[0], np.cumsum(wgs)])[:-1]) and wgs.sum() == l["wgs"][k]
            assert e["qblocks"][s_].sum() == l["qblocks"][k]
        assert pl["max_rec_rows"] == (l["rec_rows"].max() if len(l["e0"]) else 0)
        tiles = -(-e["nt"] // 128)
        assert ((e["slices"] - 1) * e["tps"] < tiles).all() and (e["slices"] * e["tps"] >= tiles).all()          # no slice is empty
    assert lone > 0 and cut > 0 and closed_by_records > 0, "the sets are unfit: %d lone entries above the limit, %d cut pairs, %d launches closed by records" % (
        lone, cut, closed_by_records)


def test_a_cut_pair_under_the_librarys_limits(guided):
    """2^20 + 77 queries against 40 train rows between two small pairs: two ranges in two launches, each with its own records"""
    seg = np.array([0, 40, 40 + LAUNCH_ROWS + 77, 40 + LAUNCH_ROWS + 77 + 9], np.int64)
    pairs = np.array([[2, 0], [1, 0], [0, 2]], np.int32)
    for both, side in FORMS:
        pl = gplan(guided, "float", seg, pairs, 256, dict(both=both, side=side))
        e, l, o = pl["e"], pl["l"], pl["o"]
        assert e["pair"].tolist() == [0, 1, 1, 2] and e["nq"].tolist() == [9, LAUNCH_ROWS, 77, 40] and l["n"].tolist() == [1, 1, 2]
        q, t = both or side == 0, both or side == 1
        assert o["nqrec"].tolist() == [9 * q, LAUNCH_ROWS * q, 77 * q, 40 * q] and o["ntrec"].tolist() == [40 * t, 40 * t, 40 * t, 9 * t]
        assert o["rec0"].tolist() == [0, 0, 0, 77 * q + 40 * t]
        assert l["rec_rows"].tolist() == [9 * q + 40 * t, LAUNCH_ROWS * q + 40 * t, 117 * q + 49 * t] and pl["max_rec_rows"] == max(LAUNCH_ROWS * q + 40 * t, 117 * q + 49 * t)


def test_planner_and_record_indexing_under_address_and_undefined_sanitizers(tmp_path):
    """the stand-alone program walks the same kind of plans and replays the record kernel's index arithmetic over every record row"""
    exe = tmp_path / "match_batch_guided_asan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(SHIM, "match_batch_guided_asan_main.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "match_batch_guided_asan: ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
