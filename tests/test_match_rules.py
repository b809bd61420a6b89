"""CPU tests of the match tool's filters (the rule of opencv-dlco_amd/csrc/select_rules.hpp on one pair, through
tests/shim/match_rules_shim.cpp): Lowe's ratio test stated on squared distances, the mutual (cross) check, both together.
Nothing here needs a GPU or libdlco.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libmatchshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(ROOT, "tests", "shim", "match_rules_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_match_ratio_keep.argtypes = [C.c_float, C.c_float, C.c_int32, C.c_float]
    L.shim_match_select.argtypes = [C.c_int64, C.c_int32, i32p, f32p, C.c_int, C.c_float, i32p, i32p, f32p]
    L.shim_match_select.restype = C.c_int64
    return L


def select(L, nearest, sqdist, ratio=None, back=None):
    nearest = np.ascontiguousarray(nearest, np.int32).reshape(-1, 2)
    sqdist = np.ascontiguousarray(sqdist, np.float32).reshape(-1, 2)
    nq = len(nearest)
    pairs, dists = np.full((max(nq, 1), 2), -99, np.int32), np.full(max(nq, 1), -99, np.float32)
    b = None if back is None else np.ascontiguousarray(back, np.int32)
    nt = len(b) if b is not None else int(nearest.max(initial=0)) + 1      # the back table's rows, else above every index used
    m = L.shim_match_select(nq, nt, nearest.ctypes.data_as(i32p), sqdist.ctypes.data_as(f32p), 0 if ratio is None else 1,
                            1.0 if ratio is None else ratio, None if b is None else b.ctypes.data_as(i32p),
                            pairs.ctypes.data_as(i32p), dists.ctypes.data_as(f32p))
    return pairs[:m], dists[:m]


def test_ratio_rule_at_the_boundary(rules):
    keep = rules.shim_match_ratio_keep
    # f = 0.5: f^2 = 0.25 exactly, so d1 == f^2 d2 is representable: dropped (strict), one ulp below is kept
    assert keep(0.25, 1.0, 7, 0.5) == 0
    assert keep(float(np.nextafter(np.float32(0.25), np.float32(0))), 1.0, 7, 0.5) == 1
    assert keep(float(np.nextafter(np.float32(0.25), np.float32(1))), 1.0, 7, 0.5) == 0
    # the comparison is in double on the float f: 0.8f squared times d2, not a float product
    f = np.float32(0.8)
    lim = float(f) * float(f) * 3.0
    below, above = np.float32(lim), np.nextafter(np.float32(lim), np.float32(10))
    if float(below) >= lim:
        below = np.nextafter(below, np.float32(0))
    assert keep(float(below), 3.0, 1, float(f)) == 1 and keep(float(above), 3.0, 1, float(f)) == 0
    # no second neighbour: kept whatever the distances
    assert keep(5.0, float("inf"), -1, 0.5) == 1 and keep(0.0, 0.0, -1, 0.5) == 1
    # d1 = d2 = 0 (an exact repeat in train): 0 < 0 is false
    assert keep(0.0, 0.0, 3, 0.8) == 0 and keep(0.0, 0.0, 3, 1.0) == 0
    # f = 1: kept iff strictly nearer
    assert keep(1.0, 1.0, 3, 1.0) == 0 and keep(1.0, float(np.nextafter(np.float32(1), np.float32(2))), 3, 1.0) == 1


# five queries against four train rows; queries 1 and 3 share the nearest train row 2, whose own nearest query is 3
NEAREST = [[0, 1], [2, 0], [3, 2], [2, 3], [1, 0]]
SQDIST = [[1.0, 8.0], [2.0, 2.5], [0.5, 4.0], [1.0, 9.0], [3.0, 3.0]]
BACK = [[0, 4], [4, 0], [3, 1], [0, 2]]          # train row -> (nearest query, second); row 3's nearest query is 0, not 2


def test_plain_selection_lists_every_query_in_order(rules):
    p, d = select(rules, NEAREST, SQDIST)
    assert p.tolist() == [[0, 0], [1, 2], [2, 3], [3, 2], [4, 1]]
    assert d.tolist() == [1.0, 2.0, 0.5, 1.0, 3.0]


def test_ratio_selection(rules):
    p, d = select(rules, NEAREST, SQDIST, ratio=0.8)         # 0.64 d2: 5.12, 1.6, 2.56, 5.76, 1.92
    assert p.tolist() == [[0, 0], [2, 3], [3, 2]] and d.tolist() == [1.0, 0.5, 1.0]


def test_mutual_selection_with_a_shared_nearest_row(rules):
    p, d = select(rules, NEAREST, SQDIST, back=BACK)
    # query 1 loses train row 2 to query 3; query 2's row 3 prefers query 0
    assert p.tolist() == [[0, 0], [3, 2], [4, 1]] and d.tolist() == [1.0, 1.0, 3.0]


def test_both_rules_together(rules):
    p, d = select(rules, NEAREST, SQDIST, ratio=0.8, back=BACK)
    assert p.tolist() == [[0, 0], [3, 2]] and d.tolist() == [1.0, 1.0]
    assert (np.diff(p[:, 0]) > 0).all()


def test_an_empty_result_is_valid(rules):
    p, d = select(rules, NEAREST, SQDIST, ratio=0.1)
    assert p.shape == (0, 2) and d.shape == (0,)
    p, d = select(rules, [[0, -1]], [[2.0, INF]], back=[[-1, -1]])       # nobody's nearest
    assert len(p) == 0
    p, d = select(rules, np.zeros((0, 2)), np.zeros((0, 2)))
    assert len(p) == 0


def test_a_single_train_row_passes_the_ratio_rule(rules):
    p, d = select(rules, [[0, -1], [0, -1]], [[2.0, INF], [7.0, INF]], ratio=0.5, back=[[0, 1]])
    assert p.tolist() == [[0, 0]] and d.tolist() == [2.0]
