"""CPU tests of the quantiser (opencv-dlco_amd/csrc/quant_rules.hpp, through tests/shim/quant_rules_shim.cpp) against its numpy
float32 restatement, and of the integer twins of the match tool's filters (opencv-dlco_amd/csrc/select_rules.hpp, through
tests/shim/match_rules_u8_shim.cpp).  Nothing here needs a GPU or libdlco.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def quantize_ref(Y, scale, offset=None):
    """The rule in numpy float32: t = y - o, v = t * s (each rounded to float), rint (half to even), NaN -> 0, clipped."""
    Y = np.asarray(Y, np.float32)
    o = np.zeros(Y.shape[1], np.float32) if offset is None else np.asarray(offset, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((Y - o).astype(np.float32) * np.float32(scale)).astype(np.float32)
        q = np.rint(v)
    return np.where(np.isnan(v), 0, np.clip(q, 0, 255)).astype(np.uint8)


def fit_ref(Y):
    Y = np.asarray(Y, np.float32)
    o = Y.min(0)
    R = np.float32((Y.max(0) - o).astype(np.float32).max())
    return (np.float32(1) if R == 0 else np.float32(255) / R), o


def _compile(tmp_path_factory, name, src):
    out = tmp_path_factory.mktemp("shim") / name
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), os.path.join(ROOT, "tests", "shim", src)])
    return C.CDLL(str(out))


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    L = _compile(tmp_path_factory, "libquantshim.so", "quant_rules_shim.cpp")
    L.shim_quant_one.argtypes = [C.c_float, C.c_float, C.c_float]
    L.shim_quantize.argtypes = [f32p, C.c_int64, C.c_int, C.c_float, f32p, u8p]
    L.shim_quantize.restype = None
    L.shim_quant_fit.argtypes = [f32p, C.c_int64, C.c_int, C.POINTER(C.c_float), f32p]
    return L


def quantize(L, Y, scale, offset=None):
    Y = np.ascontiguousarray(Y, np.float32)
    out = np.full(Y.shape, 77, np.uint8)
    o = None if offset is None else np.ascontiguousarray(offset, np.float32)
    L.shim_quantize(Y.ctypes.data_as(f32p), Y.shape[0], Y.shape[1], scale, None if o is None else o.ctypes.data_as(f32p), out.ctypes.data_as(u8p))
    return out


def fit(L, Y):
    Y = np.ascontiguousarray(Y, np.float32)
    s, o = C.c_float(), np.zeros(Y.shape[1], np.float32)
    ok = L.shim_quant_fit(Y.ctypes.data_as(f32p), Y.shape[0], Y.shape[1], C.byref(s), o.ctypes.data_as(f32p))
    return (np.float32(s.value), o) if ok else None


def test_stated_cases(rules):
    one = rules.shim_quant_one
    inf, nan = float("inf"), float("nan")
    # o = 0, s = 1: v is y itself.  Half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert [one(v, 0.0, 1.0) for v in (0.5, 1.5, 2.5, -0.4, 255.5, inf, -inf, nan)] == [0, 2, 2, 0, 255, 255, 0, 0]
    assert [one(v, 0.0, 1.0) for v in (254.5, 254.49, 255.0, 256.0, 1e30, -1e30, 0.0, -0.0, 3.5)] == [254, 254, 255, 255, 255, 0, 0, 0, 4]
    # the offset is subtracted first, then the scale: (5 - 3) * 10
    assert one(5.0, 3.0, 10.0) == 20 and one(3.0, 5.0, 10.0) == 0
    # inf - inf and 0 * inf are NaN: 0
    assert one(inf, inf, 1.0) == 0


def test_the_product_is_not_fused_with_the_subtraction(rules):
    """t = y - o is rounded to float before the product: on a table with small offsets the twice-rounded restatement and a
    once-rounded (y - o) s in double differ on some bytes, and the rule sides with the restatement on all of them."""
    rng = np.random.default_rng(5)
    y = rng.uniform(0, 1, (500000, 8)).astype(np.float32)
    o = rng.uniform(-1, 1, 8).astype(np.float32) * np.float32(1e-3)
    s = np.float32(254.73)
    want = quantize_ref(y, s, o)
    once = np.clip(np.rint((y.astype(np.float64) - o.astype(np.float64)) * np.float64(s)), 0, 255).astype(np.uint8)
    print("bytes on which a single rounding differs: %d" % (once != want).sum())
    assert (once != want).any()                              # the case can tell the two apart
    assert np.array_equal(quantize(rules, y, s, o), want)


def test_the_rule_equals_the_numpy_restatement_on_a_random_table(rules):
    rng = np.random.default_rng(1)
    Y = (rng.standard_normal((700, 67)) * 0.3).astype(np.float32)
    Y[3, 5], Y[9, 0], Y[11, 66] = np.nan, np.inf, -np.inf
    o = (rng.standard_normal(67) * 0.1 - 0.8).astype(np.float32)
    for s in (np.float32(100.0), np.float32(311.7), np.float32(1e-3)):
        got = quantize(rules, Y, s, o)
        assert np.array_equal(got, quantize_ref(Y, s, o)), float(s)
    assert quantize(rules, Y, 100.0, o)[3, 5] == 0 and quantize(rules, Y, 100.0, o)[9, 0] == 255 and quantize(rules, Y, 100.0, o)[11, 66] == 0
    # no offsets: zeros
    assert np.array_equal(quantize(rules, Y, 50.0), quantize_ref(Y, 50.0))
    # values on the half-way points
    H = (np.arange(0, 600, dtype=np.float32) * np.float32(0.5) - 20).reshape(-1, 4)
    assert np.array_equal(quantize(rules, H, 1.0), quantize_ref(H, 1.0))


def test_fit_of_a_stated_table(rules):
    Y = np.array([[1.0, -2.0, 5.0], [3.0, -2.5, 5.0], [2.0, 1.5, 5.0]], np.float32)
    s, o = fit(rules, Y)
    assert o.tolist() == [1.0, -2.5, 5.0]                    # the minima
    assert s == np.float32(255.0) / np.float32(4.0)          # ranges 2, 4, 0: R = 4
    assert quantize(rules, Y, s, o).tolist() == [[0, 32, 0], [128, 0, 0], [64, 255, 0]]      # 0.5 * 63.75 = 31.875, 63.75 -> 64, 127.5 -> 128
    # R == 0: s = 1
    s, o = fit(rules, np.full((4, 3), 7.25, np.float32))
    assert s == 1.0 and o.tolist() == [7.25] * 3
    s, o = fit(rules, np.array([[2.0, -1.0]], np.float32))   # one row
    assert s == 1.0 and o.tolist() == [2.0, -1.0]
    # a non-finite entry: no quantiser
    for bad in (np.nan, np.inf, -np.inf):
        Z = Y.copy()
        Z[1, 2] = bad
        assert fit(rules, Z) is None


def test_fit_equals_the_restatement_and_its_own_sample_never_clamps(rules):
    rng = np.random.default_rng(2)
    for n, r, sc in ((500, 64, 0.25), (33, 128, 40.0), (2, 5, 1e-6), (1000, 3, 1e6)):
        Y = (rng.standard_normal((n, r)) * sc + rng.standard_normal(r) * sc).astype(np.float32)
        s, o = fit(rules, Y)
        s_ref, o_ref = fit_ref(Y)
        assert s == s_ref and np.array_equal(o, o_ref)
        with np.errstate(over="ignore"):
            q = np.rint(((Y - o).astype(np.float32) * s).astype(np.float32))
        assert q.min() == 0 and q.max() == 255              # nothing below 0 or above 255 before the clamp
        u = quantize(rules, Y, s, o)
        assert np.array_equal(u, q.astype(np.uint8)) and u.min() == 0 and u.max() == 255


# ---- the integer twins of the match filters -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mrules(tmp_path_factory):
    L = _compile(tmp_path_factory, "libmatchu8shim.so", "match_rules_u8_shim.cpp")
    L.shim_match_ratio_keep_i32.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_float]
    L.shim_match_select_i32.argtypes = [C.c_int64, C.c_int32, i32p, i32p, C.c_int, C.c_float, i32p, i32p, i32p]
    L.shim_match_select_i32.restype = C.c_int64
    return L


def keep_ref(d1, d2, idx2, f):
    return idx2 == -1 or float(d1) < float(np.float32(f)) * float(np.float32(f)) * float(d2)


def select_ref(nearest, sqdist, ratio=None, back=None):
    """(pairs, dists): the two rules restated; shared with the GPU test of the tools."""
    pairs, dists = [], []
    for i, ((j, j2), (d1, d2)) in enumerate(zip(np.asarray(nearest).tolist(), np.asarray(sqdist).tolist())):
        if j < 0:
            continue
        if ratio is not None and not keep_ref(d1, d2, j2, ratio):
            continue
        if back is not None and int(back[j][0]) != i:
            continue
        pairs.append([i, j])
        dists.append(d1)
    return np.array(pairs, np.int32).reshape(-1, 2), np.array(dists, np.int32)


def select(L, nearest, sqdist, ratio=None, back=None):
    nearest = np.ascontiguousarray(nearest, np.int32).reshape(-1, 2)
    sqdist = np.ascontiguousarray(sqdist, np.int32).reshape(-1, 2)
    nq = len(nearest)
    pairs, dists = np.full((max(nq, 1), 2), -99, np.int32), np.full(max(nq, 1), -99, np.int32)
    b = None if back is None else np.ascontiguousarray(back, np.int32)
    nt = len(b) if b is not None else int(nearest.max(initial=0)) + 1      # the back table's rows, else above every index used
    m = L.shim_match_select_i32(nq, nt, nearest.ctypes.data_as(i32p), sqdist.ctypes.data_as(i32p), 0 if ratio is None else 1,
                                1.0 if ratio is None else ratio, None if b is None else b.ctypes.data_as(i32p),
                                pairs.ctypes.data_as(i32p), dists.ctypes.data_as(i32p))
    return pairs[:m], dists[:m]


def test_integer_ratio_rule(mrules):
    keep = mrules.shim_match_ratio_keep_i32
    # f = 0.5: f^2 d2 = 25 exactly: d1 == f^2 d2 is dropped, one below is kept
    assert keep(25, 100, 7, 0.5) == 0 and keep(24, 100, 7, 0.5) == 1 and keep(26, 100, 7, 0.5) == 0
    # no second neighbour: kept whatever the distances
    assert keep(5, 2 ** 31 - 1, -1, 0.5) == 1 and keep(0, 0, -1, 0.5) == 1
    # d1 = d2 = 0: dropped; f = 1: kept iff strictly nearer
    assert keep(0, 0, 3, 0.8) == 0 and keep(7, 7, 3, 1.0) == 0 and keep(7, 8, 3, 1.0) == 1
    # the largest distances: no overflow, the product is formed in double
    big = 66585600
    assert keep(big - 1, big, 3, 1.0) == 1 and keep(int(0.64 * big) + 2, big, 3, 0.8) == 0 and keep(int(0.64 * big), big, 3, 0.8) == 1
    rng = np.random.default_rng(3)
    for d1, d2, f in zip(rng.integers(0, 70000, 500), rng.integers(0, 70000, 500), rng.uniform(0.05, 1.0, 500)):
        assert keep(int(d1), int(d2), 1, float(f)) == int(keep_ref(int(d1), int(d2), 1, f))


def test_integer_select_agrees_with_the_restatement(mrules):
    rng = np.random.default_rng(4)
    nq, nt = 400, 90
    nearest = np.stack([rng.integers(0, nt, nq), rng.integers(0, nt, nq)], 1).astype(np.int32)
    d1 = rng.integers(0, 5000, nq)
    sqdist = np.stack([d1, d1 + rng.integers(0, 5000, nq)], 1).astype(np.int32)
    nearest[5] = (-1, -1)                                    # no usable neighbour: never a match
    nearest[6, 1] = -1                                       # no second: passes the ratio rule
    sqdist[7] = (2500, 10000)                                # d1 == f^2 d2 at f = 0.5: dropped
    back = np.stack([rng.integers(0, nq, nt), rng.integers(0, nq, nt)], 1).astype(np.int32)
    back[nearest[::3, 0], 0] = np.arange(nq)[::3]            # make a good share of them mutual
    for ratio, b in ((None, None), (0.5, None), (0.8, None), (None, back), (0.8, back), (1.0, back)):
        p, d = select(mrules, nearest, sqdist, ratio, b)
        wp, wd = select_ref(nearest, sqdist, ratio, b)
        assert np.array_equal(p, wp) and np.array_equal(d, wd), (ratio, b is not None)
        assert len(p) == 0 or (np.diff(p[:, 0]) > 0).all()
    p, _ = select(mrules, nearest, sqdist, 0.5)
    assert 6 in p[:, 0] and 7 not in p[:, 0] and 5 not in p[:, 0]
    assert len(select(mrules, np.zeros((0, 2)), np.zeros((0, 2)))[0]) == 0
