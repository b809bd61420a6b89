"""CPU tests of the epipolar guided-matching rule (opencv-dlco_amd/csrc/guided_epipolar_rules.hpp, through
tests/shim/guided_epipolar_rules_shim.cpp), and the numpy restatement and the shared cases that the GPU tests
(tests/test_guided_epipolar_gpu.py) use as well.  The rule is IEEE double + - x in a stated order, so every verdict is compared
with equality.  Nothing here needs a GPU or libdlco.so."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_epipolar_rules import inliers_ref
from test_guided_rules import INF, SPECIAL, case_model, guided_case, top2_of_masked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim")
i32p, u8p, f32p, f64p = (C.POINTER(t) for t in (C.c_int32, C.c_uint8, C.c_float, C.c_double))
THRESHOLD = 2.0
STEREO_F = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
# l0 = l1 = 1 and m0 = m1 = -1 for every point, so S is exactly 4, and e = (u - x) + (v - y)
BOUNDARY_F = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [-1.0, -1.0, 0.0]])
# the shapes of the GPU tests with 100 train rows or more
SHARED_SHAPES = ((3000, 5000), (300, 500), (4100, 4100), (20000, 300), (130, 129), (3, 40000), (1009, 700))


# ---- the rule restated and the shared cases ------------------------------------------------------------------------------------
def epi_mask(F, qxy, txy, threshold, f_side=0):
    """P(i, j) [nq, nt] of the rule in numpy float64, one operation at a time in the order of epipolar_rules::inlier.
    f_side 0: the query's point is src (x, y) and the train point dst (u, v); f_side 1: the roles swapped."""
    F = np.asarray(F, np.float64).reshape(9)
    q, t = (np.asarray(a, np.float32).astype(np.float64) for a in (qxy, txy))
    t2 = float(np.float32(threshold)) * float(np.float32(threshold))
    out = np.empty((len(q), len(t)), bool)
    step = max(1, (1 << 21) // max(1, len(t)))
    with np.errstate(all="ignore"):
        for i0 in range(0, len(q), step):
            qx, qy, tx, ty = q[i0:i0 + step, 0, None], q[i0:i0 + step, 1, None], t[None, :, 0], t[None, :, 1]
            (x, y, u, v) = (qx, qy, tx, ty) if f_side == 0 else (tx, ty, qx, qy)
            l0 = (F[0] * x + F[1] * y) + F[2]
            l1 = (F[3] * x + F[4] * y) + F[5]
            l2 = (F[6] * x + F[7] * y) + F[8]
            e = (u * l0 + v * l1) + l2
            m0 = (F[0] * u + F[3] * v) + F[6]
            m1 = (F[1] * u + F[4] * v) + F[7]
            S = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
            out[i0:i0 + step] = (S > 0.0) & (e * e <= t2 * S)
    return out


def case_F(nt):
    """the stated F of the shared cases: [e']x H_case with the epipole e' = (3 S, 0.4 S, 1), divided by its largest magnitude"""
    H, S = case_model(nt)
    ex, ey = 3.0 * S, 0.4 * S
    F = np.array([[0.0, -1.0, ey], [1.0, 0.0, -ex], [-ey, ex, 0.0]]) @ H
    return F / np.abs(F).max()


def epipolar_case(nq, nt):
    """(qxy, txy, F) of the shared cases: the keypoints of guided_case under case_F; THRESHOLD admits a band of train points"""
    qxy, txy, _ = guided_case(nq, nt)
    return qxy, txy, case_F(nt)


def boundary_pairs():
    """[(src [1,2], dst [1,2], k)] under BOUNDARY_F: integer points with e = 2 k, so threshold k admits (e e = 4 k k = t2 S) and the
    float below does not"""
    return [(np.array([(x, y)], np.float32), np.array([(x + 3 * k, y - k)], np.float32), k)
            for x, y, k in ((0, 0, 1), (100, 2000, 7), (-5000, 30, 1000), (1 << 19, 1 << 19, 1 << 17), (-(1 << 20), 1 << 20, 3))]


# F = [0 0 a; 0 0 b; -a -b 0] and the src point (0, 0): l = (a, b, 0) and m = (-a, -b).  Found by a random search with exact
# rationals.  S-tuples (t, u, a, b), dst point (u, 0); E-tuples (t, u, v, a, b), dst point (u, v).
S_TUPLES = [("0x1.75aad2p+2", "0x1.69dd98p+3", "0x1.b1756ad9b2596p-1", "0x1.959de09e4ca16p-1"),
            ("0x1.7d7776p+2", "0x1.bea292p+3", "0x1.30a853f8970fbp-1", "0x1.9211a8cb55ba2p-1"),
            ("0x1.894096p+1", "0x1.ae3a9p+2", "0x1.b7c2324562c87p-2", "0x1.03965238b838bp-1"),
            ("0x1.756b36p+2", "0x1.45a136p+4", "0x1.9fc7bd360041fp-2", "0x1.d4b78653117dbp-1")]
E_TUPLES = [("0x1.c28028p+2", "0x1.1bb6f4p+4", "-0x1.80ec42p+2", "0x1.7ad075c040849p-1", "0x1.345f99714a57cp-1"),
            ("0x1.e62fep+2", "0x1.797a42p+4", "0x1.d5e7a8p+0", "0x1.78a6942995809p-2", "0x1.c57f3f626ac56p-1"),
            ("0x1.ca1dfp+2", "0x1.b145aep+4", "-0x1.a72cfcp+2", "0x1.efb44c4256333p-2", "0x1.61c2abbeec2f4p-1"),
            ("0x1.7151f2p+0", "0x1.54c30ep+1", "0x1.2e8374p-1", "0x1.8c57e266fdd94p-2", "0x1.1194ccba2bb26p-1")]


def _fl(x):
    """the double nearest the rational x (ties to even), as a rational again: one IEEE rounding"""
    return Fraction(float(x))


def _verdict(t, u, v, a, b, fuse):
    """the rule on the tuple with exact rationals and explicit roundings.  fuse names the products that are not rounded before
    their sum: 'L0' / 'L1' the first / second product of L = l0 l0 + l1 l1, 'S' the products m0 m0 and m1 m1 as well as L's
    first, 'E0' / 'E1' the first / second product of u l0 + v l1; '' is the rule itself."""
    t, u, v, a, b = (Fraction(z) for z in (t, u, v, a, b))
    l0, l1, l2 = a, b, Fraction(0)                                            # (0 + 0) + a and so on: exact
    p0 = l0 * l0 if fuse in ("L0", "S") else _fl(l0 * l0)
    p1 = l1 * l1 if fuse == "L1" else _fl(l1 * l1)
    L = _fl(p0 + p1)
    A, B = ((-a) * (-a), (-b) * (-b)) if fuse == "S" else (_fl(a * a), _fl(b * b))
    S = _fl(_fl(L + A) + B)
    e0 = u * l0 if fuse == "E0" else _fl(u * l0)
    e1 = v * l1 if fuse == "E1" else _fl(v * l1)
    e = _fl(_fl(e0 + e1) + l2)
    return S > 0 and _fl(e * e) <= _fl(_fl(t * t) * S)


def contraction_pairs():
    """[(F [3,3], src [1,2], dst [1,2], t)] of the S- and the E-tuples.  Each verdict is recomputed here with exact rationals:
    the rule admits; an evaluation that fuses a product of L with its sum (either one), or every product of S, rejects the
    S-tuples, and one that fuses either product of u l0 + v l1 rejects the E-tuples."""
    out = []
    for tup, fused in ([(s[:2] + ("0x0p+0",) + s[2:], ("L0", "L1", "S")) for s in S_TUPLES] + [(e, ("E0", "E1")) for e in E_TUPLES]):
        t, u, v, a, b = (float.fromhex(s) for s in tup)
        assert all(float(np.float32(z)) == z for z in (t, u, v))
        assert _verdict(t, u, v, a, b, ""), tup
        for f in fused:
            assert not _verdict(t, u, v, a, b, f), (tup, f)
        out.append((np.array([[0.0, 0.0, a], [0.0, 0.0, b], [-a, -b, 0.0]]), np.zeros((1, 2), np.float32), np.array([(u, v)], np.float32), t))
    return out


# ---- the header through the shim -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libguidedepishim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(SHIM, "guided_epipolar_rules_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_epi_threshold_sq.argtypes, L.shim_epi_threshold_sq.restype = [C.c_float], C.c_double
    L.shim_epi_src_record.argtypes, L.shim_epi_src_record.restype = [f64p, C.c_double, C.c_double, f64p], None
    L.shim_epi_dst_record.argtypes, L.shim_epi_dst_record.restype = [f64p, C.c_double, C.c_double, f64p], None
    L.shim_epi_pairs.argtypes, L.shim_epi_pairs.restype = [f64p, C.c_double, f64p, f64p, f64p, f64p, C.c_int64, u8p, u8p], None
    L.shim_epi_mask.argtypes, L.shim_epi_mask.restype = [f64p, C.c_float, C.c_int32, f32p, C.c_int64, f32p, C.c_int64, u8p], None
    L.shim_epi_top2.argtypes = [f32p, f32p, C.c_int64, f32p, C.c_int64, f64p, C.c_float, C.c_int32, i32p, f32p]
    L.shim_epi_top2.restype = None
    return L


def shim_mask(L, F, qxy, txy, threshold, f_side):
    F, qxy, txy = np.ascontiguousarray(F, np.float64), np.ascontiguousarray(qxy, np.float32), np.ascontiguousarray(txy, np.float32)
    mask = np.empty((len(qxy), len(txy)), np.uint8)
    L.shim_epi_mask(F.ctypes.data_as(f64p), threshold, f_side, qxy.ctypes.data_as(f32p), len(qxy), txy.ctypes.data_as(f32p), len(txy), mask.ctypes.data_as(u8p))
    return mask.astype(bool)


@pytest.mark.parametrize("nq,nt", [(300, 500), (130, 129), (37, 2)])
@pytest.mark.parametrize("model", ["generic", "stereo", "zero"])
@pytest.mark.parametrize("threshold", [0.5, 2.0, 2.0 ** 20])
def test_admits_of_the_two_records_is_the_inlier_test_on_every_pair(rules, nq, nt, model, threshold):
    qxy, txy, F = epipolar_case(nq, nt)
    F = np.ascontiguousarray({"generic": F, "stereo": STEREO_F, "zero": np.zeros((3, 3))}[model])
    qxy = np.concatenate([qxy, SPECIAL]).astype(np.float32)
    txy = np.concatenate([txy, SPECIAL]).astype(np.float32)
    t2 = rules.shim_epi_threshold_sq(threshold)
    assert t2 == float(np.float32(threshold)) ** 2
    for f_side in (0, 1):
        a, b = (qxy, txy) if f_side == 0 else (txy, qxy)                     # a: src, the side F applies to
        ia, ib = np.divmod(np.arange(len(a) * len(b)), len(b))
        cols = [np.ascontiguousarray(c, np.float64) for c in (a[ia, 0], a[ia, 1], b[ib, 0], b[ib, 1])]
        adm, inl = np.empty(len(ia), np.uint8), np.empty(len(ia), np.uint8)
        rules.shim_epi_pairs(F.ctypes.data_as(f64p), t2, *[c.ctypes.data_as(f64p) for c in cols], len(ia), adm.ctypes.data_as(u8p), inl.ctypes.data_as(u8p))
        want = inliers_ref(F.reshape(9), a[ia], b[ib], threshold)
        assert np.array_equal(adm, inl) and np.array_equal(adm.astype(bool), want)
        grid = want.reshape(len(a), len(b))
        grid = grid if f_side == 0 else grid.T
        assert np.array_equal(epi_mask(F, qxy, txy, threshold, f_side), grid)
        assert np.array_equal(shim_mask(rules, F, qxy, txy, threshold, f_side), grid)
        # the transpose: the tables swapped and the other side see the same set
        assert np.array_equal(shim_mask(rules, F, txy, qxy, threshold, 1 - f_side), grid.T)
        if model == "zero":
            assert not grid.any()                                            # S = 0 admits nothing
        if model == "generic":
            assert grid[:nq, :nt].any()
            # a NaN admits nothing and nothing admits it
            assert not grid[nq, :].any() and not grid[nq + 1, :].any() and not grid[:, nt].any() and not grid[:, nt + 1].any()
            if nq >= 100:
                assert not grid[2, :].any()                                  # the planted NaN query of guided_case
    # the records hold what the rule says
    x, y = 10.0, 20.0
    s, d = np.empty(4), np.empty(4)
    rules.shim_epi_src_record(F.ctypes.data_as(f64p), x, y, s.ctypes.data_as(f64p))
    rules.shim_epi_dst_record(F.ctypes.data_as(f64p), x, y, d.ctypes.data_as(f64p))
    f = F.reshape(9)
    l0, l1, l2 = (f[0] * x + f[1] * y) + f[2], (f[3] * x + f[4] * y) + f[5], (f[6] * x + f[7] * y) + f[8]
    m0, m1 = (f[0] * x + f[3] * y) + f[6], (f[1] * x + f[4] * y) + f[7]
    assert s.tolist() == [l0, l1, l2, l0 * l0 + l1 * l1] and d.tolist() == [x, y, m0 * m0, m1 * m1]


def test_side_1_with_swapped_tables_is_the_transpose(rules):
    for nq, nt in ((300, 500), (130, 129)):
        qxy, txy, F = epipolar_case(nq, nt)
        for f_side in (0, 1):
            m = epi_mask(F, qxy, txy, THRESHOLD, f_side)
            assert np.array_equal(epi_mask(F, txy, qxy, THRESHOLD, 1 - f_side), m.T)
            assert np.array_equal(shim_mask(rules, F, txy, qxy, THRESHOLD, 1 - f_side), m.T)
        assert not np.array_equal(epi_mask(F, qxy, txy, THRESHOLD, 0), epi_mask(F, qxy, txy, THRESHOLD, 1))        # the sides differ


def test_the_boundary_is_inclusive_and_exact(rules):
    for src, dst, k in boundary_pairs():
        t_in = np.float32(k)
        t_out = np.nextafter(t_in, np.float32(0))
        # in exact arithmetic: S = 4, e = 2 k, e e = 4 k k
        x, y, u, v = (Fraction(float(z)) for z in (src[0, 0], src[0, 1], dst[0, 0], dst[0, 1]))
        assert (u - x) + (v - y) == 2 * k and 4 * k * k <= Fraction(float(t_in)) ** 2 * 4 and 4 * k * k > Fraction(float(t_out)) ** 2 * 4
        # src on the query side with f_side 0, on the train side with f_side 1
        for qxy, txy, f_side in ((src, dst, 0), (dst, src, 1)):
            assert shim_mask(rules, BOUNDARY_F, qxy, txy, t_in, f_side).all() and epi_mask(BOUNDARY_F, qxy, txy, t_in, f_side).all(), k
            assert not shim_mask(rules, BOUNDARY_F, qxy, txy, t_out, f_side).any() and not epi_mask(BOUNDARY_F, qxy, txy, t_out, f_side).any(), k


def test_a_fused_multiply_add_would_be_visible(rules):
    pairs = contraction_pairs()
    assert len(pairs) == 8
    for F, src, dst, t in pairs:
        for qxy, txy, f_side in ((src, dst, 0), (dst, src, 1)):
            assert shim_mask(rules, F, qxy, txy, t, f_side).all() and epi_mask(F, qxy, txy, t, f_side).all()


def test_host_top_two_against_numpy_on_a_masked_matrix(rules):
    for (nq, nt), threshold in (((300, 500), 2.0), ((130, 129), 2.0), ((200, 300), 0.05), ((5, 1), 2.0 ** 20), ((37, 2), 2.0)):
        qxy, txy, F = epipolar_case(nq, nt)
        F = np.ascontiguousarray(F)
        rng = np.random.default_rng(nq)
        D = rng.integers(0, 6, (nq, nt)).astype(np.float32) * np.float32(0.25)                         # ties everywhere
        for f_side in (0, 1):
            mask = epi_mask(F, qxy, txy, threshold, f_side)
            per_row = mask.sum(1)
            if threshold == 0.05:
                assert (per_row == 0).any() and (per_row == 1).any() and (per_row >= 2).any()
            want_i, want_d = top2_of_masked(np.where(mask, D, INF))
            idx, d = np.full((nq, 2), -9, np.int32), np.full((nq, 2), -9, np.float32)
            rules.shim_epi_top2(D.ctypes.data_as(f32p), qxy.ctypes.data_as(f32p), nq, txy.ctypes.data_as(f32p), nt, F.ctypes.data_as(f64p), threshold, f_side,
                                idx.ctypes.data_as(i32p), d.ctypes.data_as(f32p))
            assert np.array_equal(idx, want_i) and np.array_equal(d.view(np.uint32), want_d.view(np.uint32)), (nq, nt, f_side)
            assert ((idx[:, 0] == -1) == (per_row == 0)).all() and ((idx[:, 1] == -1) == (per_row <= 1)).all()


def test_the_shared_cases_admit_two_or_more_for_nine_queries_in_ten():
    for nq, nt in SHARED_SHAPES:
        qxy, txy, F = epipolar_case(nq, nt)
        for f_side in (0, 1):
            mask = epi_mask(F, qxy, txy, THRESHOLD, f_side)
            per_row = mask.sum(1)
            assert (per_row >= 2).mean() >= 0.9 and not mask.all(), (nq, nt, f_side, (per_row >= 2).mean())
            if nq >= 100:
                assert per_row[2] == 0                                       # the planted NaN query


# ---- the header's host loop under the sanitizers, as a program of its own ------------------------------------------------------
def test_host_loop_under_address_and_undefined_sanitizers(tmp_path):
    exe = tmp_path / "guided_epipolar_asan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(SHIM, "guided_epipolar_asan_main.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "guided_epipolar_asan: ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
