"""CPU tests of the guided-matching rule (opencv-dlco_amd/csrc/guided_rules.hpp, through tests/shim/guided_rules_shim.cpp), and
the numpy restatement and the shared generator that the GPU tests (tests/test_guided_gpu.py) use as well.  The rule is IEEE
double + - x in a stated order, so every verdict is compared with equality.  Nothing here needs a GPU or libdlco.so."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_verify_rules import inliers_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim")
i32p, u8p, f32p, f64p = (C.POINTER(t) for t in (C.c_int32, C.c_uint8, C.c_float, C.c_double))
INF = np.float32(np.inf)
RADIUS = 12.0


# ---- the rule restated and the shared generator --------------------------------------------------------------------------------
def pair_mask(H, qxy, txy, radius, h_side=0):
    """P(i, j) [nq, nt] of the rule in numpy float64, one operation at a time in the stated order.  h_side 0: H applies to
    the query's point and the train point is compared; h_side 1: the roles swapped."""
    H = np.asarray(H, np.float64).reshape(9)
    q, t = (np.asarray(a, np.float32).astype(np.float64) for a in (qxy, txy))
    t2 = float(np.float32(radius)) * float(np.float32(radius))
    out = np.empty((len(q), len(t)), bool)
    step = max(1, (1 << 22) // max(1, len(t)))
    with np.errstate(all="ignore"):
        for i0 in range(0, len(q), step):
            qx, qy, tx, ty = q[i0:i0 + step, 0, None], q[i0:i0 + step, 1, None], t[None, :, 0], t[None, :, 1]
            (x, y, u, v) = (qx, qy, tx, ty) if h_side == 0 else (tx, ty, qx, qy)
            X = (H[0] * x + H[1] * y) + H[2]
            Y = (H[3] * x + H[4] * y) + H[5]
            W = (H[6] * x + H[7] * y) + H[8]
            ex, ey = X - u * W, Y - v * W
            out[i0:i0 + step] = (W > 0.0) & (ex * ex + ey * ey <= t2 * (W * W))
    return out


def case_model(nt):
    """the mild homography of the shared cases and the side S of their square"""
    S = 8.0 * math.sqrt(nt)
    return np.array([[0.98, -0.05, 0.03 * S], [0.04, 1.02, -0.02 * S], [0.02 / S, -0.01 / S, 1.0]]), S


def guided_case(nq, nt, seed=None):
    """(qxy [nq,2], txy [nt,2], H [3,3]) of the shared cases: keypoints uniform in [0, S)^2, S = 8 sqrt(nt), one per 64 px^2,
    drawn in the order train, query; radius RADIUS admits about seven train points a query.  Where nq >= 100 two rows are
    planted: query 1 at (-60 S, 0), where W < 0, and query 2 with a NaN coordinate: neither admits anything (h_side 0)."""
    rng = np.random.default_rng(1000 + nt if seed is None else seed)
    H, S = case_model(nt)
    txy = (rng.random((nt, 2)) * S).astype(np.float32)
    qxy = (rng.random((nq, 2)) * S).astype(np.float32)
    if nq >= 100:
        qxy[1] = (-60.0 * S, 0.0)
        qxy[2, 1] = np.nan
    return qxy, txy, H


def top2_of_masked(M):
    """(idx [n,2] int32, d [n,2] float32): the first two finite entries of every row of M (no NaN) under the (distance, index)
    key, -1 / +inf where a row has fewer.  argmin returns the first of equal minima, i.e. the smaller index."""
    M = np.array(M, np.float32)
    n = len(M)
    rows = np.arange(n)
    idx, d = np.empty((n, 2), np.int32), np.empty((n, 2), np.float32)
    for k in range(2):
        j = M.argmin(1)
        d[:, k] = M[rows, j]
        idx[:, k] = np.where(np.isfinite(d[:, k]), j, -1)
        M[rows, j] = INF
    return idx, np.where(idx >= 0, d, INF).astype(np.float32)


# (rho, v, c): fl(fl(c c) + v v) <= rho rho < fl(c c + v v), i.e. the rule admits and a fused multiply-add does not; the first
# is the documented one, the others came out of a random search with exact rationals
CONTRACTION = [("0x1.0dce68p+0", "0x1.745ep-2", "0x1.fa79b67f46790p-1"), ("0x1.60dfc2p+3", "0x1.14be84p+3", "0x1.b5def75aa6406p+2"),
               ("0x1.09ab24p+3", "0x1.a8d78ap+1", "0x1.e70731ea8e7afp+2"), ("0x1.ac3ad8p+2", "0x1.695166p+2", "0x1.cbb2380072370p+1")]


def contraction_pairs():
    """[(H [3,3], qxy [1,2], txy [1,2], radius)]: for every triple the pair with c in H[0][2] and the train point at (0, v), and
    the mirrored one with c in H[1][2] and the train point at (v, 0).  Each verdict is recomputed here with exact rationals:
    the rule admits, and an evaluation that fuses either product with the sum does not."""
    out = []
    for rho, v, c in (tuple(float.fromhex(s) for s in t) for t in CONTRACTION):
        assert float(np.float32(rho)) == rho and float(np.float32(v)) == v
        t2, v2 = Fraction(rho) ** 2, Fraction(v) ** 2
        assert Fraction(rho * rho) == t2 and Fraction(v * v) == v2          # both products are exact in double
        unfused = Fraction(float(Fraction(c) ** 2)) + v2                    # fl(c c) + v v, then one rounding
        assert float(unfused) <= rho * rho < float(Fraction(c) ** 2 + v2)
        for mirrored in (False, True):
            H = np.eye(3)
            H[1 if mirrored else 0, 2] = c
            out.append((H, np.zeros((1, 2), np.float32), np.array([(v, 0.0) if mirrored else (0.0, v)], np.float32), rho))
    return out


def boundary_pairs():
    """[(qxy [1,2], txy [1,2], k)] with H = I: integer points (3 k, 4 k) apart, so radius 5 k admits and the float below does not"""
    return [(np.array([(x, y)], np.float32), np.array([(x + 3 * k, y - 4 * k)], np.float32), k)
            for x, y, k in ((0, 0, 1), (100, 2000, 7), (-5000, 30, 1000), (1 << 19, 1 << 19, 1 << 17), (-(1 << 20), 1 << 20, 3))]


# ---- the header through the shim -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libguidedshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), os.path.join(SHIM, "guided_rules_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_guided_threshold_sq.argtypes, L.shim_guided_threshold_sq.restype = [C.c_float], C.c_double
    L.shim_guided_record.argtypes, L.shim_guided_record.restype = [f64p, C.c_double, C.c_double, C.c_double, f64p], None
    L.shim_guided_pairs.argtypes, L.shim_guided_pairs.restype = [f64p, C.c_double, f64p, f64p, f64p, f64p, C.c_int64, u8p, u8p], None
    L.shim_guided_mask.argtypes, L.shim_guided_mask.restype = [f64p, C.c_float, C.c_int32, f32p, C.c_int64, f32p, C.c_int64, u8p], None
    L.shim_guided_top2.argtypes = [f32p, f32p, C.c_int64, f32p, C.c_int64, f64p, C.c_float, C.c_int32, i32p, f32p]
    L.shim_guided_top2.restype = None
    return L


def shim_mask(L, H, qxy, txy, radius, h_side):
    H, qxy, txy = np.ascontiguousarray(H, np.float64), np.ascontiguousarray(qxy, np.float32), np.ascontiguousarray(txy, np.float32)
    mask = np.empty((len(qxy), len(txy)), np.uint8)
    L.shim_guided_mask(H.ctypes.data_as(f64p), radius, h_side, qxy.ctypes.data_as(f32p), len(qxy), txy.ctypes.data_as(f32p), len(txy), mask.ctypes.data_as(u8p))
    return mask.astype(bool)


SPECIAL = np.array([(np.nan, 3.0), (5.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (np.inf, np.inf), (2.0 ** 20, -2.0 ** 20), (-2.0 ** 20, 2.0 ** 20),
                    (2.0 ** 20, 2.0 ** 20), (0.0, 0.0)], np.float32)


@pytest.mark.parametrize("nq,nt", [(300, 500), (130, 129), (37, 2)])
@pytest.mark.parametrize("radius", [0.5, 12.0, 2.0 ** 20])
def test_admits_of_a_record_is_the_inlier_test_on_every_pair(rules, nq, nt, radius):
    qxy, txy, H = guided_case(nq, nt)
    S = case_model(nt)[1]
    qxy = np.concatenate([qxy, SPECIAL, [(-60.0 * S, 0.0), (-50.0 * S, 10.0)]]).astype(np.float32)       # W <= 0 among them
    txy = np.concatenate([txy, SPECIAL, [(-60.0 * S, 0.0)]]).astype(np.float32)
    t2 = rules.shim_guided_threshold_sq(radius)
    assert t2 == float(np.float32(radius)) ** 2
    for h_side in (0, 1):
        a, b = (qxy, txy) if h_side == 0 else (txy, qxy)                     # a: the side H applies to
        ia, ib = np.divmod(np.arange(len(a) * len(b)), len(b))
        cols = [np.ascontiguousarray(c, np.float64) for c in (a[ia, 0], a[ia, 1], b[ib, 0], b[ib, 1])]
        adm, inl = np.empty(len(ia), np.uint8), np.empty(len(ia), np.uint8)
        rules.shim_guided_pairs(np.ascontiguousarray(H).ctypes.data_as(f64p), t2, *[c.ctypes.data_as(f64p) for c in cols], len(ia), adm.ctypes.data_as(u8p),
                                inl.ctypes.data_as(u8p))
        want = inliers_ref(H.reshape(9), a[ia], b[ib], radius)
        assert np.array_equal(adm, inl) and np.array_equal(adm.astype(bool), want)
        grid = want.reshape(len(a), len(b))
        grid = grid if h_side == 0 else grid.T
        assert np.array_equal(pair_mask(H, qxy, txy, radius, h_side), grid)
        assert np.array_equal(shim_mask(rules, H, qxy, txy, radius, h_side), grid)
        if radius == 12.0 and nq >= 100:
            clean = grid[:nq, :nt]
            assert 4.0 <= clean.sum() / nq <= 10.0 and not clean[1].any() and not clean[2].any()
        # a NaN admits nothing and nothing admits it
        assert not grid[nq, :].any() and not grid[nq + 1, :].any() and not grid[:, nt].any() and not grid[:, nt + 1].any()
    # W <= 0 leaves T = -1, W > 0 leaves t2 (W W)
    rec = np.empty(4)
    rules.shim_guided_record(np.ascontiguousarray(H).ctypes.data_as(f64p), -60.0 * S, 0.0, t2, rec.ctypes.data_as(f64p))
    assert rec[2] < 0 and rec[3] == -1.0
    rules.shim_guided_record(np.ascontiguousarray(H).ctypes.data_as(f64p), 10.0, 20.0, t2, rec.ctypes.data_as(f64p))
    assert rec[2] > 0 and rec[3] == t2 * (rec[2] * rec[2])


def test_the_boundary_is_inclusive(rules):
    for qxy, txy, k in boundary_pairs():
        r_in = np.float32(5 * k)
        r_out = np.nextafter(r_in, np.float32(0))
        for h_side in (0, 1):
            assert shim_mask(rules, np.eye(3), qxy, txy, r_in, h_side).all() and pair_mask(np.eye(3), qxy, txy, r_in, h_side).all(), k
            assert not shim_mask(rules, np.eye(3), qxy, txy, r_out, h_side).any() and not pair_mask(np.eye(3), qxy, txy, r_out, h_side).any(), k


def test_a_fused_multiply_add_would_be_visible(rules):
    pairs = contraction_pairs()
    assert len(pairs) == 8
    for H, qxy, txy, rho in pairs:
        assert shim_mask(rules, H, qxy, txy, rho, 0).all() and pair_mask(H, qxy, txy, rho, 0).all()
        assert not shim_mask(rules, H, qxy, txy, np.nextafter(np.float32(rho), np.float32(0)), 0).any()


def test_host_top_two_against_numpy_on_a_masked_matrix(rules):
    for (nq, nt), radius in (((300, 500), 12.0), ((130, 129), 12.0), ((200, 300), 3.0), ((5, 1), 2.0 ** 20), ((37, 2), 12.0)):
        qxy, txy, H = guided_case(nq, nt)
        rng = np.random.default_rng(nq)
        D = rng.integers(0, 6, (nq, nt)).astype(np.float32) * np.float32(0.25)                         # ties everywhere
        for h_side in (0, 1):
            mask = pair_mask(H, qxy, txy, radius, h_side)
            per_row = mask.sum(1)
            if nq >= 100:
                assert (per_row == 0).any() and (per_row == 1).any() and (per_row >= 2).any()
            want_i, want_d = top2_of_masked(np.where(mask, D, INF))
            idx, d = np.full((nq, 2), -9, np.int32), np.full((nq, 2), -9, np.float32)
            rules.shim_guided_top2(D.ctypes.data_as(f32p), qxy.ctypes.data_as(f32p), nq, txy.ctypes.data_as(f32p), nt, np.ascontiguousarray(H).ctypes.data_as(f64p),
                                   radius, h_side, idx.ctypes.data_as(i32p), d.ctypes.data_as(f32p))
            assert np.array_equal(idx, want_i) and np.array_equal(d.view(np.uint32), want_d.view(np.uint32)), (nq, nt, h_side)
            assert ((idx[:, 0] == -1) == (per_row == 0)).all() and ((idx[:, 1] == -1) == (per_row <= 1)).all()


def test_the_shared_cases_admit_two_or_more_for_nine_queries_in_ten():
    for nq, nt in ((3000, 5000), (300, 500), (4100, 4100), (20000, 300), (130, 129), (3, 40000)):
        qxy, txy, H = guided_case(nq, nt)
        per_row = pair_mask(H, qxy, txy, RADIUS).sum(1)
        assert (per_row >= 2).mean() >= 0.9 and 5.0 <= per_row.mean() <= 9.0, (nq, nt, per_row.mean())


# ---- the header's host loop under the sanitizers, as a program of its own ------------------------------------------------------
def test_host_loop_under_address_and_undefined_sanitizers(tmp_path):
    exe = tmp_path / "guided_asan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(SHIM, "guided_asan_main.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "guided_asan: ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
