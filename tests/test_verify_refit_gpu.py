"""The refit round on the device, alone: refit_pairs_kernel through dlco_desc_verify_pairs_refit_round on masks of the test's.
The contract is equality in every bit, the `ok` flag included, with verify_rules::refit_round and epipolar_rules::refit_round
on the host (tests/shim/verify_rules_shim.cpp, epipolar_rules_shim.cpp) and with their numpy restatements
(test_verify_rules.refit_round_ref, test_epipolar_rules.refit_round_ref).  The rule's sums run over the inliers in ascending
index and the kernel stages its matches in chunks of C = verify_rules::kRefitChunk, so the inlier counts and positions sit around
C; the device's double sqrt and division must be the host's, which these tests are the first to run.  All pairs go in one batch,
so that every pair has neighbours; the same pairs alone, as batches of one, show that no pair depends on them."""
import ctypes as C

import numpy as np
import pytest

import test_epipolar_rules as E
import test_verify_refit_rules as R
import test_verify_rules as V
from test_verify_rules import bits

pytestmark = pytest.mark.gpu
f32p, f64p, u8p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_uint8))


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    return V.build_shim(tmp_path_factory), E.build_shim(tmp_path_factory), R.build_shim(tmp_path_factory)


def first_mask(shim, fundamental, src, dst):
    """the mask of the best hypothesis of the CPU frame: what the first round of a verify call refits on"""
    if fundamental:
        return E.shim_fundamental(shim, src, dst, threshold=1.0, n_hyp=65, seed=5, refine=0)["mask"]
    return V.shim_verify(shim, src, dst, threshold=3.0, n_hyp=65, seed=5, refine=0)["mask"]


def at(m, idx):
    k = np.zeros(m, bool)
    k[list(idx)] = True
    return k


def cases(fundamental, shim, chunk):
    """(name, src, dst, mask) of one model's batch"""
    c, few = chunk, 8 if fundamental else 4
    planted = (lambda m, seed: E.planted_case(m, 0 if m < 32 else 0.3, seed, sigma=0.5)[:2]) if fundamental else \
              (lambda m, seed: V.planted_case(m, 0 if m < 16 else 0.5, seed)[:2])
    out = []
    for m in (few, c - 1, c, c + 1, 3 * c + 7):
        s, d = planted(m, 100 + m)
        out.append(("planted%d first mask" % m, s, d, first_mask(shim, fundamental, s, d)))
        out.append(("planted%d all" % m, s, d, np.ones(m, bool)))
    m = 3 * c + 7
    s, d = planted(m, 7)
    ends = [c - 1, 2 * c - 1, 3 * c - 1, m - 1]
    hole, late = np.ones(m, bool), np.ones(m, bool)
    hole[c:2 * c], late[:c] = False, False
    hand = [("last of every chunk", at(m, ends)), ("last two of every chunk", at(m, ends + [e - 1 for e in ends])), ("a chunk without an inlier", hole),
            ("first inlier at C", late), ("first inlier at C, %d inliers" % few, at(m, range(c, c + few))),
            ("%d inliers" % few, at(m, [0, c - 1, c, m - 1] + ([1, 2 * c, 2 * c + 1, 3 * c] if fundamental else []))),
            ("7 inliers", at(m, [0, 1, c - 1, c, 2 * c, 2 * c + 1, 3 * c])), ("no inlier", at(m, []))]
    out += [(name, s, d, k) for name, k in hand]
    full = lambda name, sd: (name, sd[0], sd[1], np.ones(len(sd[0]), bool))
    out += [full("point", E.point_case()), full("collinear", V.collinear_case()), full("nan masked in", E.nan_case() if fundamental else V.nan_case()[:2]),
            full("far", E.far_case() if fundamental else V.far_case()), full("stereo", E.stereo_case()), full("translation", V.translation_case())]
    s, d = E.nan_case() if fundamental else V.nan_case()[:2]
    out.append(("nan masked out", s, d, ~at(len(s), E.NAN_ROWS)))
    return out


def jacobi_sweeps(shim, src, dst, mask):
    """the sweeps that rotated in the 9 x 9 Jacobi of an accepted round of the fundamental matrix, N summed as the rule sums it"""
    src, dst = src.astype(np.float64), dst.astype(np.float64)
    sel = np.flatnonzero(mask)
    ps, pd = [tuple(map(float, p)) for p in src[sel]], [tuple(map(float, p)) for p in dst[sel]]
    (cxs, cys, ss), (cxd, cyd, sd) = V._hartley(ps), V._hartley(pd)
    N = np.zeros((9, 9))
    for (px, py), (pu, pv) in zip(ps, pd):
        x, y, u, v = (px - cxs) * ss, (py - cys) * ss, (pu - cxd) * sd, (pv - cyd) * sd
        a = np.array([u * x, u * y, u, v * x, v * y, v, x, y, 1.0])
        N = N + np.outer(a, a)
    return E.shim_jacobi(shim, N)[2]


_batch = {}


def batch(fundamental, shims):
    """(cases, the host's rounds through the shim, the numpy restatement's), computed once"""
    if fundamental not in _batch:
        shim = shims[1] if fundamental else shims[0]
        cs = cases(fundamental, shim, shims[2].shim_refit_chunk())
        call, ref = (shim.shim_epipolar_refit_round, E.refit_round_ref) if fundamental else (shim.shim_verify_refit_round, V.refit_round_ref)
        host, restated = [], []
        for _, s, d, k in cs:
            M = np.zeros(9)
            s, d = np.ascontiguousarray(s, np.float32), np.ascontiguousarray(d, np.float32)
            ok = call(s.ctypes.data_as(f32p), d.ctypes.data_as(f32p), len(s), k.astype(np.uint8).ctypes.data_as(u8p), M.ctypes.data_as(f64p))
            host.append(M if ok else None)
            restated.append(ref(s, d, k))
        _batch[fundamental] = (cs, host, restated)
    return _batch[fundamental]


def check(name, M, ok, want):
    if want is None:
        assert not ok and not bits(M).any(), name
    else:
        assert ok and np.array_equal(bits(M).reshape(9), bits(want)), (name, M.reshape(9), want)


@pytest.mark.parametrize("fundamental", [False, True])
def test_a_round_of_the_kernel_is_the_hosts_round_in_every_bit(ctx, shims, fundamental):
    cs, host, restated = batch(fundamental, shims)
    # conditions on the references, before the device is asked
    for (name, _, _, _), h, r in zip(cs, host, restated):
        assert (h is None) == (r is None) and (h is None or np.array_equal(bits(h), bits(r))), name
    assert sum(h is not None for h in host) >= 10 and sum(h is None for h in host) >= 3
    rejected = {name for (name, _, _, _), h in zip(cs, host) if h is None}
    assert {"no inlier", "point"} <= rejected and ("7 inliers" in rejected) == fundamental and ("collinear" in rejected or fundamental)
    if fundamental:
        assert any(h is not None and jacobi_sweeps(shims[1], s, d, k) >= 2 for (_, s, d, k), h in zip(cs, host))
    M, ok = ctx.verify_pairs_refit_round([(s, d) for _, s, d, _ in cs], [k for _, _, _, k in cs], fundamental)
    assert M.shape == (len(cs), 3, 3) and ok.shape == (len(cs),) and ctx.last_kernel_ms() > 0
    for p, ((name, _, _, _), h) in enumerate(zip(cs, host)):
        check(name, M[p], ok[p], h)


@pytest.mark.parametrize("fundamental", [False, True])
def test_a_pair_alone_gives_what_it_gives_among_neighbours(ctx, shims, fundamental):
    cs, host, _ = batch(fundamental, shims)
    for (name, s, d, k), h in zip(cs, host):
        M, ok = ctx.verify_pairs_refit_round([(s, d)], [k], fundamental)
        check(name, M[0], ok[0], h)


@pytest.mark.parametrize("fundamental", [False, True])
def test_pairs_below_the_sample_are_rejected(ctx, shims, fundamental):
    cs, host, _ = batch(fundamental, shims)
    few = 8 if fundamental else 4
    (name, s, d, k), h = cs[1], host[1]
    empty = (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    lists = [empty, (s[:few - 1], d[:few - 1]), (s, d), empty]
    M, ok = ctx.verify_pairs_refit_round(lists, [np.zeros(0, bool), np.ones(few - 1, bool), k, np.zeros(0, bool)], fundamental)
    assert ok.tolist() == [False, False, h is not None, False] and not bits(M[[0, 1, 3]]).any()
    check(name, M[2], ok[2], h)
