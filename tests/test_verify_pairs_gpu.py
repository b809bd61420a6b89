"""Batched verification on a GPU: dlco_desc_verify_pairs_* over one segmented match list.  Both rules are IEEE double arithmetic
in a stated order and integer counts, a hypothesis depends on (seed, h, m) and its pair's own matches only, so every pair's
answer in a batch is compared byte for byte with a loop of the single calls (ctx.verify_homography, ctx.verify_fundamental and
their _hypotheses forms), and with the numpy restatements of tests/test_verify_rules.py and tests/test_epipolar_rules.py.  A
single call is a batch of one pair on the same kernels, so the loop shows that a pair's answer does not depend on its
neighbours and no more; the independent yardsticks are the numpy restatements and, where those would take too long, the C++
host frame verify_rules::verify_host<Model> on the CPU (tests/shim/verify_batch_shim.cpp)."""
import ctypes as C

import numpy as np
import pytest

import test_epipolar_rules as E
import test_verify_batch_rules as B
import test_verify_rules as V
from test_verify_rules import bits

pytestmark = pytest.mark.gpu
f32p, f64p, i64p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int64))
MODELS = ("homography", "fundamental")
SETTINGS = dict(threshold=0.75, n_hyp=65, seed=5, refine=8)
EMPTY = (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))


class Model:
    """the calls, the restatement and the planted cases of one model"""
    def __init__(self, ctx, name):
        f = name == "fundamental"
        self.name, self.sample, self.key = name, 8 if f else 4, "F" if f else "H"
        self.single, self.batch = (ctx.verify_fundamental, ctx.verify_pairs_fundamental) if f else (ctx.verify_homography, ctx.verify_pairs_homography)
        self.single_hyp, self.batch_hyp = ((ctx.verify_fundamental_hypotheses, ctx.verify_pairs_fundamental_hypotheses) if f else
                                           (ctx.verify_hypotheses, ctx.verify_pairs_hypotheses))
        self.ref = E.fundamental_ref if f else V.verify_ref
        self.call = ctx.L.dlco_desc_verify_pairs_fundamental if f else ctx.L.dlco_desc_verify_pairs_homography

    def planted(self, m, seed=None):
        seed = 10 + m if seed is None else seed
        return (E.planted_case(m, 0 if m < 32 else 0.3, seed, sigma=0.5) if self.name == "fundamental" else V.planted_case(m, 0 if m < 16 else 0.5, seed))[:2]


_main = {}


def main_batch(name):
    """(names, lists, restated answers or None for a pair below the sample) of the issue's main batch, computed once"""
    if name not in _main:
        if name == "fundamental":
            sizes = (0, 7, 8, 9, 17, 63, 64, 65, 255, 257, 300, 775)
            lists = [E.planted_case(m, 0 if m < 32 else 0.3, 10 + m, sigma=0.5)[:2] for m in sizes] + [E.stereo_case(), E.point_case(), E.nan_case()]
            names = ["planted%d" % m for m in sizes] + ["stereo", "point", "nan"]
            want = [E.fundamental_ref(s, d, **SETTINGS) if len(s) >= 8 else None for s, d in lists]
        else:
            sizes = (0, 3, 4, 5, 9, 63, 255, 256, 257, 300, 775)
            lists = [V.planted_case(m, 0 if m < 16 else 0.5, 10 + m)[:2] for m in sizes] + [V.collinear_case(), V.translation_case(), V.nan_case()[:2], V.far_case()]
            names = ["planted%d" % m for m in sizes] + ["collinear", "translation", "nan", "far"]
            want = [V.verify_ref(s, d, **SETTINGS) if len(s) >= 4 else None for s, d in lists]
        _main[name] = (names, lists, want)
    return _main[name]


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_frame(tmp_path_factory):
    return B.build_shim(tmp_path_factory)


def same_triple(a, b):
    """two (M [3,3], inlier [m] bool, best_hyp): every bit"""
    return np.array_equal(bits(a[0]), bits(b[0])) and a[1].dtype == b[1].dtype == bool and np.array_equal(a[1], b[1]) and a[2] == b[2]


def no_model(t, m):
    return t[0].shape == (3, 3) and not bits(t[0]).any() and t[1].shape == (m,) and not t[1].any() and t[2] == -1


def loop(M, lists, **kw):
    """the single call on every pair; the documented "no model" for a pair below the sample, which the single call refuses"""
    return [M.single(s, d, **kw) if len(s) >= M.sample else (np.zeros((3, 3)), np.zeros(len(s), bool), -1) for s, d in lists]


def check_against_loop(M, lists, **kw):
    got, want = M.batch(lists, **kw), loop(M, lists, **kw)
    assert len(got) == len(lists)
    for p, (g, w) in enumerate(zip(got, want)):
        assert same_triple(g, w), (M.name, p, len(lists[p][0]), kw)
    return got


def check_against_restatement(M, got, lists, want):
    for p, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert no_model(g, len(lists[p][0])), p
        else:
            assert np.array_equal(bits(g[0]).reshape(9), bits(w[M.key])) and np.array_equal(g[1], w["mask"]) and g[2] == w["best"], (M.name, p)


def check_against_host_frame(M, rules, got, lists, pairs, threshold, n_hyp, seed, refine):
    """the pairs `pairs` of a batch's answers against the whole rule in C++ on the CPU, which runs no kernel"""
    for p in pairs:
        s, d = lists[p]
        if len(s) < M.sample:
            assert no_model(got[p], len(s)), (M.name, p)
            continue
        w = B.shim_whole_rule(rules, M.name == "fundamental", s, d, threshold, n_hyp, seed, refine)
        g = got[p]
        assert np.array_equal(bits(g[0]).reshape(9), bits(w["M"])) and np.array_equal(g[1], w["mask"]) and g[2] == w["best"], (M.name, p, len(s))


# ---- the main batch: pairs that leave the lockstep refit at different rounds -----------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_main_batch(ctx, name):
    M = Model(ctx, name)
    names, lists, want = main_batch(name)
    # conditions on the restatement, not on the code under test: the batch holds what it should
    rounds = [len(w["rounds"]) if w else 0 for w in want]
    assert len(set(rounds)) >= (4 if name == "fundamental" else 5), rounds
    assert any(w is not None and w["best"] == -1 for w in want)
    assert all(w["count"] >= 10 for n, w in zip(names, want) if n.startswith("planted") and int(n[7:]) >= 63)
    assert sum(w is None for w in want) == 2 and len(lists[0][0]) == 0
    got = check_against_loop(M, lists, **SETTINGS)
    check_against_restatement(M, got, lists, want)
    assert ctx.last_kernel_ms() > 0
    # the hypotheses form
    M_all, count = M.batch_hyp(lists, SETTINGS["threshold"], SETTINGS["n_hyp"], SETTINGS["seed"])
    assert M_all.shape == (len(lists), 65, 3, 3) and count.shape == (len(lists), 65) and count.dtype == np.int32
    for p, ((s, d), w) in enumerate(zip(lists, want)):
        if w is None:
            assert not bits(M_all[p]).any() and not count[p].any()
            continue
        one_M, one_count = M.single_hyp(s, d, SETTINGS["threshold"], SETTINGS["n_hyp"], SETTINGS["seed"])
        assert np.array_equal(bits(M_all[p]), bits(one_M)) and np.array_equal(count[p], one_count), p
        assert np.array_equal(bits(M_all[p]).reshape(65, 9), bits(w[M.key + "_all"])) and np.array_equal(count[p], w["counts"]), p
    assert ctx.last_kernel_ms() > 0


# ---- the borders of the grids ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 255, 256, 257, 300])
def test_grid_borders(ctx, name, n_hyp):
    M = Model(ctx, name)
    chunk = 256                                                              # verify_rules::kScoreChunk, asserted by tests/test_verify_gpu.py's shim
    lists = [M.planted(m, m) for m in (chunk - 1, chunk, chunk + 1, 3 * chunk + 7)]
    got = check_against_loop(M, lists, threshold=1.5, n_hyp=n_hyp, seed=3, refine=2)
    want = [M.ref(s, d, threshold=1.5, n_hyp=n_hyp, seed=3, refine=2) for s, d in lists]
    check_against_restatement(M, got, lists, want)
    M_all, count = M.batch_hyp(lists, 1.5, n_hyp, 3)
    for p, (s, d) in enumerate(lists):
        one_M, one_count = M.single_hyp(s, d, 1.5, n_hyp, 3)
        assert np.array_equal(bits(M_all[p]), bits(one_M)) and np.array_equal(count[p], one_count), p
        assert np.array_equal(count[p], want[p]["counts"])


def test_the_score_chunk_is_what_the_borders_assume(tmp_path_factory):
    assert V.build_shim(tmp_path_factory).shim_verify_score_chunk() == 256


# ---- no result depends on the other pairs, on their order, or on the run ----------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_independence(ctx, name):
    M = Model(ctx, name)
    _, lists, want = main_batch(name)
    first = M.batch(lists, **SETTINGS)
    check_against_restatement(M, first, lists, want)
    back = M.batch(lists[::-1], **SETTINGS)[::-1]
    again = M.batch(lists, **SETTINGS)
    k = 9                                                                    # a pair that refits for several rounds, three times in a batch
    repeated = M.batch(lists[:4] + [lists[k]] + lists[4:] + [lists[k]], **SETTINGS)
    assert len(want[k]["rounds"]) >= 3
    for p in range(len(lists)):
        assert same_triple(first[p], back[p]) and same_triple(first[p], again[p]), p
        assert same_triple(first[p], repeated[p if p < 4 else p + 1]), p
    assert same_triple(repeated[4], first[k]) and same_triple(repeated[-1], first[k])
    for p, (s, d) in enumerate(lists):                                       # a batch of one is the single call
        one = M.batch([(s, d)], **SETTINGS)
        assert len(one) == 1 and same_triple(one[0], first[p]), p
        if len(s) >= M.sample:
            assert same_triple(one[0], M.single(s, d, **SETTINGS)), p
    no_refit = dict(SETTINGS, refine=0)
    got = check_against_loop(M, lists, **no_refit)
    check_against_restatement(M, got, lists, [M.ref(s, d, **no_refit) if w else None for (s, d), w in zip(lists, want)])


# ---- more than one launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_several_launches(ctx, dlco, host_frame, name):
    M = Model(ctx, name)
    lists = [M.planted(12, 40 + k) for k in range(5)]
    launch = dlco.verify_pairs_launches(np.arange(6) * 12, 2 ** 20, name == "fundamental")
    assert launch.max() >= 1 and launch.tolist() == sorted(launch.tolist()) and launch.min() == 0
    kw = dict(threshold=1.5, n_hyp=2 ** 20, seed=7, refine=2)
    got = check_against_loop(M, lists, **kw)
    # The host frame on the first pair of every launch, as verify_pairs_launches numbers them.  All five pairs took the frame
    # 1.0 s for the homography and 10.2 s for the fundamental matrix (about 2 s a pair) on one CPU core: over ten seconds for
    # the two models together, so not all five.
    firsts = [p for p in range(len(lists)) if p == 0 or launch[p] != launch[p - 1]]
    assert len(firsts) == launch.max() + 1 >= 2
    check_against_host_frame(M, host_frame, got, lists, firsts, **kw)


# ---- many small pairs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_many_small_pairs(ctx, host_frame, name):
    M = Model(ctx, name)
    lists = [M.planted(4 + k % 37, 1000 + k) for k in range(600)]
    assert {len(s) for s, _ in lists} == set(range(4, 41))
    kw = dict(threshold=1.5, n_hyp=65, seed=11, refine=2)
    got = check_against_loop(M, lists, **kw)
    check_against_host_frame(M, host_frame, got, lists, range(len(lists)), **kw)
    assert sum(g[2] >= 0 for g in got) >= 300                                # most pairs have a model: the test is not one of "no model"


# ---- other cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_a_larger_call_before_leaves_nothing_behind(ctx, name):
    M = Model(ctx, name)
    _, lists, want = main_batch(name)
    big = [M.planted(775, 20 + k) for k in range(6)]
    M.batch(big, n_hyp=2048)
    check_against_restatement(M, M.batch(lists, **SETTINGS), lists, want)
    M.batch_hyp(big, n_hyp=2048)
    M.single(*big[0])
    check_against_restatement(M, M.batch(lists, **SETTINGS), lists, want)
    small = lists[3:6]
    check_against_restatement(M, M.batch(small, **SETTINGS), small, want[3:6])


@pytest.mark.parametrize("name", MODELS)
def test_optional_outputs_may_be_null(ctx, name):
    M = Model(ctx, name)
    _, lists, want = main_batch(name)
    src, dst = (np.ascontiguousarray(np.concatenate([l[k] for l in lists])) for k in (0, 1))
    moff = np.concatenate([[0], np.cumsum([len(s) for s, _ in lists])]).astype(np.int64)
    P = len(lists)
    out, n = np.full((P, 9), -1.0), np.full(P, -1, np.int64)
    assert M.call(ctx.h, src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p), moff.ctypes.data_as(i64p), P, SETTINGS["threshold"], SETTINGS["n_hyp"],
                  SETTINGS["seed"], SETTINGS["refine"], out.ctypes.data_as(f64p), None, n.ctypes.data_as(i64p), None) == 0
    for p, w in enumerate(want):
        assert n[p] == (w["count"] if w else 0) and np.array_equal(bits(out[p]), bits(w[M.key]) if w else np.zeros(9, np.uint64)), p


@pytest.mark.parametrize("name", MODELS)
def test_a_batch_without_a_single_match(ctx, name):
    M = Model(ctx, name)
    got = M.batch([EMPTY, EMPTY, EMPTY], **SETTINGS)
    assert len(got) == 3 and all(no_model(g, 0) for g in got)
    M_all, count = M.batch_hyp([EMPTY, EMPTY], n_hyp=7)
    assert M_all.shape == (2, 7, 3, 3) and not bits(M_all).any() and not count.any()
    short = [M.planted(M.sample - 1, 3), EMPTY]
    assert all(no_model(g, len(l[0])) for g, l in zip(M.batch(short, **SETTINGS), short))
