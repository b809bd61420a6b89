"""Epipolar verification on a GPU: dlco_desc_verify_fundamental_hypotheses / dlco_desc_verify_fundamental.  The rule
(opencv-dlco_amd/csrc/epipolar_rules.hpp) is IEEE double + - x / in a stated order and integer counts, so every hypothesis, every
count, the winner, the mask and the refitted matrix are compared bit for bit against the numpy restatement of
tests/test_epipolar_rules.py (which the CPU tests hold against the header)."""
import ctypes as C

import numpy as np
import pytest

import test_verify_rules as hom
from test_epipolar_rules import NAN_ROWS, OTHER_ARGUMENTS, bits, build_shim, fundamental_ref, other_reference, planted_case, reference

pytestmark = pytest.mark.gpu
f32p, f64p, i64p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int64))


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return build_shim(tmp_path_factory)


def same(ctx, src, dst, want, threshold=1.0, n_hyp=2048, seed=0, refine=2):
    """the library's two calls against a restated answer: F_all, counts, best, mask, final F and inlier count, every bit"""
    F_all, count = ctx.verify_fundamental_hypotheses(src, dst, threshold, n_hyp, seed)
    ok = F_all.shape == (n_hyp, 3, 3) and np.array_equal(bits(F_all).reshape(n_hyp, 9), bits(want["F_all"])) and np.array_equal(count, want["counts"])
    F, mask, best = ctx.verify_fundamental(src, dst, threshold, n_hyp, seed, refine)
    return (ok and best == want["best"] and mask.dtype == bool and np.array_equal(mask, want["mask"]) and int(mask.sum()) == want["count"]
            and np.array_equal(bits(F).reshape(9), bits(want["F"])))


def case(m, seed):
    return planted_case(m, 0.0 if m < 16 else 0.3, seed, 0.3)[:2]


# ---- parity with the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m, n_hyp", [(8, 65), (9, 63), (63, 1), (65, 300), (257, 2048)])
@pytest.mark.parametrize("refine", [0, 2])
def test_small_match_lists_against_the_restatement(ctx, m, n_hyp, refine):
    if (m, refine) == (257, 2):
        src, dst, want = reference("planted257")
        assert same(ctx, src, dst, want) and want["count"] >= 170
    else:
        src, dst = case(m, 10 + m)
        want = fundamental_ref(src, dst, n_hyp=n_hyp, seed=m, refine=refine)
        assert same(ctx, src, dst, want, n_hyp=n_hyp, seed=m, refine=refine)
        assert n_hyp == 1 or want["best"] >= 0
    assert ctx.last_kernel_ms() > 0


def test_match_lists_around_the_scoring_chunk(ctx, rules):
    chunk = rules.shim_epipolar_score_chunk()
    assert chunk >= 64
    for m in (chunk - 1, chunk, chunk + 1, 3 * chunk + 7):                   # the last spans four workgroups of the grid's second dimension
        src, dst = case(m, m)
        want = fundamental_ref(src, dst, n_hyp=300, seed=3, refine=2)
        assert want["count"] >= 0.5 * m and same(ctx, src, dst, want, n_hyp=300, seed=3), m


@pytest.mark.parametrize("args", OTHER_ARGUMENTS[3:])
def test_a_tight_threshold_on_noisy_matches_runs_several_rounds(ctx, args):
    _, refine, seed, n_hyp, threshold = args
    src, dst, want = other_reference(args)
    assert same(ctx, src, dst, want, threshold=threshold, n_hyp=n_hyp, seed=seed, refine=refine)
    assert len(want["rounds"]) >= 2 or want["accepted"] == 0                 # several accepted rounds, or one that was rejected by its count


@pytest.mark.parametrize("name", ["planted1000", "stereo", "point", "nan", "far"])
def test_the_cases_of_the_cpu_tests(ctx, name):
    src, dst, want = reference(name)
    assert same(ctx, src, dst, want)
    F, mask, best = ctx.verify_fundamental(src, dst)
    if name == "point":                                                      # no model is no error
        assert best == -1 and not mask.any() and (F == 0).all() and not want["valid"].any()
    if name == "stereo":
        assert best == int(np.flatnonzero(want["valid"])[0]) and mask.all() and (want["counts"][want["valid"]] == len(src)).all()
        assert abs(F[2, 2]) < 1e-9 and abs(F[2, 1]) >= 1
    if name == "nan":
        assert not mask[NAN_ROWS].any() and mask.sum() == len(src) - 3 and np.isfinite(F).all()
    if name == "far":
        assert np.isfinite(F).all() and np.isfinite(ctx.verify_fundamental_hypotheses(src, dst)[0]).all()


def test_the_same_call_twice_and_another_seed(ctx):
    src, dst, want = reference("planted257")
    first, again = ctx.verify_fundamental(src, dst), ctx.verify_fundamental(src, dst)
    assert all(np.array_equal(a, b) for a, b in zip(first[:2], again[:2])) and first[2] == again[2] == want["best"]
    other = fundamental_ref(src, dst, seed=1)
    assert other["best"] != want["best"] and same(ctx, src, dst, other, seed=1)


def test_a_larger_call_before_leaves_nothing_behind(ctx):
    big_src, big_dst = case(775, 20)
    ctx.verify_fundamental(big_src, big_dst, n_hyp=2048)
    src, dst = case(63, 21)
    want = fundamental_ref(src, dst, n_hyp=65, seed=9)
    assert same(ctx, src, dst, want, n_hyp=65, seed=9)
    ctx.verify_fundamental_hypotheses(big_src, big_dst, n_hyp=2048)
    assert same(ctx, src, dst, want, n_hyp=65, seed=9)


@pytest.mark.parametrize("m", [8, 257])
def test_a_pairs_call_before_leaves_nothing_behind(ctx, m):
    """a single call is a launch of one entry on the plan buffer and the scratch that the pairs calls use: after a batch of
    several pairs and more hypotheses it still answers as the restatement, the model form and the _hypotheses form alike"""
    big = [case(300 + 75 * k, 30 + k) for k in range(4)]
    src, dst = case(m, 40 + m)
    want = fundamental_ref(src, dst, n_hyp=65, seed=9)
    ctx.verify_pairs_fundamental(big, n_hyp=2048)
    F, mask, best = ctx.verify_fundamental(src, dst, n_hyp=65, seed=9)
    assert best == want["best"] and np.array_equal(mask, want["mask"]) and int(mask.sum()) == want["count"]
    assert np.array_equal(bits(F).reshape(9), bits(want["F"]))
    ctx.verify_pairs_fundamental_hypotheses(big, n_hyp=2048)
    F_all, count = ctx.verify_fundamental_hypotheses(src, dst, n_hyp=65, seed=9)
    assert np.array_equal(bits(F_all).reshape(65, 9), bits(want["F_all"])) and np.array_equal(count, want["counts"])
    assert same(ctx, src, dst, want, n_hyp=65, seed=9)


def test_optional_outputs_may_be_null(ctx):
    src, dst, want = reference("planted257")
    F, n = np.zeros(9), C.c_int64(-1)
    assert ctx.L.dlco_desc_verify_fundamental(ctx.h, src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p), len(src), 1.0, 2048, 0, 2, F.ctypes.data_as(f64p), None,
                                              C.byref(n), None) == 0
    assert n.value == want["count"] and np.array_equal(bits(F), bits(want["F"]))


def test_a_homography_call_before_and_after_a_fundamental_call(ctx):
    """the two models share the context's buffers and the host path: neither moves the other"""
    hs, hd, hwant = hom.reference("planted257")
    src, dst, want = reference("planted1000")

    def homography_holds():
        H_all, count = ctx.verify_hypotheses(hs, hd)
        H, mask, best = ctx.verify_homography(hs, hd)
        return (np.array_equal(bits(H_all).reshape(-1, 9), bits(hwant["H_all"])) and np.array_equal(count, hwant["counts"]) and best == hwant["best"]
                and np.array_equal(mask, hwant["mask"]) and np.array_equal(bits(H).reshape(9), bits(hwant["H"])))

    assert homography_holds()
    assert same(ctx, src, dst, want)
    assert homography_holds()
    assert same(ctx, src, dst, want)
