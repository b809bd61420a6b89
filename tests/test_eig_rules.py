"""CPU tests of the eigen tracker's host rules (opencv-dlco_amd/csrc/eig_rules.hpp, through tests/shim/host_logic_shim.cpp):
what the comments beside each rule promise, stated independently in float64.  Nothing here needs a GPU or libdlco.so.

Tolerances: the rules work in fp32 (unit round-off 6e-8); a bound that a rule enforces in fp32 is checked in float64 with a
relative slack of 1e-5, a few hundred round-offs, which no input of these tests comes near by design."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHOL_INV_MAX_N = 160            # dlco_internal.hpp: rows of the largest panel the Cholesky-inverse kernel takes
AMP_CAP = 12.2                  # cosh(12.2) = 9.9e4: the "about 1e5" amplification cap of the filter
SLACK = 1e-5
f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libhostshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(ROOT, "tests", "shim", "host_logic_shim.cpp")])
    L = C.CDLL(str(out))
    f, i = C.c_float, C.c_int
    L.shim_eig_plan_filter.argtypes = [f32p, f32p, i, i, i, f, f, f, i, i, i, i, f, f, f, i, i, f, i32p, f32p]
    L.shim_eig_cut_panels.argtypes = [f32p, i, i, i, f, f, i, i, i, i32p]
    L.shim_eig_lam_cut.argtypes = [f32p, i, i, f, i]
    L.shim_eig_lam_cut.restype = f
    L.shim_eig_judge.argtypes = [f32p, f32p, i, i, i, f, f, f, i, i32p, f32p]
    L.shim_eig_lower_bound_period.argtypes = [C.c_int64]
    L.shim_eig_lowered_bound.argtypes = [f, f]
    L.shim_eig_lowered_bound.restype = f
    L.shim_eig_reaches_guards.argtypes = [i, i, i]
    L.shim_eig_growth_rows.argtypes = [i, i, i, i]
    L.shim_eig_next_deg0.argtypes = [i, i, i, f, f]
    L.shim_eig_trimmed_rows.argtypes = [i, i, i]
    return L


def fptr(a):
    return a.ctypes.data_as(f32p)


def plan(L, theta, res, *, live, guard=32, mu, cscale=1.0, tol=2e-4, n_ritz=None, nw=None, it=0, deg0=4, lo, block_min=None,
         locking=True, cheap_ok=False, last_crit=1.0):
    theta, res = np.ascontiguousarray(theta, np.float32), np.ascontiguousarray(res, np.float32)
    m = theta.size
    n_ritz = m if n_ritz is None else n_ritz
    nw = int((theta > np.float32(mu)).sum()) if nw is None else nw
    block_min = min(float(theta[-1]), mu) if block_min is None else block_min
    io, fo = (C.c_int * 4)(), (C.c_float * 2)()
    L.shim_eig_plan_filter(fptr(theta), fptr(res), m, live, guard, mu, cscale, tol, n_ritz, nw, it, deg0, lo, block_min,
                           float(theta[0]), int(locking), int(cheap_ok), last_crit, io, fo)
    return dict(filtered=bool(io[0]), d=io[1], n_lock=io[2], cheap=bool(io[3]), c0=fo[0], e0=fo[1])


def cheb_x(theta, c0, e0):
    """Where a Ritz value sits on the filter's axis: the interval [a, b] = [c0 - e0, c0 + e0] maps to [-1, 1].  The
    difference is formed in fp32 like the input the rule sees; everything after it is float64."""
    return float(np.float32(theta) - np.float32(c0)) / float(e0)


# ---------------------------------------------------------------------------------------------------------------------
# degree, interval, cheap pass
# ---------------------------------------------------------------------------------------------------------------------
def test_filter_degree_respects_the_amplification_cap_and_is_the_largest_that_does(rules):
    n = 0
    for lo, bmin, mu, top, it, deg0 in itertools.product((-1.0, -40.0, -3e-3), (-0.5, 5e-4, 2e-3), (1e-3, 4e-3), (2e-3, 0.3, 7.0, 900.0),
                                                         (0, 1, 3, 9), (2, 4, 10)):
        if bmin <= lo:
            continue
        theta = np.linspace(top, min(bmin, mu), 48)
        p = plan(rules, theta, np.ones(48), live=8192, mu=mu, it=it, deg0=deg0, lo=lo, block_min=bmin, locking=False)
        assert p["filtered"] and not p["cheap"] and p["n_lock"] == 0
        # the interval that is damped: from the lower bound to the bottom of the block, never above mu, never empty
        a, b = p["c0"] - p["e0"], p["c0"] + p["e0"]
        assert abs(a - lo) <= SLACK * abs(lo) and p["e0"] > 0
        width = abs(lo) + abs(mu)
        assert b <= min(bmin, mu) + SLACK * width or b - a <= 1.01e-3 * width + 1e-12
        wanted = min(12, deg0 + 2 * it)                           # what the step asks for before the cap
        d = p["d"]
        assert 2 <= d <= 16 and d <= max(2, wanted)
        ac = math.acosh(max(1.5, cheb_x(max(top, mu), p["c0"], p["e0"])))
        if d > 2:                                                 # (at the floor of 2 the cap may have had to give way)
            assert d * ac <= AMP_CAP * (1 + SLACK), (d, ac)       # T_d(xmax) = cosh(d acosh xmax) <= cosh(12.2) ~ 1e5
        if d < wanted:                                            # held back by the cap only: one more degree breaks it
            assert (d + 1) * ac > AMP_CAP * (1 - SLACK), (d, ac)
        n += 1
    assert n >= 500


def test_no_filter_without_ritz_values_or_on_a_dense_block(rules):
    theta = np.linspace(5.0, -1.0, 40)
    assert not plan(rules, theta, np.ones(40), live=8192, mu=1e-3, lo=-9.0, n_ritz=0)["filtered"]
    assert not plan(rules, theta, np.ones(40), live=40, mu=1e-3, lo=-9.0)["filtered"]
    assert plan(rules, theta, np.ones(40), live=41, mu=1e-3, lo=-9.0)["filtered"]


def test_cheap_pass_only_after_a_narrow_miss_of_a_later_pass(rules):
    theta = np.linspace(5.0, -1.0, 40)
    tol = 2e-4
    kw = dict(live=8192, mu=1e-3, lo=-9.0, tol=tol)
    # what a later pass must reach is half the tolerance; a miss within 1.6x of that (0.8 tol) is worth the cheap pass
    hit = plan(rules, theta, np.ones(40), it=1, cheap_ok=True, last_crit=0.79 * tol, **kw)
    assert hit["cheap"] and hit["d"] == 1 and hit["n_lock"] == 0
    for it, ok, crit in ((1, True, 0.81 * tol), (0, True, 0.1 * tol), (1, False, 0.1 * tol), (4, True, 5 * tol)):
        p = plan(rules, theta, np.ones(40), it=it, cheap_ok=ok, last_crit=crit, **kw)
        assert not p["cheap"] and p["d"] >= 2, (it, ok, crit)


# ---------------------------------------------------------------------------------------------------------------------
# locking
# ---------------------------------------------------------------------------------------------------------------------
def transient_block(quiet, m=100, nw=60, noisy_at=(), ntop=20):
    """The start-up transient: ntop Ritz values far above mu (50 .. 5), the rest of the kept ones near it (0.5 .. 2e-3), guards
    below; `quiet` leading rows have a residual far below a quarter of the tolerance, the others far above.  With lo = -1 the
    filter's axis is x ~ 2 theta + 1: the cap is 2 while a top row is unlocked and 9 behind them."""
    mu = 1e-3
    theta = np.concatenate([np.linspace(50.0, 5.0, ntop), np.geomspace(0.5, 2e-3, nw - ntop), np.linspace(9e-4, 5e-4, m - nw)])
    res = np.full(m, 1.0)
    res[:quiet] = 1e-9
    for i in noisy_at:
        res[i] = 1.0
    return theta, res, mu


def test_locking_lifts_the_cap_to_the_first_unlocked_ritz_value(rules):
    theta, res, mu = transient_block(quiet=20)
    kw = dict(live=8192, mu=mu, lo=-1.0, it=1, deg0=4, tol=2e-4)
    free = plan(rules, theta, res, locking=False, **kw)
    # x ~ 2 theta + 1 here: the top pair at x ~ 101 holds the degree at 2 (12.2 / acosh(101) = 2.3)
    assert free["d"] == 2 and free["n_lock"] == 0
    p = plan(rules, theta, res, locking=True, **kw)
    assert p["n_lock"] == 20 and not p["cheap"]
    ac = math.acosh(max(1.5, cheb_x(theta[p["n_lock"]], p["c0"], p["e0"])))      # the cap is now taken at theta[20] = 0.5, x ~ 2
    assert 2 < p["d"] <= 16 and p["d"] * ac <= AMP_CAP * (1 + SLACK)
    assert p["d"] == 9                                                            # floor(12.2 / acosh(2.0)) = floor(9.26), below the 6 + 4 asked for
    assert (p["c0"], p["e0"]) == (free["c0"], free["e0"])                          # locking does not move the interval


@pytest.mark.parametrize("quiet,noisy_at,ntop,m,nw,it,locking,want", [
    (7, (), 7, 100, 60, 1, True, 0),           # fewer than 8 converged rows: not worth it, although the cap would rise
    (8, (), 8, 100, 60, 1, True, 8),           # at least 8 rows are locked ...
    (30, (10,), 10, 100, 60, 1, True, 10),     # ... and only the leading run of converged rows
    (12, (), 20, 100, 60, 1, True, 0),         # the first unlocked row is still a top row: the cap would not rise, nothing is locked
    (20, (), 20, 100, 60, 0, True, 0),         # never in the first pass
    (20, (), 20, 100, 60, 1, False, 0),        # switched off
    (99, (), 20, 100, 95, 1, True, 84),        # never more than m - 16 rows
    (99, (), 20, 100, 70, 1, True, 70),        # never a row at or below mu
    (20, (), 20, 32, 28, 1, True, 0),          # blocks of up to 32 rows are left alone
])
def test_locking_takes_the_converged_leading_rows_only(rules, quiet, noisy_at, ntop, m, nw, it, locking, want):
    theta, res, mu = transient_block(quiet, m=m, nw=nw, noisy_at=noisy_at, ntop=ntop)
    tol, cscale = 2e-4, 3.0
    p = plan(rules, theta, res, live=8192, mu=mu, lo=-1.0, it=it, deg0=4, tol=tol, cscale=cscale, locking=locking)
    n_lock = p["n_lock"]
    assert n_lock == want
    assert n_lock == 0 or 8 <= n_lock <= m - 16
    quarter = 0.25 * tol * cscale * (theta[0] - mu)
    assert all(cscale * res[i] <= quarter * (1 + SLACK) for i in range(n_lock))


# ---------------------------------------------------------------------------------------------------------------------
# panels
# ---------------------------------------------------------------------------------------------------------------------
def cut(L, theta, n_ritz, *, filtered=True, c0=-0.5, e0=0.5, d=8, n_lock=0):
    theta = np.ascontiguousarray(theta, np.float32)
    ends = (C.c_int * (theta.size + 4))()
    n = L.shim_eig_cut_panels(fptr(theta), theta.size, n_ritz, int(filtered), c0, e0, d, n_lock, CHOL_INV_MAX_N, ends)
    return list(ends[:n])


def check_panels(ends, theta, m, n_ritz, n_lock, c0, e0, d):
    assert all(a < b for a, b in zip(ends, ends[1:])) and ends[0] > 0 and ends[-1] == m
    if 0 < n_lock < m:
        assert n_lock in ends
    if 0 < n_ritz < m:
        assert n_ritz in ends
    amp = lambda j: math.cosh(d * math.acosh(max(1.0, cheb_x(theta[j], c0, e0))))
    start = 0
    for k, end in enumerate(ends):
        rows = end - start
        if start >= n_lock:                           # (the locked rows ahead are not a panel: they are only projected against)
            assert rows <= CHOL_INV_MAX_N
        if start >= n_ritz:
            assert rows == 64 or end == m             # rows without a Ritz value: panels of 64
        elif start >= n_lock:
            assert end <= n_ritz
            assert all(amp(start) <= 1e5 * amp(j) * (1 + 1e-9) for j in range(start, end))
            if end < n_ritz:                          # a cut inside the Ritz rows has a reason: the size or the amplification
                assert rows == CHOL_INV_MAX_N or amp(start) > 1e5 * amp(end) * (1 - 1e-9)
        start = end


def test_panels_follow_the_predicted_amplification(rules):
    # a transient-like block of 200 Ritz rows (x from ~100 down to 1) and 100 freshly appended rows
    m, n_ritz, c0, e0 = 300, 200, -0.5, 0.5
    theta = np.concatenate([np.geomspace(50.0, 1e-3, n_ritz), np.full(m - n_ritz, 1e-3)])
    seen_amp_cut = False
    for d, n_lock in ((2, 0), (8, 0), (8, 12), (16, 40), (12, 184)):
        ends = cut(rules, theta, n_ritz, c0=c0, e0=e0, d=d, n_lock=n_lock)
        check_panels(ends, theta, m, n_ritz, n_lock, c0, e0, d)
        assert ends[-3:] == [200, 264, 300]
        seen_amp_cut = seen_amp_cut or any(n_lock < e < n_ritz for e in ends)
    assert seen_amp_cut
    # T_8 spans cosh(8 acosh(101)) ~ 1e18 over these rows: at least four panels of ratio <= 1e5
    assert len([e for e in cut(rules, theta, n_ritz, c0=c0, e0=e0, d=8) if e <= n_ritz]) >= 4


def test_panels_are_capped_by_the_cholesky_kernel_and_default_to_64_rows(rules):
    flat = np.linspace(2e-3, 1.9e-3, 400)                          # amplification ratio ~1 throughout: only the size cuts
    ends = cut(rules, flat, 400, d=6)
    assert ends == [160, 320, 400]
    check_panels(ends, flat, 400, 400, 0, -0.5, 0.5, 6)
    ends = cut(rules, flat, 400, d=6, n_lock=300)                  # 300 locked rows ahead: one cut there, none inside them
    assert ends == [300, 400]
    assert cut(rules, flat[:96], 0, filtered=False) == [64, 96]    # a block without Ritz values (first pass of a run)
    assert cut(rules, flat[:64], 0, filtered=False) == [64]
    assert cut(rules, flat[:130], 130, filtered=False) == [130]    # a dense block is not filtered: one panel


# ---------------------------------------------------------------------------------------------------------------------
# Jacobi cut, convergence
# ---------------------------------------------------------------------------------------------------------------------
def test_jacobi_cut_sits_a_quarter_of_the_guard_depth_below_mu(rules):
    theta = np.ascontiguousarray(np.concatenate([[9.0, 4.0, 2.0], np.linspace(0.9, 0.1, 37)]), np.float32)   # mu = 1: nw = 3
    no_cut = np.float32(-3.0e38)
    assert rules.shim_eig_lam_cut(fptr(theta), 40, 32, 1.0, 1) == theta[3 + 8]
    assert rules.shim_eig_lam_cut(fptr(theta), 40, 4, 1.0, 1) == theta[3 + 2]       # at least two guards above the cut
    assert rules.shim_eig_lam_cut(fptr(theta), 40, 32, 1.0, 0) == no_cut            # rows without a Ritz value: every pair counts
    assert rules.shim_eig_lam_cut(fptr(theta), 11, 32, 1.0, 1) == no_cut            # the cut would lie behind the block
    assert rules.shim_eig_lam_cut(fptr(theta), 12, 32, 1.0, 1) == theta[11]


def judge(L, theta, res, *, live=1000, guard=32, mu=1.0, cscale=2.0, tol=1e-3, it=0):
    theta, res = np.ascontiguousarray(theta, np.float32), np.ascontiguousarray(res, np.float32)
    io, crit = (C.c_int * 3)(), C.c_float()
    L.shim_eig_judge(fptr(theta), fptr(res), theta.size, live, guard, mu, cscale, tol, it, io, C.byref(crit))
    return dict(nw=io[0], guards_ok=bool(io[1]), conv=bool(io[2]), crit=crit.value)


def weighted_crit(theta, res, mu, cscale):
    """max_i cscale res_i min(1, (theta_i - mu + res_i) / (theta_i - b)) over the pairs above mu, b at the middle guard,
    relative to emax = cscale (theta_0 - mu): the rule's comment, in float64."""
    theta, res = np.asarray(theta, np.float64), np.asarray(res, np.float64)
    m, nw = theta.size, int((theta > mu).sum())
    b = min(mu, theta[nw + (m - nw) // 2]) if nw < m else mu
    w = np.minimum(1.0, (theta[:nw] - mu + res[:nw]) / (theta[:nw] - b))
    return float((cscale * res[:nw] * w).max() / (cscale * (theta[0] - mu)))


def judged_block(m=40):
    """mu = 1, cscale = 2: three pairs above mu (emax = 20), 37 rows below; the guard depth 32 makes the first 8 of them count."""
    theta = np.concatenate([[11.0, 6.0, 3.0], np.linspace(0.9, 0.1, m - 3)])
    return theta, np.full(m, 1e-9)


def test_judge_applies_the_first_pass_and_later_pass_factors(rules):
    theta, res = judged_block()
    tol = 1e-3
    for frac, conv0, conv_later in ((0.4, True, True), (0.6, True, False), (0.9, False, False)):
        r = res.copy()
        # residual of the top pair so that its weighted criterion is frac * tol: weight (10 + r) / (11 - b) with b = theta[21]
        r[0] = frac * tol * 10.0 * (11.0 - theta[21]) / 10.0
        want = weighted_crit(theta, r, 1.0, 2.0)
        assert abs(want / tol - frac) < 0.02
        first, later = judge(rules, theta, r, tol=tol, it=0), judge(rules, theta, r, tol=tol, it=1)
        assert first["nw"] == 3 and first["guards_ok"]
        assert abs(first["crit"] - want) <= SLACK * want and later["crit"] == first["crit"]
        assert (first["conv"], later["conv"], judge(rules, theta, r, tol=tol, it=7)["conv"]) == (conv0, conv_later, conv_later)


def test_judge_weighs_a_pair_just_above_mu_by_its_share_of_the_projection(rules):
    theta, res = judged_block()
    theta[2], res[2] = 1.001, 0.05
    # unweighted this residual is 2 * 0.05 / 20 = 5 tol; with the weight (0.001 + 0.05) / (1.001 - 0.5) = 0.102 it is 0.51 tol
    want = weighted_crit(theta, res, 1.0, 2.0)
    assert 0.50e-3 < want < 0.52e-3
    first = judge(rules, theta, res, it=0)
    assert abs(first["crit"] - want) <= SLACK * want and first["conv"] and not judge(rules, theta, res, it=1)["conv"]
    # b is taken at the middle guard (row 3 + 37 // 2 = 21): raising that one row from 0.5 to 0.8 raises the weight to 0.254
    theta[4:22] = np.linspace(0.9, 0.8, 18)
    want = weighted_crit(theta, res, 1.0, 2.0)
    assert 1.2e-3 < want < 1.3e-3
    moved = judge(rules, theta, res, it=0)
    assert abs(moved["crit"] - want) <= SLACK * want and not moved["conv"]
    # a pair well above mu keeps the weight 1 of the plain residual test when every guard sits at mu (b = mu)
    top = np.concatenate([[11.0, 6.0, 3.0], np.full(37, 1.0)])
    r = np.full(40, 1e-9)
    r[1] = 0.02
    assert abs(judge(rules, top, r)["crit"] - 2 * 0.02 / 20) <= SLACK * 2e-3


@pytest.mark.parametrize("row,theta_g,res_g,ok", [
    (3, 0.90, 0.05, True),        # theta + res < mu: nothing of that pair's interval reaches mu
    (3, 0.99, 0.05, False),       # reaches 0.04 above mu: 2 * 0.04 against gtol = tol * emax = 0.02
    (3, 0.99, 0.015, True),       # reaches above mu by less than the tolerance (2 * 0.005 <= 0.02)
    (3, 0.999, 0.009, True),      # a small residual (2 * 0.009 <= 0.02)
    (10, 0.70, 0.5, False),       # the eighth guard still counts (guard / 4 = 8 of them) ...
    (11, 0.68, 0.5, True),        # ... the ninth does not
])
def test_judge_needs_the_leading_guards_resolved(rules, row, theta_g, res_g, ok):
    """(A guard has theta <= mu, so its excess theta + res - mu never exceeds its residual: the small-residual clause cannot
    decide a case on its own, it is covered together with the excess clause.)"""
    theta, res = judged_block()
    theta[3:] = np.linspace(0.85, 0.1, 37)
    theta[row], res[row] = theta_g, res_g
    assert np.all(np.diff(theta) <= 0)
    v = judge(rules, theta, res, it=0)
    assert v["nw"] == 3 and v["crit"] < 1e-6                   # the kept pairs are converged: the guards decide
    assert v["guards_ok"] == ok and v["conv"] == ok


def test_judge_without_a_positive_pair_and_on_a_dense_block(rules):
    theta = np.linspace(0.9, 0.1, 40)                          # nothing above mu = 1: emax = 0, gtol = tol * cscale * 1e-3 * |mu| = 2e-6
    quiet, loud = np.full(40, 1e-9), np.full(40, 0.5)
    assert judge(rules, theta, quiet, it=0) == dict(nw=0, guards_ok=True, conv=True, crit=0.0)
    for it, conv in ((0, False), (5, False), (6, True), (9, True)):      # unresolved guards: given up after six passes
        v = judge(rules, theta, loud, it=it)
        assert v["nw"] == 0 and not v["guards_ok"] and v["conv"] == conv
    # a block as large as the problem is the dense eigensolver: Rayleigh-Ritz is exact whatever the residuals say
    t2, _ = judged_block()
    assert judge(rules, t2, np.full(40, 0.5), live=40)["conv"] and judge(rules, t2, np.full(40, 0.5), live=39)["conv"]
    assert not judge(rules, t2, np.full(40, 0.5), live=41)["conv"]


# ---------------------------------------------------------------------------------------------------------------------
# trim, growth, starting degree, lower bound
# ---------------------------------------------------------------------------------------------------------------------
def test_trim_worked_cases(rules):
    assert rules.shim_eig_trimmed_rows(87, 55, 32) == 80       # the reference's own shape: a multiple of 16 that keeps 25 >= 24 guards
    assert rules.shim_eig_trimmed_rows(96, 64, 32) == 96       # fills its padding exactly
    assert rules.shim_eig_trimmed_rows(152, 120, 32) == 152    # no 16-row rule above 96 rows (144 would keep 24 guards)
    assert rules.shim_eig_trimmed_rows(128, 85, 32) == 117     # 117 rows -> 96 would keep 11 guards, fewer than half: stays
    assert rules.shim_eig_trimmed_rows(128, 79, 32) == 96      # 111 rows -> 96 keeps 17 >= 16 guards
    assert rules.shim_eig_trimmed_rows(128, 81, 32) == 113     # 96 would keep 15: one too few
    assert rules.shim_eig_trimmed_rows(40, 55, 32) == 40       # never more rows than the block has
    assert rules.shim_eig_trimmed_rows(5, 0, 0) == 1           # never an empty block


def test_trim_keeps_enough_guards_and_prefers_whole_padding(rules):
    for guard, nw, m in itertools.product((0, 2, 8, 32, 48), range(0, 200, 3), (1, 50, 96, 160, 400)):
        got = rules.shim_eig_trimmed_rows(m, nw, guard)
        full = nw + guard
        cands = [full]
        if full // 32 * 32 >= nw + max(4, guard // 2):
            cands = [full // 32 * 32]
        elif full <= 96 and full // 16 * 16 >= nw + max(4, 3 * guard // 4):
            cands = [full // 16 * 16]
        assert got == max(1, min(m, cands[0])), (guard, nw, m)
        assert 1 <= got <= max(1, m) and got <= max(1, full)
        if got < min(m, full):                                 # rows were given up for the padding: the guards that must stay did
            assert got % 16 == 0 and got - nw >= max(4, guard // 2)
            assert got % 32 == 0 or (full <= 96 and got - nw >= max(4, 3 * guard // 4))


def test_growth_starting_degree_and_lower_bound_rules_on_their_boundaries(rules):
    L = rules
    # the block grows when fewer than max(2, guard / 2) rows are left below the kept pairs
    assert [L.shim_eig_reaches_guards(nw, 96, 32) for nw in (79, 80, 81)] == [0, 0, 1]
    assert [L.shim_eig_reaches_guards(nw, 96, 2) for nw in (94, 95)] == [0, 1]
    # by a guard's worth of rows, a quarter of the rank once that is more, and never beyond the capacity
    assert L.shim_eig_growth_rows(96, 1024, 32, 81) == 32
    assert L.shim_eig_growth_rows(96, 1024, 32, 128) == 32 and L.shim_eig_growth_rows(96, 1024, 32, 132) == 33
    assert L.shim_eig_growth_rows(500, 1024, 32, 490) == 122
    assert L.shim_eig_growth_rows(1000, 1024, 32, 990) == 24
    # starting degree: +2 (up to 10) after a step of two or more passes, -1 (down to 2) after a single pass that
    # converged below 0.15 of the tolerance, otherwise unchanged
    tol = 2e-4
    assert [L.shim_eig_next_deg0(d, 2, 1, 0.0, tol) for d in (2, 8, 9, 10)] == [4, 10, 10, 10]
    assert L.shim_eig_next_deg0(6, 5, 0, 1.0, tol) == 8
    assert [L.shim_eig_next_deg0(d, 1, 1, 0.14 * tol, tol) for d in (2, 3, 10)] == [2, 2, 9]
    assert L.shim_eig_next_deg0(6, 1, 1, 0.16 * tol, tol) == 6 and L.shim_eig_next_deg0(6, 1, 0, 0.0, tol) == 6
    # the lower bound is refreshed every step at first, then every 5, 20, 50 updates
    assert [L.shim_eig_lower_bound_period(u) for u in (1, 19, 20, 199, 200, 399, 400, 10 ** 6)] == [1, 1, 5, 5, 20, 20, 50, 50]
    # a Ritz value below the bound pushes the bound below it; one above leaves it alone
    assert L.shim_eig_lowered_bound(-3.0, -2.0) == -3.0 and L.shim_eig_lowered_bound(-3.0, -3.0) == -3.0
    assert L.shim_eig_lowered_bound(-3.0, -4.0) == -6.0 and L.shim_eig_lowered_bound(1.0, 0.5) == 0.25
    assert L.shim_eig_lowered_bound(0.5, 0.0) < 0.0
