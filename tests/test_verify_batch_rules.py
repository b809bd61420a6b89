"""CPU tests of the plan of a batched verification (opencv-dlco_amd/csrc/verify_batch.hpp, through
tests/shim/verify_batch_shim.cpp): how dlco_desc_verify_pairs_* cuts one segmented match list into launches and entries, the
check of the offsets, and the refit loop of verify_rules.hpp after its round was split off as refit_step.  Nothing here needs
a GPU or libdlco.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_epipolar_rules as E
import test_verify_rules as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim")
i64p, i32p, f32p, f64p, u8p = (C.POINTER(t) for t in (C.c_int64, C.c_int32, C.c_float, C.c_double, C.c_uint8))
E_FIELDS = ("m0", "m", "pair", "swg0", "mwg0")
L_FIELDS = ("e0", "n", "match0", "matches", "hyps", "score_wgs", "mask_wgs")
SIZES = (0, 3, 4, 7, 8, 9, 255, 256, 257, 775)


def build_shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libverifybatchshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), os.path.join(SHIM, "verify_batch_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_vbatch_launch_hyp.restype = L.shim_vbatch_launch_wgs.restype = C.c_int64
    L.shim_vbatch_offsets_ok.argtypes = [i64p, C.c_int64]
    L.shim_vbatch_plan.argtypes, L.shim_vbatch_plan.restype = [i64p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int64], C.c_void_p
    L.shim_vbatch_free.argtypes, L.shim_vbatch_free.restype = [C.c_void_p], None
    L.shim_vbatch_count.argtypes, L.shim_vbatch_count.restype = [C.c_void_p, C.c_int], C.c_int64
    L.shim_vbatch_entries.argtypes = L.shim_vbatch_launches.argtypes = [C.c_void_p, i64p]
    L.shim_vbatch_launch_of_pair.argtypes = [C.c_void_p, i32p]
    L.shim_vbatch_verify.argtypes = [C.c_int, f32p, f32p, C.c_int64, C.c_float, C.c_int32, C.c_uint64, C.c_int32, f64p, i32p, f64p, u8p, i64p, i32p, f64p, i32p]
    L.shim_vbatch_verify.restype = None
    L.shim_vbatch_refit_step.argtypes = [C.c_int64, f64p, u8p, i64p, f64p, u8p, C.c_int64]
    return L


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return build_shim(tmp_path_factory)


def plan(L, moff, n_hyp, fundamental=False, max_hyp=0, max_wgs=0):
    """the plan as dicts of int64 columns: e (entries), l (launches); launch [n_pairs]; the largest launch's figures"""
    moff = np.ascontiguousarray(moff, np.int64)
    h = L.shim_vbatch_plan(moff.ctypes.data_as(i64p), len(moff) - 1, n_hyp, int(fundamental), max_hyp, max_wgs)
    try:
        def table(what, fn, fields):
            a = np.zeros((L.shim_vbatch_count(h, what), len(fields)), np.int64)
            fn(h, a.ctypes.data_as(i64p))
            return {f: a[:, k] for k, f in enumerate(fields)}
        launch = np.zeros(len(moff) - 1, np.int32)
        L.shim_vbatch_launch_of_pair(h, launch.ctypes.data_as(i32p))
        return dict(e=table(0, L.shim_vbatch_entries, E_FIELDS), l=table(1, L.shim_vbatch_launches, L_FIELDS), launch=launch,
                    max_entries=L.shim_vbatch_count(h, 2), max_matches=L.shim_vbatch_count(h, 3), max_hyps=L.shim_vbatch_count(h, 4))
    finally:
        L.shim_vbatch_free(h)


def seeded_offsets():
    rng = np.random.default_rng(20240702)
    out = [np.concatenate([[0], np.cumsum(SIZES)])]
    for k in range(6):
        P = 1 if k == 0 else int(rng.integers(1, 800))
        sizes = [int(rng.choice(SIZES)) if rng.integers(2) else int(rng.integers(0, 1500)) for _ in range(P)]
        out.append(np.concatenate([[0], np.cumsum(sizes)]))
    out.append(np.zeros(5, np.int64))                       # four pairs without a match
    return [o.astype(np.int64) for o in out]


OFFSETS = seeded_offsets()
ceil_div = lambda a, b: -(-a // b)


@pytest.mark.parametrize("fundamental", [False, True])
@pytest.mark.parametrize("limits", ["library", "four_entries", "one_entry", "seven_workgroups", "both"])
def test_plan_properties(rules, fundamental, limits):
    lanes, k_sample = rules.shim_vbatch_lanes(), rules.shim_vbatch_sample(int(fundamental))
    assert lanes == 256 and k_sample == (8 if fundamental else 4)
    assert rules.shim_vbatch_launch_hyp() == 2 ** 22 and rules.shim_vbatch_launch_wgs() == 2 ** 31 - 1
    for moff in OFFSETS:
        for n_hyp in (1, 65, 256, 300):
            max_hyp = {"library": 0, "four_entries": 4 * n_hyp, "one_entry": n_hyp, "seven_workgroups": 0, "both": 3 * n_hyp}[limits]
            max_wgs = {"seven_workgroups": 7, "both": 40}.get(limits, 0)
            pl = plan(rules, moff, n_hyp, fundamental, max_hyp, max_wgs)
            e, l = pl["e"], pl["l"]
            lim_hyp, lim_wgs = max_hyp or 2 ** 22, max_wgs or 2 ** 31 - 1
            m = np.diff(moff)
            # every pair with a sample's matches is an entry, in order, and in exactly one launch; the others are in none
            assert np.array_equal(e["pair"], np.flatnonzero(m >= k_sample)) and np.array_equal(e["m"], m[e["pair"]])
            assert (pl["launch"][m < k_sample] == -1).all()
            assert np.array_equal(l["e0"], np.concatenate([[0], np.cumsum(l["n"])])[:-1]) and l["n"].sum() == len(e["m"]) and (l["n"] >= 1).all()
            assert np.array_equal(pl["launch"][e["pair"]], np.repeat(np.arange(len(l["n"])), l["n"]))
            hb = ceil_div(n_hyp, lanes)
            for k in range(len(l["n"])):
                s_ = slice(int(l["e0"][k]), int(l["e0"][k] + l["n"][k]))
                mm, chunks = e["m"][s_], ceil_div(e["m"][s_], lanes)
                # the launch's matches: from its first entry's first match to its last entry's end, m0 counted from there
                assert l["match0"][k] == moff[e["pair"][s_][0]] and l["match0"][k] + l["matches"][k] == moff[e["pair"][s_][-1] + 1]
                assert np.array_equal(l["match0"][k] + e["m0"][s_], moff[e["pair"][s_]])
                # workgroup ranges are disjoint and cover both grids
                assert np.array_equal(e["swg0"][s_], np.concatenate([[0], np.cumsum(hb * chunks)])[:-1]) and (hb * chunks).sum() == l["score_wgs"][k]
                assert np.array_equal(e["mwg0"][s_], np.concatenate([[0], np.cumsum(chunks)])[:-1]) and chunks.sum() == l["mask_wgs"][k]
                # no launch exceeds a limit, but for an entry that alone exceeds the grid's
                assert l["hyps"][k] == l["n"][k] * n_hyp <= lim_hyp
                assert l["score_wgs"][k] <= lim_wgs or l["n"][k] == 1
                assert l["n"][k] <= pl["max_entries"] and l["matches"][k] <= pl["max_matches"] and l["hyps"][k] <= pl["max_hyps"]
                # launches are as full as the limits allow: the next entry would not have fitted
                if k + 1 < len(l["n"]):
                    nxt = int(l["e0"][k + 1])
                    assert l["hyps"][k] + n_hyp > lim_hyp or l["score_wgs"][k] + hb * ceil_div(e["m"][nxt], lanes) > lim_wgs
            if limits == "one_entry":
                assert (l["n"] == 1).all() and len(l["n"]) == (m >= k_sample).sum()
            if limits == "library":
                assert len(l["n"]) == (1 if (m >= k_sample).any() else 0)


def test_the_sets_hold_what_they_should():
    assert any(len(o) == 2 for o in OFFSETS) and any(len(o) > 400 for o in OFFSETS) and any(o[-1] == 0 for o in OFFSETS)
    assert set(SIZES) <= set(int(x) for o in OFFSETS for x in np.diff(o))


def test_the_librarys_limits_cut_a_large_call(rules):
    """5 pairs at 2^20 hypotheses are more than 2^22: two launches; 4096 pairs at 1024 fill one launch exactly"""
    moff = np.arange(6, dtype=np.int64) * 12
    pl = plan(rules, moff, 2 ** 20)
    assert pl["l"]["n"].tolist() == [4, 1] and pl["launch"].tolist() == [0, 0, 0, 0, 1] and pl["max_hyps"] == 2 ** 22
    assert plan(rules, np.arange(4097, dtype=np.int64) * 5, 1024)["l"]["n"].tolist() == [4096]
    assert plan(rules, np.arange(4098, dtype=np.int64) * 5, 1024)["l"]["n"].tolist() == [4096, 1]
    # short pairs between entries ride along in the launch's match range
    pl = plan(rules, np.array([0, 3, 13, 13, 15, 25], np.int64), 64)
    assert pl["e"]["pair"].tolist() == [1, 4] and pl["e"]["m0"].tolist() == [0, 12] and pl["l"]["match0"].tolist() == [3] and pl["l"]["matches"].tolist() == [22]


@pytest.mark.parametrize("fundamental", [False, True])
def test_the_plan_of_one_pair(rules, fundamental):
    """what a single call (dlco_desc_verify_homography and its kin) hands the batch path: n_pairs = 1, moff = {0, m} under the
    library's limits is one launch of one entry that starts every range at 0"""
    lanes, k_sample = rules.shim_vbatch_lanes(), rules.shim_vbatch_sample(int(fundamental))
    for m in (k_sample, 255, 256, 257):
        for n_hyp in (1, 256, 257):
            pl = plan(rules, [0, m], n_hyp, fundamental)
            e, l = pl["e"], pl["l"]
            assert {f: e[f].tolist() for f in E_FIELDS} == dict(m0=[0], m=[m], pair=[0], swg0=[0], mwg0=[0])
            assert {f: l[f].tolist() for f in L_FIELDS} == dict(e0=[0], n=[1], match0=[0], matches=[m], hyps=[n_hyp],
                                                                 score_wgs=[ceil_div(n_hyp, lanes) * ceil_div(m, lanes)], mask_wgs=[ceil_div(m, lanes)])
            assert pl["launch"].tolist() == [0] and (pl["max_entries"], pl["max_matches"], pl["max_hyps"]) == (1, m, n_hyp)


def test_offsets_validation(rules):
    ok = lambda o, n=None: bool(rules.shim_vbatch_offsets_ok(np.asarray(o, np.int64).ctypes.data_as(i64p), len(o) - 1 if n is None else n))
    assert ok([0, 0]) and ok([0, 5, 5, 9]) and ok([0, 2 ** 31 - 1]) and ok([0, 2 ** 31 - 1, 2 ** 32 - 2])
    assert not ok([1, 5]) and not ok([0, 5, 4]) and not ok([0, -1]) and not ok([0, 2 ** 31]) and not ok([0, 1], 0) and not ok([0, 1], -3)
    assert not ok([0, 1], 2 ** 31) and not rules.shim_vbatch_offsets_ok(None, 1)


def shim_whole_rule(L, fundamental, src, dst, threshold, n_hyp, seed, refine):
    src, dst = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    m = len(src)
    M_all, counts, M, mask = np.empty((n_hyp, 9)), np.empty(n_hyp, np.int32), np.empty(9), np.empty(m, np.uint8)
    rounds, count, best, n_rounds = np.zeros((max(refine, 1), 9)), C.c_int64(), C.c_int32(), C.c_int32()
    L.shim_vbatch_verify(int(fundamental), src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p), m, threshold, n_hyp, seed, refine, M_all.ctypes.data_as(f64p),
                         counts.ctypes.data_as(i32p), M.ctypes.data_as(f64p), mask.ctypes.data_as(u8p), C.byref(count), C.byref(best),
                         rounds.ctypes.data_as(f64p), C.byref(n_rounds))
    return dict(M_all=M_all, counts=counts, best=best.value, M=M, mask=mask.astype(bool), count=count.value, rounds=list(rounds[:n_rounds.value]))


@pytest.mark.parametrize("threshold, n_hyp, seed, refine", [(3.0, 2048, 0, 2), (0.75, 65, 5, 8)])
def test_the_refit_loop_through_its_step_is_still_the_restatement_homography(rules, threshold, n_hyp, seed, refine):
    src, dst, want = V.reference("planted257")
    if (threshold, n_hyp, seed, refine) != (3.0, 2048, 0, 2):
        want = V.verify_ref(src, dst, threshold, n_hyp, seed, refine)
        assert len(want["rounds"]) >= 2
    got = shim_whole_rule(rules, False, src, dst, threshold, n_hyp, seed, refine)
    got.update(H_all=got["M_all"], H=got["M"])
    assert V.same_answer(got, want)


@pytest.mark.parametrize("threshold, n_hyp, seed, refine", [(1.0, 2048, 0, 2), (0.5, 65, 7, 8)])
def test_the_refit_loop_through_its_step_is_still_the_restatement_fundamental(rules, threshold, n_hyp, seed, refine):
    src, dst, want = E.reference("planted257")
    if (threshold, n_hyp, seed, refine) != (1.0, 2048, 0, 2):
        want = E.fundamental_ref(src, dst, threshold, n_hyp, seed, refine)
        assert len(want["rounds"]) >= 1
    got = shim_whole_rule(rules, True, src, dst, threshold, n_hyp, seed, refine)
    got.update(F_all=got["M_all"], F=got["M"])
    assert E.same_answer(got, want)


def test_refit_step(rules):
    """accept iff the count does not fall; go on iff accepted and the mask changed"""
    def step(count, c, mask, trial):
        M, Mn = np.arange(9, dtype=np.float64), np.arange(9, dtype=np.float64) + 100
        mask, trial, n = np.array(mask, np.uint8), np.array(trial, np.uint8), C.c_int64(count)
        go = rules.shim_vbatch_refit_step(len(mask), M.ctypes.data_as(f64p), mask.ctypes.data_as(u8p), C.byref(n), Mn.ctypes.data_as(f64p),
                                          trial.ctypes.data_as(u8p), c)
        return bool(go), M[0] == 100, mask.tolist(), n.value
    assert step(3, 2, [1, 1, 1, 0], [1, 1, 0, 0]) == (False, False, [1, 1, 1, 0], 3)      # rejected: nothing moves
    assert step(2, 3, [1, 1, 0, 0], [1, 1, 1, 0]) == (True, True, [1, 1, 1, 0], 3)
    assert step(2, 2, [1, 1, 0, 0], [1, 0, 1, 0]) == (True, True, [1, 0, 1, 0], 2)        # equal count, other mask: accepted, goes on
    assert step(2, 2, [1, 1, 0, 0], [1, 1, 0, 0]) == (False, True, [1, 1, 0, 0], 2)       # same mask: accepted, ends


def test_planner_under_address_and_undefined_sanitizers(tmp_path):
    """the stand-alone program walks the planner, the kernels' index arithmetic and the refit loop with its own checks"""
    exe = tmp_path / "verify_batch_asan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(SHIM, "verify_batch_asan_main.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "verify_batch_asan: ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
