"""CPU tests of the verification rule (opencv-dlco_amd/csrc/verify_rules.hpp, through tests/shim/verify_rules_shim.cpp) against
the numpy restatement below, which the GPU tests (tests/test_verify_gpu.py) use as well.  The rule is IEEE double + - x in a
stated order, so sample indices, the nine doubles of every hypothesis, counts, masks and the refit's matrices are compared
with equality of bits.  Nothing here needs a GPU or libdlco.so."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim")
i64p, i32p, u8p, f32p, f64p = (C.POINTER(t) for t in (C.c_int64, C.c_int32, C.c_uint8, C.c_float, C.c_double))

# ---- the rule restated: Python integers for the sampler, float64 operations one at a time in the stated order ---------------
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
DBL_MAX = 1.7976931348623157e308


def mix_ref(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_ref(seed, h, m):
    """(idx [4] with -1 where none was found, ok) of hypothesis h among m matches"""
    s = seed ^ (((h + 1) * G) & M64)
    idx = []
    for _ in range(16):
        if len(idx) == 4:
            break
        s = (s + G) & M64
        j = ((mix_ref(s) >> 32) * m) >> 32
        if j not in idx:
            idx.append(j)
    return idx + [-1] * (4 - len(idx)), len(idx) == 4


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _basis(p):
    """p [4] points of three components each (arrays over the hypotheses): the columns a_i and the four areas"""
    r = (_cross(p[1], p[2]), _cross(p[2], p[0]), _cross(p[0], p[1]))
    lam = [_dot(r[0], p[3]), _dot(r[1], p[3]), _dot(r[2], p[3]), _dot(r[0], p[0])]
    a = [tuple(lam[i] * c for c in p[i]) for i in range(3)]
    return a, lam


def _pow2(n):
    return ((n + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)


def normalise_ref(H):
    """H [9, n] -> (H scaled [9, n], ok [n]); a column that is not ok is returned as it came"""
    a = np.abs(H)
    finite = (a <= DBL_MAX).all(axis=0)
    mx = np.zeros(H.shape[1])
    for i in range(9):
        mx = np.where(a[i] > mx, a[i], mx)
    ok = finite & (mx > 0.0)
    k = 1023 - ((np.where(ok, mx, 1.0).view(np.int64) >> 52) & 0x7FF)
    k1 = (k - (k & 1)) // 2
    out = (H * _pow2(k1)) * _pow2(k - k1)
    return np.where(ok, out, H), ok


def model_ref(sx, sy, dx, dy):
    """(H [n, 9], valid [n]) from the samples' coordinates, arrays [4, n] of float64; H is zero where invalid"""
    with np.errstate(all="ignore"):
        one = np.ones_like(sx[0])
        A, la = _basis([(sx[i], sy[i], one) for i in range(4)])
        B, lb = _basis([(dx[i], dy[i], one) for i in range(4)])
        valid = np.ones(sx.shape[1], bool)
        for a, b in zip(la, lb):
            valid &= ((a > 1.0) & (b > 1.0)) | ((a < -1.0) & (b < -1.0))
        R = (_cross(A[1], A[2]), _cross(A[2], A[0]), _cross(A[0], A[1]))
        H = np.array([(B[0][i] * R[0][j] + B[1][i] * R[1][j]) + B[2][i] * R[2][j] for i in range(3) for j in range(3)])
        H, ok = normalise_ref(H)
        valid &= ok
        flip = (H[6] * sx[0] + H[7] * sy[0]) + H[8] < 0.0
        H = np.where(flip, -H, H)
        return np.where(valid, H, 0.0).T.copy(), valid


def hypotheses_ref(src, dst, seed, n_hyp):
    """(H_all [n, 9], valid [n], idx [n, 4]) of the call"""
    src, dst = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    samples = [sample_ref(seed, h, len(src)) for h in range(n_hyp)]
    idx = np.array([s[0] for s in samples], np.int64).reshape(n_hyp, 4)
    drawn = np.array([s[1] for s in samples], bool)
    g = np.where(idx < 0, 0, idx).T                                          # [4, n]
    H, valid = model_ref(src[g, 0].astype(np.float64), src[g, 1].astype(np.float64), dst[g, 0].astype(np.float64), dst[g, 1].astype(np.float64))
    valid &= drawn
    H[~valid] = 0.0
    return H, valid, idx.astype(np.int32)


def inliers_ref(H, src, dst, threshold):
    """mask [..., m] of H [..., 9] over the matches"""
    with np.errstate(all="ignore"):
        H = np.asarray(H, np.float64)[..., None]
        x, y, u, v = (np.asarray(a, np.float32).astype(np.float64) for a in (src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]))
        t2 = float(np.float32(threshold)) * float(np.float32(threshold))
        X = (H[..., 0, :] * x + H[..., 1, :] * y) + H[..., 2, :]
        Y = (H[..., 3, :] * x + H[..., 4, :] * y) + H[..., 5, :]
        W = (H[..., 6, :] * x + H[..., 7, :] * y) + H[..., 8, :]
        ex, ey = X - u * W, Y - v * W
        return (W > 0.0) & (ex * ex + ey * ey <= t2 * (W * W))


def counts_ref(H_all, src, dst, threshold):
    return np.concatenate([inliers_ref(H_all[h0:h0 + 256], src, dst, threshold).sum(axis=1) for h0 in range(0, len(H_all), 256)]).astype(np.int32)


def select_ref(counts):
    """the best hypothesis: largest count, smallest h; -1 when every count is 0"""
    best = max(range(len(counts)), key=lambda h: (int(counts[h]), -h))
    return best if counts[best] > 0 else -1


def _hartley(pts):
    sx = sy = 0.0
    for x, y in pts:
        sx += x
        sy += y
    n = float(len(pts))
    cx, cy = sx / n, sy / n
    sd = 0.0
    for x, y in pts:
        dx, dy = x - cx, y - cy
        sd += math.sqrt(dx * dx + dy * dy)
    d = sd / n
    if not (d > 0.0) or not (d <= DBL_MAX):
        return None
    return cx, cy, 1.4142135623730951 / d


def _mul3(A, B):
    return [(A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def refit_round_ref(src, dst, mask):
    """H' [9] of one round on the inliers of mask, None when the round is rejected; Python floats are IEEE doubles"""
    src, dst = np.asarray(src, np.float32).astype(np.float64), np.asarray(dst, np.float32).astype(np.float64)
    sel = np.flatnonzero(mask)
    if len(sel) == 0:
        return None
    ps, pd = [tuple(map(float, p)) for p in src[sel]], [tuple(map(float, p)) for p in dst[sel]]
    hs, hd = _hartley(ps), _hartley(pd)
    if hs is None or hd is None:
        return None
    (cxs, cys, ss), (cxd, cyd, sd) = hs, hd
    N, r = np.zeros((8, 8)), np.zeros(8)
    for (px, py), (pu, pv) in zip(ps, pd):
        x, y, u, v = (px - cxs) * ss, (py - cys) * ss, (pu - cxd) * sd, (pv - cyd) * sd
        a1 = np.array([x, y, 1.0, 0.0, 0.0, 0.0, -(u * x), -(u * y)])
        a2 = np.array([0.0, 0.0, 0.0, x, y, 1.0, -(v * x), -(v * y)])
        N = N + (np.outer(a1, a1) + np.outer(a2, a2))
        r = r + (a1 * u + a2 * v)
    floor_pivot = 1e-12 * float(np.abs(N).max())
    N, r = [[float(v) for v in row] for row in N], [float(v) for v in r]
    for k in range(8):
        piv, best = k, abs(N[k][k])
        for i in range(k + 1, 8):
            if abs(N[i][k]) > best:
                piv, best = i, abs(N[i][k])
        if not best > floor_pivot:
            return None
        N[k], N[piv], r[k], r[piv] = N[piv], N[k], r[piv], r[k]
        for i in range(k + 1, 8):
            f = N[i][k] / N[k][k]
            for q in range(k + 1, 8):
                N[i][q] = N[i][q] - f * N[k][q]
            r[i] = r[i] - f * r[k]
    h = [0.0] * 8
    for i in range(7, -1, -1):
        acc = r[i]
        for q in range(i + 1, 8):
            acc = acc - N[i][q] * h[q]
        h[i] = acc / N[i][i]
    isd = 1.0 / sd
    T = _mul3([isd, 0.0, cxd, 0.0, isd, cyd, 0.0, 0.0, 1.0], h + [1.0])
    T = _mul3(T, [ss, 0.0, -(ss * cxs), 0.0, ss, -(ss * cys), 0.0, 0.0, 1.0])
    with np.errstate(all="ignore"):
        Hn, ok = normalise_ref(np.array(T, np.float64).reshape(9, 1))
    if not ok[0]:
        return None
    Hn = [float(v) for v in Hn[:, 0]]
    W = (Hn[6] * ps[0][0] + Hn[7] * ps[0][1]) + Hn[8]
    if W == 0.0:
        return None
    return np.array([-v for v in Hn] if W < 0.0 else Hn, np.float64)


def verify_ref(src, dst, threshold=3.0, n_hyp=2048, seed=0, refine=2):
    """The whole rule: dict of H_all [n, 9], valid, idx, counts, best, H [9], mask [m] bool, count, rounds (every H' formed) and
    trail (the count after the selection and after every accepted round)."""
    src, dst = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    H_all, valid, idx = hypotheses_ref(src, dst, seed, n_hyp)
    counts = counts_ref(H_all, src, dst, threshold)
    best = select_ref(counts)
    out = dict(H_all=H_all, valid=valid, idx=idx, counts=counts, best=best, H=np.zeros(9), mask=np.zeros(len(src), bool), count=0, rounds=[], trail=[])
    if best < 0:
        return out
    H = H_all[best].copy()
    mask = inliers_ref(H, src, dst, threshold)
    count = int(mask.sum())
    out["trail"].append(count)
    for _ in range(refine):
        Hn = refit_round_ref(src, dst, mask)
        if Hn is None:
            break
        out["rounds"].append(Hn)
        trial = inliers_ref(Hn, src, dst, threshold)
        if int(trial.sum()) < count:
            break
        same = np.array_equal(trial, mask)
        H, mask, count = Hn, trial, int(trial.sum())
        out["trail"].append(count)
        if same:
            break
    out.update(H=H, mask=mask, count=count)
    return out


# ---- the cases, shared with the GPU tests ------------------------------------------------------------------------------------
H_PLANTED = np.array([[0.92, -0.11, 140.0], [0.08, 1.05, -60.0], [1.5e-5, -1.0e-5, 1.0]])


def planted_case(m, outliers, seed):
    """(src, dst [m,2] f32, planted [m] bool): a homography on a 4000 x 3000 frame with 0.5-pixel noise; the fraction `outliers` of
    the matches is uniform in the frame on both sides"""
    rng = np.random.default_rng(seed)
    src = rng.uniform((0, 0), (4000, 3000), (m, 2))
    p = np.c_[src, np.ones(m)] @ H_PLANTED.T
    dst = p[:, :2] / p[:, 2:] + rng.normal(0, 0.5, (m, 2))
    planted = np.ones(m, bool)
    planted[rng.permutation(m)[:int(round(outliers * m))]] = False
    dst[~planted] = rng.uniform((0, 0), (4000, 3000), (int((~planted).sum()), 2))
    return src.astype(np.float32), dst.astype(np.float32), planted


def collinear_case(m=64):
    t = np.arange(m, dtype=np.float32)
    return np.c_[10 + 7 * t, 20 + 3 * t].astype(np.float32), np.c_[5 + 2 * t, 400 - 5 * t].astype(np.float32)


def translation_case(m=200, seed=3):
    """integer points and an exact integer translation: every valid hypothesis has all m matches as inliers"""
    src = np.random.default_rng(seed).integers(0, 2000, (m, 2)).astype(np.float32)
    return src, src + np.array([37, -12], np.float32)


def nan_case(m=120, seed=4):
    """a planted case without outliers whose rows 0, 5 and 17 hold a NaN on one side or the other"""
    src, dst, _ = planted_case(m, 0.0, seed)
    src[0, 0] = dst[5, 1] = src[17, 1] = np.nan
    return src, dst, [0, 5, 17]


def far_case(m=150, seed=5):
    """coordinates that reach +-2^20: a similarity of points spread over the whole permitted square"""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-2.0 ** 20, 2.0 ** 20, (m, 2))
    src[:4] = [(-2.0 ** 20, -2.0 ** 20), (2.0 ** 20, -2.0 ** 20), (2.0 ** 20, 2.0 ** 20), (-2.0 ** 20, 2.0 ** 20)]
    dst = np.clip(src @ np.array([[0.6, 0.3], [-0.3, 0.6]]).T + (1000, -3000), -2.0 ** 20, 2.0 ** 20)
    return src.astype(np.float32), dst.astype(np.float32)


_cache = {}


def reference(name):
    """(src, dst, verify_ref at n_hyp = 2048, seed 0, refine 2, threshold 3) of the named case, computed once and left unchanged"""
    if name not in _cache:
        src, dst = {"planted257": lambda: planted_case(257, 0.5, 1)[:2], "planted1000": lambda: planted_case(1000, 0.75, 2)[:2],
                    "collinear": collinear_case, "translation": translation_case, "nan": lambda: nan_case()[:2], "far": far_case}[name]()
        _cache[name] = (src, dst, verify_ref(src, dst))
    return _cache[name]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the header through the shim ---------------------------------------------------------------------------------------------
def build_shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libverifyshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), os.path.join(SHIM, "verify_rules_shim.cpp")])
    return bind(C.CDLL(str(out)))


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return build_shim(tmp_path_factory)


def bind(L):
    L.shim_verify_score_chunk.restype = C.c_int
    L.shim_verify_mix.argtypes, L.shim_verify_mix.restype = [C.c_uint64], C.c_uint64
    L.shim_verify_sample.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, i32p]
    L.shim_verify_model.argtypes = [f64p, f64p]
    L.shim_verify_hypotheses.argtypes = [f32p, f32p, C.c_int64, C.c_int32, C.c_uint64, f64p, i32p, u8p]
    L.shim_verify_hypotheses.restype = None
    L.shim_verify_counts.argtypes = [f32p, f32p, C.c_int64, C.c_float, f64p, C.c_int32, i32p]
    L.shim_verify_counts.restype = None
    L.shim_verify_mask.argtypes, L.shim_verify_mask.restype = [f32p, f32p, C.c_int64, C.c_float, f64p, u8p], C.c_int64
    L.shim_verify_select.argtypes, L.shim_verify_select.restype = [i32p, C.c_int32], C.c_int32
    L.shim_verify_refit_round.argtypes = [f32p, f32p, C.c_int64, u8p, f64p]
    L.shim_verify.argtypes = [f32p, f32p, C.c_int64, C.c_float, C.c_int32, C.c_uint64, C.c_int32, f64p, i32p, f64p, u8p, i64p, i32p, f64p, i32p]
    L.shim_verify.restype = None
    return L


def shim_sample(L, seed, h, m):
    idx = np.zeros(4, np.int32)
    ok = L.shim_verify_sample(seed, h, m, idx.ctypes.data_as(i32p))
    return idx.tolist(), bool(ok)


def shim_hypotheses(L, src, dst, seed, n_hyp):
    src, dst = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    H, idx, valid = np.empty((n_hyp, 9)), np.empty((n_hyp, 4), np.int32), np.empty(n_hyp, np.uint8)
    L.shim_verify_hypotheses(src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p), len(src), n_hyp, seed, H.ctypes.data_as(f64p), idx.ctypes.data_as(i32p),
                             valid.ctypes.data_as(u8p))
    return H, valid.astype(bool), idx


def shim_verify(L, src, dst, threshold=3.0, n_hyp=2048, seed=0, refine=2):
    """the header's whole rule, shaped like verify_ref's answer (without idx, valid and trail)"""
    src, dst = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    m = len(src)
    H_all, counts, H, mask = np.empty((n_hyp, 9)), np.empty(n_hyp, np.int32), np.empty(9), np.empty(m, np.uint8)
    rounds, count, best, n_rounds = np.zeros((max(refine, 1), 9)), C.c_int64(), C.c_int32(), C.c_int32()
    L.shim_verify(src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p), m, threshold, n_hyp, seed, refine, H_all.ctypes.data_as(f64p),
                  counts.ctypes.data_as(i32p), H.ctypes.data_as(f64p), mask.ctypes.data_as(u8p), C.byref(count), C.byref(best),
                  rounds.ctypes.data_as(f64p), C.byref(n_rounds))
    return dict(H_all=H_all, counts=counts, best=best.value, H=H, mask=mask.astype(bool), count=count.value, rounds=list(rounds[:n_rounds.value]))


def same_answer(got, want):
    """every part of two answers that both hold, bit for bit"""
    return (np.array_equal(bits(got["H_all"]), bits(want["H_all"])) and np.array_equal(got["counts"], want["counts"]) and got["best"] == want["best"]
            and np.array_equal(bits(got["H"]), bits(want["H"])) and np.array_equal(got["mask"], want["mask"]) and got["count"] == want["count"]
            and len(got["rounds"]) == len(want["rounds"]) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(got["rounds"], want["rounds"])))


# ---- the sampler -------------------------------------------------------------------------------------------------------------
def test_sampler_against_hand_computed_values_and_the_restatement(rules):
    assert rules.shim_verify_mix(0) == 0 and rules.shim_verify_mix(G) == 0xE220A8397B1DCDAF      # splitmix64's first output from state 0
    # worked by hand from the rule (Python integers): seed 0, h 0, m 1000 and seed 2^63 + 12345, h 77, m 5 (three draws repeat)
    assert shim_sample(rules, 0, 0, 1000) == (HAND_A, True) and sample_ref(0, 0, 1000) == (HAND_A, True)
    assert shim_sample(rules, 2 ** 63 + 12345, 77, 5) == (HAND_B, True) and sample_ref(2 ** 63 + 12345, 77, 5) == (HAND_B, True)
    failed = 0
    for m in (4, 5, 7, 1000, 2 ** 31 - 1):
        for seed in (0, 1, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0):
            for h in list(range(40)) + [255, 256, 65535, 2 ** 20 - 1]:
                idx, ok = shim_sample(rules, seed, h, m)
                assert (idx, ok) == sample_ref(seed, h, m), (seed, h, m)
                found = [j for j in idx if j >= 0]
                assert len(set(found)) == len(found) and all(0 <= j < m for j in found) and ok == (len(found) == 4)
                failed += not ok
    assert 0 < failed < 30                                                   # m = 4: 16 draws sometimes miss one of the four


HAND_A = [431, 26, 970, 106]                                                 # the first four draws
HAND_B = [3, 1, 4, 2]                                                        # of the draws 3, 3, 1, 4, 1, 1, 2


# ---- hypotheses, counts, selection, refit against the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["planted257", "planted1000"])
def test_planted_model_against_the_restatement(rules, name):
    src, dst, want = reference(name)
    m, outliers = (257, 0.5) if name == "planted257" else (1000, 0.75)
    planted = planted_case(m, outliers, 1 if m == 257 else 2)[2]
    H, valid, idx = shim_hypotheses(rules, src, dst, 0, 2048)
    assert np.array_equal(idx, want["idx"]) and np.array_equal(valid, want["valid"]) and np.array_equal(bits(H), bits(want["H_all"]))
    assert (H[~valid] == 0).all() and not valid.all()                        # random pairs reverse an orientation now and then
    wholly = planted[idx].all(axis=1)                                        # a sample of planted matches is valid: its areas span a 4000 x 3000 frame
    assert wholly.sum() >= 5 and valid[wholly].mean() >= 0.9
    scaled = np.abs(H[valid]).max(axis=1)
    assert ((scaled >= 1) & (scaled < 2)).all()
    got = shim_verify(rules, src, dst)
    assert same_answer(got, want)
    # what the rule promises on such data
    own = np.array([inliers_ref(want["H_all"][h], src[idx[h]], dst[idx[h]], 3.0).all() for h in np.flatnonzero(valid)])
    assert own.all()                                                         # a valid hypothesis counts its own four matches
    assert (want["counts"][~valid] == 0).all() and want["counts"][want["best"]] == want["counts"].max()
    assert want["best"] == int(np.flatnonzero(want["counts"] == want["counts"].max())[0])
    print(name, "planted", int(planted.sum()), "counts after selection and rounds", want["trail"])
    assert want["trail"] == sorted(want["trail"]) and 1 <= len(want["rounds"]) <= 2            # no round lowers the count
    assert want["trail"][0] >= 0.9 * planted.sum()                           # the best hypothesis itself, before any refit
    assert want["count"] >= 0.9 * planted.sum() and (want["mask"] & planted).sum() >= 0.9 * planted.sum()
    corners = np.array([(0, 0, 1), (4000, 0, 1), (4000, 3000, 1), (0, 3000, 1)], np.float64)
    a, b = corners @ want["H"].reshape(3, 3).T, corners @ H_PLANTED.T
    assert np.abs(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:]).max() < 3.0     # the planted model, to within the threshold
    # each round on its own: H' of the mask that went in
    mask = inliers_ref(want["H_all"][want["best"]], src, dst, 3.0)
    for Hn in want["rounds"]:
        out = np.empty(9)
        assert rules.shim_verify_refit_round(src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p), m, mask.astype(np.uint8).ctypes.data_as(u8p),
                                             out.ctypes.data_as(f64p)) == 1
        assert np.array_equal(bits(out), bits(Hn))
        mask = inliers_ref(Hn, src, dst, 3.0)


@pytest.mark.parametrize("refine, seed, n_hyp, threshold", [(0, 0, 300, 3.0), (1, 7, 65, 1.5), (8, 2 ** 64 - 1, 1, 3.0), (2, 5, 63, 0.75)])
def test_other_arguments_against_the_restatement(rules, refine, seed, n_hyp, threshold):
    src, dst, _ = reference("planted257")
    assert same_answer(shim_verify(rules, src, dst, threshold, n_hyp, seed, refine), verify_ref(src, dst, threshold, n_hyp, seed, refine))


def test_counts_mask_and_selection_entry_points(rules):
    src, dst, want = reference("planted257")
    counts = np.empty(2048, np.int32)
    rules.shim_verify_counts(src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p), 257, 3.0, want["H_all"].ctypes.data_as(f64p), 2048, counts.ctypes.data_as(i32p))
    assert np.array_equal(counts, want["counts"]) and rules.shim_verify_select(counts.ctypes.data_as(i32p), 2048) == want["best"]
    mask = np.empty(257, np.uint8)
    n = rules.shim_verify_mask(src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p), 257, 3.0, want["H"].ctypes.data_as(f64p), mask.ctypes.data_as(u8p))
    assert n == want["count"] and np.array_equal(mask.astype(bool), want["mask"])
    for c, best in (([0, 0, 0], -1), ([0, 5, 5], 1), ([7, 5, 7], 0), ([0, 0, 1], 2), ([2 ** 31 - 1, 2 ** 31 - 1], 0)):
        a = np.array(c, np.int32)
        assert rules.shim_verify_select(a.ctypes.data_as(i32p), len(a)) == best == select_ref(a)


def test_collinear_points_give_no_model(rules):
    src, dst, want = reference("collinear")
    got = shim_verify(rules, src, dst)
    assert same_answer(got, want)
    assert not want["valid"].any() and got["best"] == -1 and got["count"] == 0 and not got["mask"].any() and (got["H"] == 0).all()
    assert (got["H_all"] == 0).all() and (got["counts"] == 0).all() and got["rounds"] == []


def test_four_matches(rules):
    src, dst, _ = planted_case(4, 0.0, 6)
    want = verify_ref(src, dst, n_hyp=64)
    assert same_answer(shim_verify(rules, src, dst, n_hyp=64), want)
    drawn = (want["idx"] >= 0).all(axis=1)
    assert drawn.sum() >= 48 and all(sorted(i) == [0, 1, 2, 3] for i in want["idx"][drawn].tolist())
    assert want["valid"].any() and (want["counts"][want["valid"]] == 4).all() and want["count"] == 4     # one model: the four matches'
    assert want["best"] == int(np.flatnonzero(want["valid"])[0])


def test_a_nan_row_is_never_an_inlier(rules):
    src, dst, rows = nan_case()
    _, _, want = reference("nan")
    assert same_answer(shim_verify(rules, src, dst), want)
    holds = np.isin(want["idx"], rows).any(axis=1)
    assert holds.sum() > 100 and not want["valid"][holds].any() and (want["counts"][holds] == 0).all()
    assert want["count"] == len(src) - 3 and not want["mask"][rows].any() and np.isfinite(want["H"]).all()
    assert not inliers_ref(want["H_all"], src, dst, 3.0)[:, rows].any()


def test_coordinates_up_to_two_to_the_20(rules):
    src, dst, want = reference("far")
    assert np.abs(src).max() == 2.0 ** 20 and np.abs(dst).max() > 2.0 ** 19
    assert same_answer(shim_verify(rules, src, dst), want)
    assert np.isfinite(want["H_all"]).all() and np.isfinite(want["H"]).all() and all(np.isfinite(r).all() for r in want["rounds"])
    assert want["valid"].sum() > 1000 and want["count"] >= 0.9 * len(src)


def test_an_exact_translation_ties_and_the_smallest_hypothesis_wins(rules):
    src, dst, want = reference("translation")
    assert same_answer(shim_verify(rules, src, dst), want)
    m = len(src)
    assert want["valid"].sum() > 1000 and (want["counts"][want["valid"]] == m).all()
    assert want["best"] == int(np.flatnonzero(want["valid"])[0]) and want["count"] == m
    Hn = want["H"].reshape(3, 3) / want["H"][8]
    assert np.abs(Hn - np.array([[1, 0, 37], [0, 1, -12], [0, 0, 1]])).max() < 1e-6


def test_model_entry_point_on_degenerate_samples(rules):
    """three collinear points, a reflection (orientation reversed), areas of exactly 1 (not above 1), an infinite coordinate"""
    sq = [(0, 0), (1, 0), (1, 1), (0, 1)]
    cases = [([(0, 0), (5, 5), (10, 10), (3, 9)], [(0, 0), (5, 0), (5, 5), (0, 5)]),
             ([(0, 0), (9, 0), (9, 9), (0, 9)], [(9, 0), (0, 0), (0, 9), (9, 9)]),
             (sq, sq), ([(2 * x, 2 * y) for x, y in sq], [(2 * x, 2 * y) for x, y in sq]),
             ([(0, 0), (9, 0), (9, 9), (0, float("inf"))], [(0, 0), (9, 0), (9, 9), (0, 9)])]
    want_valid = [False, False, False, True, False]
    for (s, d), wv in zip(cases, want_valid):
        pts = np.array([a + b for a, b in zip(s, d)], np.float64)
        H = np.full(9, 7.0)
        ok = rules.shim_verify_model(pts.ctypes.data_as(f64p), H.ctypes.data_as(f64p))
        Hr, vr = model_ref(*(pts[:, k].reshape(4, 1) for k in range(4)))
        assert bool(ok) == wv == bool(vr[0]) and np.array_equal(bits(H), bits(Hr[0])) and (wv or (H == 0).all())


# ---- the header's host loops under the sanitizers, as a program of its own -----------------------------------------------------
def test_host_loops_under_address_and_undefined_sanitizers(tmp_path):
    exe = tmp_path / "verify_asan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(SHIM, "verify_asan_main.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "verify_asan: ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
