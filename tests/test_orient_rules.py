"""CPU tests of the orientation rule (opencv-dlco_amd/csrc/orient_rules.hpp, through tests/shim/orient_rules_shim.cpp) against
the numpy restatement below, which the GPU tests (tests/test_orient_gpu.py) use as well.  Vectors, status and the bits of an
angle are compared with equality.  Nothing here needs a GPU or libdlco.so."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from test_detect_rules import box_ref, integral_ref
from test_keypoints_gpu import frame_ref, patch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64p, i32p, u32p, u8p, f32p = (C.POINTER(t) for t in (C.c_int64, C.c_int32, C.c_uint32, C.c_uint8, C.c_float))


# ---- the rule restated in numpy: int64 sums that never wrap, Python integers for the score ------------------------------
W_REF = [int(math.floor(1024 * math.exp(-d2 / 8.0) + 0.5)) for d2 in range(36)]
B9 = [(1024, 0), (1008, 178), (962, 350), (887, 512), (784, 658), (658, 784), (512, 887), (350, 962), (178, 1008)]
B_REF = list(B9)
for _k in range(9, 36):
    B_REF.append((-B_REF[_k - 9][1], B_REF[_k - 9][0]))
OFFSETS = [(i, j) for j in range(-6, 7) for i in range(-6, 7) if i * i + j * j < 36]


def centre_ref(x, y, size):
    """(X, Y, s) of a keypoint as the library sees it (f32 in, double arithmetic), None when it is invalid."""
    x, y, size = (float(np.float32(v)) for v in (x, y, size))
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(size)) or not size > 0 or abs(x) > 2 ** 20 or abs(y) > 2 ** 20:
        return None
    s = min(128.0, max(1.0, math.floor(size / 7.5 + 0.5)))
    return int(math.floor(x + 0.5)), int(math.floor(y + 0.5)), int(s)


def windows_ref(S, kp):
    """(status, [(score, k, SX, SY) for the 36 windows]) of one keypoint on the int64 integral image S; status 0: no windows."""
    c = centre_ref(kp[0], kp[1], kp[2])
    if c is None:
        return 0, []
    X, Y, s = c
    H, W = S.shape[0] - 1, S.shape[1] - 1
    I, J = (np.array(v, np.int64) for v in zip(*OFFSETS))
    cx, cy, h = X + I * s, Y + J * s, 2 * s
    used = (cx - h >= 0) & (cx + h <= W - 1) & (cy - h >= 0) & (cy + h <= H - 1)
    I, J, cx, cy = I[used], J[used], cx[used], cy[used]
    dx = box_ref(S, cx + 1, cy - h, cx + h, cy + h) - box_ref(S, cx - h, cy - h, cx - 1, cy + h)
    dy = box_ref(S, cx - h, cy + 1, cx + h, cy + h) - box_ref(S, cx - h, cy - h, cx + h, cy - 1)
    norm = lambda d: np.sign(d) * ((16 * np.abs(d) + 4 * s * s) // (8 * s * s))
    w = np.array(W_REF, np.int64)[I * I + J * J]
    gx, gy = w * norm(dx), w * norm(dy)
    assert len(gx) == 0 or max(np.abs(gx).max(), np.abs(gy).max()) <= 1024 * 5100
    cr = np.array([bx * gy - by * gx for bx, by in B_REF])                   # [36, samples]
    nonzero = (gx != 0) | (gy != 0)
    member = (cr >= 0) & (np.roll(cr, -1, axis=0) < 0) & nonzero
    assert (member.sum(axis=0) == nonzero).all()                             # exactly one bin for a non-zero g
    HX = [int(gx[member[k]].sum()) for k in range(36)]
    HY = [int(gy[member[k]].sum()) for k in range(36)]
    wins = []
    for k in range(36):
        SX, SY = sum(HX[(k + t) % 36] for t in range(6)), sum(HY[(k + t) % 36] for t in range(6))
        assert SX * SX + SY * SY < 2 ** 60
        wins.append((SX * SX + SY * SY, k, SX, SY))
    return (2 if used.all() else 1), wins


def orient_ref(img, kps):
    """(vectors [n,2] i64, status [n] u8, tied [n] bool) of keypoints [n,4] on img; tied: another window has the winner's score and another
    vector (windows that hold the same samples tie too, but whichever of them wins, the vector is theirs)."""
    S = integral_ref(img)
    vec, st, tied = np.zeros((len(kps), 2), np.int64), np.zeros(len(kps), np.uint8), np.zeros(len(kps), bool)
    for n, kp in enumerate(np.asarray(kps, np.float32)):
        st[n], wins = windows_ref(S, kp)
        if wins:
            order = sorted(wins, key=lambda t: (-t[0], t[1]))
            vec[n] = order[0][2:]
            tied[n] = any(w[0] == order[0][0] and w[2:] != order[0][2:] for w in order[1:])
    return vec, st, tied


def angle_ref(SX, SY):
    if SX == 0 and SY == 0:
        return np.float32(-1)
    a = math.atan2(float(SY), float(SX)) * 180.0 / math.pi
    a = a + 360.0 if a < 0 else a
    f = np.float32(a)
    return np.float32(0) if f >= 360 else f


def noise_image_96():
    """96 x 128 uniform noise inside rows of 144 bytes; the padding holds other values."""
    return np.random.default_rng(41).integers(0, 256, (96, 144), dtype=np.uint8)[:, :128]


def smooth_image(H, W, seed, pitch=None):
    """Smooth random H x W image, in integers throughout: noise under three 9 x 9 box filters (wrapped), stretched to 0 .. 255."""
    a = np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.int64)
    for _ in range(3):
        a = sum(np.roll(a, d, axis=0) for d in range(-4, 5))
        a = sum(np.roll(a, d, axis=1) for d in range(-4, 5))
    a = (a - a.min()) * 255 // (a.max() - a.min())
    buf = np.full((H, pitch or W), 77, np.uint8)
    buf[:, :W] = a
    return buf[:, :W]


def case_keypoints(H, W, n=300, seed=5):
    """n keypoints on an H x W image: sizes that give s = 1, 2, 3, 5 (and 2 through the tie 11.25 / 7.5 + 0.5 = 2), centres in the
    middle, near every border (samples partly skipped), on the four corner pixels, at non-integer positions including .5, and
    outside the image; four invalid ones."""
    rng = np.random.default_rng(seed)
    sizes = [9, 15, 21, 39, 11.25]
    kp = [(0, 0, 9, -1), (W - 1, 0, 15, 0), (0, H - 1, 21, 90), (W - 1, H - 1, 9, 10), (-3, 5, 9, 0), (W + 10, H / 2, 15, 0), (1e5, -1e5, 9, 0),
          (W / 2 + 0.5, H / 2 - 0.5, 39, 0), (W / 2 - 0.5, H / 2 + 0.25, 9, 0), (W / 2, H / 2, 21, 45), (W / 2, H / 2, 39, 359), (17.5, 16.5, 9, 0),
          (float("nan"), 10, 9, 0), (10, float("inf"), 9, 0), (10, 10, 0, 0), (2.0 ** 20 + 1, 10, 9, 0)]
    while len(kp) < n:
        size = sizes[len(kp) % len(sizes)]
        where = len(kp) % 3
        if where == 0:                                                       # the middle: every sample of s = 1 .. 3 is used
            x, y = rng.uniform(30, W - 31), rng.uniform(30, H - 31)
        elif where == 1:                                                     # anywhere, a little beyond the border too
            x, y = rng.uniform(-4, W + 3), rng.uniform(-4, H + 3)
        else:                                                                # integers and halves
            x, y = rng.integers(0, 2 * W) / 2.0, rng.integers(0, 2 * H) / 2.0
        kp.append((x, y, size, float(rng.uniform(-1, 360))))
    return np.array(kp[:n], np.float32)


_cache = {}


def reference(name):
    """(img, keypoints, vectors, status) of the two images of the parity tests, computed once."""
    if name not in _cache:
        img = noise_image_96() if name == "noise" else smooth_image(97, 131, 42, pitch=160)
        kp = case_keypoints(*img.shape)
        vec, st, _ = orient_ref(img, kp)
        _cache[name] = (img, kp, vec, st)
    return _cache[name]


def meaning_case():
    """A smooth 160 x 200 image, its quarter turn and 24 keypoints of size 9 .. 15 kept 50 pixels off the border, with the
    keypoints' places in the turned image: np.rot90 takes the pixel (x, y) to (y, W - 1 - x)."""
    img = smooth_image(160, 200, 43)
    rng = np.random.default_rng(44)
    kp = np.array([(rng.integers(50, 150), rng.integers(50, 110), rng.uniform(9, 15), -1) for _ in range(24)], np.float32)
    turned = np.ascontiguousarray(np.rot90(img))
    kpt = kp.copy()
    kpt[:, 0], kpt[:, 1] = kp[:, 1], img.shape[1] - 1 - kp[:, 0]
    return img, kp, turned, kpt


def patch_differences(img, kp, turned, kpt):
    """per keypoint the mean absolute difference of the patches of the two images at scale factor 6.25: (oriented, upright)"""
    diff = lambda p, q: float(np.abs(p.astype(np.int64) - q.astype(np.int64)).mean())
    oriented, upright = [], []
    for a, b in zip(kp, kpt):
        pa, pb = (patch_ref(im, frame_ref(*k, scale_factor=6.25))[0] for im, k in ((img, a), (turned, b)))
        ua, ub = (patch_ref(im, frame_ref(*k, scale_factor=6.25, use_orientation=False))[0] for im, k in ((img, a), (turned, b)))
        oriented.append(diff(pa, pb))
        upright.append(diff(ua, ub))
    return oriented, upright


# ---- the header through the shim ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "liborientshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(ROOT, "tests", "shim", "orient_rules_shim.cpp")])
    return bind(C.CDLL(str(out)))


def bind(L):
    L.shim_orient_tables.argtypes = [i32p, i64p]
    L.shim_orient_tables.restype = None
    L.shim_orient_offsets.argtypes = [i32p]
    L.shim_orient_offsets.restype = None
    L.shim_orient_centre.argtypes = [C.c_float, C.c_float, C.c_float, i32p]
    L.shim_orient_centre.restype = None
    L.shim_orient_bin.argtypes = [C.c_int64, C.c_int64]
    L.shim_orient_bin.restype = C.c_int
    L.shim_orient_angle_of.argtypes = [C.c_int64, C.c_int64]
    L.shim_orient_angle_of.restype = C.c_float
    L.shim_orient.argtypes = [u32p, C.c_int, C.c_int, f32p, C.c_int64, i64p, u8p, f32p]
    L.shim_orient.restype = None
    return L


def orient(L, img, kp):
    """(vectors, status, angles) of the header's rule on the uint32 integral image of img"""
    H, W = img.shape
    S = np.ascontiguousarray((integral_ref(img) % 2 ** 32).astype(np.uint32))
    kp = np.ascontiguousarray(kp, np.float32)
    vec, st, ang = np.zeros((len(kp), 2), np.int64), np.zeros(len(kp), np.uint8), np.zeros(len(kp), np.float32)
    L.shim_orient(S.ctypes.data_as(u32p), W, H, kp.ctypes.data_as(f32p), len(kp), vec.ctypes.data_as(i64p), st.ctypes.data_as(u8p),
                  ang.ctypes.data_as(f32p))
    return vec, st, ang


def angles_of(L, vec):
    return np.array([L.shim_orient_angle_of(int(x), int(y)) for x, y in vec], np.float32)


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_tables_and_sample_order(rules):
    w, b, ij = np.zeros(36, np.int32), np.zeros((36, 2), np.int64), np.zeros((109, 2), np.int32)
    rules.shim_orient_tables(w.ctypes.data_as(i32p), b.ctypes.data_as(i64p))
    rules.shim_orient_offsets(ij.ctypes.data_as(i32p))
    assert w.tolist() == W_REF and W_REF[:4] == [1024, 904, 797, 704] and W_REF[-1] == 13
    assert min(abs(1024 * math.exp(-d2 / 8.0) % 1 - 0.5) for d2 in range(36)) > 0.0079    # no weight near a rounding tie
    assert [tuple(v) for v in b[:9].tolist()] == B9 and [tuple(v) for v in b.tolist()] == B_REF
    for k in range(36):
        (ax, ay), (bx, by) = B_REF[k], B_REF[(k + 1) % 36]
        assert ax * by - ay * bx > 0                                         # strictly counter-clockwise
        assert tuple(b[(k + 9) % 36]) == (-b[k][1], b[k][0])
        assert abs(ax - 1024 * math.cos(math.radians(10 * k))) < 1 and abs(ay - 1024 * math.sin(math.radians(10 * k))) < 1
    assert len(OFFSETS) == 109 and [tuple(v) for v in ij.tolist()] == OFFSETS


def test_bins_on_and_beside_the_boundaries(rules):
    assert rules.shim_orient_bin(0, 0) == -1
    for k in range(36):
        bx, by = B_REF[k]
        assert rules.shim_orient_bin(bx, by) == k                            # on a boundary: the bin that starts there
        assert rules.shim_orient_bin(5000 * bx + by, 5000 * by - bx) == (k - 1) % 36      # a hair clockwise of it
        assert rules.shim_orient_bin(5000 * bx - by, 5000 * by + bx) == k
    assert [rules.shim_orient_bin(*g) for g in ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-5222400, -1))] == [0, 9, 18, 27, 4, 18]
    # the definition itself on random vectors, small ones (many on a boundary or an axis) and the largest a sample can give
    rng = np.random.default_rng(40)
    for lim in (4, 1100, 1024 * 5100):
        for gx, gy in rng.integers(-lim, lim + 1, (1500, 2)):
            gx, gy = int(gx), int(gy)
            cr = [bx * gy - by * gx for bx, by in B_REF]
            want = [k for k in range(36) if cr[k] >= 0 and cr[(k + 1) % 36] < 0] if (gx, gy) != (0, 0) else [-1]
            assert [rules.shim_orient_bin(gx, gy)] == want, (gx, gy)


def test_centre_and_scale(rules):
    out = np.zeros(4, np.int32)
    cases = [(10.5, 7.49, 9), (-0.5, -0.51, 15), (3.5, 2.5, 11.25), (0, 0, 0.1), (260, 260, 1e30), (5, 5, 963.75), (5, 5, 956.2), (1048576, -1048576, 195),
             (float("nan"), 0, 9), (0, float("-inf"), 9), (0, 0, float("inf")), (0, 0, float("nan")), (0, 0, 0), (0, 0, -3), (1048577, 0, 9), (0, -1048577, 9)]
    for x, y, size in cases:
        rules.shim_orient_centre(x, y, size, out.ctypes.data_as(i32p))
        want = centre_ref(x, y, size)
        assert (tuple(out[:3]) if out[3] else None) == want, (x, y, size)
    assert centre_ref(10.5, 7.49, 9) == (11, 7, 1) and centre_ref(-0.5, -0.51, 15) == (0, -1, 2) and centre_ref(3.5, 2.5, 11.25) == (4, 3, 2)
    assert centre_ref(0, 0, 0.1)[2] == 1 and centre_ref(0, 0, 1e30)[2] == 128 and centre_ref(0, 0, 195)[2] == 26 and centre_ref(0, 0, 9)[2] == 1


@pytest.mark.parametrize("name", ["noise", "smooth"])
def test_vectors_and_status_against_the_restatement(rules, name):
    img, kp, want_vec, want_st = reference(name)
    assert img.shape == ((96, 128) if name == "noise" else (97, 131)) and img.strides[0] > img.shape[1]
    vec, st, ang = orient(rules, img, kp)
    assert np.array_equal(st, want_st) and np.array_equal(vec, want_vec)
    assert np.array_equal(fbits(ang), fbits([angle_ref(int(x), int(y)) for x, y in want_vec]))
    # what the cases cover: every status, every scale with all samples used, vectors in all four quadrants
    s = np.array([(centre_ref(*k[:3]) or (0, 0, 0))[2] for k in kp])
    assert set(s.tolist()) == {0, 1, 2, 3, 5} and all(((s == v) & (st == 2)).any() and ((s == v) & (st == 1)).any() for v in (1, 2, 3, 5))
    assert (st == 0).sum() == 4 and (vec[st == 0] == 0).all() and (ang[st == 0] == -1).all()
    live = vec[(vec != 0).any(axis=1)]
    assert len(live) >= 250 and all(((np.sign(live[:, 0]) == a) & (np.sign(live[:, 1]) == b)).any() for a in (-1, 1) for b in (-1, 1))
    # a keypoint wholly outside has no sample: status 1 and no vector
    far = np.flatnonzero((kp[:, 0] == 1e5))
    assert len(far) == 1 and st[far[0]] == 1 and (vec[far[0]] == 0).all() and ang[far[0]] == -1
    assert ((ang >= 0) & (ang < 360) | (ang == -1)).all()


def test_invalid_keypoints(rules):
    img = noise_image_96()
    nan, inf = float("nan"), float("inf")
    kp = np.array([(nan, 5, 9, 0), (5, nan, 9, 0), (5, 5, nan, 0), (inf, 5, 9, 0), (5, -inf, 9, 0), (5, 5, inf, 0), (5, 5, 0, 0), (5, 5, -9, 0),
                   (2.0 ** 20 + 1, 5, 9, 0), (5, -2.0 ** 20 - 1, 9, 0), (64, 48, 9, nan)], np.float32)
    vec, st, ang = orient(rules, img, kp)
    want_vec, want_st, _ = orient_ref(img, kp)
    assert np.array_equal(vec, want_vec) and np.array_equal(st, want_st)
    assert (st[:10] == 0).all() and (vec[:10] == 0).all() and (ang[:10] == -1).all()
    assert st[10] == 2 and vec[10].any()                                     # the incoming angle is ignored, NaN or not


def test_size_extremes(rules):
    img = np.random.default_rng(45).integers(0, 256, (520, 520), dtype=np.uint8)
    kp = np.array([(260, 260, 1e30, 0), (260, 260, 0.1, 0), (260, 260, 195, 0), (260, 260, 960, 0), (250, 270, 3e38, 0)], np.float32)
    assert [centre_ref(*k[:3])[2] for k in kp] == [128, 1, 26, 128, 128]
    vec, st, ang = orient(rules, img, kp)
    want_vec, want_st, _ = orient_ref(img, kp)
    assert np.array_equal(vec, want_vec) and np.array_equal(st, want_st) and st.tolist() == [1, 2, 2, 1, 1]
    # s = 128 at the centre of 520 x 520: the Haar square of 513 pixels fits for the sample (0, 0) alone, which has weight 1024
    S = integral_ref(img)
    dx = int(box_ref(S, 261, 4, 516, 516) - box_ref(S, 4, 4, 259, 516))
    dy = int(box_ref(S, 4, 261, 516, 516) - box_ref(S, 4, 4, 516, 259))
    norm = lambda d: (1 if d >= 0 else -1) * ((16 * abs(d) + 4 * 128 * 128) // (8 * 128 * 128))
    assert tuple(vec[0]) == (1024 * norm(dx), 1024 * norm(dy)) and tuple(vec[3]) == tuple(vec[0])


def test_a_constant_image_has_no_orientation(rules):
    img = np.full((96, 128), 173, np.uint8)
    kp = np.array([(64, 48, 9, 0), (64, 48, 39, 0), (3, 3, 9, 0)], np.float32)
    vec, st, ang = orient(rules, img, kp)
    assert (vec == 0).all() and (ang == -1).all() and st.tolist() == [2, 2, 1]


def test_a_ramp_points_down_its_gradient(rules):
    """Grey levels that grow along one axis by 2 a pixel: every sample has the same g along that axis, all in one bin, so
    the winning window holds them all: the vector is (sum of the weights) * N(d) along the axis."""
    x = np.arange(128, dtype=np.int64)
    total = sum(W_REF[i * i + j * j] for i, j in OFFSETS)
    n1 = (16 * (2 * 6 * 5) + 4) // 8                                         # s = 1: columns +1, +2 against -2, -1 (6 apart), 5 rows
    for img, want in ((np.tile(2 * x, (96, 1)), (1, 0)), (np.tile(2 * x[::-1], (96, 1)), (-1, 0)), (np.tile(2 * x[:96, None], (1, 128)), (0, 1)),
                      (np.tile(2 * x[:96, None][::-1], (1, 128)), (0, -1))):
        vec, st, ang = orient(rules, img.astype(np.uint8), np.array([(64, 48, 9, 0)], np.float32))
        assert st[0] == 2 and tuple(vec[0]) == (want[0] * total * n1, want[1] * total * n1)
        assert ang[0] == {(1, 0): 0, (0, 1): 90, (-1, 0): 180, (0, -1): 270}[want]


def test_a_quarter_turn_of_the_image_turns_the_vector(rules):
    img = smooth_image(96, 128, 46)
    H, W = img.shape
    rng = np.random.default_rng(47)
    kp = np.array([(rng.integers(0, W), rng.integers(0, H), (9, 15, 21, 39)[n % 4], -1) for n in range(60)], np.float32)
    turned = np.ascontiguousarray(np.rot90(img))                             # the pixel (x, y) goes to (y, W - 1 - x)
    kpt = kp.copy()
    kpt[:, 0], kpt[:, 1] = kp[:, 1], W - 1 - kp[:, 0]
    vec, st, _ = orient(rules, img, kp)
    vect, stt, _ = orient(rules, turned, kpt)
    _, _, tied = orient_ref(img, kp)
    assert tied.sum() <= 3 and (st == 2).sum() >= 10 and (st == 1).sum() >= 10          # at most 5 % may be left out
    keep = ~tied
    assert np.array_equal(stt, st)
    assert np.array_equal(vect[keep, 0], vec[keep, 1]) and np.array_equal(vect[keep, 1], -vec[keep, 0])   # (vx, vy) -> (vy, -vx)
    score = lambda v: [int(a) ** 2 + int(b) ** 2 for a, b in v]
    assert score(vect) == score(vec)                                         # the score is equal even where the winner is a tie


def test_angle_of(rules):
    f = rules.shim_orient_angle_of
    assert [f(1, 0), f(0, 1), f(-1, 0), f(0, -1), f(0, 0)] == [0, 90, 180, 270, -1]
    assert f(10 ** 9, -1) == 0 and f(5 * 10 ** 8, -1) == 0                   # 360 - 6e-8 rounds to 360 in float: 0
    rng = np.random.default_rng(48)
    cases = [(int(a), int(b)) for a, b in rng.integers(-2 ** 30, 2 ** 30, (2000, 2))] + [(int(a), int(b)) for a, b in rng.integers(-3, 4, (200, 2))]
    cases += [(2 ** 30, -1), (2 ** 30, 1), (-2 ** 30, -1), (-2 ** 30, 1), (1, -2 ** 30), (-1, -2 ** 30), (1, 1), (-1, 1), (-1, -1), (1, -1)]
    for SX, SY in cases:
        a = f(SX, SY)
        assert fbits(a) == fbits(angle_ref(SX, SY)), (SX, SY)
        if (SX, SY) == (0, 0):
            assert a == -1
            continue
        assert 0 <= a < 360
        want = math.degrees(math.atan2(SY, SX)) % 360.0
        assert min(abs(a - want), 360 - abs(a - want)) <= 1e-4, (SX, SY, a, want)


def test_assigned_angles_make_patches_of_a_turned_image_agree(rules):
    """What the rule is for.  An image and its quarter turn, patches cut by the patch rule at scale factor 6.25: with the
    assigned angles the two patches of a keypoint differ by at most 1 grey level a pixel on average, upright by at least 10."""
    img, kp, turned, kpt = meaning_case()
    vec, st, ang = orient(rules, img, kp)
    vect, stt, angt = orient(rules, turned, kpt)
    assert (st == 2).all() and (stt == 2).all() and (ang >= 0).all() and (angt >= 0).all()
    kp[:, 3], kpt[:, 3] = ang, angt
    oriented, upright = patch_differences(img, kp, turned, kpt)
    print("oriented: max %.4f, upright: min %.2f" % (max(oriented), min(upright)))
    assert max(oriented) <= 1.0 and min(upright) >= 10.0, (max(oriented), min(upright))
