"""CPU tests of the detector's rule (opencv-dlco_amd/csrc/detect_rules.hpp, through tests/shim/detect_rules_shim.cpp) against
the numpy restatement below, which the GPU tests (tests/test_detect_gpu.py) use as well.  Everything is compared with
equality, the three floats of a keypoint by their bit patterns.  Nothing here needs a GPU or libdlco.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64p, i32p, u32p, u8p, f32p = (C.POINTER(t) for t in (C.c_int64, C.c_int32, C.c_uint32, C.c_uint8, C.c_float))


# ---- the rule restated in numpy: int64 sums that never wrap, float64 for the one division per axis -----------------------
def filter_side(o, i):
    return 3 * (2 ** (o + 1) * (i + 1) + 1)


def margin(o):
    return (filter_side(o, 3) - 1) // 2


def grid_size(extent, o):
    room = extent - 1 - 2 * margin(o)
    return room // 2 ** o + 1 if room >= 0 else 0


def integral_ref(img):
    """S [(H+1), (W+1)] in int64: the true sums, not reduced modulo 2^32."""
    S = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.int64)
    S[1:, 1:] = img.astype(np.int64).cumsum(axis=0).cumsum(axis=1)
    return S


def box_ref(S, x0, y0, x1, y1):
    return S[y1 + 1, x1 + 1] - S[y0, x1 + 1] - S[y1 + 1, x0] + S[y0, x0]


def normalise_ref(D, L):
    q = L * L
    return np.sign(D) * ((256 * np.abs(D) + q // 2) // q)


def responses_ref(img, o):
    """R [4, ny, nx] int64 of octave o."""
    H, W = img.shape
    S = integral_ref(img)
    st, m, nx, ny = 2 ** o, margin(o), grid_size(W, o), grid_size(H, o)
    X, Y = np.meshgrid(m + st * np.arange(nx, dtype=np.int64), m + st * np.arange(ny, dtype=np.int64))
    R = np.zeros((4, ny, nx), np.int64)
    for layer in range(4):
        L = filter_side(o, layer)
        l, h = L // 3, (L - 1) // 2
        hw, hl = l - 1, (l - 1) // 2
        Dyy = box_ref(S, X - hw, Y - h, X + hw, Y + h) - 3 * box_ref(S, X - hw, Y - hl, X + hw, Y + hl)
        Dxx = box_ref(S, X - h, Y - hw, X + h, Y + hw) - 3 * box_ref(S, X - hl, Y - hw, X + hl, Y + hw)
        Dxy = (box_ref(S, X + 1, Y - l, X + l, Y - 1) + box_ref(S, X - l, Y + 1, X - 1, Y + l) - box_ref(S, X - l, Y - l, X - 1, Y - 1)
               - box_ref(S, X + 1, Y + 1, X + l, Y + l))
        R[layer] = 100 * normalise_ref(Dxx, L) * normalise_ref(Dyy, L) - 81 * normalise_ref(Dxy, L) ** 2
    return R


def parabola_ref(Rm, R0, Rp, scale_n, scale_c):
    n, c = Rm - Rp, Rm - 2 * R0 + Rp
    return 0.0 if c == 0 else float(np.float64(scale_n * n) / np.float64(scale_c * c))


def detect_ref(img, n_octaves, threshold, origin=(0, 0)):
    """Every keypoint of img in the rule's order: (kp [n,4] f32, resp [n] i64, where [n,4] i32 = (octave, layer, j, i)).
    origin = (x, y) of img's first pixel when img is a crop of a larger image: added to the grid point before the refinement."""
    found = []
    for o in range(n_octaves):
        R = responses_ref(img, o)
        _, ny, nx = R.shape
        if nx < 3 or ny < 3:
            continue
        st, m = 2 ** o, margin(o)
        for layer in (1, 2):
            centre = R[layer, 1:-1, 1:-1]
            ok = centre >= threshold
            for dl in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    for di in (-1, 0, 1):
                        if (dl, dj, di) == (0, 0, 0):
                            continue
                        nb = R[layer + dl, 1 + dj:ny - 1 + dj, 1 + di:nx - 1 + di]
                        ok &= (centre > nb) if (dl, dj, di) < (0, 0, 0) else (centre >= nb)
            for j, i in zip(*np.nonzero(ok)):
                j, i = int(j) + 1, int(i) + 1
                r0 = int(R[layer, j, i])
                x = np.float32(np.float64(origin[0] + m + st * i) + st * parabola_ref(int(R[layer, j, i - 1]), r0, int(R[layer, j, i + 1]), 1, 2))
                y = np.float32(np.float64(origin[1] + m + st * j) + st * parabola_ref(int(R[layer, j - 1, i]), r0, int(R[layer, j + 1, i]), 1, 2))
                size = np.float32(np.float64(filter_side(o, layer)) + st * parabola_ref(int(R[layer - 1, j, i]), r0, int(R[layer + 1, j, i]), 3, 1))
                found.append((-r0, o, layer, j, i, x, y, size))
    found.sort(key=lambda t: t[:5])
    kp = np.array([(t[5], t[6], t[7], -1.0) for t in found], np.float32).reshape(-1, 4)
    resp = np.array([-t[0] for t in found], np.int64)
    where = np.array([t[1:5] for t in found], np.int32).reshape(-1, 4)
    return kp, resp, where


def bits(kp):
    return np.ascontiguousarray(kp, np.float32).view(np.uint32)


def noise_image():
    """157 x 203 uniform noise inside rows of 224 bytes; the padding holds other values."""
    buf = np.random.default_rng(21).integers(0, 256, (157, 224), dtype=np.uint8)
    return buf[:, :203]


def blob_image(H, W, cx, cy, sigma):
    y, x = np.mgrid[0:H, 0:W]
    return np.rint(128 + 100 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma * sigma))).astype(np.uint8)


_cache = {}


def noise_reference():
    """detect_ref of the noise image at 3 octaves and threshold 1, computed once."""
    if "noise" not in _cache:
        _cache["noise"] = detect_ref(noise_image(), 3, 1)
    return _cache["noise"]


# ---- the header through the shim ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libdetectshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(ROOT, "tests", "shim", "detect_rules_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_detect_geometry.argtypes = [C.c_int, C.c_int, C.c_int, i32p]
    L.shim_detect_geometry.restype = None
    L.shim_detect_normalise.argtypes = [C.c_int64, C.c_int]
    L.shim_detect_normalise.restype = C.c_int64
    L.shim_detect_box.argtypes = [u32p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    L.shim_detect_box.restype = C.c_int64
    L.shim_detect_integral.argtypes = [u8p, C.c_int, C.c_int, C.c_int64, u32p]
    L.shim_detect_integral.restype = None
    L.shim_detect_responses.argtypes = [u32p, C.c_int, C.c_int, C.c_int, i64p]
    L.shim_detect_responses.restype = None
    for f in (L.shim_detect_offset, L.shim_detect_offset6):
        f.argtypes = [C.c_int64, C.c_int64, C.c_int64]
        f.restype = C.c_double
    L.shim_detect.argtypes = [u32p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, f32p, i64p, i32p]
    L.shim_detect.restype = C.c_int64
    return L


def geometry(L, o, i, extent):
    out = np.zeros(4, np.int32)
    L.shim_detect_geometry(o, i, extent, out.ctypes.data_as(i32p))
    return tuple(int(v) for v in out)


def integral(L, img):
    """The header's S [(H+1), (W+1)] u32 of an image whose rows may be strided."""
    H, W = img.shape
    S = np.zeros((H + 1, W + 1), np.uint32)
    L.shim_detect_integral(C.cast(C.c_void_p(img.ctypes.data), u8p), W, H, img.strides[0], S.ctypes.data_as(u32p))
    return S


def detect(L, img, n_octaves, threshold, cap=1 << 16):
    H, W = img.shape
    S = integral(L, img)
    kp, resp, where = np.zeros((cap, 4), np.float32), np.zeros(cap, np.int64), np.zeros((cap, 4), np.int32)
    n = L.shim_detect(S.ctypes.data_as(u32p), W, H, n_octaves, threshold, cap, kp.ctypes.data_as(f32p), resp.ctypes.data_as(i64p),
                      where.ctypes.data_as(i32p))
    return kp[:min(n, cap)], resp[:min(n, cap)], where[:min(n, cap)], n


def test_filter_sides_margins_and_grid_sizes(rules):
    sides = [[geometry(rules, o, i, 100)[0] for i in range(4)] for o in range(4)]
    assert sides == [[9, 15, 21, 27], [15, 27, 39, 51], [27, 51, 75, 99], [51, 99, 147, 195]]
    assert sides == [[filter_side(o, i) for i in range(4)] for o in range(4)]
    assert [geometry(rules, o, 0, 100)[1:3] for o in range(4)] == [(13, 1), (25, 2), (49, 4), (97, 8)]
    assert [margin(o) for o in range(4)] == [13, 25, 49, 97]
    # the grids the GPU tests rely on: 27 has one point, 28 two, 29 three (the smallest with a candidate); a 213 x 230 image
    # has a 3 x 5 grid at octave 3; 26 pixels and 1 pixel have none
    assert [geometry(rules, 0, 0, e)[3] for e in (1, 26, 27, 28, 29, 157, 203)] == [0, 0, 1, 2, 3, 131, 177]
    assert (geometry(rules, 3, 0, 213)[3], geometry(rules, 3, 0, 230)[3]) == (3, 5)
    for o in range(4):
        for extent in list(range(1, 260)) + [4096, 32768]:
            n = geometry(rules, o, 0, extent)[3]
            assert n == grid_size(extent, o)
            if n:                                           # the last grid point still has its margin inside the image
                assert margin(o) + 2 ** o * (n - 1) + margin(o) <= extent - 1 < margin(o) + 2 ** o * n + margin(o)


def test_normalisation_on_both_signs_and_around_the_halves(rules):
    """L^2 is odd and 256 |D| is even, so 256 |D| / L^2 is never an exact half: the nearest cases are a remainder of
    (L^2 - 1) / 2, which rounds down, and of (L^2 + 1) / 2, which rounds up."""
    from fractions import Fraction
    rng = np.random.default_rng(4)
    for L in (9, 15, 21, 27, 39, 51, 75, 99, 147, 195):
        q = L * L
        cases = [0, 1, -1, 255 * q, -255 * q] + [int(v) for v in rng.integers(-255 * q, 255 * q, 200)]
        for r in ((q - 1) // 2, (q + 1) // 2):
            a = r * pow(256, -1, q) % q                      # 256 a = r modulo L^2
            assert (256 * a) % q == r
            cases += [a, -a, a + q, -a - q]
        for D in cases:
            exact = Fraction(256 * abs(D), q)
            want = int(exact + Fraction(1, 2))               # round to nearest: no tie exists
            assert exact - int(exact) != Fraction(1, 2)
            want = want if D >= 0 else -want
            assert rules.shim_detect_normalise(D, L) == want == int(normalise_ref(np.int64(D), L)), (D, L)
        assert rules.shim_detect_normalise(170 * q, L) == 43520 and rules.shim_detect_normalise(-170 * q, L) == -43520


def test_integral_image_and_responses_of_three_octaves(rules):
    img = noise_image()
    assert img.strides == (224, 1)
    S = integral(rules, img)
    assert np.array_equal(S.astype(np.int64), integral_ref(img))          # 157 x 203 x 255 < 2^32: nothing wraps here
    for o in range(3):
        want = responses_ref(img, o)
        got = np.zeros_like(want)
        rules.shim_detect_responses(S.ctypes.data_as(u32p), 203, 157, o, got.ctypes.data_as(i64p))
        assert want.shape == (4, grid_size(157, o), grid_size(203, o)) and np.array_equal(got, want), o
        assert np.abs(want).max() < 2 ** 38 and (want != 0).any()


def test_host_detection_gives_every_keypoint_in_order(rules):
    want_kp, want_resp, want_where = noise_reference()
    kp, resp, where, n = detect(rules, noise_image(), 3, 1)
    per_octave = np.bincount(want_where[:, 0], minlength=3)
    assert len(want_kp) >= 100 and (per_octave >= 1).all(), per_octave
    assert n == len(want_kp)
    assert np.array_equal(where, want_where) and np.array_equal(resp, want_resp) and np.array_equal(bits(kp), bits(want_kp))
    assert (kp[:, 3] == -1).all() and (np.diff(resp) <= 0).all() and resp.min() >= 1
    assert len(np.unique(resp)) == len(resp)                                # what the transposition test of the GPU suite needs
    # a cap returns the prefix and still counts them all; a threshold drops the tail
    kp2, resp2, where2, n2 = detect(rules, noise_image(), 3, 1, cap=17)
    assert n2 == n and np.array_equal(bits(kp2), bits(want_kp[:17])) and np.array_equal(resp2, want_resp[:17])
    t = int(want_resp[40])
    kp3, resp3, _, n3 = detect(rules, noise_image(), 3, t)
    assert n3 == int((want_resp >= t).sum()) and np.array_equal(bits(kp3), bits(want_kp[:n3]))


def test_keypoints_of_blobs_and_what_leaves_them_unchanged(rules):
    for (H, W, cx, cy, sigma, n_oct, octave) in ((120, 150, 61, 58, 3, 2, 0), (120, 150, 80, 60, 5, 2, 1), (200, 220, 100, 90, 10, 3, 2)):
        img = blob_image(H, W, cx, cy, sigma)
        kp, resp, where, n = detect(rules, img, n_oct, 1000)
        assert n >= 1 and abs(kp[0, 0] - cx) <= 0.5 and abs(kp[0, 1] - cy) <= 0.5 and tuple(where[0, :2]) == (octave, 1), (sigma, kp[0], where[0])
        for other in (255 - img, img - 40):                  # inverted, and a constant apart (the blob is 128 .. 228)
            kp2, resp2, where2, n2 = detect(rules, other, n_oct, 1000)
            assert n2 == n and np.array_equal(bits(kp2), bits(kp)) and np.array_equal(resp2, resp)
    assert detect(rules, np.full((90, 110), 77, np.uint8), 3, 1)[3] == 0


def test_a_tie_between_neighbours_keeps_exactly_one(rules):
    """An image mirrored about the line between columns 39 and 40: R is the same at both, the blob's maximum sits on the
    line, and the twin that comes first in the order (layer, j, i) is the keypoint."""
    img = blob_image(90, 80, 39.5, 44, 3)
    assert np.array_equal(img, img[:, ::-1])
    R = responses_ref(img, 0)
    j, i = 44 - 13, 39 - 13
    assert R[1, j, i] == R[1, j, i + 1] == R[1].max()
    kp, resp, where, n = detect(rules, img, 1, 1000)
    want_kp, want_resp, want_where = detect_ref(img, 1, 1000)
    assert np.array_equal(where, want_where) and np.array_equal(bits(kp), bits(want_kp)) and np.array_equal(resp, want_resp)
    twins = [tuple(w) for w in where if tuple(w) in ((0, 1, j, i), (0, 1, j, i + 1))]
    assert twins == [(0, 1, j, i)] and tuple(where[0]) == (0, 1, j, i)


def test_a_flat_parabola_gives_offset_zero(rules):
    for f in (rules.shim_detect_offset, rules.shim_detect_offset6):
        assert f(5, 5, 5) == 0.0 and f(1, 2, 3) == 0.0 and f(-7, 0, 7) == 0.0
    assert rules.shim_detect_offset(10, 20, 10) == 0.0 and rules.shim_detect_offset(10, 20, 16) == (10 - 16) / (2.0 * (10 - 40 + 16))
    assert rules.shim_detect_offset6(10, 20, 16) == 3.0 * (10 - 16) / (10 - 40 + 16)
    assert rules.shim_detect_offset(2 ** 37, 2 ** 37, 2 ** 37 - 1) == -0.5    # the largest offset: R0 ties with a neighbour


def test_boxes_on_a_wrapped_integral_image(rules):
    """S of a 300 x 300 block that sits at (4100, 4100) of an image of 255s: the entries are near 4.9e9, beyond 2^32.  The
    header's box on S modulo 2^32 is the int64 sum."""
    rng = np.random.default_rng(6)
    block = rng.integers(0, 256, (300, 300), dtype=np.uint8)
    Sb = integral_ref(block)
    y, x = np.mgrid[0:301, 0:301].astype(np.int64)
    S_true = 255 * ((4100 + y) * (4100 + x) - y * x) + Sb
    assert S_true.max() > 2 ** 32
    S = np.ascontiguousarray((S_true % 2 ** 32).astype(np.uint32))
    for _ in range(300):
        x0, y0 = int(rng.integers(0, 300)), int(rng.integers(0, 300))
        x1, y1 = int(rng.integers(x0, min(300, x0 + 195))), int(rng.integers(y0, min(300, y0 + 195)))
        want = int(block[y0:y1 + 1, x0:x1 + 1].astype(np.int64).sum())
        assert rules.shim_detect_box(S.ctypes.data_as(u32p), 301, x0, y0, x1, y1) == want == int(box_ref(Sb, x0, y0, x1, y1))
