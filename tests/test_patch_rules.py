"""CPU tests of the keypoint sampling rule (opencv-dlco_amd/csrc/patch_rules.hpp, through tests/shim/patch_rules_shim.cpp):
the frame of a keypoint, its status, the LDS staging decision, and the patch bytes against the numpy restatement that the
GPU tests use.  Nothing here needs a GPU or libdlco.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_keypoints_gpu import frame_ref, odd_image_and_keypoints, patch_ref, thin_images_and_keypoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64p, i32p, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libpatchshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(ROOT, "tests", "shim", "patch_rules_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_patch_frame.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, i64p]
    L.shim_patch_frame.restype = None
    L.shim_patch_status.argtypes = [i64p, C.c_int, C.c_int]
    L.shim_patch_stage.argtypes = [i64p, C.c_int, C.c_int, i32p]
    L.shim_patch_stage.restype = None
    L.shim_patch_sample.argtypes = [u8p, C.c_int, C.c_int, C.c_int64, i64p, u8p]
    L.shim_patch_sample.restype = None
    return L


def frame(L, x, y, size, angle, scale_factor=1.0, use_orientation=True):
    """(X0, Y0, A, B, k), None when invalid."""
    out = np.zeros(6, np.int64)
    L.shim_patch_frame(x, y, size, angle, scale_factor, 1 if use_orientation else 0, out.ctypes.data_as(i64p))
    return tuple(int(v) for v in out[:5]) if out[5] else None


def raw(fr):
    return np.array(list(fr) + [1] if fr is not None else [0, 0, 0, 0, 1, 0], np.int64)


def test_frames_of_the_stated_keypoints(rules):
    assert frame(rules, 31.5, 31.5, 64, 0) == (2064384, 2064384, 32768, 0, 1)
    assert frame(rules, 31.5, 31.5, 64, 90) == (2064384, 2064384, 0, 32768, 1)
    assert frame(rules, 31.5, 31.5, 64, 180) == (2064384, 2064384, -32768, 0, 1)
    assert frame(rules, 31.5, 31.5, 64, 270) == (2064384, 2064384, 0, -32768, 1)
    assert frame(rules, 127.5, 127.5, 256, 0) == (8355840, 8355840, 32768, 0, 4)
    # the scale factor multiplies the size: 40.96 * 6.25 = 256
    assert frame(rules, 127.5, 127.5, 40.96, 0, scale_factor=6.25) == (8355840, 8355840, 32768, 0, 4)
    assert frame(rules, 10, 10, 7.9 * 64, 0)[4] == 8 and frame(rules, 10, 10, 20 * 64, 0)[4] == 8
    assert [frame(rules, 10, 10, s * 64, 0)[4] for s in (0.25, 1, 1.01, 2, 2.5, 7, 7.01, 64)] == [1, 1, 2, 2, 3, 7, 8, 8]
    # negative coordinates round half up, like floor(t + 0.5)
    assert frame(rules, -0.5, -1.25, 64, 0)[:2] == (-32768, -81920)


def test_invalid_keypoints(rules):
    nan, inf = float("nan"), float("inf")
    for kp in ((10, 10, 0, 0), (10, 10, -3, 0), (nan, 10, 64, 0), (10, nan, 64, 0), (10, 10, nan, 0), (inf, 10, 64, 0), (10, 10, inf, 0),
               (10, 10, 64.5 * 64, 0), (2.0 ** 20 + 1, 10, 64, 0), (10, -(2.0 ** 20) - 1, 64, 0)):
        assert frame(rules, *kp) is None, kp
    assert frame(rules, 10, 10, 64, 0, scale_factor=64.5) is None
    # the limits themselves are valid
    assert frame(rules, 2.0 ** 20, -(2.0 ** 20), 64 * 64, 0) == (2 ** 36, -(2 ** 36), 262144, 0, 8)
    # an invalid keypoint has status 0 on any image
    assert rules.shim_patch_status(raw(None).ctypes.data_as(i64p), 100, 100) == 0


def test_no_angle_and_upright_mean_angle_zero(rules):
    zero = frame(rules, 5, 6, 100, 0)
    assert frame(rules, 5, 6, 100, -1) == zero and frame(rules, 5, 6, 100, -0.001) == zero
    assert frame(rules, 5, 6, 100, 33, use_orientation=False) == zero
    assert frame(rules, 5, 6, 100, 33) != zero


def test_frames_agree_with_the_restatement(rules):
    rng = np.random.default_rng(1)
    for _ in range(300):
        kp = (rng.uniform(-300, 300), rng.uniform(-300, 300), rng.uniform(0.5, 5000), rng.uniform(-20, 400))
        kp = tuple(float(np.float32(v)) for v in kp)
        assert frame(rules, *kp) == frame_ref(*kp), kp


def test_status_and_patch_bytes_agree_with_the_restatement(rules):
    img, kps = odd_image_and_keypoints()
    tight = np.ascontiguousarray(img)
    statuses, staged = [], []
    for kp in kps:
        fr = frame(rules, *(float(v) for v in kp))
        assert fr == frame_ref(*kp)
        want, want_st = patch_ref(tight, fr)
        r = raw(fr)
        st = rules.shim_patch_status(r.ctypes.data_as(i64p), 97, 61)
        assert st == want_st, kp
        statuses.append(st)
        if fr is None:
            continue
        plan = np.zeros(6, np.int32)
        rules.shim_patch_stage(r.ctypes.data_as(i64p), 97, 61, plan.ctypes.data_as(i32p))
        staged.append((float(kp[2]) / 64, int(plan[0])))
        got = np.zeros((64, 64), np.uint8)
        rules.shim_patch_sample(C.cast(C.c_void_p(img.ctypes.data), u8p), 97, 61, 112, r.ctypes.data_as(i64p), got.ctypes.data_as(u8p))
        assert np.array_equal(got, want), kp
    assert statuses.count(0) == 2 and statuses.count(1) >= 10 and statuses.count(2) >= 2
    # the keypoint set has patches on both sides of the LDS budget: s <= 2 is staged at every angle, s >= 5.3 is not
    assert all(flag == (1 if step <= 2 else 0) for step, flag in staged)
    assert sum(flag for _, flag in staged) == 24 and len(staged) == 42


def test_thin_images_agree_with_the_restatement(rules):
    images, kps = thin_images_and_keypoints()
    for img in images:
        H, W = img.shape
        for kp in kps:
            fr = frame(rules, *(float(v) for v in kp))
            want, want_st = patch_ref(img, fr)
            got = np.zeros((64, 64), np.uint8)
            rules.shim_patch_sample(img.ctypes.data_as(u8p), W, H, W, raw(fr).ctypes.data_as(i64p), got.ctypes.data_as(u8p))
            assert np.array_equal(got, want) and rules.shim_patch_status(raw(fr).ctypes.data_as(i64p), W, H) == want_st, (img.shape, kp)


def test_the_staged_box_holds_every_tap_and_fits_the_budget(rules):
    budget = rules.shim_patch_stage_budget()
    assert budget == 40 * 1024
    rng = np.random.default_rng(2)
    W, H = 300, 200
    seen = set()
    for _ in range(400):
        kp = (rng.uniform(-50, 350), rng.uniform(-50, 250), rng.uniform(10, 400), rng.uniform(-10, 360))
        fr = frame(rules, *kp)
        X0, Y0, A, B, k = fr
        plan = np.zeros(6, np.int32)
        rules.shim_patch_stage(raw(fr).ctypes.data_as(i64p), W, H, plan.ctypes.data_as(i32p))
        staged, bx0, by0, bw, bh, pitch = (int(v) for v in plan)
        # the taps of the four corner samples bound those of all samples (SX and SY are linear in m and n)
        e = 64 * k - 1
        xs = [X0 + m * A - n * B for m in (-e, e) for n in (-e, e)]
        ys = [Y0 + m * B + n * A for m in (-e, e) for n in (-e, e)]
        cl = lambda v, hi: min(max(v, 0), hi)
        assert bx0 == cl(min(xs) >> 16, W - 1) and bx0 + bw - 1 == cl((max(xs) >> 16) + 1, W - 1)
        assert by0 == cl(min(ys) >> 16, H - 1) and by0 + bh - 1 == cl((max(ys) >> 16) + 1, H - 1)
        assert pitch % 16 == 0 and pitch >= bw + 15
        if staged:
            assert pitch * bh <= budget
        seen.add(staged)
    assert seen == {0, 1}
    # the decision is the frame's alone: s = 2 is staged at any angle, on any image
    for angle in (0, 45, 33):
        plan = np.zeros(6, np.int32)
        rules.shim_patch_stage(raw(frame(rules, 1000, 1000, 128, angle)).ctypes.data_as(i64p), 4096, 3072, plan.ctypes.data_as(i32p))
        assert plan[0] == 1 and plan[5] * plan[4] <= budget
