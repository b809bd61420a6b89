"""Orientation of keypoints on a GPU: dlco_desc_orient / dlco_desc_detect_oriented and detect -orient.  The rule
(opencv-dlco_amd/csrc/orient_rules.hpp) is integer up to the winning vector, so vectors and status are compared with
equality against the numpy restatement of tests/test_orient_rules.py (which the CPU tests hold against the header), and an
angle bit for bit against the header's angle_of of the vector."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_detect_rules import noise_image
from test_keypoints_gpu import frame_ref, patch_ref
from test_orient_rules import angles_of, bind, case_keypoints, centre_ref, fbits, noise_image_96, orient_ref, reference, smooth_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "liborientshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(ROOT, "tests", "shim", "orient_rules_shim.cpp")])
    return bind(C.CDLL(str(out)))


def same(rules, got, want_vec, want_st):
    """got = (angles, vectors, status) of the library: the restatement's vectors and status, and the header's angle of each vector"""
    ang, vec, st = got
    return np.array_equal(st, want_st) and np.array_equal(vec, want_vec) and np.array_equal(fbits(ang), fbits(angles_of(rules, want_vec)))


# ---- parity with the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise", "smooth"])
def test_odd_images_with_a_pitch_against_the_restatement(ctx, rules, name):
    img, kp, want_vec, want_st = reference(name)                             # 300 keypoints: 75 workgroups, every path of the CPU cases
    assert img.strides[0] > img.shape[1] and len(kp) == 300
    ctx.set_image(img)
    got = ctx.orient(kp)
    assert same(rules, got, want_vec, want_st)
    assert ctx.last_orient_ms() > 0 and ctx.last_kernel_ms() >= ctx.last_orient_ms()
    again = ctx.orient(kp)                                                   # S is cached now: the kernel alone
    assert same(rules, again, want_vec, want_st) and abs(ctx.last_kernel_ms() - ctx.last_orient_ms()) < 1e-9
    # one keypoint, and 257: a last workgroup with one wave of four at work
    for n in (1, 257):
        assert same(rules, ctx.orient(kp[16:16 + n]), want_vec[16:16 + n], want_st[16:16 + n]), n
    # vectors and status may be NULL
    f32p = C.POINTER(C.c_float)
    ang = np.full(300, -777, np.float32)
    k = np.ascontiguousarray(kp)
    assert ctx.L.dlco_desc_orient(ctx.h, k.ctypes.data_as(f32p), 300, ang.ctypes.data_as(f32p), None, None) == 0
    assert np.array_equal(fbits(ang), fbits(got[0]))


def test_the_largest_scales(ctx, rules):
    img = np.random.default_rng(45).integers(0, 256, (520, 520), dtype=np.uint8)
    kp = np.array([(260, 260, 195, 0), (259.5, 260.4, 1e30, 0), (260, 260, 960, 0), (200, 300, 195, 0), (181.6, 182.4, 195, 0), (100, 100, 195, 0),
                   (250, 270, 3e38, 0), (260, 260, 90, 0), (300.5, 222.5, 60, 0)], np.float32)
    assert [centre_ref(*k[:3])[2] for k in kp] == [26, 128, 128, 26, 26, 26, 128, 12, 8]
    want_vec, want_st, _ = orient_ref(img, kp)
    assert want_st.tolist() == [2, 1, 1, 2, 2, 1, 1, 2, 2] and want_vec[:6].any(axis=1).all()
    ctx.set_image(img)
    assert same(rules, ctx.orient(kp), want_vec, want_st)


def test_an_integral_image_beyond_two_to_the_32(ctx, rules):
    """The image of the detector's test of this kind: 4352 x 4100 pixels of 255 sum to 4.5e9 > 2^32, so S has wrapped on the way
    to the random block in the bottom-right corner.  Keypoints whose samples stay inside the block, or leave the image through
    its bottom or right border, are those of the block alone, shifted."""
    H, W, B = 4352, 4100, 200
    img = np.full((H, W), 255, np.uint8)
    block = np.random.default_rng(24).integers(0, 256, (B, B), dtype=np.uint8)
    img[H - B:, W - B:] = block
    local = np.array([(100, 100, 9, 0), (150.5, 120.25, 15, 0), (199, 199, 9, 0), (195, 60, 21, 0), (60, 196.5, 39, 0), (100, 101, 97.5, 0),
                      (180, 185, 39, 0)], np.float32)
    for x, y, size, _ in local:                                              # nothing reaches over the block's left or top edge
        X, Y, s = centre_ref(x, y, size)
        assert X - 7 * s >= 0 and Y - 7 * s >= 0
    want_vec, want_st, _ = orient_ref(block, local)
    assert want_st.tolist() == [2, 2, 1, 1, 1, 2, 1] and want_vec.any(axis=1).all()
    kp = local + np.array([W - B, H - B, 0, 0], np.float32)
    ctx.set_image(img)
    assert same(rules, ctx.orient(kp), want_vec, want_st)


# ---- detect and detect_oriented --------------------------------------------------------------------------------------------
def test_detect_oriented_is_detect_with_the_angles_of_orient(ctx, rules):
    img = noise_image()
    ctx.set_image(img)
    kp, resp, n_found = ctx.detect(3, 1, 1 << 16)
    stages = ctx.detect_stage_ms()
    assert n_found == len(kp) >= 100 and (kp[:, 3] == -1).all()
    okp, oresp, on_found = ctx.detect_oriented(3, 1, 1 << 16)
    ostages, o_ms, total = ctx.detect_stage_ms(), ctx.last_orient_ms(), ctx.last_kernel_ms()
    assert on_found == n_found and np.array_equal(oresp, resp) and np.array_equal(fbits(okp[:, :3]), fbits(kp[:, :3]))
    assert sorted(ostages) == sorted(stages) and len(ostages["octaves"]) == 4 and o_ms > 0
    assert abs(total - (ostages["integral"] + sum(ostages["octaves"]) + ostages["selection"] + o_ms)) < 1e-9
    ang, vec, st = ctx.orient(kp)
    assert np.array_equal(fbits(okp[:, 3]), fbits(ang))
    want_vec, want_st, _ = orient_ref(img, kp)
    assert same(rules, (ang, vec, st), want_vec, want_st) and (ang >= 0).sum() >= 100
    # max_keypoints cuts the list: the prefix, with its angles; rows beyond it keep what they held
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    kbuf, rbuf = np.full((40, 4), -777.0, np.float32), np.full(40, -777, np.int64)
    n_out, found = C.c_int64(), C.c_int64()
    assert ctx.L.dlco_desc_detect_oriented(ctx.h, 3, 1, 33, kbuf.ctypes.data_as(f32p), rbuf.ctypes.data_as(i64p), C.byref(n_out), C.byref(found)) == 0
    assert (n_out.value, found.value) == (33, n_found) and np.array_equal(fbits(kbuf[:33]), fbits(okp[:33])) and np.array_equal(rbuf[:33], resp[:33])
    assert (kbuf[33:] == -777.0).all() and (rbuf[33:] == -777).all()
    # detect itself still writes -1
    assert (ctx.detect(3, 1, 50)[0][:, 3] == -1).all()


def test_detect_oriented_without_keypoints_is_no_error(ctx):
    ctx.set_image(np.full((90, 131), 77, np.uint8))
    kp, resp, n_found = ctx.detect_oriented(3, 1, 100)
    assert n_found == 0 and kp.shape == (0, 4) and resp.shape == (0,) and ctx.last_orient_ms() == 0
    ctx.set_image(np.random.default_rng(1).integers(0, 256, (20, 26), dtype=np.uint8))     # too small for octave 0
    assert ctx.detect_oriented(4, 1, 100)[2] == 0


# ---- the cached integral image ---------------------------------------------------------------------------------------------
def test_a_new_image_replaces_the_cached_integral_image(ctx, rules):
    a, b = noise_image_96(), np.random.default_rng(49).integers(0, 256, (96, 128), dtype=np.uint8)
    kp = case_keypoints(96, 128, n=64)
    want_a, want_b = orient_ref(a, kp), orient_ref(b, kp)
    assert not np.array_equal(want_a[0], want_b[0])
    ctx.set_image(a)
    assert same(rules, ctx.orient(kp), want_a[0], want_a[1])
    assert ctx.last_kernel_ms() > ctx.last_orient_ms()                       # the integral image was formed by this call
    ctx.set_image(b)                                                         # same size, other pixels
    assert same(rules, ctx.orient(kp), want_b[0], want_b[1])
    assert ctx.last_kernel_ms() > ctx.last_orient_ms()
    ctx.detect(1, 1, 10)                                                     # shared with detect: it finds S cached
    assert ctx.detect_stage_ms()["integral"] == 0
    c = smooth_image(61, 77, 50)                                             # another size
    kpc = case_keypoints(61, 77, n=40)
    want_c = orient_ref(c, kpc)
    ctx.set_image(c)
    assert same(rules, ctx.orient(kpc), want_c[0], want_c[1])


def test_orient_needs_an_image(dlco):
    c = dlco.DescContext()
    with pytest.raises(dlco.DlcoError) as e:
        c.orient(np.array([[5, 5, 9, 0]], np.float32))
    assert e.value.code == dlco.ERR_INVALID and "image" in str(e.value)
    with pytest.raises(dlco.DlcoError) as e:
        c.detect_oriented(3, 1, 10)
    assert e.value.code == dlco.ERR_INVALID and "image" in str(e.value)
    c.close()


# ---- the chain -------------------------------------------------------------------------------------------------------------
def test_patches_of_the_oriented_keypoints(ctx):
    img = np.ascontiguousarray(noise_image())
    ctx.set_image(img)
    kp, _, _ = ctx.detect_oriented(2, 1, 24)
    assert len(kp) == 24 and (kp[:, 3] >= 0).all() and len(np.unique(kp[:, 3])) > 12
    patches, st = ctx.extract_patches(kp, scale_factor=6.25, use_orientation=True)
    for k, p, s in zip(kp, patches, st):
        want, want_s = patch_ref(img, frame_ref(*k, scale_factor=6.25))
        assert np.array_equal(p, want) and s == want_s
    upright, _ = ctx.extract_patches(kp, scale_factor=6.25, use_orientation=False)
    plain = kp.copy()
    plain[:, 3] = -1                                                         # what detect gives today
    today, _ = ctx.extract_patches(plain, scale_factor=6.25, use_orientation=True)
    assert np.array_equal(upright, today) and not np.array_equal(upright, patches)


def test_detect_tool_with_and_without_orient(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CLI])
    dlco = importlib.import_module("opencv-dlco_amd")
    src = tmp_path / "image"
    src.mkdir()
    img = np.random.default_rng(26).integers(0, 256, (120, 160), dtype=np.uint8)
    np.save(src / "Image.npy", img)
    thr, cap = 2000000, 60
    c = dlco.DescContext()
    c.set_image(img)
    want, want_resp, n_found = c.detect_oriented(2, thr, cap)
    c.close()
    assert len(want) == cap and (want[:, 3] >= 0).all()
    for flag in ([], ["-orient"]):
        out = tmp_path / ("keypoints" + "".join(flag))
        q = subprocess.run([os.path.join(CLI, "detect"), str(src), "-out", str(out), "-octaves", "2", "-threshold", str(thr), "-max", str(cap)] + flag,
                           capture_output=True, text=True, timeout=600)
        assert q.returncode == 0, q.stderr
        kp, resp = np.load(out / "Keypoints.npy"), np.load(out / "Response.npy")
        assert kp.dtype == np.float32 and kp.shape == (cap, 4) and np.array_equal(resp, want_resp) and np.array_equal(np.load(out / "Image.npy"), img)
        assert np.array_equal(fbits(kp[:, :3]), fbits(want[:, :3])) and "Keypoints: %d of %d" % (cap, n_found) in q.stdout
        if flag:
            assert np.array_equal(fbits(kp[:, 3]), fbits(want[:, 3]))
        else:
            assert (kp[:, 3] == -1).all()
