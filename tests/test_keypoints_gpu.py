"""Keypoints of an image on a GPU: dlco_desc_set_image* / extract_patches / describe_keypoints* and the tool describe-image.
The sampling rule (opencv-dlco_amd/csrc/patch_rules.hpp) is stated in integers, so every comparison here is equality:
cases whose answer can be written down without the rule (the patch is the image, a rotation of it, its block means),
a numpy restatement of the rule on an odd image with a pitch, and the chain describe_keypoints == describe(extract_patches)."""
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")


# ---- the rule restated (no GPU needed: tests/test_patch_rules.py runs it against the header on the CPU) ----------------
def frame_ref(x, y, size, angle, scale_factor=1.0, use_orientation=True):
    """(X0, Y0, A, B, k) of one keypoint, None when it is invalid.  Floats as the library sees them (f32), sums in double."""
    x, y, size, angle, scale_factor = (float(np.float32(v)) for v in (x, y, size, angle, scale_factor))
    s = size * scale_factor / 64.0
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(s)) or s <= 0 or s > 64 or abs(x) > 2 ** 20 or abs(y) > 2 ** 20:
        return None
    a = 0.0 if (angle < 0 or not use_orientation) else angle * math.pi / 180.0
    k = min(8, max(1, math.ceil(s)))
    rnd = lambda t: int(math.floor(t + 0.5))
    return rnd(x * 65536.0), rnd(y * 65536.0), rnd(s * math.cos(a) * 65536.0 / (2.0 * k)), rnd(s * math.sin(a) * 65536.0 / (2.0 * k)), k


def patch_ref(img, frame):
    """(patch [64,64] u8, status) of a frame on img [H,W] u8: every sample of every pixel at once, in int64."""
    if frame is None:
        return np.zeros((64, 64), np.uint8), 0
    X0, Y0, A, B, k = frame
    H, W = img.shape
    im = img.astype(np.int64)
    pix, sub = np.arange(64, dtype=np.int64), np.arange(k, dtype=np.int64)
    off = ((2 * pix - 63) * k)[:, None] + (2 * sub + 1 - k)[None, :]          # [pixel, sub-sample]
    m = off[None, :, None, :]                                                   # (v, u, b, a): m from (u, a)
    n = off[:, None, :, None]                                                   #               n from (v, b)
    SX, SY = X0 + m * A - n * B, Y0 + m * B + n * A
    ix, fx, iy, fy = SX >> 16, (SX & 0xFFFF) >> 8, SY >> 16, (SY & 0xFFFF) >> 8
    x0, x1, y0, y1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1), np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    val = (256 - fx) * (256 - fy) * im[y0, x0] + fx * (256 - fy) * im[y0, x1] + (256 - fx) * fy * im[y1, x0] + fx * fy * im[y1, x1]
    tot = val.sum(axis=(2, 3))
    assert tot.max() < 2 ** 31
    inside = (SX >= 0).all() and (SX <= (W - 1) * 65536).all() and (SY >= 0).all() and (SY <= (H - 1) * 65536).all()
    return ((tot + k * k * 32768) // (k * k * 65536)).astype(np.uint8), 2 if inside else 1


def patches_ref(img, kp, scale_factor=1.0, use_orientation=True):
    out = [patch_ref(img, frame_ref(*row, scale_factor=scale_factor, use_orientation=use_orientation)) for row in np.asarray(kp, np.float32)]
    return np.stack([p for p, _ in out]), np.array([s for _, s in out], np.uint8)


def odd_image_and_keypoints():
    """A 61 x 97 image inside rows of 112 bytes (the rest holds other values) and 44 keypoints, at scale factor 1:
    s = size / 64 in {0.25, 1, 1.7, 2, 5.3, 8, 20} (the footprints of the first four are staged in LDS, those of the last
    three go beyond the budget and are gathered directly), every angle with every s, centres inside, on the four
    corners and outside the image, and two invalid keypoints."""
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, (61, 112), dtype=np.uint8)
    img = buf[:, :97]
    steps, angles = [0.25, 1, 1.7, 2, 5.3, 8, 20], [-1, 0, 33, 90, 180, 271.5]
    centres = [(48.3, 30.6), (0, 0), (96, 0), (0, 60), (96, 60), (-40.5, 30), (130.25, 75.5), (50, -200), (30.5, 28.25), (90.1, 58.9)]
    kp = []
    for i in range(42):
        cx, cy = centres[i % len(centres)]
        kp.append((cx, cy, 64 * steps[i % 7], angles[i % 6]))                  # 7 and 6 are coprime: all 42 pairs
    kp.insert(5, (10, 10, 0, 0))                                                # invalid: size 0
    kp.insert(20, (float("nan"), 10, 64, 0))                                    # invalid: x is NaN
    return img, np.array(kp, np.float32)


# ---- GPU ------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


def one_patch(ctx, img, kp):
    ctx.set_image(img)
    p, st = ctx.extract_patches(np.array([kp], np.float32), scale_factor=1.0)
    return p[0], int(st[0])


@gpu
def test_patches_whose_answer_needs_no_restatement(ctx):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    for angle, want in ((0, img), (-1, img), (90, np.rot90(img, 1)), (180, img[::-1, ::-1]), (270, np.rot90(img, 3))):
        p, st = one_patch(ctx, img, (31.5, 31.5, 64, angle))
        assert np.array_equal(p, want) and st == 2, angle
    for side, k in ((128, 2), (256, 4)):
        img = rng.integers(0, 256, (side, side), dtype=np.uint8)
        sums = img.astype(np.int64).reshape(64, k, 64, k).sum(axis=(1, 3))
        p, st = one_patch(ctx, img, ((side - 1) / 2, (side - 1) / 2, side, 0))
        assert np.array_equal(p, (sums + k * k // 2) // (k * k)) and st == 2, side


@gpu
def test_a_constant_image_gives_constant_patches(ctx):
    img = np.full((50, 70), 173, np.uint8)
    ctx.set_image(img)
    # inside, over the border, wholly outside on two sides, far larger than the image, on a corner
    kp = np.array([(35, 25, 20, 30), (35.3, 24.7, 100, 17), (-500, -500, 40, 45), (1e5, 3, 640, 200), (0, 49, 4000, 300), (69, 0, 7, 90)], np.float32)
    p, st = ctx.extract_patches(kp, scale_factor=1.0)
    assert (p == 173).all()
    assert st.tolist() == [patch_ref(img, frame_ref(*k))[1] for k in kp] and st[0] == 2 and (st[1:] == 1).all()


@gpu
def test_odd_image_with_a_pitch_against_the_restatement(ctx):
    img, kp = odd_image_and_keypoints()
    assert img.strides == (112, 1)
    want, want_st = patches_ref(img, kp)
    ctx.set_image(img)
    p, st = ctx.extract_patches(kp, scale_factor=1.0)
    assert np.array_equal(st, want_st)
    assert (st == 0).sum() == 2 and (st == 1).sum() >= 10 and (st == 2).sum() >= 2
    for i in range(len(kp)):
        assert np.array_equal(p[i], want[i]), (i, kp[i].tolist())
    # the options: a scale factor, and upright patches
    for sf, orient in ((0.5, True), (1.0, False)):
        want, want_st = patches_ref(img, kp, sf, orient)
        p, st = ctx.extract_patches(kp, scale_factor=sf, use_orientation=orient)
        assert np.array_equal(p, want) and np.array_equal(st, want_st), (sf, orient)


def thin_images_and_keypoints():
    """Images of one row, one column and one pixel: every tap is clamped along the thin axis."""
    rng = np.random.default_rng(13)
    kp = np.array([(3, 0, 16, 0), (10.5, 0.25, 64, 40), (0, 5, 100, 90), (2, 2, 400, 10), (-30, 8, 30, 200)], np.float32)
    return [rng.integers(0, 256, shape, dtype=np.uint8) for shape in ((1, 37), (23, 1), (1, 1))], kp


@gpu
def test_images_of_one_row_one_column_and_one_pixel(ctx):
    images, kp = thin_images_and_keypoints()
    for img in images:
        want, want_st = patches_ref(img, kp)
        ctx.set_image(img)
        p, st = ctx.extract_patches(kp, scale_factor=1.0)
        assert np.array_equal(p, want) and np.array_equal(st, want_st), img.shape
    assert (p == images[-1][0, 0]).all()


@pytest.fixture(scope="module")
def model(dlco, ctx):
    from test_describe_gpu import make_w
    from test_descriptors import make_filters
    ctx.set_filters(make_filters(16, seed=4))
    ctx.set_projection(make_w(12, 128, seed=2))
    return ctx


@gpu
def test_describe_keypoints_is_describe_of_the_extracted_patches(model):
    img, kp = odd_image_and_keypoints()
    model.set_image(img)
    patches, st = model.extract_patches(kp, scale_factor=1.0)
    sample_ms = model.last_kernel_ms()
    Y, st2 = model.describe_keypoints(kp, scale_factor=1.0)
    assert model.last_kernel_ms() > sample_ms > 0                               # the sampling kernel is part of the time
    assert np.array_equal(st, st2) and Y.shape == (len(kp), 12)
    ok = st != 0
    assert np.array_equal(Y[ok], model.describe(patches[ok]))
    assert (Y[~ok] == 0).all() and (~ok).sum() == 2 and (patches[~ok] == 0).all()
    assert (Y[ok] != 0).any(axis=1).all()


@gpu
def test_keypoints_across_the_chunk_boundary(model):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (80, 90), dtype=np.uint8)
    n = 2048 + 5
    kp = np.stack([rng.uniform(-5, 95, n), rng.uniform(-5, 85, n), rng.uniform(8, 40, n), rng.uniform(-30, 360, n)], axis=1).astype(np.float32)
    kp[2047, 2] = 0                                                             # an invalid keypoint on each side of the boundary
    kp[2050, 0] = np.inf
    model.set_image(img)
    patches, st = model.extract_patches(kp, scale_factor=1.0)
    for i in (0, 1000, 2046, 2047, 2048, 2049, 2050, 2052):
        want, want_st = patch_ref(img, frame_ref(*kp[i]))
        assert np.array_equal(patches[i], want) and st[i] == want_st, i
    Y, st2 = model.describe_keypoints(kp, scale_factor=1.0)
    ok = st != 0
    assert np.array_equal(st, st2) and (~ok).sum() == 2
    assert np.array_equal(Y[ok], model.describe(patches[ok])) and (Y[~ok] == 0).all()


@gpu
def test_an_image_in_device_memory_gives_the_same_bytes(model):
    import torch
    img, kp = odd_image_and_keypoints()
    model.set_image(img)
    want, want_st = model.extract_patches(kp, scale_factor=1.0)
    # the same rows at a pitch and at an address that are no multiples of 16: every row sits differently in its 16-byte blocks
    flat = torch.full((3 + 61 * 101,), 255, dtype=torch.uint8, device="cuda")
    flat[3:].view(61, 101)[:, :97] = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    torch.cuda.synchronize()
    model.set_image_device(flat.data_ptr() + 3, 97, 61, 101)
    got, got_st = model.extract_patches(kp, scale_factor=1.0)
    assert np.array_equal(got, want) and np.array_equal(got_st, want_st)
    # rows into a wider table: the padding keeps what it held
    r, ld = model.projected_size, 16
    table = torch.full((len(kp), ld), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = model.describe_keypoints_device(kp, table.data_ptr(), ld=ld, scale_factor=1.0)
    Y, _ = model.describe_keypoints(kp, scale_factor=1.0)
    t = table.cpu().numpy()
    assert np.array_equal(st, want_st) and np.array_equal(t[:, :r], Y) and (t[:, r:] == -7.0).all()


@gpu
def test_keypoint_calls_need_an_image(dlco):
    c = dlco.DescContext()
    with pytest.raises(dlco.DlcoError) as e:
        c.extract_patches(np.array([(5, 5, 64, 0)], np.float32))
    assert e.value.code == dlco.ERR_INVALID and "image" in str(e.value)
    c.set_image(np.zeros((8, 8), np.uint8))
    with pytest.raises(dlco.DlcoError) as e:                                   # an image, but no model: patches yes, descriptors no
        c.describe_keypoints(np.array([(5, 5, 64, 0)], np.float32))
    assert e.value.code == dlco.ERR_INVALID
    p, st = c.extract_patches(np.array([(4, 4, 64, 0)], np.float32), scale_factor=1.0)
    assert (p == 0).all() and st.tolist() == [1]
    c.close()


@gpu
def test_describe_image_tool(tmp_path):
    from test_describe_gpu import make_w
    from test_descriptors import make_filters
    subprocess.check_call(["make", "-s", "-C", CLI])
    dlco = importlib.import_module("opencv-dlco_amd")
    wcols = 3
    PR = make_filters(wcols * 8, seed=3)
    w = np.array([[0.3, 0.0, 0.2]], np.float32)
    nsel = len(dlco.select_filters(PR, w[0]))
    flt, prj, pj, src = (tmp_path / s for s in ("filters", "prj", "pj", "image"))
    for d in (flt, prj, pj, src):
        d.mkdir()
    np.save(flt / "PRFilters.npy", PR.reshape(-1, 64, 64))
    np.save(prj / "w.npy", w)
    np.save(pj / "W.npy", make_w(10, nsel * 8, seed=5))
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (120, 160), dtype=np.uint8)
    kp = np.stack([rng.uniform(0, 159, 30), rng.uniform(0, 119, 30), rng.uniform(4, 20, 30), rng.uniform(-20, 360, 30)], axis=1).astype(np.float32)
    np.save(src / "Image.npy", img)
    np.save(src / "Keypoints.npy", kp)
    model = ["-prj", str(prj), "-id", "0", "-pj", str(pj)]
    out = tmp_path / "out"
    q = subprocess.run([os.path.join(CLI, "describe-image"), str(flt), str(src)] + model + ["-out", str(out), "-patches"],
                       capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    Y, st, patches = np.load(out / "Descriptor.npy"), np.load(out / "Status.npy"), np.load(out / "Patches.npy")
    want, want_st = patches_ref(img, kp, scale_factor=6.25)                    # the tool's default scale factor
    assert patches.dtype == np.uint8 and np.array_equal(patches, want) and np.array_equal(st, want_st) and (st != 0).all()
    assert Y.dtype == np.float32 and Y.shape == (30, 10)
    # describe on the patches it wrote gives the same rows
    again = tmp_path / "again"
    q = subprocess.run([os.path.join(CLI, "describe"), str(flt), str(out)] + model + ["-out", str(again)], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    assert np.array_equal(np.load(again / "Descriptor.npy"), Y)
    # -scale and -upright reach the library; without -patches none are written
    up = tmp_path / "up"
    q = subprocess.run([os.path.join(CLI, "describe-image"), str(flt), str(src)] + model + ["-out", str(up), "-scale", "3", "-upright"],
                       capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    assert not (up / "Patches.npy").exists()
    ctx = dlco.DescContext()
    ctx.set_filters(dlco.select_filters(PR, w[0]))
    ctx.set_projection(np.load(pj / "W.npy"))
    ctx.set_image(img)
    Yu, stu = ctx.describe_keypoints(kp, scale_factor=3.0, use_orientation=False)
    ctx.close()
    assert np.array_equal(np.load(up / "Descriptor.npy"), Yu) and np.array_equal(np.load(up / "Status.npy"), stu)
    # match takes the tool's output
    m = tmp_path / "matches"
    q = subprocess.run([os.path.join(CLI, "match"), str(out), str(up), "-out", str(m)], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    assert np.load(m / "Nearest.npy").shape == (30, 2)
