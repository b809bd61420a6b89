"""Keypoints detected on a GPU: dlco_desc_detect / detect_device and the tool detect.  The rule
(opencv-dlco_amd/csrc/detect_rules.hpp) is stated in integers and correctly rounded double operations, so every comparison
here is equality, the floats of a keypoint by their bit patterns: cases whose answer can be written down without the rule, the
numpy restatement of tests/test_detect_rules.py (which the CPU tests hold against the header), the cap and the order, an
integral image that wraps, the device form and the cache, and the chain detect -> describe -> match."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_detect_rules import bits, blob_image, detect_ref, filter_side, noise_image, noise_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


def run(ctx, img, n_octaves, threshold, max_keypoints=1 << 16):
    ctx.set_image(img)
    return ctx.detect(n_octaves, threshold, max_keypoints)


def same(got, want):
    """got = (kp, resp, n_found) of the library against want = (kp, resp, where) of the restatement: every keypoint, in order"""
    kp, resp, n_found = got
    return n_found == len(want[0]) and np.array_equal(resp, want[1]) and np.array_equal(bits(kp), bits(want[0]))


# ---- cases whose answer needs no rule ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,cx,cy,sigma,n_octaves,octave", [(120, 150, 61, 58, 3, 2, 0), (120, 150, 80, 60, 5, 2, 1), (200, 220, 100, 90, 10, 3, 2)])
def test_a_gaussian_blob_is_found_at_its_centre(ctx, H, W, cx, cy, sigma, n_octaves, octave):
    img = blob_image(H, W, cx, cy, sigma)
    kp, resp, n_found = run(ctx, img, n_octaves, 1000)
    want = detect_ref(img, n_octaves, 1000)
    assert n_found >= 1 and abs(kp[0, 0] - cx) <= 0.5 and abs(kp[0, 1] - cy) <= 0.5 and kp[0, 3] == -1
    # octave and layer: the restatement's first keypoint is there, the library's first keypoint is that one, and its size lies
    # within half a layer distance (3 steps of the octave) of the layer's filter side
    assert tuple(want[2][0, :2]) == (octave, 1) and np.array_equal(bits(kp[0]), bits(want[0][0])) and resp[0] == want[1][0]
    assert abs(kp[0, 2] - filter_side(octave, 1)) <= 3 * 2 ** octave
    assert same((kp, resp, n_found), want)
    # inverted, and a constant apart (the blob is 128 .. 228, so the constant is taken off)
    for other in (255 - img, img - 40):
        kp2, resp2, n2 = run(ctx, other, n_octaves, 1000)
        assert n2 == n_found and np.array_equal(bits(kp2), bits(kp)) and np.array_equal(resp2, resp)


def test_a_constant_added_to_noise_changes_nothing(ctx):
    img = np.random.default_rng(31).integers(0, 216, (90, 101), dtype=np.uint8)
    kp, resp, n_found = run(ctx, img, 2, 1)
    kp2, resp2, n2 = run(ctx, img + 40, 2, 1)
    assert n_found >= 50 and n2 == n_found and np.array_equal(bits(kp2), bits(kp)) and np.array_equal(resp2, resp)
    kp3, resp3, n3 = run(ctx, 255 - img, 2, 1)
    assert n3 == n_found and np.array_equal(bits(kp3), bits(kp)) and np.array_equal(resp3, resp)


def test_a_constant_image_gives_none(ctx):
    for value in (0, 77, 255):
        kp, resp, n_found = run(ctx, np.full((90, 131), value, np.uint8), 3, 1)
        assert n_found == 0 and kp.shape == (0, 4) and resp.shape == (0,)


def test_the_transposed_image_gives_the_transposed_keypoints(ctx):
    img = np.ascontiguousarray(noise_image())
    want_kp, want_resp, _ = noise_reference()
    assert len(np.unique(want_resp)) == len(want_resp)                      # all distinct: no tie whose winner a transposition changes
    kp, resp, n_found = run(ctx, img, 3, 1)
    kpt, respt, nt = run(ctx, np.ascontiguousarray(img.T), 3, 1)
    assert nt == n_found == len(want_resp)
    a = set(zip(bits(kp[:, 0]).tolist(), bits(kp[:, 1]).tolist(), bits(kp[:, 2]).tolist(), resp.tolist()))
    b = set(zip(bits(kpt[:, 1]).tolist(), bits(kpt[:, 0]).tolist(), bits(kpt[:, 2]).tolist(), respt.tolist()))
    assert len(a) == n_found and a == b
    assert np.array_equal(respt, resp)                                      # distinct responses: the order is the same too


# ---- against the numpy restatement ---------------------------------------------------------------------------------------
def test_odd_image_with_a_pitch_against_the_restatement(ctx):
    img = noise_image()
    assert img.strides == (224, 1)
    want = noise_reference()
    per_octave = np.bincount(want[2][:, 0], minlength=3)
    assert len(want[0]) >= 100 and (per_octave >= 1).all(), per_octave
    assert same(run(ctx, img, 3, 1), want)
    assert ctx.last_kernel_ms() > 0
    # fewer octaves and a threshold: the same keypoints without those of the octaves left out or below it
    for n_oct, thr in ((1, 1), (2, 1), (3, int(want[1][40]))):
        keep = (want[2][:, 0] < n_oct) & (want[1] >= thr)
        assert same(run(ctx, img, n_oct, thr), tuple(w[keep] for w in want)), (n_oct, thr)


def test_four_octaves_down_to_the_smallest_grid_with_candidates(ctx):
    img = np.random.default_rng(22).integers(0, 256, (213, 230), dtype=np.uint8)
    want = detect_ref(img, 4, 1)
    assert same(run(ctx, img, 4, 1), want)
    assert (np.bincount(want[2][:, 0], minlength=4)[:3] >= 1).all()
    # octave 3 has a 3 x 5 grid: one row of three candidates.  A blob of its scale puts a keypoint there.
    blob = blob_image(213, 230, 97 + 16, 97 + 8, 19)
    want = detect_ref(blob, 4, 1000)
    assert (want[2][:, 0] == 3).any()
    assert same(run(ctx, blob, 4, 1000), want)


@pytest.mark.parametrize("shape", [(27, 27), (28, 29), (29, 29), (29, 40), (1, 1), (26, 400), (400, 26), (1, 37)])
def test_images_around_the_smallest_size(ctx, shape):
    img = np.random.default_rng(shape[0] * 1000 + shape[1]).integers(0, 256, shape, dtype=np.uint8)
    want = detect_ref(img, 4, 1)
    got = run(ctx, img, 4, 1)
    assert same(got, want)
    if min(shape) < 29:
        assert got[2] == 0 and got[0].shape == (0, 4)
    if shape == (29, 29):                                                    # one candidate position: a blob on it is the keypoint
        blob = blob_image(29, 29, 14, 14, 3)
        want = detect_ref(blob, 4, 1000)
        assert len(want[0]) == 1 and same(run(ctx, blob, 4, 1000), want)


def test_more_keypoints_than_the_first_survivor_buffer_holds(dlco):
    """The library sizes its survivor buffers from the image (a 128th of its pixels at first) and runs the octaves again when
    they overflow: noise at threshold 1 has more keypoints than that, and every one of them comes back."""
    img = np.random.default_rng(23).integers(0, 256, (300, 320), dtype=np.uint8)
    want = detect_ref(img, 2, 1)
    assert len(want[0]) > max(1024, 300 * 320 // 128)
    c = dlco.DescContext()                                                   # a fresh context: its buffers have not grown yet
    assert same(run(c, img, 2, 1), want)
    assert same(run(c, img, 2, 1), want)
    c.close()


# ---- cap and order -------------------------------------------------------------------------------------------------------
def test_the_cap_returns_the_prefix_and_leaves_the_rest_untouched(dlco, ctx):
    import ctypes as C
    img = noise_image()
    want_kp, want_resp, _ = noise_reference()
    n_all = len(want_kp)
    ctx.set_image(img)
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    for cap in (n_all, n_all - 1, 1, n_all + 7):
        kp, resp, n_found = ctx.detect(3, 1, cap)
        n = min(cap, n_all)
        assert n_found == n_all and len(kp) == n and np.array_equal(bits(kp), bits(want_kp[:n])) and np.array_equal(resp, want_resp[:n])
        # rows at and beyond n_out keep the sentinel
        rows = max(cap, n_all) + 3
        kbuf, rbuf = np.full((rows, 4), -777.0, np.float32), np.full(rows, -777, np.int64)
        n_out, found = C.c_int64(), C.c_int64()
        rc = ctx.L.dlco_desc_detect(ctx.h, 3, 1, cap, kbuf.ctypes.data_as(f32p), rbuf.ctypes.data_as(i64p), C.byref(n_out), C.byref(found))
        assert rc == dlco.OK and (n_out.value, found.value) == (n, n_all)
        assert np.array_equal(bits(kbuf[:n]), bits(want_kp[:n])) and (kbuf[n:] == -777.0).all() and (rbuf[n:] == -777).all()
    # response and n_found may be NULL
    kbuf = np.full((5, 4), -777.0, np.float32)
    assert ctx.L.dlco_desc_detect(ctx.h, 3, 1, 5, kbuf.ctypes.data_as(f32p), None, C.byref(n_out), None) == dlco.OK
    assert n_out.value == 5 and np.array_equal(bits(kbuf), bits(want_kp[:5]))


# ---- wrap-around ---------------------------------------------------------------------------------------------------------
def test_an_integral_image_beyond_two_to_the_32(ctx):
    """4352 x 4100 pixels of 255 sum to 4.5e9 > 2^32, so S wraps on the way to the random block in the bottom-right corner.
    Octave 0 has step 1, so detection is exact under translation: the keypoints whose 3 x 3 x 3 neighbourhood has its
    27-pixel footprints inside the block are those of the block alone, shifted."""
    H, W, B = 4352, 4100, 200
    img = np.full((H, W), 255, np.uint8)
    block = np.random.default_rng(24).integers(0, 256, (B, B), dtype=np.uint8)
    img[H - B:, W - B:] = block
    assert int(img.sum(dtype=np.int64)) > 2 ** 32
    x0, y0 = W - B, H - B
    want_kp, want_resp, want_where = detect_ref(block, 1, 1, origin=(x0, y0))
    assert len(want_kp) >= 100
    kp, resp, n_found = run(ctx, img, 1, 1, max_keypoints=1 << 17)
    assert n_found == len(kp) >= len(want_kp)
    # grid columns 1 .. nx-2 of the block are the pixels x0+14 .. x0+B-15; an offset lies in (-1/2, 1/2]
    lo, hi = 13 + 1 - 0.5, B - 14 - 1 + 0.5
    inside = (kp[:, 0] > x0 + lo) & (kp[:, 0] <= x0 + hi) & (kp[:, 1] > y0 + lo) & (kp[:, 1] <= y0 + hi)
    assert np.array_equal(bits(kp[inside]), bits(want_kp)) and np.array_equal(resp[inside], want_resp)
    # the 255s far from the block are flat: nothing is found there
    assert (kp[:, 0] > x0 - 15).all() and (kp[:, 1] > y0 - 15).all()


# ---- device form and cache -----------------------------------------------------------------------------------------------
def test_the_device_form_and_an_image_in_device_memory(ctx):
    import torch
    img = noise_image()
    want = noise_reference()
    n_all = len(want[0])
    ctx.set_image(img)
    rows = n_all + 5
    kbuf = torch.full((rows, 4), -777.0, dtype=torch.float32, device="cuda")
    rbuf = torch.full((rows,), -777, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n, found = ctx.detect_device(kbuf.data_ptr(), rbuf.data_ptr(), 3, 1, rows)
    k, r = kbuf.cpu().numpy(), rbuf.cpu().numpy()
    assert (n, found) == (n_all, n_all) and np.array_equal(bits(k[:n]), bits(want[0])) and np.array_equal(r[:n], want[1])
    assert (k[n:] == -777.0).all() and (r[n:] == -777).all()
    n, found = ctx.detect_device(kbuf.data_ptr(), None, 3, 1, 9)             # no responses asked for
    assert (n, found) == (9, n_all) and np.array_equal(bits(kbuf.cpu().numpy()[:9]), bits(want[0][:9]))
    # the same rows at a pitch and at an address that are no multiples of 16
    flat = torch.full((3 + 157 * 211,), 255, dtype=torch.uint8, device="cuda")
    flat[3:].view(157, 211)[:, :203] = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    torch.cuda.synchronize()
    ctx.set_image_device(flat.data_ptr() + 3, 203, 157, 211)
    assert same(ctx.detect(3, 1, 1 << 16), want)


def test_a_new_image_replaces_the_cached_integral_image(ctx):
    a, b = noise_image(), np.random.default_rng(25).integers(0, 256, (157, 203), dtype=np.uint8)
    want_a, want_b = noise_reference(), detect_ref(b, 3, 1)
    assert not np.array_equal(want_a[1][:20], want_b[1][:20])
    first = run(ctx, a, 3, 1)
    with_integral = ctx.detect_stage_ms()
    again = ctx.detect(3, 1, 1 << 16)                                        # two detects in a row: the second finds S cached
    cached = ctx.detect_stage_ms()
    assert same(first, want_a) and same(again, want_a)
    assert with_integral["integral"] > 0 and cached["integral"] == 0 and cached["octaves"][0] > 0 and cached["octaves"][3] == 0
    assert abs(ctx.last_kernel_ms() - (cached["integral"] + sum(cached["octaves"]) + cached["selection"])) < 1e-9
    assert same(run(ctx, b, 3, 1), want_b)                                   # same size, other pixels: S is formed anew
    assert ctx.detect_stage_ms()["integral"] > 0
    assert same(run(ctx, a[:100, :120], 3, 1), detect_ref(a[:100, :120], 3, 1))


def test_detect_needs_an_image(dlco):
    c = dlco.DescContext()
    with pytest.raises(dlco.DlcoError) as e:
        c.detect(3, 1, 10)
    assert e.value.code == dlco.ERR_INVALID and "image" in str(e.value)
    c.close()


# ---- the chain -----------------------------------------------------------------------------------------------------------
def test_describe_keypoints_of_the_detected_keypoints(ctx):
    from test_describe_gpu import make_w
    from test_descriptors import make_filters
    ctx.set_filters(make_filters(16, seed=4))                                # the tiny model of tests/test_keypoints_gpu.py
    ctx.set_projection(make_w(12, 128, seed=2))
    img = noise_image()
    kp, resp, n_found = run(ctx, img, 3, 1)
    assert len(kp) == n_found >= 100
    Y, st = ctx.describe_keypoints(kp)
    patches, st2 = ctx.extract_patches(kp)
    assert np.array_equal(st, st2) and (st != 0).all() and (st == 2).any()
    assert np.array_equal(Y, ctx.describe(patches)) and (Y != 0).any(axis=1).all()
    Yu, _ = ctx.describe_keypoints(kp, use_orientation=False)                # no orientation is assigned: upright or not is the same
    assert np.array_equal(Yu, Y)
    assert same(ctx.detect(3, 1, 1 << 16), noise_reference())                # the describe calls leave the detector's state alone


def test_detect_tool_feeds_describe_image_and_match(tmp_path):
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
    r = 10
    np.save(pj / "W.npy", make_w(r, nsel * 8, seed=5))
    img = np.random.default_rng(26).integers(0, 256, (120, 160), dtype=np.uint8)
    np.save(src / "Image.npy", img)
    thr, cap = 2000000, 60
    found = tmp_path / "keypoints"
    q = subprocess.run([os.path.join(CLI, "detect"), str(src), "-out", str(found), "-octaves", "2", "-threshold", str(thr), "-max", str(cap)],
                       capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    kp, resp = np.load(found / "Keypoints.npy"), np.load(found / "Response.npy")
    assert kp.dtype == np.float32 and resp.dtype == np.int64 and np.array_equal(np.load(found / "Image.npy"), img)
    c = dlco.DescContext()
    c.set_image(img)
    bkp, bresp, n_found = c.detect(2, thr, cap)
    c.close()
    assert n_found > cap and len(kp) == cap and np.array_equal(bits(kp), bits(bkp)) and np.array_equal(resp, bresp)
    assert "Keypoints: %d of %d" % (cap, n_found) in q.stdout
    # its output is describe-image's second argument as it stands
    out = tmp_path / "out"
    q = subprocess.run([os.path.join(CLI, "describe-image"), str(flt), str(found), "-prj", str(prj), "-id", "0", "-pj", str(pj), "-out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    Y = np.load(out / "Descriptor.npy")
    assert Y.shape == (cap, r) and (np.load(out / "Status.npy") != 0).all()
    # the table against itself: every row is its own nearest neighbour, at a distance within the bound tests/test_match_gpu.py
    # derives (here d = 0: 4 (r + 2) 2^-53 * 2 |y|^2), as long as no other row lies within that bound - the reference says so
    m = tmp_path / "matches"
    q = subprocess.run([os.path.join(CLI, "match"), str(out), str(out), "-out", str(m)], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr
    Y64 = Y.astype(np.float64)
    D = ((Y64[:, None, :] - Y64[None, :, :]) ** 2).sum(2)
    gate = 8 * (r + 2) * 2.0 ** -53 * (Y64 ** 2).sum(1)
    np.fill_diagonal(D, np.inf)
    assert (D.min(axis=1) > 4 * gate).all()
    nearest, d = np.load(m / "Nearest.npy"), np.load(m / "NearestSqDist.npy")
    assert np.array_equal(nearest[:, 0], np.arange(cap)) and (d[:, 0] <= gate).all()
