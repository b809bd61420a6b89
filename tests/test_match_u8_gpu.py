"""The eight-bit line on the GPU: dlco_desc_match_u8 / match_u8_device / cross_sqdists_u8 against numpy int64 on the same
bytes, the direct form ((q - t)^2).sum(), with equality everywhere: the distances are integers, there are no ambiguous
queries and nothing is excluded.  Then the _u8 forms of describe against quantize() of the float calls, byte for byte,
and a derived bound on what quantisation can do to a nearest neighbour.

That bound: without clamping every coordinate of u_a - u_b is within 1 of s (y_a - y_b) (two roundings to an integer of at
most 1/2 each; the float roundings of v <= 255 add below 1e-4), so ||u_a - u_b|| is within sqrt(r) of s ||y_a - y_b||, and
whenever the float64 reference has s (sqrt(d2) - sqrt(d1)) > 2.002 sqrt(r), the nearest row of the byte table must be the
nearest row of the float table."""
import numpy as np
import pytest

from test_describe_gpu import make_w, pair_set
from test_descriptors import make_filters
from test_keypoints_gpu import odd_image_and_keypoints
from test_match_gpu import make_tables, ref_dists, top_by_key

pytestmark = pytest.mark.gpu

I32MAX = np.int32(2 ** 31 - 1)


def ref_u8(Q, T):
    """[nq, nt] int64 of the exact squared distances."""
    Q64, T64 = Q.astype(np.int64), T.astype(np.int64)
    D = np.empty((len(Q), len(T)), np.int64)
    step = max(1, (1 << 23) // T64.size)
    for i0 in range(0, len(Q), step):
        d = Q64[i0:i0 + step, None, :] - T64[None, :, :]
        D[i0:i0 + step] = (d * d).sum(2)
    return D


def byte_tables(nq, nt, r, hi=256):
    """Uniform bytes below hi (asymmetric: nq != nt wherever it matters, nothing repeats by design); with the full range, one
    query row all 0 and one train row all 255, so that the largest possible distance r * 255^2 is met."""
    rng = np.random.default_rng(7000 + 31 * r + nt + hi)
    Q = rng.integers(0, hi, (nq, r), dtype=np.uint8)
    T = rng.integers(0, hi, (nt, r), dtype=np.uint8)
    if hi == 256:
        Q[nq // 2] = 0
        T[nt - 1] = 255
    return Q, T


def want_top2(D):
    nq, nt = D.shape
    order = top_by_key(D, 2)
    want_i, want_d = order.astype(np.int32), D[np.arange(nq)[:, None], order].astype(np.int32)
    if nt == 1:
        want_i = np.concatenate([want_i, np.full((nq, 1), -1, np.int32)], 1)
        want_d = np.concatenate([want_d, np.full((nq, 1), I32MAX, np.int32)], 1)
    return want_i, want_d


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()                                # no filters, no projection: matching needs neither
    yield c
    c.close()


# ---- 1. the matrix ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nt,r", [(70, 90, r) for r in (1, 3, 15, 16, 17, 63, 64, 65, 128, 129, 200, 1024)] + [(1, 1, 64), (37, 2, 64), (129, 17, 64)])
def test_cross_sqdists_u8_is_exact(ctx, nq, nt, r):
    Q, T = byte_tables(nq, nt, r)
    D = ref_u8(Q, T)
    X = ctx.cross_sqdists_u8(Q, T)
    assert X.shape == (nq, nt) and X.dtype == np.int32
    print("cross_sqdists_u8 %d x %d r %d: %d of %d entries differ, largest %d" % (nq, nt, r, (X != D).sum(), X.size, X.max()))
    assert np.array_equal(X, D)
    assert D[nq // 2, nt - 1] == r * 255 * 255 and (r != 1024 or X.max() == 66585600)


# ---- 2. the top two ----------------------------------------------------------------------------------------------------------
TOP2 = ([(300, 500, r, 256) for r in (1, 3, 64, 128, 129, 1024)] + [(300, 500, r, 4) for r in (1, 3, 64)]      # 0..3: ties are the rule
        + [(40, 1, 64, 256), (40, 2, 64, 256), (5, 4000, 64, 256), (257, 1000, 128, 256)])


@pytest.mark.parametrize("nq,nt,r,hi", TOP2)
def test_match_u8_is_the_top_two_of_the_reference(ctx, nq, nt, r, hi):
    Q, T = byte_tables(nq, nt, r, hi)
    D = ref_u8(Q, T)
    want_i, want_d = want_top2(D)
    if hi == 4 and nt > 2:
        s = np.sort(D, axis=1)
        assert ((s[:, 0] == s[:, 1]) | (s[:, 1] == s[:, 2])).mean() > 0.05                 # exact ties among the first three are common
    idx, d = ctx.match_u8(Q, T)
    assert idx.shape == (nq, 2) and idx.dtype == np.int32 and d.shape == (nq, 2) and d.dtype == np.int32
    print("match_u8 %d x %d r %d bytes < %d: %d index and %d distance mismatches" % (nq, nt, r, hi, (idx != want_i).sum(), (d != want_d).sum()))
    assert np.array_equal(idx, want_i)
    assert np.array_equal(d, want_d)
    # and they are the top two of the matrix the library itself returns
    assert np.array_equal(ctx.cross_sqdists_u8(Q, T), D)


# ---- 3. the device form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [67, 128])
def test_match_u8_device_with_pitches_and_garbage_beyond_r(ctx, dlco, r):
    import torch
    nq, nt = 150, 333
    Q, T = byte_tables(nq, nt, r)
    want_i, want_d = ctx.match_u8(Q, T)
    assert np.array_equal(want_i, want_top2(ref_u8(Q, T))[0])
    ld = (r + 15) // 16 * 16 + 16
    rng = np.random.default_rng(r)
    gq, gt = rng.integers(0, 256, (nq, ld), dtype=np.uint8), rng.integers(0, 256, (nt, ld), dtype=np.uint8)   # different garbage
    gq[:, :r], gt[:, :r] = Q, T
    bq, bt = torch.from_numpy(gq).to("cuda:0"), torch.from_numpy(gt).to("cuda:0")
    oi = torch.full((nq, 2), -5, dtype=torch.int32, device="cuda:0")
    od = torch.full((nq, 2), -5, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.match_u8_device(bq.data_ptr(), nq, bt.data_ptr(), nt, r, oi.data_ptr(), od.data_ptr(), ldq=ld, ldt=ld)
    torch.cuda.synchronize()
    assert ctx.last_kernel_ms() > 0
    assert np.array_equal(oi.cpu().numpy(), want_i) and np.array_equal(od.cpu().numpy(), want_d)
    assert np.array_equal(bq.cpu().numpy(), gq) and np.array_equal(bt.cpu().numpy(), gt)          # the tables are only read
    # the first 37 queries alone: the same rows, and nothing written behind them
    oi.fill_(-5)
    od.fill_(-5)
    torch.cuda.synchronize()
    ctx.match_u8_device(bq.data_ptr(), 37, bt.data_ptr(), nt, r, oi.data_ptr(), od.data_ptr(), ldq=ld, ldt=ld)
    torch.cuda.synchronize()
    assert np.array_equal(oi.cpu().numpy()[:37], want_i[:37]) and np.array_equal(od.cpu().numpy()[:37], want_d[:37])
    assert (oi.cpu().numpy()[37:] == -5).all() and (od.cpu().numpy()[37:] == -5).all()
    for bad_q, bad_t in ((ld + 8, ld), (ld, ld + 4), (r // 16 * 16 - 16, ld), (ld, 16)):
        with pytest.raises(dlco.DlcoError) as ei:
            ctx.match_u8_device(bq.data_ptr(), nq, bt.data_ptr(), nt, r, oi.data_ptr(), od.data_ptr(), ldq=bad_q, ldt=bad_t)
        assert ei.value.code == dlco.ERR_INVALID


# ---- 4. quantised descriptors ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dlco):
    c = dlco.DescContext()
    c.set_filters(make_filters(60, seed=60))
    c.set_projection(make_w(67, 480, seed=67))
    yield c
    c.close()


def test_describe_u8_is_quantize_of_describe(dlco, model):
    import torch
    patches, _ = pair_set(n_base=60, n_pairs=10, seed=11)                # 240 patches
    assert len(patches) >= 200
    r = model.projected_size
    with pytest.raises(dlco.DlcoError) as ei:                            # no quantiser yet
        model.describe_u8(patches)
    assert ei.value.code == dlco.ERR_INVALID
    before = model.describe(patches)
    scale, off = dlco.quant_fit(before)
    want = dlco.quantize(before, scale, off)
    assert want.min() == 0 and want.max() == 255
    model.set_quantizer(scale, off)
    got = model.describe_u8(patches)
    assert model.last_kernel_ms() > 0
    assert got.dtype == np.uint8 and got.shape == (len(patches), r)
    print("describe_u8: %d of %d bytes differ from quantize(describe)" % ((got != want).sum(), want.size))
    assert np.array_equal(got, want)
    # the device form: r bytes per row of pitch ld, the padding keeps its bytes
    ld = 96
    buf = torch.full((len(patches), ld), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    model.describe_u8_device(patches, buf.data_ptr(), ld=ld)
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert np.array_equal(g[:, :r], want) and (g[:, r:] == 0xA5).all()
    # the float call after the byte calls returns the bits it returned before
    assert model.describe(patches).tobytes() == before.tobytes()
    # a quantiser without offsets, a scale that clamps
    model.set_quantizer(scale * 3.0, None, r=r)
    assert np.array_equal(model.describe_u8(patches), dlco.quantize(before, scale * 3.0))
    # a quantiser of another width does not fit; a new projection of another r drops the one that did
    model.set_quantizer(scale, off[:r - 1])
    with pytest.raises(dlco.DlcoError) as ei:
        model.describe_u8(patches)
    assert ei.value.code == dlco.ERR_INVALID
    model.set_quantizer(scale, off)
    model.set_projection(make_w(48, 480, seed=48))
    with pytest.raises(dlco.DlcoError) as ei:
        model.describe_u8(patches)
    assert ei.value.code == dlco.ERR_INVALID
    model.set_projection(make_w(67, 480, seed=67))


def test_describe_keypoints_u8_is_quantize_of_describe_keypoints(dlco, model):
    import torch
    img, kp = odd_image_and_keypoints()
    model.set_image(img)
    r = model.projected_size
    Y, st = model.describe_keypoints(kp, scale_factor=1.0)
    assert (st == 0).sum() == 2 and (Y[st == 0] == 0).all()
    scale, off = dlco.quant_fit(Y[st != 0])
    off = off - np.float32(3.0) / np.float32(scale)                      # a zero row is then not a row of zero bytes
    want = dlco.quantize(Y, scale, off)
    model.set_quantizer(scale, off)
    got, st2 = model.describe_keypoints_u8(kp, scale_factor=1.0)
    assert np.array_equal(st, st2)
    assert np.array_equal(got, want)
    zero_row = dlco.quantize(np.zeros((1, r), np.float32), scale, off)[0]
    assert (got[st == 0] == zero_row).all() and zero_row.any()
    ld = 80
    buf = torch.full((len(kp), ld), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st3 = model.describe_keypoints_u8_device(kp, buf.data_ptr(), ld=ld, scale_factor=1.0)
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert np.array_equal(st3, st) and np.array_equal(g[:, :r], want) and (g[:, r:] == 0x5A).all()
    Y2, _ = model.describe_keypoints(kp, scale_factor=1.0)
    assert Y2.tobytes() == Y.tobytes()


# ---- 4b. the same across the boundary of a launch chunk (2048 patches) ------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(dlco):
    """The model of test_keypoints_gpu.py, the image and the 2048 + 5 keypoints of its test across the chunk boundary (an
    invalid keypoint on each side), and the patches of those keypoints: all distinct but the two of the invalid ones."""
    c = dlco.DescContext()
    c.set_filters(make_filters(16, seed=4))
    c.set_projection(make_w(12, 128, seed=2))
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (80, 90), dtype=np.uint8)
    n = 2048 + 5
    kp = np.stack([rng.uniform(-5, 95, n), rng.uniform(-5, 85, n), rng.uniform(8, 40, n), rng.uniform(-30, 360, n)], axis=1).astype(np.float32)
    kp[2047, 2] = 0
    kp[2050, 0] = np.inf
    c.set_image(img)
    patches, st = c.extract_patches(kp, scale_factor=1.0)
    assert (st == 0).tolist() == [i in (2047, 2050) for i in range(n)]
    yield c, kp, patches, st
    c.close()


def rows_differ(got, want, rows=range(2046, 2053)):
    bad = np.nonzero((got != want).any(1))[0]
    return "%d rows differ, the first at %s; %s" % (len(bad), bad[:8].tolist(), "; ".join(
        "row %d: got %s, want %s" % (i, got[i].tolist(), want[i].tolist()) for i in rows))


def test_describe_u8_across_the_chunk_boundary(dlco, tiny):
    import torch
    model, _, patches, _ = tiny
    n, r = len(patches), model.projected_size
    assert n == 2048 + 5 and r == 12
    Y = model.describe(patches)
    scale, off = dlco.quant_fit(Y)
    want = dlco.quantize(Y, scale, off)
    assert want.min() == 0 and want.max() == 255 and len(np.unique(want, axis=0)) > 0.9 * n     # a row put in another place would show
    model.set_quantizer(scale, off)
    got = model.describe_u8(patches)
    assert got.dtype == np.uint8 and got.shape == (n, r)
    print("describe_u8 of %d patches: %d rows differ from quantize(describe)" % (n, (got != want).any(1).sum()))
    assert np.array_equal(got, want), rows_differ(got, want)
    ld = 16
    buf = torch.full((n, ld), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    model.describe_u8_device(patches, buf.data_ptr(), ld=ld)
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert np.array_equal(g[:, :r], want), rows_differ(g[:, :r], want)
    assert (g[:, r:] == 0xA5).all(), "padding overwritten in rows %s" % np.nonzero((g[:, r:] != 0xA5).any(1))[0][:8].tolist()


def test_describe_keypoints_u8_across_the_chunk_boundary(dlco, tiny):
    import torch
    model, kp, _, st = tiny
    n, r = len(kp), model.projected_size
    Y, st1 = model.describe_keypoints(kp, scale_factor=1.0)
    assert np.array_equal(st1, st) and (Y[st == 0] == 0).all()
    scale, off = dlco.quant_fit(Y[st != 0])
    off = off - np.float32(3.0) / np.float32(scale)                      # a zero row is then not a row of zero bytes
    want = dlco.quantize(Y, scale, off)
    zero_row = dlco.quantize(np.zeros((1, r), np.float32), scale, off)[0]
    assert zero_row.any() and (want[[2047, 2050]] == zero_row).all()
    model.set_quantizer(scale, off)
    got, st2 = model.describe_keypoints_u8(kp, scale_factor=1.0)
    assert np.array_equal(st2, st)
    assert np.array_equal(got, want), rows_differ(got, want)
    assert (got[st == 0] == zero_row).all() and (st == 0).sum() == 2
    ld = 16
    buf = torch.full((n, ld), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st3 = model.describe_keypoints_u8_device(kp, buf.data_ptr(), ld=ld, scale_factor=1.0)
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert np.array_equal(st3, st)
    assert np.array_equal(g[:, :r], want), rows_differ(g[:, :r], want)
    assert (g[:, r:] == 0x5A).all(), "padding overwritten in rows %s" % np.nonzero((g[:, r:] != 0x5A).any(1))[0][:8].tolist()
    assert (g[st == 0][:, :r] == zero_row).all()


# ---- 5. nearest neighbours survive quantisation, with the derived bound ------------------------------------------------------
@pytest.mark.parametrize("r", [64, 128])
def test_nearest_neighbours_survive_quantisation(ctx, dlco, r):
    Q, T = make_tables(300, 500, r)
    scale, off = dlco.quant_fit(np.concatenate([Q, T]))                  # fitted on both: nothing clamps
    D = ref_dists(Q, T)                                                   # float64 on the float32 tables
    o2 = top_by_key(D, 2)
    rows = np.arange(len(Q))
    d1, d2 = D[rows, o2[:, 0]], D[rows, o2[:, 1]]
    sure = float(scale) * (np.sqrt(d2) - np.sqrt(d1)) > 2.002 * np.sqrt(r)
    print("quantised nearest neighbours r %d: %.3f of the queries meet the inequality" % (r, sure.mean()))
    assert sure.mean() >= 0.5, "the case is unfit: too few queries meet the inequality"
    # only now the bytes and the GPU's answer
    Qu, Tu = dlco.quantize(Q, scale, off), dlco.quantize(T, scale, off)
    v = (np.concatenate([Q, T]) - off) * np.float32(scale)
    assert np.rint(v).min() >= 0 and np.rint(v).max() <= 255
    idx, d = ctx.match_u8(Qu, Tu)
    assert np.array_equal(idx, want_top2(ref_u8(Qu, Tu))[0])
    worst = np.abs(np.sqrt(d[:, 0].astype(np.float64)) - float(scale) * np.sqrt(D[rows, idx[:, 0]])).max()
    print("    %d of %d sure queries keep their neighbour; largest | ||u|| - s ||y|| | %.2f against %.2f" %
          ((idx[sure, 0] == o2[sure, 0]).sum(), sure.sum(), worst, np.sqrt(r)))
    assert worst <= 1.001 * np.sqrt(r)
    assert np.array_equal(idx[sure, 0], o2[sure, 0])
