"""The learnt descriptor y = W * min(sPRFilters * get_desc(patch), 1) on the GPU (dlco_desc_set_projection / describe /
pair_sqdists / pair_stats) against float64 numpy on the ORACLE's descriptors.

Bounds are derived, not tuned.  The project gates the GPU's pooled descriptor D at rtol 3e-7, atol 1e-9 against the
oracle (test_descriptors_match_oracle); the projection accumulates in double and rounds to float once.  So, entry by entry,
    |Y - want| <= 3e-7 * (|D| |W|^T) + 1e-9 * sum_f |W_jf| + 2^-23 * |want|           (gate 1, `entry_bound`)
with want = D_oracle @ W^T in float64.  With W ~ N(0, 1/F) and a quarter of D at the crop this is a few 1e-6 of |want|:
a wrong fragment order or a dropped k block misses it by orders of magnitude."""
import numpy as np
import pytest

from test_descriptors import make_filters, make_patches

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23


def oracle_descriptors(ref, patches, sPR):
    D = np.stack([ref.patch_descriptor(p, sPR) for p in patches])
    assert D.dtype == np.float32 and (D == 1).any()                      # the crop at 1 is reached
    return D.astype(np.float64)


def make_w(r, F, seed):
    return (np.random.default_rng(seed).standard_normal((r, F)) / np.sqrt(F)).astype(np.float32)


def entry_bound(D64, W):
    W64 = W.astype(np.float64)
    want = D64 @ W64.T
    return want, 3e-7 * (np.abs(D64) @ np.abs(W64).T) + 1e-9 * np.abs(W64).sum(1)[None, :] + EPS * np.abs(want)


def check_describe(ctx, ref, patches, sPR, D64, r, tag):
    F = sPR.shape[0] * 8
    W = make_w(r, F, seed=1000 * sPR.shape[0] + r)
    ctx.set_projection(W)
    assert ctx.projected_size == r and ctx.size == F
    Y = ctx.describe(patches)
    assert Y.shape == (len(patches), r) and Y.dtype == np.float32 and np.isfinite(Y).all()
    # gate 1: against the oracle
    want, e = entry_bound(D64, W)
    err = np.abs(Y.astype(np.float64) - want)
    print("%s describe vs oracle: max |err| %.3e, max err/bound %.3f, median bound/|want| %.2e, median |want| %.3f"
          % (tag, err.max(), (err / e).max(), np.median(e / np.maximum(np.abs(want), 1e-300)), np.median(np.abs(want))))
    assert (err <= e).all(), (tag, float((err / e).max()))
    # gate 2: the projection kernel alone, on the library's own pooled descriptors
    Dg = ctx.compute(patches).astype(np.float64)
    W64 = W.astype(np.float64)
    want_g = Dg @ W64.T
    e_g = EPS * np.abs(want_g) + 1e-12 * (np.abs(Dg) @ np.abs(W64).T)
    err_g = np.abs(Y.astype(np.float64) - want_g)
    print("%s projection alone: max |err| %.3e, max err/bound %.3f" % (tag, err_g.max(), (err_g / e_g).max()))
    assert (err_g <= e_g).all(), (tag, float((err_g / e_g).max()))


@pytest.mark.parametrize("nsel", [1, 60, 68, 76, 130])
def test_describe_matches_float64_product_of_oracle_descriptors(dlco, ref, nsel):
    patches, sPR = make_patches(12, seed=100 + nsel), make_filters(nsel, seed=nsel)
    D64 = oracle_descriptors(ref, patches, sPR)
    F = nsel * 8
    ctx = dlco.DescContext()
    ctx.set_filters(sPR)
    ranks = [r for r in (1, 48, 64, 67, 128) if r <= F] + ([F] if nsel == 1 else [])       # r = F for the narrowest descriptor
    for r in ranks:
        check_describe(ctx, ref, patches, sPR, D64, r, "nsel %d r %d:" % (nsel, r))
    ctx.close()


def test_describe_at_full_width(dlco, ref):
    """nsel = 1024: F = 8192 floats per patch, 128 staged k chunks per output entry."""
    nsel, r = 1024, 128
    patches, sPR = make_patches(5, seed=8192), make_filters(nsel, seed=nsel)
    D64 = oracle_descriptors(ref, patches, sPR)
    ctx = dlco.DescContext()
    ctx.set_filters(sPR)
    check_describe(ctx, ref, patches, sPR, D64, r, "nsel 1024 r 128:")
    ctx.close()


def test_describe_does_not_depend_on_the_chunking(dlco):
    import torch
    nsel, r, n_all = 68, 64, 4100                                        # two whole launch chunks (2048) and a ragged third
    base = make_patches(41, seed=5)
    patches = np.ascontiguousarray(base[np.arange(n_all) % 41])
    ctx = dlco.DescContext()
    ctx.set_filters(make_filters(nsel, seed=nsel))
    ctx.set_projection(make_w(r, nsel * 8, seed=3))
    full = ctx.describe(patches)
    assert np.array_equal(full[:41], full[41:82]) and np.array_equal(full[:41], full[4059:4100])     # a row is its patch's alone
    for n in (1, 2047, 2048, 2049, 4100):
        assert np.array_equal(ctx.describe(patches[:n]), full[:n]), n
    # the device form: r floats per row, the rest of the pitch untouched
    ld, sentinel = r + 5, -7.25
    buf = torch.full((n_all, ld), sentinel, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.describe_device(patches, buf.data_ptr(), ld=ld)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, :r], full)
    assert (got[:, r:] == np.float32(sentinel)).all()
    with pytest.raises(dlco.DlcoError) as ei:
        ctx.describe_device(patches[:4], buf.data_ptr(), ld=r - 1)
    assert ei.value.code == dlco.ERR_INVALID
    ctx.close()


def pair_set(n_base=40, copies=3, n_pairs=3000, seed=9):
    """Patches of n_base "3D points": blended, noisy views of each base patch plus one exact repeat (tied distances); pairs
    (patchID1, 3DpointID1, patchID2, 3DpointID2), half of them forced onto one point."""
    rng = np.random.default_rng(seed)
    base = make_patches(n_base, seed=seed)
    views, ids = [], []
    for i, p in enumerate(base):
        for c in range(copies):
            # a view: the point's patch blended with another point's, so that the two classes overlap
            t = rng.uniform(0.0, 0.75) if c else 0.0
            v = (1 - t) * p.astype(np.float64) + t * base[rng.integers(0, n_base)] + rng.normal(0, 4, p.shape)
            views.append(np.clip(v, 0, 255).astype(np.uint8))
            ids.append(i)
        views.append(views[-1].copy())                                   # an exact repeat of the last view
        ids.append(i)
    patches, ids = np.stack(views), np.array(ids)
    a, b = rng.integers(0, len(ids), n_pairs), rng.integers(0, len(ids), n_pairs)
    b[::2] = [rng.choice(np.nonzero(ids == ids[x])[0]) for x in a[::2]]
    return patches, np.stack([a, ids[a], b, ids[b]], 1).astype(np.int32)


def test_pair_sqdists_match_the_oracle(dlco, ref):
    nsel, r = 68, 64
    patches, pairs = pair_set()
    sPR, W = make_filters(nsel, seed=nsel), make_w(r, nsel * 8, seed=21)
    pairs[5, 2] = pairs[5, 0]                                             # identical ids
    pairs[6] = (17, 3, 17, 4)
    ctx = dlco.DescContext()
    ctx.set_filters(sPR)
    ctx.set_projection(W)
    d, lab = ctx.pair_sqdists(patches, pairs)
    assert d.shape == (len(pairs),) and d.dtype == np.float32
    assert np.array_equal(lab, (pairs[:, 1] == pairs[:, 3]).astype(np.uint8)) and 0 < lab.sum() < len(lab)
    want, e = entry_bound(oracle_descriptors(ref, patches, sPR), W)
    ia, ib = pairs[:, 0], pairs[:, 2]
    delta, es = want[ia] - want[ib], e[ia] + e[ib]
    d_want = (delta * delta).sum(1)
    bound = (2 * np.abs(delta) * es + es * es).sum(1) + EPS * d_want
    err = np.abs(d.astype(np.float64) - d_want)
    ok = bound > 0
    print("pair_sqdists vs oracle: max |err| %.3e, max err/bound %.3f, median d %.4f" % (err.max(), (err[ok] / bound[ok]).max(), np.median(d_want)))
    assert (err <= bound).all()
    assert d[5] == 0.0 and d[6] == 0.0                                   # a patch against itself: exactly zero
    # the distances are those of the rows describe() returns
    Y = ctx.describe(patches)
    dy = ((Y[ia] - Y[ib]).astype(np.float64) ** 2).sum(1)
    assert np.abs(d - dy).max() <= EPS * dy.max()
    for col, val in ((0, len(patches)), (2, -1)):
        bad = pairs.copy()
        bad[11, col] = val
        with pytest.raises(dlco.DlcoError) as ei:
            ctx.pair_sqdists(patches, bad)
        assert ei.value.code == dlco.ERR_INVALID
        with pytest.raises(dlco.DlcoError) as ei:
            ctx.pair_stats(patches, bad)
        assert ei.value.code == dlco.ERR_INVALID
    ctx.close()


def test_pair_stats_are_the_roc_of_the_pair_distances(dlco, ref):
    nsel, r = 68, 64
    patches, pairs = pair_set(seed=4)
    sPR, W = make_filters(nsel, seed=nsel), make_w(r, nsel * 8, seed=22)
    W[7] = 0
    W[40] = 0                                                            # two all-zero rows: used as given, not counted
    ctx = dlco.DescContext()
    ctx.set_filters(sPR)
    ctx.set_projection(W)
    assert ctx.projected_size == r
    assert (ctx.describe(patches[:3])[:, [7, 40]] == 0).all()
    d, lab = ctx.pair_sqdists(patches, pairs)
    assert len(np.unique(d)) < len(d)                                    # repeated patches: tied distances
    dim, f95, auc = ctx.pair_stats(patches, pairs)
    f_ref, a_ref = ref.roc_stats(d, lab)
    assert dim == r - 2
    assert f95 == f_ref
    assert abs(auc - a_ref) <= 1e-12
    assert 0.0 < f95 < 1.0 and 0.5 < auc < 1.0                           # overlapping classes: neither statistic is at an end of its range
    # not gated: the route through the un-projected N x F matrix is another rounding of the same quantity
    dist, lab2 = ctx.pair_dists(patches, pairs)
    tr = dlco.Context(nsel * 8, len(pairs), B=32)
    tr.set_data(dist, lab2)
    dim_u, f_u, a_u = tr.stats(W)
    tr.close()
    print("pair_stats: dim %d fpr95 %.6f auc %.9f; through the un-projected matrix: dim %d, fpr95 differs by %.3e, auc by %.3e"
          % (dim, f95, auc, dim_u, f95 - f_u, auc - a_u))
    ctx.close()


def test_existing_surface_is_untouched_and_a_projection_follows_the_filters(dlco):
    patches, pairs = pair_set(n_base=12, n_pairs=200, seed=2)
    sPR = make_filters(60, seed=60)
    ctx = dlco.DescContext()
    ctx.set_filters(sPR)
    for call in (lambda: ctx.describe(patches), lambda: ctx.pair_sqdists(patches, pairs), lambda: ctx.pair_stats(patches, pairs)):
        with pytest.raises(dlco.DlcoError) as ei:                        # no projection yet
            call()
        assert ei.value.code == dlco.ERR_INVALID
    assert ctx.projected_size == 0
    before_c, (before_d, before_l) = ctx.compute(patches), ctx.pair_dists(patches, pairs)
    for W in (np.zeros((0, 480), np.float32), make_w(3, 472, 1), make_w(481, 480, 1)):     # r < 1, F of another bank, r > F
        with pytest.raises(dlco.DlcoError) as ei:
            ctx.set_projection(W)
        assert ei.value.code == dlco.ERR_INVALID
    ctx.set_projection(make_w(48, 480, seed=1))
    Y = ctx.describe(patches)
    ctx.pair_stats(patches, pairs)
    after_c, (after_d, after_l) = ctx.compute(patches), ctx.pair_dists(patches, pairs)
    assert np.array_equal(before_c, after_c) and np.array_equal(before_d, after_d) and np.array_equal(before_l, after_l)
    # filters of another nsel: the projection no longer fits and is dropped
    ctx.set_filters(make_filters(68, seed=68))
    assert ctx.projected_size == 0 and ctx.size == 544
    with pytest.raises(dlco.DlcoError) as ei:
        ctx.describe(patches)
    assert ei.value.code == dlco.ERR_INVALID
    ctx.set_projection(make_w(48, 544, seed=1))
    assert ctx.describe(patches).shape == (len(patches), 48)
    # filters of the same nsel keep it
    ctx.set_filters(sPR)
    ctx.set_projection(make_w(48, 480, seed=1))
    ctx.set_filters(sPR)
    assert ctx.projected_size == 48 and np.array_equal(ctx.describe(patches), Y)
    # a context without filters has nothing to project
    fresh = dlco.DescContext()
    with pytest.raises(dlco.DlcoError) as ei:
        fresh.set_projection(make_w(4, 8, seed=1))
    assert ei.value.code == dlco.ERR_INVALID
    fresh.close()
    ctx.close()
