"""Batched verification on match lists in device memory with the refit on the device: dlco_desc_verify_pairs_homography_device
and dlco_desc_verify_pairs_fundamental_device.  The contract is that pair p's matrix, mask slice, count and best hypothesis are
byte for byte what the host forms return for the same lists, so every answer is compared with the host form (whose refit is
formed on the host), with the numpy restatements of tests/test_verify_rules.py and tests/test_epipolar_rules.py and, for the
largest pairs, with the C++ host frame on the CPU.  The batches are those of tests/test_verify_pairs_gpu.py, whose pairs leave
the lockstep refit at different rounds."""
import numpy as np
import pytest

import test_verify_batch_rules as B
from test_verify_pairs_gpu import EMPTY, MODELS, SETTINGS, Model, check_against_host_frame, check_against_restatement, main_batch, same_triple
from test_verify_rules import bits

pytestmark = pytest.mark.gpu
POISON = 9


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.DescContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_frame(tmp_path_factory):
    return B.build_shim(tmp_path_factory)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def device_form(ctx, name, lists, with_mask=True, **kw):
    """the device form on lists uploaded with torch: a list of (M [3,3], inlier [m] bool or None, best_hyp), and the counts"""
    import torch
    s, d, moff = ctx._match_lists(lists)                                     # one list with a row of padding, and the offsets
    ts, td = dev(s), dev(d)
    mask = torch.full((len(s),), POISON, dtype=torch.uint8, device="cuda:0") if with_mask else None
    torch.cuda.synchronize()
    call = ctx.verify_pairs_fundamental_device if name == "fundamental" else ctx.verify_pairs_homography_device
    M, n, best = call(ts.data_ptr(), td.data_ptr(), moff, inlier_ptr=mask.data_ptr() if with_mask else None, **kw)
    torch.cuda.synchronize()
    assert ts.cpu().numpy().tobytes() == s.tobytes() and td.cpu().numpy().tobytes() == d.tobytes()           # the lists are read in place, not written
    if not with_mask:
        return [(M[p], None, int(best[p])) for p in range(len(lists))], n
    k = mask.cpu().numpy()
    assert (k[moff[-1]:] == POISON).all() and set(np.unique(k[:moff[-1]]).tolist()) <= {0, 1}
    out = [(M[p], k[moff[p]:moff[p + 1]].astype(bool), int(best[p])) for p in range(len(lists))]
    assert all(int(o[1].sum()) == n[p] for p, o in enumerate(out))
    return out, n


@pytest.mark.parametrize("name", MODELS)
def test_main_batch(ctx, host_frame, name):
    M = Model(ctx, name)
    _, lists, want = main_batch(name)
    got, _ = device_form(ctx, name, lists, **SETTINGS)
    assert ctx.last_kernel_ms() > 0
    host = M.batch(lists, **SETTINGS)
    for p, (g, h) in enumerate(zip(got, host)):
        assert same_triple(g, h), (name, p, len(lists[p][0]))
    check_against_restatement(M, got, lists, want)
    largest = sorted(range(len(lists)), key=lambda p: -len(lists[p][0]))[:3]
    check_against_host_frame(M, host_frame, got, lists, largest, **SETTINGS)


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("refine", [0, 1])
def test_no_round_and_one_round(ctx, name, refine):
    M = Model(ctx, name)
    _, lists, want = main_batch(name)
    kw = dict(SETTINGS, refine=refine)
    got, _ = device_form(ctx, name, lists, **kw)
    for p, (g, h) in enumerate(zip(got, M.batch(lists, **kw))):
        assert same_triple(g, h), (name, p, refine)
    check_against_restatement(M, got, lists, [M.ref(s, d, **kw) if w else None for (s, d), w in zip(lists, want)])


@pytest.mark.parametrize("name", MODELS)
def test_without_a_mask_and_without_a_match(ctx, name):
    M = Model(ctx, name)
    _, lists, want = main_batch(name)
    got, n = device_form(ctx, name, lists, with_mask=False, **SETTINGS)
    for p, w in enumerate(want):
        assert n[p] == (w["count"] if w else 0) and got[p][2] == (w["best"] if w else -1), p
        assert np.array_equal(bits(got[p][0]).reshape(9), bits(w[M.key]) if w else np.zeros(9, np.uint64)), p
    none, n = device_form(ctx, name, [EMPTY, EMPTY, EMPTY], **SETTINGS)
    assert all(not bits(g[0]).any() and g[1].shape == (0,) and g[2] == -1 for g in none) and not n.any()
    short = [M.planted(M.sample - 1, 3), EMPTY, lists[5]]
    got, n = device_form(ctx, name, short, **SETTINGS)
    assert not bits(got[0][0]).any() and not got[0][1].any() and got[0][2] == -1 and n[0] == 0 and same_triple(got[2], M.batch(lists[5:6], **SETTINGS)[0])


@pytest.mark.parametrize("name", MODELS)
def test_the_batch_twice_in_one_call_the_second_copy_reversed(ctx, name):
    """live flags and slots do not leak between entries: the answers are permuted, nothing else"""
    _, lists, want = main_batch(name)
    P = len(lists)
    once, _ = device_form(ctx, name, lists, **SETTINGS)
    got, _ = device_form(ctx, name, lists + lists[::-1], **SETTINGS)
    for p in range(P):
        assert same_triple(got[p], once[p]) and same_triple(got[2 * P - 1 - p], once[p]), (name, p)
    check_against_restatement(Model(ctx, name), got[:P], lists, want)


@pytest.mark.parametrize("name", MODELS)
def test_several_launches(ctx, dlco, name):
    """five pairs at the library's largest hypothesis count, which the plan cuts into more than one launch"""
    M = Model(ctx, name)
    lists = [M.planted(12, 40 + k) for k in range(5)]
    launch = dlco.verify_pairs_launches(np.arange(6) * 12, 2 ** 20, name == "fundamental")
    assert launch.max() >= 1 and launch.min() == 0
    kw = dict(threshold=1.5, n_hyp=2 ** 20, seed=7, refine=2)
    got, _ = device_form(ctx, name, lists, **kw)
    for p, (g, h) in enumerate(zip(got, M.batch(lists, **kw))):
        assert same_triple(g, h) and g[2] >= 0, (name, p)


# ---- the chain on the device -----------------------------------------------------------------------------------------------------
R_CHAIN, SIZES_CHAIN = 16, (300, 257, 129)
H_CHAIN = [np.eye(3), np.array([[0.95, -0.05, 20.0], [0.04, 1.02, -10.0], [1e-5, -2e-5, 1.0]]), np.array([[1.05, 0.02, -15.0], [-0.03, 0.97, 12.0], [-1e-5, 1e-5, 1.0]])]


def chain_images():
    """three views of one set of 300 keypoints: most rows of a view are noisy copies of the set's descriptors at the set's
    coordinates under the view's homography, the rest are fresh"""
    rng = np.random.default_rng(9)
    base, bxy = rng.standard_normal((300, R_CHAIN)) * 0.25, rng.uniform(0, 640, (300, 2))
    tabs, xys = [], []
    for n, H in zip(SIZES_CHAIN, H_CHAIN):
        rows, keep = rng.permutation(300)[:n], int(0.7 * n)
        tab = base[rows] + rng.standard_normal((n, R_CHAIN)) * 0.02
        tab[keep:] = rng.standard_normal((n - keep, R_CHAIN)) * 0.25
        p = np.c_[bxy[rows], np.ones(n)] @ H.T
        xy = p[:, :2] / p[:, 2:] + rng.normal(0, 0.3, (n, 2))
        xy[keep:] = rng.uniform(0, 640, (n - keep, 2))
        tabs.append(tab.astype(np.float32))
        xys.append(xy.astype(np.float32))
    return tabs, xys


def test_the_chain_stays_on_the_device(ctx, dlco):
    """match_pairs_device -> select_pairs_device -> verify_pairs_homography_device -> match_pairs_guided_device against the same
    chain through the host forms: only moff and the matrices come down in between"""
    import torch
    tabs, xys = chain_images()
    pairs = [(a, b) for a in range(3) for b in range(3) if a != b]
    reverse = [pairs.index((b, a)) for a, b in pairs]
    kw = dict(threshold=2.0, n_hyp=256, seed=1, refine=4)
    # the host forms
    ans = ctx.match_pairs(tabs, pairs)
    sel, lists = ctx.select_pairs(ans, SIZES_CHAIN, pairs, 0.8, reverse, xys)
    ver = ctx.verify_pairs_homography(lists, **kw)
    H = np.array([v[0] for v in ver])
    guided = ctx.match_pairs_guided(tabs, xys, pairs, H, radius=4.0)
    assert all(v[2] >= 0 and v[1].sum() >= 20 for v in ver)                 # every pair has a model worth guiding with
    # the same on the device
    seg = np.concatenate([[0], np.cumsum(SIZES_CHAIN)]).astype(np.int64)
    row0 = dlco.match_pairs_rows(seg, pairs)
    R = int(row0[-1])
    table, xy = dev(np.concatenate(tabs)), dev(np.concatenate(xys))
    idx, d = torch.empty((R, 2), dtype=torch.int32, device="cuda:0"), torch.empty((R, 2), dtype=torch.float32, device="cuda:0")
    m, dd = torch.empty((R, 2), dtype=torch.int32, device="cuda:0"), torch.empty((R,), dtype=torch.float32, device="cuda:0")
    src, dst = torch.empty((R, 2), dtype=torch.float32, device="cuda:0"), torch.empty((R, 2), dtype=torch.float32, device="cuda:0")
    mask = torch.full((R,), POISON, dtype=torch.uint8, device="cuda:0")
    idx2, d2 = torch.empty((R, 2), dtype=torch.int32, device="cuda:0"), torch.empty((R, 2), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.match_pairs_device(table.data_ptr(), seg, pairs, R_CHAIN, idx.data_ptr(), d.data_ptr())
    moff = ctx.select_pairs_device(idx.data_ptr(), d.data_ptr(), seg, pairs, m.data_ptr(), dd.data_ptr(), ratio=0.8, back_idx_ptr=idx.data_ptr(),
                                   back_row0=row0[reverse], n_back_rows=R, xy_ptr=xy.data_ptr(), ldxy=2, src_ptr=src.data_ptr(), dst_ptr=dst.data_ptr())
    Hd, n, best = ctx.verify_pairs_homography_device(src.data_ptr(), dst.data_ptr(), moff, inlier_ptr=mask.data_ptr(), **kw)
    ctx.match_pairs_guided_device(table.data_ptr(), xy.data_ptr(), seg, pairs, R_CHAIN, Hd, idx2.data_ptr(), d2.data_ptr(), radius=4.0)
    torch.cuda.synchronize()
    assert moff.tolist() == np.concatenate([[0], np.cumsum([len(s[0]) for s in sel])]).tolist()
    k, i2, s2 = mask.cpu().numpy(), idx2.cpu().numpy(), d2.cpu().numpy()
    assert (k[moff[-1]:] == POISON).all()
    for p in range(len(pairs)):
        assert Hd[p].tobytes() == ver[p][0].tobytes() and best[p] == ver[p][2] and n[p] == ver[p][1].sum(), p
        assert np.array_equal(k[moff[p]:moff[p + 1]].astype(bool), ver[p][1]), p
        assert i2[row0[p]:row0[p + 1]].tobytes() == guided[p][0].tobytes() and s2[row0[p]:row0[p + 1]].tobytes() == guided[p][1].tobytes(), p
