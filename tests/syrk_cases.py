"""References and the case table of the gradient SYRK tests (test_syrk_reference.py on the CPU, test_grad_syrk_gpu.py on
the device).  Plain numpy: no GPU, no fixtures.

The operation (kernels_syrk.hip):  C <- beta * C + alpha * (P^T diag(rho) P - N^T diag(kap) N), P = D[pr], N = D[nr], with
the rows of non-zero weight compacted into one list, positives first, w_k = rho_i or -kap_j.  Three arithmetics form the
products: the default three-way split of fl(w_k x_k) and x_k into bf16 parts (16-row K blocks), operands rounded to bf16
once (48-row blocks, cfg.grad_bf16) and v_mfma_f32_32x32x2_f32 on fp32 operands (32-row blocks, DLCO_SYRK_FP32=1).

Integer data makes all three exact, so the result must be the integer computation byte for byte: entries of D in
[-4, 4], weights in [1, 40] (|w x| <= 160 < 256 is exact in bf16, its other two parts are zero), at most 2600 rows (every
partial sum <= 2600 * 40 * 16 < 2^24), old values integers in [-1000, 1000], alpha in {1, 1/4}, beta in {1, 1/2, -2, 0}
(the result is a multiple of 1/4 below 2^22).  Float data is held elementwise to TOL * scale, scale = the sum of the
absolute values of the terms of that element - the gate the tracker products already have (test_tracker_product_kernels)."""
from collections import namedtuple

import numpy as np

TOL = 2e-6                      # the project's constant for split operands / fp32 operands with fp32 accumulation
ALPHAS = (1.0, 0.25)
BETAS = (1.0, 0.5, -2.0, 0.0)
PAIRS = tuple((a, b) for a in ALPHAS for b in BETAS)
NROWS = 64                      # rows of data a context of these tests holds


def bf16_round(x):
    """float32 -> bf16 by round-to-nearest-even, returned as float32: what (__bf16)x does to a finite x."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split3(x):
    """split_f32<3>: x = h + m + l, every part the bf16 rounding of what the parts before it left over."""
    x = np.asarray(x, np.float32)
    h = bf16_round(x)
    r1 = (x - h).astype(np.float32)
    m = bf16_round(r1)
    return h, m, bf16_round((r1 - m).astype(np.float32))


def active_list(pr, nr, rho, kap):
    """The compacted row list of active_rows_body: positives of non-zero rho in slot order, then negatives of non-zero
    kappa; weights as float32 (rho, -kappa)."""
    pr, nr, rho, kap = (np.asarray(v) for v in (pr, nr, rho, kap))
    ids = np.concatenate([pr[rho != 0], nr[kap != 0]]).astype(np.int64)
    w = np.concatenate([rho[rho != 0], -kap[kap != 0]]).astype(np.float32)
    return ids, w


def mirror_upper(M):
    """The matrix whose upper triangle (diagonal included) is M's and whose lower triangle is its mirror."""
    return np.triu(M) + np.triu(M, 1).T


def gram_exact(D, pr, nr, rho, kap):
    """float64 P^T diag(rho) P - N^T diag(kap) N and the sum of the absolute values of its terms."""
    ids, w = active_list(pr, nr, rho, kap)
    X = np.asarray(D, np.float32)[ids].astype(np.float64)
    w = w.astype(np.float64)
    return (X * w[:, None]).T @ X, (np.abs(X) * np.abs(w)[:, None]).T @ np.abs(X)


def once_operands(D, pr, nr, rho, kap):
    """What the bf16-once line multiplies: A[k] = bf16(fl32(w_k x_k)) and B[k] = bf16(x_k), as float32."""
    ids, w = active_list(pr, nr, rho, kap)
    X = np.asarray(D, np.float32)[ids]
    return bf16_round(X * w[:, None]), bf16_round(X)


def gram_once(D, pr, nr, rho, kap):
    """The same from the operands of the bf16-once line, in float64, for i <= j and mirrored: tile (bi, bj), bi <= bj,
    takes A from the row side, a diagonal tile stores il <= jl and mirrors it."""
    A, B = (v.astype(np.float64) for v in once_operands(D, pr, nr, rho, kap))
    return mirror_upper(A.T @ B), mirror_upper(np.abs(A).T @ np.abs(B))


def combine(G, S, alpha, beta, old):
    """(want, scale) of beta * old + alpha * G in float64; old (None: zeros) is read from its upper triangle."""
    F = G.shape[0]
    old = np.zeros((F, F)) if old is None or beta == 0 else mirror_upper(np.asarray(old, np.float64))
    return beta * old + alpha * G, abs(beta) * np.abs(old) + abs(alpha) * S


def want_exact(D, pr, nr, rho, kap, alpha, beta, old):
    return combine(*gram_exact(D, pr, nr, rho, kap), alpha, beta, old)


def want_once(D, pr, nr, rho, kap, alpha, beta, old):
    return combine(*gram_once(D, pr, nr, rho, kap), alpha, beta, old)


def want_int(G, alpha, beta, old):
    """Integer data: the result from the exact Gram matrix G, through int64.  4 * want = (4 beta) old + (4 alpha) G has
    integer coefficients for the (alpha, beta) of this table; the quotient is a multiple of 1/4 below 2^22: a float32."""
    Gi = np.rint(G).astype(np.int64)
    assert np.array_equal(Gi, G) and np.abs(Gi).max(initial=0) < 2 ** 24      # float64 held the integers exactly
    a4, b4 = int(round(4 * alpha)), int(round(4 * beta))
    assert a4 == 4 * alpha and b4 == 4 * beta
    oi = mirror_upper(np.rint(np.asarray(old, np.float64)).astype(np.int64)) if old is not None else np.zeros_like(Gi)
    q = b4 * oi + a4 * Gi
    assert np.abs(q).max(initial=0) < 2 ** 24
    return (q.astype(np.float64) / 4.0).astype(np.float32)


# ---- the cases ------------------------------------------------------------------------------------------------------
# kind: "int" (integer data, byte equality), "normal", "decades" (rows scaled by 10^U(-3, 3)), "cancel" (negative rows =
# positive rows, kap = rho: the exact result is what the one unpaired row of an odd count leaves, or zero).
Case = namedtuple("Case", "F B kact kind alpha beta")
FLOAT_AB = (0.3, 0.9)           # float data: coefficients that round in the epilogue


def planted(B, kact, seed, kind="normal"):
    """(pr, nr, rho, kap) of length B with exactly kact non-zero weights in [1, 40], at random slots among the 2B; row
    ids drawn with replacement from the NROWS rows, so duplicates occur.  kind "cancel": kact // 2 slots carry the same
    row and the same weight on both sides; an odd kact has one more positive row, which nothing cancels."""
    rng = np.random.default_rng(seed)
    assert 0 <= kact <= 2 * B
    pr = rng.integers(0, NROWS, B).astype(np.int32)
    nr = rng.integers(0, NROWS, B).astype(np.int32)
    wt = rng.integers(1, 41, 2 * B).astype(np.int32)
    if kind == "cancel":
        assert (kact + 1) // 2 <= B
        slots = rng.permutation(B)
        rho, kap = np.zeros(B, np.int32), np.zeros(B, np.int32)
        both = slots[:kact // 2]
        rho[both] = kap[both] = wt[both]
        nr[both] = pr[both]
        if kact % 2:
            rho[slots[kact // 2]] = wt[slots[kact // 2]]
    else:
        w = np.zeros(2 * B, np.int32)
        on = rng.permutation(2 * B)[:kact]
        w[on] = wt[on]
        rho, kap = w[:B].copy(), w[B:].copy()
    assert np.count_nonzero(rho) + np.count_nonzero(kap) == kact
    return pr, nr, rho, kap


def data(kind, F, seed):
    """NROWS rows of width F, float32."""
    rng = np.random.default_rng(seed)
    if kind == "int":
        return rng.integers(-4, 5, (NROWS, F)).astype(np.float32)
    D = rng.standard_normal((NROWS, F))
    if kind == "decades":
        D *= 10.0 ** rng.uniform(-3, 3, (NROWS, 1))
    return D.astype(np.float32)


def old_matrix(kind, F, seed, G=None):
    """The dual average that goes in: its upper triangle is what counts, below the diagonal it carries garbage.  Float
    cases: normal entries at the size of the update's own (G: the exact Gram matrix of the case)."""
    rng = np.random.default_rng(seed + 1)
    if kind == "int":
        up = rng.integers(-1000, 1001, (F, F)).astype(np.float32)
    else:
        size = float(np.abs(G).mean()) if G is not None and G.size and np.abs(G).max() > 0 else 1.0
        up = (rng.standard_normal((F, F)) * size).astype(np.float32)
    return (np.triu(up) + np.tril(rng.standard_normal((F, F)) * 1e6 + 12345.0, -1)).astype(np.float32)


def seed_of(c):
    return (c.F * 1000003 + c.B * 7919 + c.kact * 31 + {"int": 0, "normal": 1, "decades": 2, "cancel": 3}[c.kind]) % (2 ** 31)


def inputs(c, D=None):
    """(D, pr, nr, rho, kap) of a case; D may be given (pair mode forms its own)."""
    s = seed_of(c)
    if D is None:
        D = data(c.kind, c.F, c.F + {"int": 0, "normal": 1, "decades": 2, "cancel": 1}[c.kind])    # one matrix per kind and width
    return (D,) + planted(c.B, c.kact, s, c.kind)


# (active rows, B): batches whose 2B is and is not a multiple of 32; B = 17 pads its list 34 -> 64
SWEEP16 = ((0, 17), (1, 32), (15, 17), (16, 32), (17, 17), (32, 17), (33, 17), (48, 32), (49, 40), (64, 32), (65, 40))
# the 48-row blocks of the bf16-once line; B = 24 and B = 32 have kmax = 64, no multiple of 48
SWEEP48 = ((0, 17), (1, 32), (16, 17), (17, 17), (47, 24), (48, 24), (49, 40), (96, 48), (97, 50), (144, 72), (145, 80),
           (64, 32))
SWEEP_AB = (0.25, 0.5)
EDGE_COUNTS = (17, 33, 49, 16, 32, 48, 65)       # where the other seven (alpha, beta) pairs run at the swept widths


def _swept(F, sweep):
    t = []
    for kact, B in sweep:
        t.append(Case(F, B, kact, "int", *SWEEP_AB))
        t.append(Case(F, B, kact, "normal", *FLOAT_AB))
    others = [p for p in PAIRS if p != SWEEP_AB]
    for (a, b), kact in zip(others, EDGE_COUNTS):
        t.append(Case(F, 40, kact, "int", a, b))
    return t


def _wide(F):
    # 400 of 460 slots: every (alpha, beta) on integer data (one Gram matrix serves them all), one float case
    return [Case(F, 230, 400, "int", a, b) for a, b in PAIRS] + [Case(F, 230, 400, "normal", *FLOAT_AB)]


def default_table(F):
    """The cases of the default arithmetic (and of the two switch-selected forms) at user width F."""
    if F in (128, 384):
        t = _swept(F, SWEEP16)
        for kind in ("cancel", "decades"):
            t += [Case(F, 40, 17, kind, *FLOAT_AB), Case(F, 40, 49, kind, *FLOAT_AB), Case(F, 230, 400, kind, *FLOAT_AB)]
        if F == 128:
            t += [Case(F, 1300, 2600, "int", 1.0, 1.0), Case(F, 1300, 2600, "normal", *FLOAT_AB)]
        return t
    if F > 2000:                                 # 19 MB a matrix: the integer cases and one float case
        return _wide(F)
    return _wide(F) + [Case(F, 230, 400, "decades", *FLOAT_AB), Case(F, 230, 400, "cancel", *FLOAT_AB)]


def once_table(F):
    """The cases of the bf16-once line at user width F."""
    return _swept(F, SWEEP48) if F in (128, 384) else _wide(F)


DEFAULT_WIDTHS = (100, 128, 384, 1152, 2176)
ONCE_WIDTHS = (128, 384, 1152)
SWITCH_WIDTHS = (100, 128, 384, 1152)


# ---- numpy emulations of the arithmetic (test_syrk_reference.py) ----------------------------------------------------
def _epilogue(acc, alpha, beta, old):
    a, b = np.float32(alpha), np.float32(beta)
    if beta == 0 or old is None:
        return a * acc
    return (a * acc + b * mirror_upper(np.asarray(old, np.float32))).astype(np.float32)


def emulate_split(D, pr, nr, rho, kap, alpha, beta, old, drop_term=None, drop_row=None):
    """syrk_split_rows_kernel + syrk_planes_kernel<ONCE = false> in numpy: fl32(w x) and x split three ways, per 16-row
    block the six products in the kernel's order (h*l, l*h, m*m, h*m, m*h, h*h; A part first), every rank-1 update
    added to a float32 accumulator in turn, then the epilogue.  drop_term in (0, 1, 2) leaves one of the 2^-16 terms out."""
    ids, w = active_list(pr, nr, rho, kap)
    if drop_row is not None:
        ids, w = np.delete(ids, drop_row), np.delete(w, drop_row)
    X = np.asarray(D, np.float32)[ids]
    Ap, Bp = split3(X * w[:, None]), split3(X)
    terms = [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)]
    F = X.shape[1]
    acc = np.zeros((F, F), np.float32)
    for k0 in range(0, len(ids), 16):
        for n, (pa, pb) in enumerate(terms):
            if n == drop_term:
                continue
            for k in range(k0, min(k0 + 16, len(ids))):
                acc += np.outer(Ap[pa][k], Bp[pb][k])            # the product of two bf16 values is exact in float32
    return mirror_upper(_epilogue(acc, alpha, beta, old))


def emulate_once(D, pr, nr, rho, kap, alpha, beta, old, drop_row=None):
    """syrk_round_rows_kernel + syrk_planes_kernel<ONCE = true>: operands rounded to bf16 once, rank-1 updates added to a
    float32 accumulator in row order."""
    A, B = once_operands(D, pr, nr, rho, kap)
    if drop_row is not None:
        A, B = np.delete(A, drop_row, 0), np.delete(B, drop_row, 0)
    F = B.shape[1]
    acc = np.zeros((F, F), np.float32)
    for k in range(A.shape[0]):
        acc += np.outer(A[k], B[k])
    return mirror_upper(_epilogue(acc, alpha, beta, old))
