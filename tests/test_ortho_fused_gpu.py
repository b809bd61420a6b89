"""The tail of a tracker pass through dlco_ortho_probe: last filter product -> CholQR2 -> exact product -> T = Yb Qo^T.

In the steady state (packed dual average, one panel, nothing locked, at most 96 rows) the reductions of the two products
also form the K-slice partials of the Gram product behind them (reduce_gram_kernel, kernels_bf16x2.hip), and CholQR
applies L^-1 by column slabs that leave the second pass's Gram partials and then the three-way planes of Qo behind
(linv_apply_kernel); the probe's `unfused` flag forces the launches those forms replace.  The fused form may change where the arithmetic runs, never the
arithmetic: for every case
  * Qo, Yb and T of the fused and the unfused run are equal bit for bit, and
  * their SHA-256 equal those in tests/golden/ortho_fused_hashes.json, taken with tests/golden/make_ortho_golden.py from
    the kernels and launches of the commit before the fused form existed (a helper both forms share cannot drift unseen).
Cases, the smallest that reach every branch: F = 256 (two slabs of two 64-column slices) and F = 640 (five slabs: the
padded tile count of the symmetric product is odd) with m = 32, 33, 64, 96 (row-tile boundaries, a padded row tile);
at F = 640, m = 96 a block with an all-zero row and one with a duplicated row (the dead-row rule must see the same Gram
entries); F = 8192, m = 96, the only width at which a slab is a single 128-column slice and the wide ordered reduce runs.
Inputs: Z, Zprev [m, F] standard normal with rows scaled over two decades, G's packed upper tiles standard normal /
sqrt(F) with symmetric diagonal tiles, coefficients of a Chebyshev term (alpha, b1, b2) = (-0.37, 0.21, -1).
The fallbacks (m = 97, two panels, locked rows) must report through the counters that CholQR ran unfused."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ortho_fused_hashes.json")
ALPHA, B1, B2 = -0.37, 0.21, -1.0


def packed_g(F, seed):
    """Packed upper tiles of a symmetric G (layout: dlco.h, dlco_ortho_probe)."""
    nt = F // 128
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((nt * (nt + 1) // 2, 128, 128), dtype=np.float32) / np.float32(np.sqrt(F))
    t = 0
    for i in range(nt):
        g[t] = np.triu(g[t]) + np.triu(g[t], 1).T              # tile (i, i)
        t += nt - i
    return g


def rows(m, F, seed):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((m, F), dtype=np.float32)
    return (Z * (10.0 ** rng.uniform(-1.0, 1.0, size=(m, 1))).astype(np.float32)).astype(np.float32)


def _cases():
    """name -> (F, m, row to zero or None, (copy, original) or None)"""
    out = {}
    for F in (256, 640):
        for m in (32, 33, 64, 96):
            out["F%d_m%d" % (F, m)] = (F, m, None, None)
    out["F640_m96_zero_row"] = (640, 96, 40, None)
    out["F640_m96_copy_row"] = (640, 96, None, (5, 3))
    out["F8192_m96"] = (8192, 96, None, None)
    return out


CASES = _cases()


def inputs(name):
    F, m, zero, copy = CASES[name]
    seed = 1000 * F + m
    Z, Zprev = rows(m, F, seed), rows(m, F, seed + 1)
    if zero is not None:
        Z[zero] = 0.0
        Zprev[zero] = 0.0
    if copy is not None:
        Z[copy[0]] = Z[copy[1]]
        Zprev[copy[0]] = Zprev[copy[1]]
    return Z, Zprev, packed_g(F, seed + 2)


def digest(r):
    return {k: hashlib.sha256(np.ascontiguousarray(r[k]).tobytes()).hexdigest() for k in ("Qo", "Yb", "T")}


_ctx = {}


@pytest.fixture(scope="module")
def ctx_of(dlco):
    def get(F):
        if F not in _ctx:
            _ctx[F] = dlco.Context(F, 16, B=4)
        return _ctx[F]
    yield get
    for c in _ctx.values():
        c.close()
    _ctx.clear()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_equals_unfused_and_golden(ctx_of, golden, name):
    F, m, zero, copy = CASES[name]
    Z, Zprev, Gp = inputs(name)
    ctx = ctx_of(F)
    fused = ctx.ortho_probe(Z, Gp, ALPHA, B1, B2, Zprev=Zprev)
    plain = ctx.ortho_probe(Z, Gp, ALPHA, B1, B2, Zprev=Zprev, unfused=True)
    print("%s: fused reductions %d / %d, fused applications %d / %d" % (name, fused["fused"], plain["fused"], fused["applied"], plain["applied"]))
    assert fused["fused"] == 2 and fused["applied"] == 2 and plain["fused"] == 0 and plain["applied"] == 0
    for k in ("Qo", "Yb", "T"):
        assert np.array_equal(fused[k].view(np.uint32), plain[k].view(np.uint32)), "%s differs in bits between the two forms" % k
    assert digest(fused) == golden[name]
    # the block that comes out is what CholQR2 promises: orthonormal live rows, dead rows exactly zero
    Q = fused["Qo"].astype(np.float64)
    dead = [zero] if zero is not None else ([copy[0]] if copy is not None else [])
    live = [i for i in range(m) if i not in dead]
    for i in dead:
        assert not fused["Qo"][i].any()
    # (a sanity bound, the hashes are the check: the second pass forms its Gram entries as fp32 chains over F terms and
    # its rows as chains over m terms, so |Qo Qo^T - I| is below (F + 2 m) roundings of 2^-24 whatever the data)
    orth = np.abs(Q[live] @ Q[live].T - np.eye(len(live))).max()
    print("%s: |Qo Qo^T - I|max %.3e" % (name, orth))
    assert orth <= (F + 2 * m) * 2.0 ** -24


@pytest.mark.parametrize("why, kw, m", [("97 rows", {}, 97), ("two panels", dict(panel_end=48), 96), ("locked rows", dict(n_lock=8), 96)])
def test_fallbacks_take_the_unfused_launches(ctx_of, why, kw, m):
    """Outside the steady state's conditions CholQR's Gram products and applications are launches of their own (the
    counters say so); the Rayleigh-Ritz T keeps the fused form wherever the block is at most 96 rows."""
    F = 256
    Z, Zprev, Gp = rows(m, F, 7), rows(m, F, 8), packed_g(F, 9)
    if "n_lock" in kw:                                           # locked rows are orthonormal as they come and stay as they are
        Z[:8] = 0.0
        Z[:8, :8] = np.eye(8, dtype=np.float32)
    r = ctx_of(F).ortho_probe(Z, Gp, ALPHA, B1, B2, Zprev=Zprev, **kw)
    assert r["fused"] == (0 if m > 96 else 1) and r["applied"] == 0, (why, r["fused"], r["applied"])
    assert np.isfinite(r["T"]).all()
