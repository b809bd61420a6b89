"""CholQR's Cholesky-inverse kernel alone (chol_inv2_kernel, kernels_eig.hip) through dlco_chol_probe.

The kernel's schedule may change, its arithmetic may not: every entry of Linv goes through the same fused multiply-adds in
the same order whatever the LDS layout or the overlap of its phases.  tests/golden/chol_linv_hashes.json therefore holds,
per case, the SHA-256 of the Linv bytes and of the dead flags as the kernel produced them before its LDS images were re-laid
for wide reads, and |Linv M Linv^T - I|max over the live rows as measured then.  Each case asks for
  * the same bits: both hashes equal the golden ones,
  * dead == the float64 rule on the same float32 M (pivot of the float64 elimination <= rel_thresh * M_jj, or M_jj <= 0;
    a dead row is eliminated from nothing), and
  * |Linv M Linv^T - I|max over the live rows <= twice the stored value (the hashes being exact, this bound only guards
    the golden file itself).
Cases: n = 1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160 (every row-block count of the three instantiations, each block
boundary from both sides) on M = Z Z^T in float64 rounded to float32, Z [n, 256] from default_rng(n) with rows scaled
log-uniformly over three decades; at n = 96 a row that is an exact copy of another, an all-zero row, and M = I + E on both
sides of the fast path's |E|_F^2 <= 1e-6."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_THRESH = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chol_linv_hashes.json")
SIZES = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160)


def _z(n, seed):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, 256))
    return Z * 10.0 ** rng.uniform(-1.5, 1.5, size=(n, 1))


def _gram(Z):
    return (Z @ Z.T).astype(np.float32)


def _near_identity(n, frob2, seed):
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((n, n))
    E = E + E.T
    E *= np.sqrt(frob2) / np.linalg.norm(E)
    return (np.eye(n) + E).astype(np.float32)


def _cases():
    """name -> (M float32 [n, n], rows expected dead or None for 'whatever the float64 rule says')"""
    out = {}
    for n in SIZES:
        out["gram_%d" % n] = (_gram(_z(n, n)), None)
    Z = _z(96, 1096)
    Z[5] = Z[3]
    out["copy_row_96"] = (_gram(Z), [5])
    Z = _z(96, 2096)
    Z[40] = 0.0
    out["zero_row_96"] = (_gram(Z), [40])
    out["fast_path_96"] = (_near_identity(96, 2.5e-7, 3096), [])
    out["slow_path_96"] = (_near_identity(96, 4e-6, 4096), [])
    return out


CASES = _cases()


def _dead_rule(M):
    """The kernel's dead-row rule carried out in float64 on the float32 matrix."""
    A = M.astype(np.float64)
    n = A.shape[0]
    dead = np.zeros(n, np.int32)
    for j in range(n):
        piv, d0 = A[j, j], float(M[j, j])
        if not (piv > REL_THRESH * d0) or not (d0 > 0.0):
            dead[j] = 1
            continue
        A[j + 1:, :] -= np.outer(A[j + 1:, j] / piv, A[j, :])
    return dead


def _residual(M, Linv, dead):
    live = np.flatnonzero(dead == 0)
    L = Linv.astype(np.float64)[live]
    R = L @ M.astype(np.float64) @ L.T - np.eye(live.size)
    return float(np.abs(R).max()) if live.size else 0.0


def measure(ctx, name):
    """What the golden file stores for one case."""
    M, _ = CASES[name]
    Linv, dead = ctx.chol_probe(M, REL_THRESH)
    return dict(linv_sha256=hashlib.sha256(np.ascontiguousarray(Linv).tobytes()).hexdigest(),
                dead_sha256=hashlib.sha256(np.ascontiguousarray(dead).tobytes()).hexdigest(),
                resid=_residual(M, Linv, dead)), Linv, dead


@pytest.fixture(scope="module")
def ctx(dlco):
    c = dlco.Context(128, 16, B=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_chol_probe(ctx, golden, name):
    M, want_dead = CASES[name]
    got, Linv, dead = measure(ctx, name)
    g = golden[name]
    print("%s: resid %.3e (golden %.3e) dead rows %s" % (name, got["resid"], g["resid"], np.flatnonzero(dead).tolist()))
    assert got["linv_sha256"] == g["linv_sha256"], "Linv differs in bits from the golden kernel's"
    assert got["dead_sha256"] == g["dead_sha256"], "dead flags differ from the golden kernel's"
    assert np.array_equal(dead, _dead_rule(M))
    if want_dead is not None:
        assert np.flatnonzero(dead).tolist() == want_dead
    for i in np.flatnonzero(dead):
        assert not Linv[i].any(), "row %d is dead but its row of Linv is not zero" % i
    if name != "fast_path_96":                                # I - E/2 is symmetric, not triangular
        assert np.array_equal(Linv, np.tril(Linv))
    assert got["resid"] <= 2.0 * g["resid"]


def test_fast_path_is_taken(ctx):
    """M = I + E with |E|_F^2 = 2.5e-7 returns I - E/2 exactly (the fast path); at 4e-6 it does not."""
    M, _ = CASES["fast_path_96"]
    Linv, _ = ctx.chol_probe(M, REL_THRESH)
    assert np.array_equal(Linv, (1.5 * np.eye(96, dtype=np.float32) - np.float32(0.5) * M).astype(np.float32))
    M, _ = CASES["slow_path_96"]
    Linv, _ = ctx.chol_probe(M, REL_THRESH)
    assert np.array_equal(Linv, np.tril(Linv)) and not np.array_equal(Linv, (1.5 * np.eye(96, dtype=np.float32) - np.float32(0.5) * M))
