"""The gradient SYRK (kernels_syrk.hip) through the dlco_grad_rda probe - active-row list, pack, grad_syrk, unpack, the
trainer's own sequence - at planted active-row counts around every path of its K loops and at tile counts with more
than one super-block and a remainder chunk; tests/syrk_cases.py has the references and the table, test_syrk_reference.py
checks both on the CPU.

Integer data: the result is the int64 computation byte for byte, in every arithmetic.  One assertion without a tolerance
sees a dropped or repeated K block, a tile computed twice or never, a row or column in the wrong place and a stale LDS
stage.  Float data: every element within 2e-6 * (sum of the absolute values of its terms) of float64 - of the exact
product in the default arithmetic and the two switch-selected forms, of the product of the rounded operands on the
bf16-once line, where fp32 accumulation is all that is left.  The two forms behind an environment switch
(DLCO_SYRK_FP32=1: syrk_rda_kernel8, 32-row blocks; DLCO_NO_PACKED=1: the mirrored store of the unpacked layout) run the
default table in a child process each, as tests/test_env_switches_gpu.py does."""
import os
import subprocess
import sys

import numpy as np
import pytest

import syrk_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_GRAMS = {}      # case inputs -> (G, S) of the exact and of the bf16-once product: computed once, shared, never written to
_OLDS = {}


def _grams(c, D, rows, once, pair):
    key = (c.F, c.B, c.kact, c.kind, pair)
    if key not in _GRAMS:
        _GRAMS[key] = {"exact": sc.gram_exact(D, *rows)}
        for v in _GRAMS[key]["exact"]:
            v.setflags(write=False)
    if once and "once" not in _GRAMS[key]:
        _GRAMS[key]["once"] = sc.gram_once(D, *rows)
        for v in _GRAMS[key]["once"]:
            v.setflags(write=False)
    return _GRAMS[key]


def _old(c, G, pair):
    key = (c.F, c.B, c.kact, c.kind, pair)
    if key not in _OLDS:
        _OLDS[key] = sc.old_matrix(c.kind, c.F, sc.seed_of(c), G)
        _OLDS[key].setflags(write=False)
    return _OLDS[key]


def _check(ctx, c, D, rows, once, pair=False):
    """One probe call under the assertions of its kind; returns the largest |got - want| / scale (0 for integer data)."""
    g = _grams(c, D, rows, once, pair)
    G, S = g["exact"]
    old = _old(c, G, pair)
    got = ctx.grad_rda(*rows, c.alpha, c.beta, old)
    assert got.shape == (c.F, c.F) and np.array_equal(got, got.T), (c, "not symmetric")
    if c.kind == "int":
        want = sc.want_int(G, c.alpha, c.beta, old)
        if got.tobytes() != want.tobytes():
            bad = np.argwhere(got != want)
            raise AssertionError("%s once=%d: %d elements differ from the integer result, first at %s: got %r, want %r"
                                 % (c, once, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))
        return 0.0
    we, se = sc.combine(G, S, c.alpha, c.beta, old)
    want, scale = sc.combine(*g["once"], c.alpha, c.beta, old) if once else (we, se)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(scale, 1e-300)).max())
    print("  %s once=%d: |got - want| / scale <= %.2e" % (c, once, ratio))
    assert (err <= sc.TOL * scale).all(), (c, once, ratio)
    if once and c.kact >= 16:                                     # the bf16 path really ran
        assert (np.abs(got - we) > 1e-4 * se).any(), (c, "as exact as the split arithmetic")
    return ratio


def _beta_zero(ctx, c, D, rows):
    """beta = 0 selects 0.f instead of beta * old: a dual average full of NaN gives the bytes of a call without one."""
    nan = np.full((c.F, c.F), np.nan, np.float32)
    a = ctx.grad_rda(*rows, c.alpha, 0.0, nan)
    b = ctx.grad_rda(*rows, c.alpha, 0.0, None)
    assert a.tobytes() == b.tobytes(), (c, "beta = 0 read the old matrix")
    assert a.tobytes() == sc.want_int(sc.gram_exact(D, *rows)[0], c.alpha, 0.0, None).tobytes(), c


def _labels():
    return (np.arange(sc.NROWS) % 2 == 0).astype(np.uint8)


def _run_table(dlco, F, table, once, tag):
    """One context of width F; the data changes with the kind of the case."""
    ctx = dlco.Context(F, sc.NROWS, B=8, grad_bf16=int(once))
    try:
        worst, loaded = 0.0, None
        for c in sorted(table, key=lambda c: c.kind):
            D, *rows = sc.inputs(c)
            kind = "normal" if c.kind == "cancel" else c.kind
            if kind != loaded:
                ctx.set_data(D, _labels())
                loaded = kind
            worst = max(worst, _check(ctx, c, D, rows, once))
            if c.kind == "int" and c.beta == 0.0:
                _beta_zero(ctx, c, D, rows)
        assert any(c.kind == "int" and c.beta == 0.0 for c in table)
    finally:
        ctx.close()
    print("worst |got - want| / scale, %s, F = %d: %.2e" % (tag, F, worst))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("F", [100, 128, 384, 1152, 2176])
def test_default_arithmetic(dlco, F):
    """Three-way split planes, 16-row K blocks: nk = 0, 1, 2, 3, 4, 5 blocks and their edges, 2600 rows, 1 to 153 tiles."""
    _run_table(dlco, F, sc.default_table(F), False, "three-way split")


@pytest.mark.gpu
@pytest.mark.parametrize("F", [128, 384, 1152])
def test_bf16_once_line(dlco, F):
    """Operands rounded once, 48-row K blocks of a list padded to 32: the k < kmax guard and a partly filled last image."""
    _run_table(dlco, F, sc.once_table(F), True, "bf16 once")


def _pair_inputs(kind):
    """test_gpu_parity._pair_case's construction at 64 pairs of 30 patches; integer descriptors in [-2, 2] for the
    integer cases (differences in [-4, 4]).  D = float32(desc1 - desc2) is the one rounding the kernels perform."""
    from test_gpu_parity import _pair_case
    desc, pairs, D, _ = _pair_case(sc.NROWS, 384, 30, seed=11)
    if kind == "int":
        desc = np.random.default_rng(12).integers(-2, 3, desc.shape).astype(np.float32)
        D = (desc[pairs[:, 0]] - desc[pairs[:, 2]]).astype(np.float32)
    return desc, pairs, D


@pytest.mark.gpu
@pytest.mark.parametrize("once", [False, True])
def test_pair_mode(dlco, once):
    """Rows formed inside the split / round kernels as D[ids] - D[ids2] (dlco_set_pairs)."""
    ctx = dlco.Context(384, sc.NROWS, B=8, grad_bf16=int(once))
    try:
        worst = 0.0
        for kind, (alpha, beta) in (("int", (0.25, -2.0)), ("normal", sc.FLOAT_AB)):
            desc, pairs, D = _pair_inputs(kind)
            ctx.set_pairs(desc, pairs)
            assert np.array_equal(ctx.get_rows(0, sc.NROWS), D)
            for kact in (17, 49):
                c = sc.Case(384, 40, kact, kind, alpha, beta)
                worst = max(worst, _check(ctx, c, D, sc.inputs(c, D)[1:], once, pair=True))
    finally:
        ctx.close()
    print("worst |got - want| / scale, pair mode, %s: %.2e" % ("bf16 once" if once else "three-way split", worst))


SWITCHES = {"syrk_fp32": {"DLCO_SYRK_FP32": "1"}, "no_packed": {"DLCO_NO_PACKED": "1"}}


def _child(name):
    import importlib
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch  # noqa: F401  (first HIP runtime in the process, see conftest.py)
    dlco = importlib.import_module("opencv-dlco_amd")
    assert all(os.environ.get(k) == v for k, v in SWITCHES[name].items())
    for F in sc.SWITCH_WIDTHS:
        _run_table(dlco, F, sc.default_table(F), False, name)
    print("child ok")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_switch_selected_form(name):
    env = dict(os.environ)
    env.update(SWITCHES[name])
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True, text=True, timeout=300,
                       env=env)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("child ok"), p.stdout[-3000:] + p.stderr[-3000:]


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child" and sys.argv[2] in SWITCHES:
        _child(sys.argv[2])
    else:
        raise SystemExit("usage: test_grad_syrk_gpu.py --child <%s>" % "|".join(sorted(SWITCHES)))
