"""The references of the gradient SYRK tests, checked on the CPU: bf16_round against torch, and numpy emulations of the
split and bf16-once arithmetic (syrk_cases.emulate_split / emulate_once) against the float64 references and the gate
that test_grad_syrk_gpu.py holds the device to.  The gate has to be one the arithmetic itself satisfies, with room, and
one a defect breaks: a split product with one of its 2^-16 terms missing, a bf16-once product with one row missing."""
import numpy as np
import pytest
import torch

import syrk_cases as sc


def _ratio(got, want, scale):
    return float((np.abs(got.astype(np.float64) - want) / np.maximum(scale, 1e-300)).max())


def _within(got, want, scale):
    return bool((np.abs(got.astype(np.float64) - want) <= sc.TOL * scale).all())


def _case_inputs(c):
    D, pr, nr, rho, kap = sc.inputs(c)
    G, _ = sc.gram_exact(D, pr, nr, rho, kap)
    old = sc.old_matrix(c.kind, c.F, sc.seed_of(c), G)
    return D, pr, nr, rho, kap, c.alpha, c.beta, old


def test_bf16_round_is_torch_round_to_nearest_even():
    rng = np.random.default_rng(1)
    x = np.concatenate([
        rng.standard_normal(20000).astype(np.float32) * np.float32(10.0) ** rng.integers(-20, 20, 20000).astype(np.float32),
        np.array([0.0, -0.0, 1.0, -1.0, 160.0, 255.0, 256.0, 257.0], np.float32),
    ])
    # exact ties: the 16 dropped bits are 0x8000; the kept mantissa's last bit even (round down) and odd (round up)
    base = rng.integers(0x00800000, 0x7F000000, 4000).astype(np.uint32)
    ties_even = (base & np.uint32(0xFFFE0000)) | np.uint32(0x8000)
    ties_odd = (base & np.uint32(0xFFFE0000)) | np.uint32(0x18000)
    # the kept mantissa all ones and the dropped half at or above the tie: rounds up into the next binade
    carry = (base & np.uint32(0xFF800000)) | np.uint32(0x007F8000) | (base & np.uint32(0x7FFF))
    bits = np.concatenate([ties_even, ties_odd, carry])
    x = np.concatenate([x, bits.view(np.float32), (bits | np.uint32(0x80000000)).view(np.float32)])
    got = sc.bf16_round(x)
    want = torch.tensor(x).to(torch.bfloat16).float().numpy()
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()          # bytes: the sign of zero counts
    t = sc.bf16_round(ties_even.view(np.float32)).view(np.uint32)
    assert np.array_equal(t, ties_even & np.uint32(0xFFFF0000))                  # ties to even went down ...
    t = sc.bf16_round(ties_odd.view(np.float32)).view(np.uint32)
    assert np.array_equal(t, (ties_odd & np.uint32(0xFFFF0000)) + np.uint32(0x10000))   # ... and up
    c = sc.bf16_round(carry.view(np.float32)).view(np.uint32)
    assert np.array_equal(c, (carry & np.uint32(0xFF800000)) + np.uint32(0x00800000))   # 2^(e+1) exactly


def test_split_parts_sum_to_the_value():
    x = (np.random.default_rng(2).standard_normal(5000) * 37.0).astype(np.float32)
    h, m, l = sc.split3(x)
    assert np.array_equal((h.astype(np.float64) + m + l).astype(np.float32), x)   # 3 x 8 bits: all 24 of the mantissa
    for p in (h, m, l):
        assert np.array_equal(sc.bf16_round(p), p)


def _int_pairs(table):
    return {(c.alpha, c.beta) for c in table if c.kind == "int"}


def test_planted_counts_and_table():
    for B, kact in ((17, 0), (17, 34), (32, 33), (1300, 2600), (40, 17)):
        for kind in ("normal", "cancel"):
            pr, nr, rho, kap = sc.planted(B, kact, 5, kind)
            assert np.count_nonzero(rho) + np.count_nonzero(kap) == kact and rho.size == kap.size == B
            assert rho.max(initial=0) <= 40 and kap.max(initial=0) <= 40 and min(rho.min(), kap.min()) >= 0
            if kind == "cancel":
                assert np.count_nonzero(rho != kap) == kact % 2 and np.array_equal(pr[kap != 0], nr[kap != 0])
    assert len(np.unique(sc.planted(200, 400, 1)[0])) < 200                        # duplicates among the row ids
    for F in (128, 384):
        counts = {c.kact for c in sc.default_table(F)}
        assert {0, 1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 400} <= counts and (2600 in counts) == (F == 128)
        assert {(c.B, c.kact) for c in sc.default_table(F)} >= {(17, 33), (32, 64)}
        assert {0, 1, 16, 17, 47, 48, 49, 96, 97, 144, 145, 64} <= {c.kact for c in sc.once_table(F)}
        assert _int_pairs(sc.once_table(F)) == set(sc.PAIRS)
    for F in sc.DEFAULT_WIDTHS:
        assert _int_pairs(sc.default_table(F)) == set(sc.PAIRS)                    # every (alpha, beta) at every width
        assert any(c.kact == 400 for c in sc.default_table(F))


def test_integer_data_is_exact_in_both_emulations():
    for c in (sc.Case(128, 40, 49, "int", 0.25, -2.0), sc.Case(100, 230, 400, "int", 1.0, 0.5)):
        args = _case_inputs(c)
        want = sc.want_int(sc.gram_exact(*args[:5])[0], c.alpha, c.beta, args[7])
        assert sc.emulate_split(*args).tobytes() == want.tobytes()
        assert sc.emulate_once(*args).tobytes() == want.tobytes()
        assert np.array_equal(sc.want_exact(*args)[0], want) and np.array_equal(sc.want_once(*args)[0], want)


@pytest.mark.parametrize("F", [100, 128])
def test_split_emulation_stays_inside_the_gate(F):
    """Every float case of the default table at one tile: |emulation - want_exact| <= 2e-6 * scale elementwise."""
    worst = 0.0
    for c in sc.default_table(F):
        if c.kind == "int":
            continue
        args = _case_inputs(c)
        got = sc.emulate_split(*args)
        want, scale = sc.want_exact(*args)
        r = _ratio(got, want, scale)
        worst = max(worst, r)
        assert _within(got, want, scale), (c, r)
        assert np.array_equal(got, got.T)
    print("three-way emulation, F = %d: worst |got - want| / scale = %.2e" % (F, worst))


def test_once_emulation_stays_inside_the_gate():
    worst = 0.0
    for c in sc.once_table(128):
        if c.kind == "int":
            continue
        args = _case_inputs(c)
        got = sc.emulate_once(*args)
        want, scale = sc.want_once(*args)
        r = _ratio(got, want, scale)
        worst = max(worst, r)
        assert _within(got, want, scale), (c, r)
        if c.kact >= 16:                                                           # and it is the bf16 arithmetic
            we, se = sc.want_exact(*args)
            assert (np.abs(got - we) > 1e-4 * se).any(), c
    print("bf16-once emulation, F = 128: worst |got - want_once| / scale = %.2e" % worst)


@pytest.mark.parametrize("kact", [1, 16, 17])
@pytest.mark.parametrize("term", [0, 1, 2])
def test_gate_sees_a_missing_split_term(kact, term):
    """One of the three 2^-16 terms (h*l, l*h, m*m) left out breaks the gate at the small counts, where no sum of many
    terms hides it."""
    c = sc.Case(128, 17, kact, "normal", *sc.FLOAT_AB)
    args = _case_inputs(c)
    want, scale = sc.want_exact(*args)
    assert _within(sc.emulate_split(*args), want, scale)
    bad = sc.emulate_split(*args, drop_term=term)
    print("rows %d, term %d left out: ratio %.2e" % (kact, term, _ratio(bad, want, scale)))
    assert not _within(bad, want, scale)


@pytest.mark.parametrize("kact,B", [(49, 40), (64, 32), (400, 230)])
def test_once_gate_sees_a_missing_row(kact, B):
    """A row of the batch missing from the bf16-once product breaks its gate and the integer equality."""
    for kind in ("normal", "int"):
        c = sc.Case(128, B, kact, kind, 1.0, 0.0)
        args = _case_inputs(c)
        bad = sc.emulate_once(*args, drop_row=kact - 1)
        if kind == "int":
            want = sc.want_int(sc.gram_exact(*args[:5])[0], c.alpha, c.beta, args[7])
            assert sc.emulate_once(*args).tobytes() == want.tobytes() and bad.tobytes() != want.tobytes()
        else:
            want, scale = sc.want_once(*args)
            assert _within(sc.emulate_once(*args), want, scale) and not _within(bad, want, scale)
