"""eig_rules::gram_slicing: the K slices of the tracker's Gram products, shared by the GEMM form (gram_rect) and by the
product reduction that emits the partials itself (reduce_gram_kernel).  No GPU.

The count must be what gram_rect computed before the rule moved (its expression is transcribed below, together with
what gemm_f32 makes of a requested split), and for every F that is whole 128-column tiles every slice must lie inside
one 128-column slab: the fused form hands a slab to one workgroup."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libgramslicing.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(ROOT, "tests", "shim", "gram_slicing_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_gram_slicing.argtypes = [C.c_long, C.c_long, C.c_long, C.POINTER(C.c_int)]
    L.shim_gram_slicing.restype = None

    def f(F, tiles, slab_cap):
        o = (C.c_int * 4)()
        L.shim_gram_slicing(F, tiles, slab_cap, o)
        return dict(split_k=o[0], chunk=o[1], slices=o[2], whole=bool(o[3]))
    return f


def old_split_k(F, tiles, slab_cap):
    """gram_rect before: kslice = max(64, F / 64 / 64 * 64); split_k_slices(tiles, 512, F, kslice, slab_cap)."""
    kslice = max(64, F // 64 // 64 * 64)
    return max(1, min((512 + tiles - 1) // tiles, F // kslice, slab_cap))


def gemm_slices(K, split_k):
    """gemm_f32: the K range per slice is whole 16-column tiles; the slice count follows from it."""
    chunk = (K + split_k - 1) // split_k
    chunk = max(16, (chunk + 15) // 16 * 16)
    return chunk, (K + chunk - 1) // chunk


def slab_cap(F, cap_rows, rows):
    """EigTracker: slab floats / output floats."""
    floats = max(min(max(4 * cap_rows * F, 8 << 20), 64 << 20), cap_rows * F)
    return floats // (rows * rows)


@pytest.mark.parametrize("rows", [32, 96])
def test_every_tile_multiple_up_to_8192(rule, rows):
    for F in range(128, 8192 + 1, 128):
        cap = slab_cap(F, 160, rows)
        got = rule(F, 1, cap)
        want = old_split_k(F, 1, cap)
        chunk, slices = gemm_slices(F, want)
        assert got["split_k"] == want and (got["chunk"], got["slices"]) == (chunk, slices), (F, got)
        # whole slices inside 128-column slabs: every slice [z * chunk, (z + 1) * chunk) has both ends in one slab
        assert got["whole"], (F, got)
        assert got["chunk"] in (64, 128) and got["chunk"] * got["slices"] == F
        for z in range(got["slices"]):
            assert (z * got["chunk"]) // 128 == ((z + 1) * got["chunk"] - 1) // 128
    assert rule(8192, 1, 10**9) == dict(split_k=64, chunk=128, slices=64, whole=True)
    assert rule(640, 1, 10**9) == dict(split_k=10, chunk=64, slices=10, whole=True)
    assert rule(256, 1, 10**9) == dict(split_k=4, chunk=64, slices=4, whole=True)


def test_shapes_the_fused_form_must_refuse(rule):
    # a slab that holds fewer slices than the rule wants: longer slices, no longer whole inside a slab
    g = rule(8192, 1, 10)
    assert g["split_k"] == 10 == old_split_k(8192, 1, 10) and not g["whole"]
    assert (g["chunk"], g["slices"]) == gemm_slices(8192, 10)
    # a width that is not whole tiles, and the projection against a tall block (several output tiles)
    for F, tiles in ((544, 1), (200, 1), (8192, 4), (8192, 1024)):
        g = rule(F, tiles, 10**9)
        want = old_split_k(F, tiles, 10**9)
        assert g["split_k"] == want and (g["chunk"], g["slices"]) == gemm_slices(F, want)
        assert g["whole"] == (F % 128 == 0 and g["chunk"] in (64, 128) and g["chunk"] * g["slices"] == F)
    assert not rule(544, 1, 10**9)["whole"] and not rule(8192, 1024, 10**9)["whole"]
