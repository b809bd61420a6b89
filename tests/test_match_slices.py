"""CPU tests of the rule that cuts the train table of a match into slices (opencv-dlco_amd/csrc/match_slices.hpp, through
tests/shim/match_slices_shim.cpp) against its Python restatement below, which the GPU tests import to know which regime a
shape puts the kernels in (how many tiles a workgroup walks, whether a merge kernel runs).  Nothing here needs a GPU or
libdlco.so."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KINDS = ("float", "u8")
# (queries per workgroup, train rows per tile, CUs to fill first, workgroups per CU wanted): the numbers of the two kernels
NUMBERS = {"float": (128, 128, 1, 8), "u8": (256, 128, 2, 16)}


def ceil_div(a, b):
    return -(-a // b)


def tiles_per_slice(nq, nt, n_cu, kind):
    """Tiles of train that one workgroup walks: enough slices to give every CU its share of workgroups, then enough for a
    number of rounds as long as a slice keeps four tiles."""
    qb, tile, fill_cu, per_cu = NUMBERS[kind]
    qblocks, tiles = ceil_div(nq, qb), ceil_div(nt, tile)
    fill = min(tiles, ceil_div(fill_cu * n_cu, qblocks))
    rounds = min(tiles // 4, ceil_div(per_cu * n_cu, qblocks))
    return ceil_div(tiles, max(1, fill, rounds))


def slices(nt, tps, kind):
    return ceil_div(ceil_div(nt, NUMBERS[kind][1]), tps)


SWEEP = list(itertools.product((1, 255, 256, 257, 4096, 2 ** 20), (1, 127, 128, 129, 700, 6204, 100000, 2 ** 31 - 1), (1, 32, 64, 256, 304), KINDS))

# every byte-table shape of tests/test_match_u8_gpu.py and tests/test_u8_cli_gpu.py before test_match_u8_tiles_gpu.py existed
OLD_BYTE_SHAPES = [(70, 90), (1, 1), (37, 2), (129, 17), (300, 500), (40, 1), (40, 2), (5, 4000), (257, 1000), (150, 333), (37, 333), (76, 82), (82, 76)]


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "libmatchslicesshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), os.path.join(ROOT, "tests", "shim", "match_slices_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_tiles_per_slice.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int]
    L.shim_slices.argtypes = [C.c_int64, C.c_int, C.c_int]
    return L


def test_the_restatement_uses_the_kernels_numbers(rules):
    for k, kind in enumerate(KINDS):
        assert (rules.shim_query_block(k), rules.shim_tile(k)) == NUMBERS[kind][:2]


def test_the_header_equals_the_restatement_over_the_sweep(rules):
    for nq, nt, n_cu, kind in SWEEP:
        k = KINDS.index(kind)
        tps = rules.shim_tiles_per_slice(nq, nt, n_cu, k)
        assert tps == tiles_per_slice(nq, nt, n_cu, kind), (nq, nt, n_cu, kind)
        assert rules.shim_slices(nt, tps, k) == slices(nt, tps, kind), (nq, nt, n_cu, kind)


def test_no_slice_is_empty_and_every_tile_is_covered(rules):
    """What the kernels' loaders rely on: the first row of every slice is a row of the table."""
    for nq, nt, n_cu, kind in SWEEP:
        k = KINDS.index(kind)
        tile = NUMBERS[kind][1]
        tiles = ceil_div(nt, tile)
        tps = rules.shim_tiles_per_slice(nq, nt, n_cu, k)
        s = rules.shim_slices(nt, tps, k)
        case = (nq, nt, n_cu, kind, tps, s)
        assert tps >= 1 and s >= 1, case
        assert s * tps >= tiles, case
        assert (s - 1) * tps < tiles, case                    # no empty slice
        jbeg = (s - 1) * tps * tile
        assert jbeg < nt and jbeg < 2 ** 31, case             # the kernels keep it in an int


def test_the_cases_the_documents_quote(rules):
    tps = rules.shim_tiles_per_slice(100000, 100000, 256, 1)
    assert (tps, rules.shim_slices(100000, tps, 1)) == (72, 11)
    assert (tiles_per_slice(100000, 100000, 256, "u8"), slices(100000, 72, "u8")) == (72, 11)
    tps = rules.shim_tiles_per_slice(100000, 100000, 256, 0)
    assert rules.shim_slices(100000, tps, 0) == 3             # "three slices": the comment of the rule
    assert slices(100000, tiles_per_slice(100000, 100000, 256, "float"), "float") == 3
    # the float suite does walk several tiles per slice
    assert tiles_per_slice(3000, 5000, 256, "float") == 4 and slices(5000, 4, "float") == 10


def test_the_small_byte_shapes_walk_one_tile_per_slice(rules):
    """Why tests/test_match_u8_tiles_gpu.py exists: at 256 CUs none of the small byte-table shapes lets a workgroup walk
    more than one tile.  If this fails the rule has changed: pick the shapes of that file again."""
    for nq, nt in OLD_BYTE_SHAPES:
        assert rules.shim_tiles_per_slice(nq, nt, 256, 1) == 1, (nq, nt)
    # and the shapes chosen there do, for the CU counts of the family
    for n_cu in (64, 128, 256, 304):
        assert tiles_per_slice(4096, 6204, n_cu, "u8") >= 2 and tiles_per_slice(16384, 8252, n_cu, "u8") >= 2, n_cu
    assert (tiles_per_slice(4096, 6204, 256, "u8"), slices(6204, 2, "u8")) == (2, 25)
    assert (tiles_per_slice(16384, 8252, 256, "u8"), slices(8252, 5, "u8")) == (5, 13)
    for n_cu in (1, 32, 64, 128, 256, 304):
        assert (tiles_per_slice(2 ** 20, 700, n_cu, "u8"), slices(700, 6, "u8")) == (6, 1), n_cu      # one slice holds all six tiles
        assert n_cu < 32 or tiles_per_slice(77, 700, n_cu, "u8") == 1, n_cu                          # the rest of 2^20 + 77 queries
