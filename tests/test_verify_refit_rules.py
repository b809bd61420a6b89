"""The pieces of the refit round that the rule headers share between the host and the refit kernel, on the CPU: the constants
the GPU tests build on, the rule that gives every lane of the kernel its sum, and the kernel's walk over chunks and lanes
restated in C++ (tests/shim/verify_refit_asan_main.cpp) under the address and undefined-behaviour sanitizers, where it must
give the host's refit_round in every bit.  No libdlco.so, no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim")


def build_shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim") / "librefitshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), os.path.join(SHIM, "verify_refit_shim.cpp")])
    L = C.CDLL(str(out))
    L.shim_refit_terms.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.shim_refit_terms.restype = None
    return L


@pytest.fixture(scope="module")
def refit(tmp_path_factory):
    return build_shim(tmp_path_factory)


def terms(L, fundamental, l):
    t = np.zeros(4, np.int32)
    L.shim_refit_terms(fundamental, l, t.ctypes.data_as(C.POINTER(C.c_int)))
    return t.tolist()


def test_the_chunk_is_a_whole_number_of_waves_with_a_lane_for_every_sum(refit):
    c = refit.shim_refit_chunk()
    assert c % 64 == 0 and c >= refit.shim_refit_sums(1) == 81 and refit.shim_refit_sums(0) == 72
    assert refit.shim_refit_row(0) == 18 and refit.shim_refit_row(1) == 9


def test_every_sum_of_the_normal_equations_has_one_lane(refit):
    # the homography: a row is a1 [8], a2 [8], u, v; N[p][q] = a1[p] a1[q] + a2[p] a2[q], r[p] = a1[p] u + a2[p] v
    got = [terms(refit, 0, l) for l in range(refit.shim_refit_chunk())]
    assert got[:64] == [[p, q, 8 + p, 8 + q] for p in range(8) for q in range(8)]
    assert got[64:72] == [[p, 16, 8 + p, 17] for p in range(8)]
    assert all(t == [0, 0, 0, 0] for t in got[72:])
    # the fundamental matrix: a row is a [9]; N[p][q] = a[p] a[q]
    got = [terms(refit, 1, l) for l in range(refit.shim_refit_chunk())]
    assert [t[:2] for t in got[:81]] == [[p, q] for p in range(9) for q in range(9)]
    assert all(t == [0, 0, 0, 0] for t in got[81:])


def test_the_kernels_walk_under_address_and_undefined_sanitizers(tmp_path):
    exe = tmp_path / "verify_refit_asan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(SHIM, "verify_refit_asan_main.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "verify_refit_asan: ok" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
