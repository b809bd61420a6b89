"""The pr-learn grid (dlco_pr_grid_*, pr-learn-grid) on a machine without a GPU: the C ABI is declared and exported,
argument checks that need no device, and the command line's usage / file-name rules."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
GRID_FUNCS = ["dlco_pr_grid_create", "dlco_pr_grid_destroy", "dlco_pr_grid_last_error", "dlco_pr_grid_steps", "dlco_pr_grid_get_state",
              "dlco_pr_grid_validate", "dlco_pr_grid_stats", "dlco_pr_grid_set_group", "dlco_pr_grid_group"]


def test_grid_functions_are_declared_and_exported(dlco):
    header = open(dlco.HEADER_PATH).read()
    assert re.search(r"typedef struct dlco_pr_grid dlco_pr_grid;", header)
    declared = set(dlco.exported_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", dlco.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    for f in GRID_FUNCS:
        assert f in declared, f + " is not declared in include/dlco.h"
        assert f in exported, f + " is not exported by libdlco.so"
    L = dlco.load()
    for f in GRID_FUNCS:
        assert getattr(L, f).argtypes is not None, f + " has no ctypes signature"
    assert hasattr(dlco, "PrGrid")


def test_grid_rejects_invalid_arguments_without_a_device(dlco):
    L = dlco.load()
    h = C.c_void_p()
    mu = np.array([0.025, 0.03], np.float32)
    ga = np.array([0.10, 0.25], np.float32)
    f32p = C.POINTER(C.c_float)
    # no source context / no grid: invalid before anything touches a device
    assert L.dlco_pr_grid_create(C.byref(h), None, 2, mu.ctypes.data_as(f32p), ga.ctypes.data_as(f32p), 2215) == dlco.ERR_INVALID
    assert not h.value
    assert L.dlco_pr_grid_create(None, None, 2, mu.ctypes.data_as(f32p), ga.ctypes.data_as(f32p), 2215) == dlco.ERR_INVALID
    assert L.dlco_pr_grid_steps(None, 10) == dlco.ERR_INVALID
    assert L.dlco_pr_grid_get_state(None, None, None, None) == dlco.ERR_INVALID
    assert L.dlco_pr_grid_validate(None, None, None, None) == dlco.ERR_INVALID
    assert L.dlco_pr_grid_set_group(None, 1) == dlco.ERR_INVALID
    L.dlco_pr_grid_destroy(None)


def _grid_tool():
    subprocess.check_call(["make", "-s", "-C", CLI])
    return os.path.join(CLI, "pr-learn-grid")


def test_pr_learn_grid_usage_exits_1():
    tool = _grid_tool()
    for args in ([], ["only_one"], ["a", "b"], ["a", "b", "c", "-bogus"], ["a", "b", "c", "-mus", "0.1,,0.2"], ["a", "b", "c", "-gammas", "x"],
                 ["a", "b", "c", "-logstep", "0"], ["-help", "a", "b", "c"]):
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, (args, p.returncode)
        assert "Usage: pr-learn-grid  src_h5_filter_file" in p.stdout, args
    p = subprocess.run([tool, "a", "b", "c", "-bogus"], capture_output=True, text=True, timeout=60)
    assert p.stdout.startswith("ERROR: Invalid -bogus option.")


def test_pr_learn_grid_file_name_collision_exits_1(tmp_path):
    """0.0251 and 0.0249 both print as 0.025: two settings would share one log; refused before any file is read."""
    tool = _grid_tool()
    p = subprocess.run([tool, "missing_filters", "missing_dists", str(tmp_path / "out"), "-mus", "0.0251,0.0249", "-gammas", "0.1"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "Usage: pr-learn-grid" in p.stdout
    assert "missing_dists-0.025-0.100-pr.log" in p.stdout
    assert not (tmp_path / "out").exists()
