"""The epipolar guided-matching surface (dlco_desc_match_guided_epipolar, dlco_desc_match_guided_epipolar_device,
dlco_desc_cross_sqdists_guided_epipolar, the DescContext methods, the -model option of the tool match) on a machine without a
GPU: the C ABI is declared, exported and bound with the stated signatures, the argument checks that need no device, and the
paths of the tool that open none."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from test_guided_abi import USAGE as OLD_USAGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
FUNCS = ["dlco_desc_match_guided_epipolar", "dlco_desc_match_guided_epipolar_device", "dlco_desc_cross_sqdists_guided_epipolar"]
METHODS = ["match_guided_epipolar", "match_guided_epipolar_device", "cross_sqdists_guided_epipolar"]
USAGE = OLD_USAGE + " [-model homography|fundamental]"
f32p, f64p, i32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int32))


def test_epipolar_functions_are_declared_exported_and_bound(dlco):
    declared = set(dlco.exported_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", dlco.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    L = dlco.load()
    for f in FUNCS:
        assert f in declared, f + " is not declared in include/dlco.h"
        assert f in exported, f + " is not exported by libdlco.so"
        assert getattr(L, f).argtypes is not None, f + " has no ctypes signature"
    for m in METHODS:
        assert callable(getattr(dlco.DescContext, m, None)), "DescContext." + m
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    assert L.dlco_desc_match_guided_epipolar.argtypes == [vp, f32p, f32p, i64, f32p, f32p, i64, i32, f64p, f32, i32, i32p, f32p]
    assert L.dlco_desc_match_guided_epipolar_device.argtypes == [vp, vp, i64, vp, i64, i64, vp, i64, vp, i64, i64, i32, f64p, f32, i32, vp, vp]
    assert L.dlco_desc_cross_sqdists_guided_epipolar.argtypes == [vp, f32p, f32p, i64, f32p, f32p, i64, i32, f64p, f32, i32, f32p]
    # the header states the same parameter lists
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    assert params("dlco_desc_match_guided_epipolar") == ["dlco_desc_ctx *ctx", "const float *query_host", "const float *query_xy_host", "int64_t nq",
                                                         "const float *train_host", "const float *train_xy_host", "int64_t nt", "int32_t r",
                                                         "const double *F", "float threshold", "int32_t f_side", "int32_t *idx_host", "float *sqdist_host"]
    assert params("dlco_desc_match_guided_epipolar_device") == ["dlco_desc_ctx *ctx", "const float *query_dev", "int64_t ldq", "const float *query_xy_dev",
                                                                "int64_t ldxy_q", "int64_t nq", "const float *train_dev", "int64_t ldt",
                                                                "const float *train_xy_dev", "int64_t ldxy_t", "int64_t nt", "int32_t r", "const double *F",
                                                                "float threshold", "int32_t f_side", "int32_t *idx_dev", "float *sqdist_dev"]
    assert params("dlco_desc_cross_sqdists_guided_epipolar") == ["dlco_desc_ctx *ctx", "const float *query_host", "const float *query_xy_host", "int64_t nq",
                                                                 "const float *train_host", "const float *train_xy_host", "int64_t nt", "int32_t r",
                                                                 "const double *F", "float threshold", "int32_t f_side", "float *out_host"]
    for name in ("match_guided_epipolar", "cross_sqdists_guided_epipolar"):
        sig = inspect.signature(getattr(dlco.DescContext, name))
        assert [(p.name, p.default) for p in list(sig.parameters.values())[6:]] == [("threshold", 3.0), ("f_side", 0)]
        assert [p.name for p in list(sig.parameters.values())[1:6]] == ["query", "query_xy", "train", "train_xy", "F"]
    dev = inspect.signature(dlco.DescContext.match_guided_epipolar_device)
    ref = inspect.signature(dlco.DescContext.match_guided_device)
    rename = {"H": "F", "radius": "threshold", "h_side": "f_side"}
    assert [p.name for p in dev.parameters.values()] == [rename.get(p.name, p.name) for p in ref.parameters.values()]
    assert {p.name: p.default for p in dev.parameters.values() if p.default is not inspect.Parameter.empty} == dict(
        threshold=3.0, f_side=0, ldq=None, ldt=None, ldxy_q=2, ldxy_t=2)
    # the header names the rule's file and says that the predicate is in scope now
    raw = " ".join(open(dlco.HEADER_PATH).read().replace(" * ", " ").split())
    for words in ("csrc/guided_epipolar_rules.hpp states the rule", "In scope since: an epipolar predicate for guided matching",
                  "In scope since: a fundamental-matrix predicate", "admits nothing", "at an epipole of F"):
        assert words in raw, words


def test_epipolar_calls_reject_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    E = dlco.ERR_INVALID
    Q, T = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32)
    qxy, txy, F = np.zeros((3, 4), np.float32), np.zeros((5, 4), np.float32), np.eye(3).reshape(9).copy()
    idx, d, X = np.full((3, 2), -5, np.int32), np.full((3, 2), -5, np.float32), np.full((3, 5), -5, np.float32)
    p = lambda a, t: a.ctypes.data_as(t)
    good = dict(q=p(Q, f32p), qxy=p(qxy, f32p), nq=3, t=p(T, f32p), txy=p(txy, f32p), nt=5, r=8, F=p(F, f64p), threshold=3.0, f_side=0, idx=p(idx, i32p),
                d=p(d, f32p), X=p(X, f32p))
    host = lambda h, **kw: L.dlco_desc_match_guided_epipolar(h, *[{**good, **kw}[k] for k in ("q", "qxy", "nq", "t", "txy", "nt", "r", "F", "threshold", "f_side",
                                                                                               "idx", "d")])
    cross = lambda h, **kw: L.dlco_desc_cross_sqdists_guided_epipolar(h, *[{**good, **kw}[k] for k in ("q", "qxy", "nq", "t", "txy", "nt", "r", "F", "threshold",
                                                                                                        "f_side", "X")])
    vq, vt, vqx, vtx, vi, vd = (C.c_void_p(a.ctypes.data) for a in (Q, T, qxy, txy, idx, d))
    dgood = dict(q=vq, ldq=8, qxy=vqx, ldxq=4, nq=3, t=vt, ldt=8, txy=vtx, ldxt=4, nt=5, r=8, F=p(F, f64p), threshold=3.0, f_side=0, idx=vi, d=vd)
    device = lambda h, **kw: L.dlco_desc_match_guided_epipolar_device(h, *[{**dgood, **kw}[k] for k in ("q", "ldq", "qxy", "ldxq", "nq", "t", "ldt", "txy", "ldxt",
                                                                                                         "nt", "r", "F", "threshold", "f_side", "idx", "d")])
    assert host(None) == E and cross(None) == E and device(None) == E       # a null handle: invalid before anything touches a device
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(Q.ctypes.data)
    F_nan, F_inf = F.copy(), F.copy()
    F_nan[4], F_inf[8] = np.nan, -np.inf
    common = [dict(q=None), dict(t=None), dict(qxy=None), dict(txy=None), dict(F=None), dict(F=p(F_nan, f64p)), dict(F=p(F_inf, f64p)), dict(threshold=0.0),
              dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(f_side=2), dict(f_side=-1), dict(nq=0), dict(nt=0),
              dict(nt=2 ** 31), dict(r=0), dict(r=1025)]
    for kw in common:
        assert host(h, **kw) == E, kw
        assert cross(h, **kw) == E, kw
        assert device(h, **kw) == E, kw
    for kw in (dict(idx=None), dict(d=None)):
        assert host(h, **kw) == E and device(h, **kw) == E, kw
    assert cross(h, X=None) == E and cross(h, nq=2 ** 20, nt=2 ** 20) == E                                # the matrix's own limit
    for kw in (dict(ldxq=1), dict(ldxt=1), dict(ldxq=0), dict(ldxt=-4), dict(ldq=9), dict(ldt=10), dict(ldq=4), dict(ldt=4),
               dict(qxy=C.c_void_p(qxy.ctypes.data + 2)), dict(q=C.c_void_p(Q.ctypes.data + 4))):
        assert device(h, **kw) == E, kw
    assert (idx == -5).all() and (d == -5).all() and (X == -5).all()
    assert not Q.any() and not T.any() and not qxy.any() and not txy.any()


def _tool():
    subprocess.check_call(["make", "-s", "-C", CLI])
    return os.path.join(CLI, "match")


def test_model_usage_errors_exit_1():
    tool = _tool()
    full = ["q", "t", "-out", "o"]
    for args, word in ((["-model", "fundamental"], "-model needs -guided"), (["-model", "homography"], "-model needs -guided"),
                       (["-guided", "v", "-kp", "a", "b", "-model", "x"], "-model must be homography or fundamental"),
                       (["-guided", "v", "-kp", "a", "b", "-model"], "Invalid -model option")):
        p = subprocess.run([tool] + full + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and USAGE in p.stdout and "ERROR" in p.stdout and word in p.stdout, (args, p.stdout)
    p = subprocess.run([tool, "-help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and USAGE in p.stdout and OLD_USAGE in p.stdout and "ERROR" not in p.stdout


def write_inputs(d, best, bits_name):
    for name, n in (("q", 4), ("t", 6)):
        (d / name).mkdir()
        np.save(d / name / "Descriptor.npy", np.ones((n, 8), np.float32))
        (d / (name + "kp")).mkdir()
        np.save(d / (name + "kp") / "Keypoints.npy", np.arange(4 * n, dtype=np.float32).reshape(n, 4))
    (d / "v").mkdir()
    np.save(d / "v" / "BestHypothesis.npy", np.array([best], np.int32))
    np.save(d / "v" / (bits_name + ".npy"), np.eye(3).reshape(9).view(np.int64))
    return [str(d / "q"), str(d / "t"), "-out", str(d / "out"), "-guided", str(d / "v"), "-kp", str(d / "qkp"), str(d / "tkp"), "-device", "99",
            "-model", "fundamental"]


def test_model_fundamental_fails_before_a_device_is_opened(tmp_path):
    """a verify output of the other model (no FundamentalBits) and one without a model: exit 2 with a message, nothing written,
    and no device touched (-device 99 is one that no machine has: reaching it would be another message)"""
    tool = _tool()
    for k, (best, bits_name, word) in enumerate(((0, "HomographyBits", "FundamentalBits"), (-1, "FundamentalBits", "found no model (BestHypothesis = -1)"))):
        d = tmp_path / ("case%d" % k)
        d.mkdir()
        p = subprocess.run([tool] + write_inputs(d, best, bits_name), capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.startswith("match: ") and word in p.stderr and not (d / "out").exists(), p.stderr
    # with a model and its bits the tool gets as far as the device, which does not exist
    d = tmp_path / "reaches"
    d.mkdir()
    p = subprocess.run([tool] + write_inputs(d, 0, "FundamentalBits"), capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "Guided: fundamental, radius 6" in p.stdout and "FundamentalBits" not in p.stderr and not (d / "out").exists()
