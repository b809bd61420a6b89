"""The orientation surface (dlco_desc_orient, dlco_desc_detect_oriented, dlco_desc_last_orient_ms, DescContext.orient /
detect_oriented / last_orient_ms, detect -orient) on a machine without a GPU: the C ABI is declared, exported and bound with
the stated signatures, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
FUNCS = ["dlco_desc_orient", "dlco_desc_detect_oriented", "dlco_desc_last_orient_ms"]
METHODS = ["orient", "detect_oriented", "last_orient_ms"]


def test_orient_functions_are_declared_exported_and_bound(dlco):
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
    vp, i64, i64p, f32p, u8p = C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    assert L.dlco_desc_orient.argtypes == [vp, f32p, i64, f32p, i64p, u8p]
    assert L.dlco_desc_detect_oriented.argtypes == L.dlco_desc_detect.argtypes == [vp, C.c_int32, i64, i64, f32p, i64p, i64p, i64p]
    assert L.dlco_desc_last_orient_ms.restype == C.c_double
    # the header states the same parameter lists
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    assert params("dlco_desc_orient") == ["dlco_desc_ctx *ctx", "const float *keypoints_host", "int64_t n", "float *angles_host",
                                          "int64_t *vectors_host", "uint8_t *status_host"]
    assert params("dlco_desc_detect_oriented") == params("dlco_desc_detect")
    assert params("dlco_desc_last_orient_ms") == ["const dlco_desc_ctx *ctx"]


def test_orient_rejects_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    f32p, i64p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    kp, ang, vec, st = np.zeros((4, 4), np.float32), np.full(4, -5, np.float32), np.full((4, 2), -5, np.int64), np.full(4, 9, np.uint8)
    Kp, A, V, S = kp.ctypes.data_as(f32p), ang.ctypes.data_as(f32p), vec.ctypes.data_as(i64p), st.ctypes.data_as(u8p)
    E = dlco.ERR_INVALID
    assert L.dlco_desc_orient(None, Kp, 4, A, V, S) == E                      # a null handle: invalid before anything touches a device
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(kp.ctypes.data)
    for n in (0, -1, -2 ** 40):
        assert L.dlco_desc_orient(h, Kp, n, A, V, S) == E, n
    assert L.dlco_desc_orient(h, None, 4, A, V, S) == E
    assert L.dlco_desc_orient(h, Kp, 4, None, V, S) == E
    assert (ang == -5).all() and (vec == -5).all() and (st == 9).all()
    assert L.dlco_desc_last_orient_ms(None) == 0.0
    # detect_oriented checks what detect checks
    resp, n, found = np.zeros(4, np.int64), C.c_int64(-5), C.c_int64(-5)
    R = resp.ctypes.data_as(i64p)
    assert L.dlco_desc_detect_oriented(None, 3, 1, 4, Kp, R, C.byref(n), C.byref(found)) == E
    for args in ((0, 1, 4, Kp, R, C.byref(n)), (5, 1, 4, Kp, R, C.byref(n)), (3, 0, 4, Kp, R, C.byref(n)), (3, 1, 0, Kp, R, C.byref(n)),
                 (3, 1, 4, None, R, C.byref(n)), (3, 1, 4, Kp, R, None)):
        assert L.dlco_desc_detect_oriented(h, *args, C.byref(found)) == E, args[:3]
    assert (n.value, found.value) == (-5, -5) and not kp.any()


def test_detect_usage_names_the_orient_flag():
    subprocess.check_call(["make", "-s", "-C", CLI])
    tool = os.path.join(CLI, "detect")
    for args in (["-help"], ["img", "-out", "o", "-orient", "-help"], ["-orient"], ["img", "-orient"]):
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, (args, p.returncode, p.stderr)
        assert "Usage: detect src_h5_img_file -out dst_h5_filename" in p.stdout and "[-orient]" in p.stdout, args
        assert "ERROR" not in p.stdout, args                                 # -orient is an option the tool knows


def test_detect_orient_fails_like_detect_before_a_device_is_opened(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CLI])
    p = subprocess.run([os.path.join(CLI, "detect"), str(tmp_path / "no_image"), "-out", str(tmp_path / "out"), "-orient"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("detect: ") and "Image.npy" in p.stderr
