"""The detector's surface (dlco_desc_detect*, DescContext.detect*, the tool detect) on a machine without a GPU: the C ABI is
declared, exported and bound with the stated signatures, argument checks that need no device, and the tool's usage rules."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
FUNCS = ["dlco_desc_detect", "dlco_desc_detect_device", "dlco_desc_detect_stage_ms"]
METHODS = ["detect", "detect_device", "detect_stage_ms"]


def test_detect_functions_are_declared_exported_and_bound(dlco):
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
    vp, i64, i64p, f32p = C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_float)
    assert L.dlco_desc_detect.argtypes == [vp, C.c_int32, i64, i64, f32p, i64p, i64p, i64p]
    assert L.dlco_desc_detect_device.argtypes == [vp, C.c_int32, i64, i64, vp, vp, i64p, i64p]
    # the header states the same parameter lists
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    for name, dev in (("dlco_desc_detect", "host"), ("dlco_desc_detect_device", "dev")):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", text)
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert params == ["dlco_desc_ctx *ctx", "int32_t n_octaves", "int64_t threshold", "int64_t max_keypoints", "float *keypoints_" + dev,
                          "int64_t *response_" + dev, "int64_t *n_out", "int64_t *n_found"], params


def test_detect_rejects_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    kp, resp = np.zeros((4, 4), np.float32), np.zeros(4, np.int64)
    n, found = C.c_int64(-5), C.c_int64(-5)
    Kp, Rp, dev = kp.ctypes.data_as(f32p), resp.ctypes.data_as(i64p), C.c_void_p(kp.ctypes.data)
    E = dlco.ERR_INVALID
    # a null handle: invalid before anything touches a device
    assert L.dlco_desc_detect(None, 3, 1, 4, Kp, Rp, C.byref(n), C.byref(found)) == E
    assert L.dlco_desc_detect_device(None, 3, 1, 4, dev, dev, C.byref(n), C.byref(found)) == E
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(kp.ctypes.data)
    for detect, K, R in ((L.dlco_desc_detect, Kp, Rp), (L.dlco_desc_detect_device, dev, dev)):
        for n_oct in (0, -1, 5, 100):
            assert detect(h, n_oct, 1, 4, K, R, C.byref(n), C.byref(found)) == E, n_oct
        for thr in (0, -1, -2 ** 40):
            assert detect(h, 3, thr, 4, K, R, C.byref(n), C.byref(found)) == E, thr
        for mx in (0, -1):
            assert detect(h, 3, 1, mx, K, R, C.byref(n), C.byref(found)) == E, mx
        assert detect(h, 3, 1, 4, None, R, C.byref(n), C.byref(found)) == E
        assert detect(h, 3, 1, 4, K, R, None, C.byref(found)) == E
    assert L.dlco_desc_detect_device(h, 3, 1, 4, C.c_void_p(kp.ctypes.data + 4), dev, C.byref(n), C.byref(found)) == E     # 16-byte rows
    assert (n.value, found.value) == (-5, -5) and not kp.any()
    assert L.dlco_desc_detect_stage_ms(None, (C.c_double * 6)()) == E and L.dlco_desc_detect_stage_ms(h, None) == E


def _tool():
    subprocess.check_call(["make", "-s", "-C", CLI])
    return os.path.join(CLI, "detect")


def test_detect_usage_exits_1():
    tool = _tool()
    full = ["img", "-out", "o"]
    cases = [[], ["img"], ["-out", "o"], ["-help"] + full, full + ["second_positional"], full + ["-bogus"], full[:-1], full + ["-octaves"],
             full + ["-octaves", "0"], full + ["-octaves", "5"], full + ["-threshold", "0"], full + ["-threshold", "-3"], full + ["-max", "0"],
             full + ["-device"]]
    for args in cases:
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, (args, p.returncode, p.stderr)
        assert "Usage: detect src_h5_img_file -out dst_h5_filename" in p.stdout, args
        assert "[-octaves n] [-threshold t] [-max n] [-device n]" in p.stdout
    p = subprocess.run([tool, "img", "-x"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stdout.startswith("ERROR: Invalid -x option.")


def test_detect_missing_or_malformed_input_exits_2(tmp_path):
    """A runtime failure is a message on stderr and exit 2, before any device is opened."""
    tool = _tool()
    p = subprocess.run([tool, str(tmp_path / "no_image"), "-out", str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("detect: ") and "Image.npy" in p.stderr
    img = tmp_path / "image"
    img.mkdir()
    np.save(img / "Image.npy", np.zeros((3, 5, 7), np.uint8))
    p = subprocess.run([tool, str(img), "-out", str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("detect: Image must be")
    assert not (tmp_path / "out").exists()
