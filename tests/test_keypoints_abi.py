"""The keypoint surface (dlco_desc_set_image* / extract_patches / describe_keypoints*, the tool describe-image) on a machine
without a GPU: the C ABI is declared, exported and bound, argument checks that need no device, and the tool's usage rules."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "opencv-dlco_amd", "cli")
FUNCS = ["dlco_desc_set_image", "dlco_desc_set_image_device", "dlco_desc_extract_patches", "dlco_desc_describe_keypoints",
         "dlco_desc_describe_keypoints_device"]
METHODS = ["set_image", "set_image_device", "extract_patches", "describe_keypoints", "describe_keypoints_device"]


def test_keypoint_functions_are_declared_exported_and_bound(dlco):
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


def test_keypoint_calls_reject_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    img = np.zeros((4, 8), np.uint8)
    kp = np.array([[2, 2, 64, 0]], np.float32)
    patches, status, out = np.zeros((1, 64, 64), np.uint8), np.zeros(1, np.uint8), np.zeros(8, np.float32)
    Ip, Kp, Pp, Sp, Op = (img.ctypes.data_as(u8p), kp.ctypes.data_as(f32p), patches.ctypes.data_as(u8p), status.ctypes.data_as(u8p),
                          out.ctypes.data_as(f32p))
    dev = C.c_void_p(out.ctypes.data)
    E = dlco.ERR_INVALID
    # a null handle: invalid before anything touches a device
    assert L.dlco_desc_set_image(None, Ip, 8, 4, 8) == E
    assert L.dlco_desc_set_image_device(None, dev, 8, 4, 8) == E
    assert L.dlco_desc_extract_patches(None, Kp, 1, 1.0, 1, Pp, Sp) == E
    assert L.dlco_desc_describe_keypoints(None, Kp, 1, 1.0, 1, Op, Sp) == E
    assert L.dlco_desc_describe_keypoints_device(None, Kp, 1, 1.0, 1, dev, 8, Sp) == E
    # null data and the limits are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(out.ctypes.data)
    for set_image, ptr in ((L.dlco_desc_set_image, Ip), (L.dlco_desc_set_image_device, dev)):
        assert set_image(h, None, 8, 4, 8) == E
        for w, hgt, pitch in ((0, 4, 8), (8, 0, 8), (-1, 4, 8), (32769, 4, 32769), (8, 32769, 8), (8, 4, 7)):
            assert set_image(h, ptr, w, hgt, pitch) == E, (w, hgt, pitch)
    nan, inf = float("nan"), float("inf")
    assert L.dlco_desc_extract_patches(h, None, 1, 1.0, 1, Pp, Sp) == E
    assert L.dlco_desc_extract_patches(h, Kp, 1, 1.0, 1, None, Sp) == E
    assert L.dlco_desc_describe_keypoints(h, None, 1, 1.0, 1, Op, Sp) == E
    assert L.dlco_desc_describe_keypoints(h, Kp, 1, 1.0, 1, None, Sp) == E
    assert L.dlco_desc_describe_keypoints_device(h, None, 1, 1.0, 1, dev, 8, Sp) == E
    assert L.dlco_desc_describe_keypoints_device(h, Kp, 1, 1.0, 1, None, 8, Sp) == E
    for n, sf in ((0, 1.0), (-3, 1.0), (1, 0.0), (1, -1.0), (1, nan), (1, inf)):
        assert L.dlco_desc_extract_patches(h, Kp, n, sf, 1, Pp, Sp) == E, (n, sf)
        assert L.dlco_desc_describe_keypoints(h, Kp, n, sf, 1, Op, Sp) == E, (n, sf)
        assert L.dlco_desc_describe_keypoints_device(h, Kp, n, sf, 1, dev, 8, Sp) == E, (n, sf)


def _tool():
    subprocess.check_call(["make", "-s", "-C", CLI])
    return os.path.join(CLI, "describe-image")


def test_describe_image_usage_exits_1():
    tool = _tool()
    full = ["flt", "img", "-prj", "p", "-id", "0", "-pj", "m", "-out", "o"]
    cases = [[], ["only_one"], ["flt", "img"], ["flt", "img", "-prj", "p"], ["-help"] + full, full + ["third_positional"], full + ["-bogus"],
             full[:-2], full + ["-scale"], full + ["-scale", "0"], full + ["-scale", "-2"], full + ["-scale", "nan"]]
    for args in cases:
        p = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, (args, p.returncode, p.stderr)
        assert "Usage: describe-image src_h5_filter_file src_h5_img_file" in p.stdout, args
        assert "[-scale f] [-upright] [-patches] [-device n]" in p.stdout
    p = subprocess.run([tool, "flt", "img", "-x"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stdout.startswith("ERROR: Invalid -x option.")


def test_describe_image_missing_or_malformed_input_exits_2(tmp_path):
    """A runtime failure is a message on stderr and exit 2, before any device is opened."""
    tool = _tool()
    args = ["-prj", str(tmp_path / "no_prj"), "-id", "0", "-pj", str(tmp_path / "no_pj"), "-out", str(tmp_path / "out"), "-patches", "-upright"]
    p = subprocess.run([tool, str(tmp_path / "no_filters"), str(tmp_path / "no_image")] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("describe-image: ")
    # filters that load, then an image file without keypoints, then keypoints of the wrong shape
    flt, img = tmp_path / "filters", tmp_path / "image"
    flt.mkdir()
    img.mkdir()
    np.save(flt / "PRFilters.npy", np.zeros((8, 64, 64), np.float32))
    p = subprocess.run([tool, str(flt), str(img)] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("describe-image: ") and "Image.npy" in p.stderr
    np.save(img / "Image.npy", np.zeros((5, 7), np.uint8))
    p = subprocess.run([tool, str(flt), str(img)] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "Keypoints.npy" in p.stderr
    np.save(img / "Keypoints.npy", np.zeros((3, 3), np.float32))
    p = subprocess.run([tool, str(flt), str(img)] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stderr.startswith("describe-image: Keypoints must be")
    assert not (tmp_path / "out").exists()
