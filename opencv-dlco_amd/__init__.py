"""ctypes binding of libdlco.so — the MI355X (gfx950) pj-learn hot path.

The package directory name carries a hyphen (it mirrors the upstream project name), so it
is loaded with importlib:  ``dlco = importlib.import_module("opencv-dlco_amd")``.

This module is plumbing only: every computation happens in the HIP kernels of
``libdlco.so`` (sources under ``csrc/``).  There is no CPU fallback — a missing library or
a missing gfx950 device raises.
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdlco.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dlco.h")

OK, ERR_INVALID, ERR_HIP, ERR_NODEVICE, ERR_NOCONV, ERR_COMM = 0, -2, -3, -4, -5, -6
BUF_DIST, BUF_GRAD, BUF_DFAVG, BUF_W, BUF_GATHER, BUF_DATA = 1, 2, 3, 4, 5, 6
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_size_t)
DETECT_THRESHOLD = 100 * 100 * 256 * 256                 # the detector's R of a determinant of 100 (csrc/detect_rules.hpp)


class DlcoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libdlco error %d: %s" % (code, msg))
        self.code = code


class Cfg(C.Structure):
    _fields_ = [
        ("F", C.c_int32), ("N", C.c_int32), ("B", C.c_int32),
        ("mu", C.c_float), ("gamma", C.c_float),
        ("seed", C.c_uint64),
        ("device", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32),
        ("eig_tol", C.c_float), ("eig_guard", C.c_int32), ("eig_max_iter", C.c_int32),
        ("shard", C.c_int32), ("strict_conv", C.c_int32), ("grad_bf16", C.c_int32),
        ("reserved", C.c_int32 * 5),
    ]


class LogEntry(C.Structure):
    _fields_ = [
        ("t", C.c_uint32), ("is_best", C.c_int32), ("saved", C.c_int32),
        ("loss_val", C.c_float), ("regul", C.c_float), ("obj", C.c_float), ("obj_best", C.c_float),
        ("rank", C.c_int32), ("rank_best", C.c_int32), ("dim", C.c_int32),
        ("auc", C.c_double), ("auc_best", C.c_double),
        ("fpr95", C.c_float), ("fpr95_best", C.c_float),
        ("vtime", C.c_double),
        ("nonconv", C.c_int32), ("reserved", C.c_int32),
    ]


class GemmOperand(C.Structure):
    _fields_ = [
        ("host", C.POINTER(C.c_float)), ("rows", C.c_int32), ("ld", C.c_int32), ("kmajor", C.c_int32),
        ("row_ids", C.POINTER(C.c_int32)), ("row_ids2", C.POINTER(C.c_int32)), ("row_scale", C.POINTER(C.c_float)),
    ]


class GemmProbeArgs(C.Structure):
    _fields_ = [
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("A", GemmOperand), ("B", GemmOperand),
        ("B2_host", C.POINTER(C.c_float)),
        ("split_k", C.c_int32), ("k_dev", C.c_int32), ("small_m_tiles", C.c_int32), ("small_n_tiles", C.c_int32),
        ("depth", C.c_int32), ("reps", C.c_int32),
        ("alpha", C.c_float), ("beta", C.c_float), ("b1", C.c_float), ("b2", C.c_float),
        ("E1_host", C.POINTER(C.c_float)), ("E2_host", C.POINTER(C.c_float)),
    ]


class OrthoProbeArgs(C.Structure):
    _fields_ = [
        ("Z_host", C.POINTER(C.c_float)), ("Zprev_host", C.POINTER(C.c_float)), ("Gp_host", C.POINTER(C.c_float)),
        ("m", C.c_int32), ("panel_end", C.c_int32), ("n_lock", C.c_int32), ("unfused", C.c_int32),
        ("alpha", C.c_float), ("b1", C.c_float), ("b2", C.c_float),
    ]


def build(verbose=False):
    """Compile libdlco.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)


_lib = None
f32p, i32p, u8p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
f64p = C.POINTER(C.c_double)
# the matcher's two lines: the tables' element type and pointer, the distances' type and pointer, the suffix of the C names
_Line = collections.namedtuple("_Line", "dtype ptr dist dptr suffix")
_FLOAT, _BYTE = _Line(np.float32, f32p, np.float32, f32p, ""), _Line(np.uint8, u8p, np.int32, i32p, "_u8")
# what DescContext.build_tracks returns: toff [n_tracks + 1] int64, obs [toff[-1]] int32 node ids, track_of [N] int32, label [N]
# int32, counts [3] int64 (csrc/track_rules.hpp), seg [n_img + 1] int64 the nodes' images; images() and rows() split obs
class Tracks(collections.namedtuple("Tracks", "toff obs track_of label counts seg")):
    __slots__ = ()

    @property
    def n_tracks(self):
        return self.toff.size - 1

    def images(self):
        """the image of every observation, [len(obs)] int32"""
        return (np.searchsorted(self.seg, self.obs, side="right") - 1).astype(np.int32)

    def rows(self):
        """the row of every observation inside its image, [len(obs)] int32"""
        return (self.obs - self.seg[self.images()]).astype(np.int32)




def load():
    """dlopen libdlco.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DlcoError(ERR_NODEVICE, "%s is missing: run __graft_entry__.build() (no CPU fallback exists)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.dlco_version.restype = C.c_char_p
    L.dlco_last_error.restype = C.c_char_p
    L.dlco_last_error.argtypes = [vp]
    L.dlco_cfg_default.argtypes = [C.POINTER(Cfg)]
    L.dlco_cfg_default.restype = None
    L.dlco_ctx_create.argtypes = [C.POINTER(vp), C.POINTER(Cfg)]
    L.dlco_ctx_destroy.argtypes = [vp]
    L.dlco_ctx_destroy.restype = None
    L.dlco_device_name.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dlco_set_data.argtypes = [vp, f32p, u8p]
    L.dlco_set_data_device.argtypes = [vp, vp, u8p]
    L.dlco_set_data_shared.argtypes = [vp, vp]
    L.dlco_device_width.argtypes = [vp]
    L.dlco_set_pairs.argtypes = [vp, f32p, C.c_int32, i32p]
    L.dlco_synth_data.argtypes = [vp, f32p, C.c_int32, C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_float]
    L.dlco_get_rows.argtypes = [vp, C.c_int32, C.c_int32, f32p]
    L.dlco_get_index.argtypes = [vp, i32p, i32p, i32p, i32p, i32p, i32p]
    for name in ("dlco_step", "dlco_step_begin", "dlco_step_grad", "dlco_step_finish", "dlco_sync"):
        getattr(L, name).argtypes = [vp]
    L.dlco_steps.argtypes = [vp, C.c_int32]
    L.dlco_dev_buffer.argtypes = [vp, C.c_int32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.dlco_bind_buffer.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    L.dlco_stream.argtypes = [vp, C.POINTER(vp)]
    L.dlco_set_allgather.argtypes = [vp, ALLGATHER_FN, vp]
    L.dlco_comm_unique_id.argtypes = [vp, C.c_size_t, C.c_char_p]
    L.dlco_comm_init.argtypes = [vp, vp, C.c_size_t, C.c_char_p]
    L.dlco_comm_destroy.argtypes = [vp]
    L.dlco_get_batch.argtypes = [vp, i32p, i32p, f32p, f32p, i32p, i32p]
    L.dlco_get_t.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.dlco_get_W.argtypes = [vp, f32p, i32p]
    L.dlco_get_A.argtypes = [vp, f32p]
    L.dlco_get_dfavg.argtypes = [vp, f32p]
    L.dlco_set_state.argtypes = [vp, C.c_uint32, f32p, f32p, C.c_int32]
    L.dlco_validate.argtypes = [vp, f32p, f32p, i32p]
    L.dlco_stats.argtypes = [vp, f32p, C.c_int32, i32p, f32p, C.POINTER(C.c_double)]
    L.dlco_project_sqdist.argtypes = [vp, i32p, C.c_int32, f32p, C.c_int32, f32p]
    L.dlco_viol_counts.argtypes = [vp, f32p, f32p, C.c_int32, i32p, i32p]
    L.dlco_grad_rda.argtypes = [vp, i32p, i32p, i32p, i32p, C.c_int32, C.c_float, C.c_float, f32p, f32p]
    L.dlco_psd_project.argtypes = [vp, f32p, C.c_uint32, f32p, i32p, f32p]
    L.dlco_hinge_sum.argtypes = [vp, f32p, C.c_int32, f32p, C.c_int32, C.POINTER(C.c_double)]
    L.dlco_sym_product.argtypes = [vp, f32p, C.c_int32, f32p, C.c_int32, f32p]
    L.dlco_gemm_probe.argtypes = [vp, C.POINTER(GemmProbeArgs), f32p, f32p, i32p, C.POINTER(C.c_double)]
    L.dlco_chol_probe.argtypes = [vp, f32p, C.c_int32, C.c_int32, C.c_float, f32p, i32p]
    L.dlco_ortho_probe.argtypes = [vp, C.POINTER(OrthoProbeArgs), f32p, f32p, f32p, C.POINTER(C.c_int64)]
    L.dlco_fused_counters.argtypes = [vp, C.POINTER(C.c_int64)]
    L.dlco_roc_stats.argtypes = [vp, f32p, u8p, C.c_int32, f32p, C.POINTER(C.c_double)]
    L.dlco_log_step.argtypes = [vp, C.POINTER(LogEntry)]
    L.dlco_get_saved.argtypes = [vp, f32p, i32p, f32p]
    L.dlco_profile_enable.argtypes = [vp, C.c_int32]
    L.dlco_profile_read.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.dlco_eig_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32p]
    L.dlco_counters.argtypes = [vp, C.POINTER(C.c_int64)]
    i64 = C.c_int64
    L.dlco_set_pairs_device.argtypes = [vp, vp, C.c_int32, i32p]
    L.dlco_desc_last_error.restype = C.c_char_p
    L.dlco_desc_last_error.argtypes = [vp]
    L.dlco_desc_create.argtypes = [C.POINTER(vp), C.c_float, C.c_int32, C.c_int32, C.c_int32]
    L.dlco_desc_destroy.argtypes = [vp]
    L.dlco_desc_destroy.restype = None
    L.dlco_desc_select_filters.argtypes = [f32p, C.c_int32, C.c_int32, f32p, C.c_int32, f32p, C.POINTER(C.c_int32)]
    L.dlco_desc_set_filters.argtypes = [vp, f32p, C.c_int32]
    L.dlco_desc_size.argtypes = [vp]
    L.dlco_desc_size.restype = C.c_int32
    L.dlco_desc_transform.argtypes = [vp, u8p, f32p]
    L.dlco_desc_compute.argtypes = [vp, u8p, i64, f32p]
    L.dlco_desc_compute_device.argtypes = [vp, u8p, i64, vp, i64]
    L.dlco_desc_pair_dists.argtypes = [vp, u8p, i64, i32p, i64, f32p, u8p]
    L.dlco_desc_full_dists.argtypes = [vp, u8p, i64, i32p, i64, f32p, u8p]
    L.dlco_desc_set_projection.argtypes = [vp, f32p, C.c_int32, C.c_int32]
    L.dlco_desc_projected_size.argtypes = [vp]
    L.dlco_desc_projected_size.restype = C.c_int32
    L.dlco_desc_describe.argtypes = [vp, u8p, i64, f32p]
    L.dlco_desc_describe_device.argtypes = [vp, u8p, i64, vp, i64]
    L.dlco_desc_set_image.argtypes = [vp, u8p, C.c_int32, C.c_int32, i64]
    L.dlco_desc_set_image_device.argtypes = [vp, vp, C.c_int32, C.c_int32, i64]
    L.dlco_desc_extract_patches.argtypes = [vp, f32p, i64, C.c_float, C.c_int32, u8p, u8p]
    L.dlco_desc_describe_keypoints.argtypes = [vp, f32p, i64, C.c_float, C.c_int32, f32p, u8p]
    L.dlco_desc_describe_keypoints_device.argtypes = [vp, f32p, i64, C.c_float, C.c_int32, vp, i64, u8p]
    i64p = C.POINTER(C.c_int64)
    L.dlco_desc_detect.argtypes = [vp, C.c_int32, i64, i64, f32p, i64p, i64p, i64p]
    L.dlco_desc_detect_device.argtypes = [vp, C.c_int32, i64, i64, vp, vp, i64p, i64p]
    L.dlco_desc_detect_stage_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.dlco_desc_orient.argtypes = [vp, f32p, i64, f32p, i64p, u8p]
    L.dlco_desc_detect_oriented.argtypes = [vp, C.c_int32, i64, i64, f32p, i64p, i64p, i64p]
    L.dlco_desc_last_orient_ms.argtypes = [vp]
    L.dlco_desc_last_orient_ms.restype = C.c_double
    L.dlco_desc_pair_sqdists.argtypes = [vp, u8p, i64, i32p, i64, f32p, u8p]
    L.dlco_desc_pair_stats.argtypes = [vp, u8p, i64, i32p, i64, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)]
    L.dlco_desc_match.argtypes = [vp, f32p, i64, f32p, i64, C.c_int32, i32p, f32p]
    L.dlco_desc_match_device.argtypes = [vp, vp, i64, i64, vp, i64, i64, C.c_int32, vp, vp]
    L.dlco_desc_cross_sqdists.argtypes = [vp, f32p, i64, f32p, i64, C.c_int32, f32p]
    L.dlco_desc_quant_fit.argtypes = [f32p, i64, C.c_int32, C.POINTER(C.c_float), f32p]
    L.dlco_desc_quantize.argtypes = [f32p, i64, C.c_int32, C.c_float, f32p, u8p]
    L.dlco_desc_set_quantizer.argtypes = [vp, C.c_float, f32p, C.c_int32]
    L.dlco_desc_describe_u8.argtypes = [vp, u8p, i64, u8p]
    L.dlco_desc_describe_u8_device.argtypes = [vp, u8p, i64, vp, i64]
    L.dlco_desc_describe_keypoints_u8.argtypes = [vp, f32p, i64, C.c_float, C.c_int32, u8p, u8p]
    L.dlco_desc_describe_keypoints_u8_device.argtypes = [vp, f32p, i64, C.c_float, C.c_int32, vp, i64, u8p]
    L.dlco_desc_match_u8.argtypes = [vp, u8p, i64, u8p, i64, C.c_int32, i32p, i32p]
    L.dlco_desc_match_u8_device.argtypes = [vp, vp, i64, i64, vp, i64, i64, C.c_int32, vp, vp]
    L.dlco_desc_cross_sqdists_u8.argtypes = [vp, u8p, i64, u8p, i64, C.c_int32, i32p]
    f64p = C.POINTER(C.c_double)
    L.dlco_desc_verify_homography.argtypes = [vp, f32p, f32p, i64, C.c_float, C.c_int32, C.c_uint64, C.c_int32, f64p, u8p, i64p, i32p]
    L.dlco_desc_verify_hypotheses.argtypes = [vp, f32p, f32p, i64, C.c_float, C.c_int32, C.c_uint64, f64p, i32p]
    L.dlco_desc_verify_fundamental.argtypes = L.dlco_desc_verify_homography.argtypes
    L.dlco_desc_verify_fundamental_hypotheses.argtypes = L.dlco_desc_verify_hypotheses.argtypes
    L.dlco_desc_verify_pairs_homography.argtypes = [vp, f32p, f32p, i64p, i64, C.c_float, C.c_int32, C.c_uint64, C.c_int32, f64p, u8p, i64p, i32p]
    L.dlco_desc_verify_pairs_hypotheses.argtypes = [vp, f32p, f32p, i64p, i64, C.c_float, C.c_int32, C.c_uint64, f64p, i32p]
    L.dlco_desc_verify_pairs_fundamental.argtypes = L.dlco_desc_verify_pairs_homography.argtypes
    L.dlco_desc_verify_pairs_fundamental_hypotheses.argtypes = L.dlco_desc_verify_pairs_hypotheses.argtypes
    L.dlco_desc_verify_pairs_launches.argtypes = [i64p, i64, C.c_int32, C.c_int32, i32p]
    L.dlco_desc_verify_pairs_homography_device.argtypes = [vp, vp, vp, i64p, i64, C.c_float, C.c_int32, C.c_uint64, C.c_int32, f64p, vp, i64p, i32p]
    L.dlco_desc_verify_pairs_fundamental_device.argtypes = L.dlco_desc_verify_pairs_homography_device.argtypes
    L.dlco_desc_verify_pairs_refit_round.argtypes = [vp, f32p, f32p, i64p, i64, u8p, C.c_int32, f64p, u8p]
    L.dlco_desc_match_guided.argtypes = [vp, f32p, f32p, i64, f32p, f32p, i64, C.c_int32, f64p, C.c_float, C.c_int32, i32p, f32p]
    L.dlco_desc_match_guided_device.argtypes = [vp, vp, i64, vp, i64, i64, vp, i64, vp, i64, i64, C.c_int32, f64p, C.c_float,
                                                C.c_int32, vp, vp]
    L.dlco_desc_cross_sqdists_guided.argtypes = [vp, f32p, f32p, i64, f32p, f32p, i64, C.c_int32, f64p, C.c_float, C.c_int32, f32p]
    L.dlco_desc_match_guided_epipolar.argtypes = L.dlco_desc_match_guided.argtypes
    L.dlco_desc_match_guided_epipolar_device.argtypes = L.dlco_desc_match_guided_device.argtypes
    L.dlco_desc_cross_sqdists_guided_epipolar.argtypes = L.dlco_desc_cross_sqdists_guided.argtypes
    L.dlco_desc_match_pairs_rows.argtypes = [i64p, C.c_int32, i32p, i64, i64p]
    L.dlco_desc_match_pairs.argtypes = [vp, f32p, i64p, C.c_int32, i32p, i64, C.c_int32, i32p, f32p]
    L.dlco_desc_match_pairs_device.argtypes = [vp, vp, i64, i64p, C.c_int32, i32p, i64, C.c_int32, vp, vp]
    L.dlco_desc_match_pairs_u8.argtypes = [vp, u8p, i64p, C.c_int32, i32p, i64, C.c_int32, i32p, i32p]
    L.dlco_desc_match_pairs_u8_device.argtypes = [vp, vp, i64, i64p, C.c_int32, i32p, i64, C.c_int32, vp, vp]
    L.dlco_desc_match_pairs_slices.argtypes = [vp, i64p, C.c_int32, i32p, i64, C.c_int32, i32p]
    L.dlco_desc_select_pairs.argtypes = [vp, i64p, C.c_int32, i32p, i64, i32p, f32p, C.c_float, i32p, i64p, i64, f32p, i64p, i32p, f32p, f32p, f32p]
    L.dlco_desc_select_pairs_device.argtypes = [vp, i64p, C.c_int32, i32p, i64, vp, vp, C.c_float, vp, i64p, i64, vp, i64, i64p, vp, vp, vp, vp]
    L.dlco_desc_select_pairs_u8.argtypes = [vp, i64p, C.c_int32, i32p, i64, i32p, i32p, C.c_float, i32p, i64p, i64, f32p, i64p, i32p, i32p, f32p, f32p]
    L.dlco_desc_select_pairs_u8_device.argtypes = L.dlco_desc_select_pairs_device.argtypes
    L.dlco_desc_build_tracks.argtypes = [vp, i64p, C.c_int32, i32p, i64, i64p, i32p, u8p, C.c_int32, C.c_int32, i64p, i64p, i32p, i32p, i32p, i64p]
    L.dlco_desc_build_tracks_device.argtypes = [vp, i64p, C.c_int32, i32p, i64, i64p, vp, vp, C.c_int32, C.c_int32, i64p, vp, vp, vp, vp, i64p]
    L.dlco_desc_match_pairs_guided.argtypes = [vp, f32p, f32p, i64p, C.c_int32, i32p, i64, C.c_int32, f64p, C.c_float, C.c_int32, i32p, f32p]
    L.dlco_desc_match_pairs_guided_device.argtypes = [vp, vp, i64, vp, i64, i64p, C.c_int32, i32p, i64, C.c_int32, f64p, C.c_float, C.c_int32,
                                                      vp, vp]
    L.dlco_desc_match_pairs_guided_epipolar.argtypes = L.dlco_desc_match_pairs_guided.argtypes
    L.dlco_desc_match_pairs_guided_epipolar_device.argtypes = L.dlco_desc_match_pairs_guided_device.argtypes
    # the byte line's guided calls: the float ones argument for argument, byte tables and int32 distances
    L.dlco_desc_match_guided_u8.argtypes = [vp, u8p, f32p, i64, u8p, f32p, i64, C.c_int32, f64p, C.c_float, C.c_int32, i32p, i32p]
    L.dlco_desc_match_guided_u8_device.argtypes = L.dlco_desc_match_guided_device.argtypes
    L.dlco_desc_cross_sqdists_guided_u8.argtypes = [vp, u8p, f32p, i64, u8p, f32p, i64, C.c_int32, f64p, C.c_float, C.c_int32, i32p]
    L.dlco_desc_match_guided_epipolar_u8.argtypes = L.dlco_desc_match_guided_u8.argtypes
    L.dlco_desc_match_guided_epipolar_u8_device.argtypes = L.dlco_desc_match_guided_u8_device.argtypes
    L.dlco_desc_cross_sqdists_guided_epipolar_u8.argtypes = L.dlco_desc_cross_sqdists_guided_u8.argtypes
    L.dlco_desc_match_pairs_guided_u8.argtypes = [vp, u8p, f32p, i64p, C.c_int32, i32p, i64, C.c_int32, f64p, C.c_float, C.c_int32, i32p, i32p]
    L.dlco_desc_match_pairs_guided_u8_device.argtypes = L.dlco_desc_match_pairs_guided_device.argtypes
    L.dlco_desc_match_pairs_guided_epipolar_u8.argtypes = L.dlco_desc_match_pairs_guided_u8.argtypes
    L.dlco_desc_match_pairs_guided_epipolar_u8_device.argtypes = L.dlco_desc_match_pairs_guided_u8_device.argtypes
    L.dlco_desc_last_kernel_ms.argtypes = [vp]
    L.dlco_desc_last_kernel_ms.restype = C.c_double
    L.dlco_pr_last_error.restype = C.c_char_p
    L.dlco_pr_last_error.argtypes = [vp]
    L.dlco_pr_create.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_int32]
    L.dlco_pr_destroy.argtypes = [vp]
    L.dlco_pr_destroy.restype = None
    L.dlco_pr_device_name.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dlco_pr_set_data.argtypes = [vp, f32p, u8p]
    L.dlco_pr_get_index.argtypes = [vp, i32p, i32p, i32p, i32p]
    L.dlco_pr_steps.argtypes = [vp, C.c_uint32]
    L.dlco_pr_get_state.argtypes = [vp, C.POINTER(C.c_uint32), f32p, f32p]
    L.dlco_pr_set_state.argtypes = [vp, C.c_uint32, f32p, f32p]
    L.dlco_pr_validate.argtypes = [vp, f32p, f32p, i32p]
    L.dlco_pr_stats.argtypes = [vp, f32p, f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, i32p, f32p, C.POINTER(C.c_double)]
    L.dlco_pr_grid_last_error.restype = C.c_char_p
    L.dlco_pr_grid_last_error.argtypes = [vp]
    L.dlco_pr_grid_create.argtypes = [C.POINTER(vp), vp, C.c_int32, f32p, f32p, C.c_uint64]
    L.dlco_pr_grid_destroy.argtypes = [vp]
    L.dlco_pr_grid_destroy.restype = None
    L.dlco_pr_grid_steps.argtypes = [vp, C.c_uint32]
    L.dlco_pr_grid_get_state.argtypes = [vp, C.POINTER(C.c_uint32), f32p, f32p]
    L.dlco_pr_grid_validate.argtypes = [vp, f32p, f32p, i32p]
    L.dlco_pr_grid_stats.argtypes = [vp, i32p, C.c_int32, f32p, f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, i32p, f32p,
                                     C.POINTER(C.c_double)]
    L.dlco_pr_grid_set_group.argtypes = [vp, C.c_int32]
    L.dlco_pr_grid_group.argtypes = [vp]
    L.dlco_pr_grid_group.restype = C.c_int32
    _lib = L
    return L


def comm_unique_id(rccl_path=None):
    """128-byte ncclUniqueId for dlco_comm_init (rank 0 creates it, every rank receives the same bytes)."""
    L = load()
    buf = C.create_string_buffer(128)
    rc = L.dlco_comm_unique_id(buf, 128, rccl_path.encode() if rccl_path else None)
    if rc != OK:
        raise DlcoError(rc, L.dlco_last_error(None).decode())
    return buf.raw


def exported_symbols():
    """Names declared in include/dlco.h (used by the ABI test)."""
    import re
    text = open(HEADER_PATH).read()
    return sorted(set(re.findall(r"\b(dlco_[a-z0-9_]+)\s*\(", text)))


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _seg_pairs(seg, pairs):
    """seg [n_img + 1] int64 and pairs [n_pairs, 2] int32 as the match_pairs calls take them"""
    s, q = np.ascontiguousarray(seg, np.int64), np.ascontiguousarray(pairs, np.int32)
    assert s.ndim == 1 and s.size >= 2 and q.ndim == 2 and q.shape[1] == 2
    return s, q


def match_pairs_rows(seg, pairs):
    """row0 [n_pairs + 1] int64 of a match_pairs call: pair p = (a, b) owns the output rows row0[p] .. row0[p + 1] - 1, as
    many as image a has rows (seg [n_img + 1]: image s owns the rows seg[s] .. seg[s + 1] - 1 of the table).  No device."""
    s, q = _seg_pairs(seg, pairs)
    row0 = np.empty(q.shape[0] + 1, np.int64)
    rc = load().dlco_desc_match_pairs_rows(_p(s, i64p), s.size - 1, _p(q, i32p), q.shape[0],
                                           _p(row0, i64p))
    if rc != OK:
        raise DlcoError(rc, "match_pairs_rows: invalid seg or pairs")
    return row0


def verify_pairs_launches(moff, n_hyp, fundamental=False):
    """launch [n_pairs] int32 of a verify_pairs call over the match offsets moff [n_pairs + 1]: the launch that carries pair p,
    -1 for a pair of fewer matches than a sample (4, or 8 with fundamental), which launches nothing.  No device."""
    o = np.ascontiguousarray(moff, np.int64)
    assert o.ndim == 1 and o.size >= 2
    out = np.empty(o.size - 1, np.int32)
    rc = load().dlco_desc_verify_pairs_launches(_p(o, i64p), o.size - 1, n_hyp, 1 if fundamental else 0, _p(out, i32p))
    if rc != OK:
        raise DlcoError(rc, "verify_pairs_launches: invalid moff or n_hyp")
    return out


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class Context:
    """One pj-learn trainer on one GPU (thin wrapper over dlco_ctx)."""

    def __init__(self, F, N, B=200, mu=0.001, gamma=0.5, seed=2215, device=0, rank=0, world=1,
                 eig_tol=None, eig_guard=None, eig_max_iter=None, shard=0, strict_conv=0, grad_bf16=0):
        self.L = load()
        cfg = Cfg()
        self.L.dlco_cfg_default(C.byref(cfg))
        cfg.F, cfg.N, cfg.B, cfg.mu, cfg.gamma, cfg.seed = F, N, B, mu, gamma, seed
        cfg.device, cfg.rank, cfg.world, cfg.shard = device, rank, world, shard
        cfg.strict_conv = strict_conv
        cfg.grad_bf16 = grad_bf16
        if eig_tol is not None:
            cfg.eig_tol = eig_tol
        if eig_guard is not None:
            cfg.eig_guard = eig_guard
        if eig_max_iter is not None:
            cfg.eig_max_iter = eig_max_iter
        self.F, self.N, self.B, self.world, self.rank = F, N, B, world, rank
        h = C.c_void_p()
        rc = self.L.dlco_ctx_create(C.byref(h), C.byref(cfg))
        if rc != OK:
            raise DlcoError(rc, self.L.dlco_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.dlco_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != OK:
            raise DlcoError(rc, self.L.dlco_last_error(self.h).decode())

    # ---- data -------------------------------------------------------------------------------
    def device_name(self):
        buf = C.create_string_buffer(256)
        a, b = C.c_int(), C.c_int()
        self._ck(self.L.dlco_device_name(self.h, buf, 256, C.byref(a), C.byref(b)))
        return buf.value.decode(), a.value, b.value

    def set_data(self, dists, labels):
        d, l = _f32(dists), np.ascontiguousarray(labels, np.uint8).ravel()
        assert d.shape == (self.N, self.F) and l.size == self.N
        self._ck(self.L.dlco_set_data(self.h, _p(d, f32p), _p(l, u8p)))

    def set_data_device(self, dev_ptr, labels):
        l = np.ascontiguousarray(labels, np.uint8).ravel()
        self._ck(self.L.dlco_set_data_device(self.h, C.c_void_p(dev_ptr), _p(l, u8p)))

    def set_data_shared(self, other):
        """Train on the resident matrix of another context (same device, F, N): shared, not copied."""
        self._ck(self.L.dlco_set_data_shared(self.h, other.h))

    def device_width(self):
        """Row width on the device: F rounded up to whole 128-column tiles (see dlco_device_width)."""
        return int(self.L.dlco_device_width(self.h))

    def set_pairs(self, desc, pairs):
        """Pair mode: per-patch descriptors [P,F] + the [N,4] Indices table (see dlco_set_pairs)."""
        d, q = _f32(desc), _i32(pairs)
        assert d.ndim == 2 and d.shape[1] == self.F and q.shape == (self.N, 4)
        self._ck(self.L.dlco_set_pairs(self.h, _p(d, f32p), d.shape[0], _p(q, i32p)))

    def set_pairs_device(self, desc_dev_ptr, P, pairs):
        """Pair mode on a descriptor table that already lives in device memory (dlco_set_pairs_device)."""
        q = _i32(pairs)
        assert q.shape == (self.N, 4)
        self._ck(self.L.dlco_set_pairs_device(self.h, C.c_void_p(desc_dev_ptr), P, _p(q, i32p)))

    def synth_data(self, U, seed, sigma_pos, sigma_neg, noise, scale_jitter=0.0):
        U = _f32(U)
        assert U.shape[1] == self.F
        self._ck(self.L.dlco_synth_data(self.h, _p(U, f32p), U.shape[0], seed, sigma_pos, sigma_neg, noise, scale_jitter))

    def get_rows(self, row0, n):
        out = np.empty((n, self.F), np.float32)
        self._ck(self.L.dlco_get_rows(self.h, row0, n, _p(out, f32p)))
        return out

    def index(self):
        a, b, c_, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self.L.dlco_get_index(self.h, None, C.byref(a), C.byref(b), None, C.byref(c_), C.byref(d)))
        pos, neg = np.empty(max(a.value, 1), np.int32), np.empty(max(c_.value, 1), np.int32)
        self._ck(self.L.dlco_get_index(self.h, _p(pos, i32p), None, None, _p(neg, i32p), None, None))
        return dict(pos=pos[:a.value], n_pos_trn=b.value, neg=neg[:c_.value], n_neg_trn=d.value)

    # ---- training ---------------------------------------------------------------------------
    def step(self):
        self._ck(self.L.dlco_step(self.h))

    def steps(self, n):
        self._ck(self.L.dlco_steps(self.h, n))

    def step_begin(self):
        self._ck(self.L.dlco_step_begin(self.h))

    def step_grad(self):
        self._ck(self.L.dlco_step_grad(self.h))

    def step_finish(self):
        self._ck(self.L.dlco_step_finish(self.h))

    def sync(self):
        self._ck(self.L.dlco_sync(self.h))

    def dev_buffer(self, which):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(self.L.dlco_dev_buffer(self.h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def bind_buffer(self, which, dev_ptr, nbytes):
        self._ck(self.L.dlco_bind_buffer(self.h, which, C.c_void_p(dev_ptr), nbytes))

    def stream(self):
        p = C.c_void_p()
        self._ck(self.L.dlco_stream(self.h, C.byref(p)))
        return p.value

    def comm_init(self, id_bytes, rccl_path=None):
        """Collective: creates the library's own RCCL communicator from a 128-byte ncclUniqueId."""
        buf = C.create_string_buffer(bytes(id_bytes), 128)
        self._ck(self.L.dlco_comm_init(self.h, buf, 128, rccl_path.encode() if rccl_path else None))

    def comm_destroy(self):
        self._ck(self.L.dlco_comm_destroy(self.h))

    def set_allgather(self, fn):
        """fn(which, bytes_per_rank) -> 0 on success; kept alive by the context (see dlco_set_allgather)."""
        def tramp(_user, which, nbytes):
            try:
                return int(fn(int(which), int(nbytes)) or 0)
            except Exception:                    # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return -1
        self._ag = ALLGATHER_FN(tramp)
        self._ck(self.L.dlco_set_allgather(self.h, self._ag, None))

    def batch(self):
        B = self.B
        pr, nr = np.empty(B, np.int32), np.empty(B, np.int32)
        pd, nd = np.empty(B, np.float32), np.empty(B, np.float32)
        rho, kap = np.empty(B, np.int32), np.empty(B, np.int32)
        self._ck(self.L.dlco_get_batch(self.h, _p(pr, i32p), _p(nr, i32p), _p(pd, f32p), _p(nd, f32p), _p(rho, i32p), _p(kap, i32p)))
        return dict(pos_rows=pr, neg_rows=nr, pd=pd, nd=nd, rho=rho, kappa=kap)

    def t(self):
        v = C.c_uint32()
        self._ck(self.L.dlco_get_t(self.h, C.byref(v)))
        return v.value

    def W(self):
        W = np.empty((self.F, self.F), np.float32)
        r = C.c_int32()
        self._ck(self.L.dlco_get_W(self.h, _p(W, f32p), C.byref(r)))
        return W[:r.value].copy()

    def A(self):
        A = np.empty((self.F, self.F), np.float32)
        self._ck(self.L.dlco_get_A(self.h, _p(A, f32p)))
        return A

    def dfavg(self):
        A = np.empty((self.F, self.F), np.float32)
        self._ck(self.L.dlco_get_dfavg(self.h, _p(A, f32p)))
        return A

    def set_state(self, t, dfavg=None, W=None):
        d = None if dfavg is None else _f32(dfavg)
        w = None if W is None or len(W) == 0 else _f32(W)
        self._ck(self.L.dlco_set_state(self.h, t, _p(d, f32p), _p(w, f32p), 0 if w is None else w.shape[0]))

    def validate(self):
        lo, rg, rk = C.c_float(), C.c_float(), C.c_int32()
        self._ck(self.L.dlco_validate(self.h, C.byref(lo), C.byref(rg), C.byref(rk)))
        return lo.value, rg.value, rk.value

    def stats(self, W=None):
        dim, f, a = C.c_int32(), C.c_float(), C.c_double()
        w = None if W is None else _f32(W)
        self._ck(self.L.dlco_stats(self.h, _p(w, f32p), 0 if w is None else w.shape[0], C.byref(dim), C.byref(f), C.byref(a)))
        return dim.value, f.value, a.value

    def log_step(self):
        e = LogEntry()
        self._ck(self.L.dlco_log_step(self.h, C.byref(e)))
        return e

    def saved(self):
        r = C.c_int32()
        self._ck(self.L.dlco_get_saved(self.h, None, C.byref(r), None))
        if r.value == 0:
            return None, None
        W, A = np.empty((r.value, self.F), np.float32), np.empty((self.F, self.F), np.float32)
        self._ck(self.L.dlco_get_saved(self.h, _p(W, f32p), C.byref(r), _p(A, f32p)))
        return W, A

    # ---- single operators -------------------------------------------------------------------
    def project_sqdist(self, row_ids, W):
        ids, w = _i32(row_ids), _f32(W)
        out = np.empty(ids.size, np.float32)
        self._ck(self.L.dlco_project_sqdist(self.h, _p(ids, i32p), ids.size, _p(w, f32p), w.shape[0] if w.size else 0, _p(out, f32p)))
        return out

    def viol_counts(self, pd, nd):
        pd, nd = _f32(pd), _f32(nd)
        rho, kap = np.empty(pd.size, np.int32), np.empty(pd.size, np.int32)
        self._ck(self.L.dlco_viol_counts(self.h, _p(pd, f32p), _p(nd, f32p), pd.size, _p(rho, i32p), _p(kap, i32p)))
        return rho, kap

    def grad_rda(self, pos_rows, neg_rows, rho, kappa, alpha, beta, dfavg_in=None):
        pr, nr, rho, kap = _i32(pos_rows), _i32(neg_rows), _i32(rho), _i32(kappa)
        d = None if dfavg_in is None else _f32(dfavg_in)
        out = np.empty((self.F, self.F), np.float32)
        self._ck(self.L.dlco_grad_rda(self.h, _p(pr, i32p), _p(nr, i32p), _p(rho, i32p), _p(kap, i32p), pr.size, alpha, beta, _p(d, f32p), _p(out, f32p)))
        return out

    def psd_project(self, dfavg, t, want_A=True):
        d = _f32(dfavg)
        W = np.empty((self.F, self.F), np.float32)
        A = np.empty((self.F, self.F), np.float32) if want_A else None
        r = C.c_int32()
        self._ck(self.L.dlco_psd_project(self.h, _p(d, f32p), t, _p(W, f32p), C.byref(r), _p(A, f32p)))
        return W[:r.value].copy(), A

    def sym_product(self, X, G, mode=0):
        x, g = _f32(X), _f32(G)
        out = np.empty_like(x)
        self._ck(self.L.dlco_sym_product(self.h, _p(x, f32p), x.shape[0], _p(g, f32p), mode, _p(out, f32p)))
        return out

    def gemm_probe(self, A, B, M, N, K, a_kmajor=False, b_kmajor=False, a_ids=None, a_ids2=None, a_scale=None, b_ids=None,
                   b_ids2=None, b_scale=None, B2=None, split_k=1, k_dev=-1, small_m_tiles=False, small_n_tiles=False, depth=0,
                   alpha=1.0, beta=0.0, C_in=None, E1=None, b1=0.0, E2=None, b2=0.0, reps=0):
        """The generic fp32 GEMM on host arrays (dlco_gemm_probe).  A, B (and B2, laid out like B) are the operands as they
        lie in memory, 2-D [rows, ld]: k-major ones hold K (or gathered) rows of M / N elements, the others M / N (or
        gathered) rows of K elements.  Returns dict(C, C2 (None without B2), depth, us (None without reps))."""
        keep = []

        def operand(x, kmajor, ids, ids2, scale):
            x = _f32(x)
            assert x.ndim == 2
            ids, ids2 = (None if i is None else _i32(i) for i in (ids, ids2))
            scale = None if scale is None else _f32(scale)
            keep.extend([x, ids, ids2, scale])
            return GemmOperand(_p(x, f32p), x.shape[0], x.shape[1], int(kmajor), _p(ids, i32p), _p(ids2, i32p), _p(scale, f32p)), x

        a = GemmProbeArgs()
        a.M, a.N, a.K = M, N, K
        a.A, _ = operand(A, a_kmajor, a_ids, a_ids2, a_scale)
        a.B, b = operand(B, b_kmajor, b_ids, b_ids2, b_scale)
        twin = None if B2 is None else _f32(B2)
        assert twin is None or twin.shape == b.shape
        e1, e2 = (None if e is None else _f32(e) for e in (E1, E2))
        assert all(e is None or e.shape == (M, N) for e in (e1, e2))
        a.B2_host, a.E1_host, a.E2_host = _p(twin, f32p), _p(e1, f32p), _p(e2, f32p)
        a.split_k, a.k_dev, a.depth, a.reps = split_k, k_dev, depth, reps
        a.small_m_tiles, a.small_n_tiles = int(small_m_tiles), int(small_n_tiles)
        a.alpha, a.beta, a.b1, a.b2 = alpha, beta, b1, b2
        out = np.zeros((M, N), np.float32) if C_in is None else np.array(C_in, dtype=np.float32, order="C")
        assert out.shape == (M, N)
        out2 = None if twin is None else out.copy()
        used, us = C.c_int32(), C.c_double()
        self._ck(self.L.dlco_gemm_probe(self.h, C.byref(a), _p(out, f32p), _p(out2, f32p), C.byref(used), C.byref(us)))
        return dict(C=out, C2=out2, depth=used.value, us=us.value if reps else None)

    def chol_probe(self, M, rel_thresh=1e-5):
        """CholQR's Cholesky inverse alone (dlco_chol_probe): M [n, n] symmetric, n <= 160.  Returns (Linv [n, n], dead [n])."""
        m = _f32(M)
        assert m.ndim == 2 and m.shape[0] == m.shape[1]
        n = m.shape[0]
        linv, dead = np.zeros((n, n), np.float32), np.zeros(n, np.int32)
        self._ck(self.L.dlco_chol_probe(self.h, _p(m, f32p), n, n, rel_thresh, _p(linv, f32p), _p(dead, i32p)))
        return linv, dead

    def ortho_probe(self, Z, Gp, alpha, b1, b2=0.0, Zprev=None, panel_end=0, n_lock=0, unfused=False):
        """The tail of one tracker pass (dlco_ortho_probe): Z [m, F], Gp = the packed upper tiles of G (a flat array,
        layout in dlco.h).  Returns dict(Qo [m, F], Yb [m, F], T [m, m], fused = reductions that formed Gram partials,
        applied = applications of L^-1 that fed the next launch)."""
        z, gp = _f32(Z), _f32(Gp).ravel()
        zp = None if Zprev is None else _f32(Zprev)
        m, F = z.shape
        nt = F // 128
        assert F == self.F and F % 128 == 0 and gp.size == nt * (nt + 1) // 2 * 128 * 128 and (zp is None or zp.shape == z.shape)
        a = OrthoProbeArgs()
        a.Z_host, a.Zprev_host, a.Gp_host = _p(z, f32p), _p(zp, f32p), _p(gp, f32p)
        a.m, a.panel_end, a.n_lock, a.unfused = m, panel_end, n_lock, int(unfused)
        a.alpha, a.b1, a.b2 = alpha, b1, b2
        qo, yb, t = np.zeros((m, F), np.float32), np.zeros((m, F), np.float32), np.zeros((m, m), np.float32)
        fused = (C.c_int64 * 2)()
        self._ck(self.L.dlco_ortho_probe(self.h, C.byref(a), _p(qo, f32p), _p(yb, f32p), _p(t, f32p), fused))
        return dict(Qo=qo, Yb=yb, T=t, fused=fused[0], applied=fused[1])

    def hinge_sum(self, pos, neg):
        p, n = _f32(pos), _f32(neg)
        out = C.c_double()
        self._ck(self.L.dlco_hinge_sum(self.h, _p(p, f32p), p.size, _p(n, f32p), n.size, C.byref(out)))
        return out.value

    def roc_stats(self, dist, labels):
        d, l = _f32(dist), np.ascontiguousarray(labels, np.uint8).ravel()
        f, a = C.c_float(), C.c_double()
        self._ck(self.L.dlco_roc_stats(self.h, _p(d, f32p), _p(l, u8p), d.size, C.byref(f), C.byref(a)))
        return f.value, a.value

    # ---- measurement ------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._ck(self.L.dlco_profile_enable(self.h, int(on)))          # True / 1: every kernel group, 2: the gradient SYRK only

    def profile_read(self, kernel="grad_syrk"):
        n, ms = C.c_int64(), C.c_double()
        self._ck(self.L.dlco_profile_read(self.h, kernel.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def counters(self):
        out = (C.c_int64 * 8)()
        self._ck(self.L.dlco_counters(self.h, out))
        fused = (C.c_int64 * 2)()
        self._ck(self.L.dlco_fused_counters(self.h, fused))
        return dict(fused_gram_reductions=fused[0], fused_applications=fused[1], steps=out[0], active_rows=out[1], nonconverged=out[2], jacobi_barrier_timeouts=out[3],
                    rank_update_passes=out[4], rank_update_check=out[5] * 1e-9, locked_passes=out[6], locked_rows=out[7])

    def eig_stats(self):
        a, b, c_, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        self._ck(self.L.dlco_eig_stats(self.h, C.byref(a), C.byref(b), C.byref(c_), C.byref(d)))
        return dict(iters=a.value, product_rows=b.value, jacobi_sweeps=c_.value, block_rows=d.value)


class PrContext:
    """pr-learn: L1-regularised dual averaging on the pooling-region weights (thin wrapper over dlco_pr_ctx)."""

    def __init__(self, F, N, mu=0.025, gamma=0.10, seed=2215, device=0):
        self.L = load()
        self.F, self.N = F, N
        h = C.c_void_p()
        rc = self.L.dlco_pr_create(C.byref(h), F, N, mu, gamma, seed, device)
        if rc != OK:
            raise DlcoError(rc, self.L.dlco_pr_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.dlco_pr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != OK:
            raise DlcoError(rc, self.L.dlco_pr_last_error(self.h).decode())

    def set_data(self, dists, labels):
        d, l = _f32(dists), np.ascontiguousarray(labels, np.uint8).ravel()
        assert d.shape == (self.N, self.F) and l.size == self.N
        self._ck(self.L.dlco_pr_set_data(self.h, _p(d, f32p), _p(l, u8p)))

    def index(self):
        a, b, c_, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self.L.dlco_pr_get_index(self.h, C.byref(a), C.byref(b), C.byref(c_), C.byref(d)))
        return dict(n_pos=a.value, n_pos_trn=b.value, n_neg=c_.value, n_neg_trn=d.value)

    def steps(self, n):
        self._ck(self.L.dlco_pr_steps(self.h, n))

    def state(self):
        t = C.c_uint32()
        w, df = np.empty(self.F, np.float32), np.empty(self.F, np.float32)
        self._ck(self.L.dlco_pr_get_state(self.h, C.byref(t), _p(w, f32p), _p(df, f32p)))
        return dict(t=t.value, w=w, dfavg=df)

    def set_state(self, t, w=None, dfavg=None):
        w = None if w is None else _f32(w)
        d = None if dfavg is None else _f32(dfavg)
        self._ck(self.L.dlco_pr_set_state(self.h, t, _p(w, f32p), _p(d, f32p)))

    def validate(self):
        lo, rg, nz = C.c_float(), C.c_float(), C.c_int32()
        self._ck(self.L.dlco_pr_validate(self.h, C.byref(lo), C.byref(rg), C.byref(nz)))
        return lo.value, rg.value, nz.value

    def stats(self, prparams, w=None, nchannels=8, max_dim=-1):
        p = _f32(prparams)
        wv = None if w is None else _f32(w)
        npr, dim, nz, f, a = C.c_int32(), C.c_int32(), C.c_int32(), C.c_float(-1.0), C.c_double(0.0)
        self._ck(self.L.dlco_pr_stats(self.h, _p(wv, f32p), _p(p, f32p), p.shape[0], p.shape[1], nchannels, max_dim,
                                      C.byref(npr), C.byref(dim), C.byref(nz), C.byref(f), C.byref(a)))
        return dict(nPR=npr.value, dim=dim.value, nzdim=nz.value, fpr95=f.value, auc=a.value)


class PrGrid:
    """A grid of pr-learn settings (mus[k], gammas[k]) trained together on the data of `src` (thin wrapper over
    dlco_pr_grid).  Setting k follows, bit for bit, a PrContext(F, N, mus[k], gammas[k], seed) on the same data;
    `src` must stay open while the grid is used, and its own state is never touched."""

    def __init__(self, src, mus, gammas, seed=2215):
        self.L = load()
        mu, ga = _f32(mus).ravel(), _f32(gammas).ravel()
        assert mu.size == ga.size
        self.src, self.F, self.N, self.G = src, src.F, src.N, int(mu.size)
        self.mus, self.gammas = mu.copy(), ga.copy()
        h = C.c_void_p()
        rc = self.L.dlco_pr_grid_create(C.byref(h), src.h, self.G, _p(mu, f32p), _p(ga, f32p), seed)
        if rc != OK:
            raise DlcoError(rc, self.L.dlco_pr_grid_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.dlco_pr_grid_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != OK:
            raise DlcoError(rc, self.L.dlco_pr_grid_last_error(self.h).decode())

    def set_group(self, per_group):
        """Settings per workgroup (0 = the library's rule, 1, 2 or 4); results do not depend on it."""
        self._ck(self.L.dlco_pr_grid_set_group(self.h, per_group))

    def group(self):
        return int(self.L.dlco_pr_grid_group(self.h))

    def steps(self, n):
        self._ck(self.L.dlco_pr_grid_steps(self.h, n))

    def state(self):
        t = C.c_uint32()
        w, df = np.empty((self.G, self.F), np.float32), np.empty((self.G, self.F), np.float32)
        self._ck(self.L.dlco_pr_grid_get_state(self.h, C.byref(t), _p(w, f32p), _p(df, f32p)))
        return dict(t=t.value, w=w, dfavg=df)

    def validate(self):
        lo, rg, nz = np.empty(self.G, np.float32), np.empty(self.G, np.float32), np.empty(self.G, np.int32)
        self._ck(self.L.dlco_pr_grid_validate(self.h, _p(lo, f32p), _p(rg, f32p), _p(nz, i32p)))
        return dict(loss=lo, regul=rg, nnz=nz)

    def stats(self, prparams, configs=None, w=None, nchannels=8, max_dim=-1):
        """ComputePRStats per listed setting (default: all); arrays in the order of `configs`."""
        p = _f32(prparams)
        cf = _i32(np.arange(self.G) if configs is None else configs).ravel()
        n = cf.size
        wv = None if w is None else _f32(w).reshape(n, self.F)
        npr, dim, nz = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        f, a = np.full(n, -1.0, np.float32), np.zeros(n, np.float64)
        self._ck(self.L.dlco_pr_grid_stats(self.h, _p(cf, i32p), n, _p(wv, f32p), _p(p, f32p), p.shape[0], p.shape[1], nchannels, max_dim,
                                           _p(npr, i32p), _p(dim, i32p), _p(nz, i32p), _p(f, f32p),
                                           a.ctypes.data_as(C.POINTER(C.c_double))))
        return dict(nPR=npr, dim=dim, nzdim=nz, fpr95=f, auc=a)


def select_filters(pr_filters, w):
    """SelectPRFilters (src/misc.cpp:78-168): host logic of the library, no device needed."""
    L = load()
    f, wv = _f32(pr_filters), _f32(w).ravel()
    assert f.ndim == 2 and f.shape[0] == 8 * wv.size
    n = C.c_int32()
    rc = L.dlco_desc_select_filters(_p(f, f32p), f.shape[0], f.shape[1], _p(wv, f32p), wv.size, None, C.byref(n))
    if rc != OK:
        raise DlcoError(rc, "dlco_desc_select_filters")
    out = np.empty((n.value, f.shape[1]), np.float32)
    if n.value:
        L.dlco_desc_select_filters(_p(f, f32p), f.shape[0], f.shape[1], _p(wv, f32p), wv.size, _p(out, f32p), C.byref(n))
    return out


def quant_fit(Y):
    """(scale, offset [r]) of the quantiser fitted to the sample Y [n, r] (csrc/quant_rules.hpp): host logic, no device needed."""
    L = load()
    y = _f32(Y)
    assert y.ndim == 2
    scale, off = C.c_float(), np.empty(y.shape[1], np.float32)
    rc = L.dlco_desc_quant_fit(_p(y, f32p), y.shape[0], y.shape[1], C.byref(scale), _p(off, f32p))
    if rc != OK:
        raise DlcoError(rc, "dlco_desc_quant_fit")
    return scale.value, off


def quantize(Y, scale, offset=None):
    """Bytes [n, r] of the rows Y [n, r] under the quantiser (scale, offset; None = zeros): host logic, no device needed."""
    L = load()
    y = _f32(Y)
    assert y.ndim == 2
    off = None if offset is None else _f32(offset).ravel()
    assert off is None or off.size == y.shape[1]
    out = np.empty(y.shape, np.uint8)
    rc = L.dlco_desc_quantize(_p(y, f32p), y.shape[0], y.shape[1], scale, _p(off, f32p), _p(out, u8p))
    if rc != OK:
        raise DlcoError(rc, "dlco_desc_quantize")
    return out


class DescContext:
    """comp-uprjdists on the GPU: get_desc + pooling product per patch (thin wrapper over dlco_desc_ctx)."""

    def __init__(self, init_sigma=1.4, n_angle_bins=8, norm=True, device=0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.dlco_desc_create(C.byref(h), init_sigma, n_angle_bins, 1 if norm else 0, device)
        if rc != OK:
            raise DlcoError(rc, self.L.dlco_desc_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.dlco_desc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != OK:
            raise DlcoError(rc, self.L.dlco_desc_last_error(self.h).decode())

    def set_filters(self, sPR):
        f = _f32(sPR)
        assert f.ndim == 2 and f.shape[1] == 4096
        self._ck(self.L.dlco_desc_set_filters(self.h, _p(f, f32p), f.shape[0]))

    @property
    def size(self):
        return self.L.dlco_desc_size(self.h)

    def transform(self, patch):
        p = np.ascontiguousarray(patch, np.uint8)
        assert p.shape == (64, 64)
        out = np.empty((4096, 8), np.float32)
        self._ck(self.L.dlco_desc_transform(self.h, _p(p, u8p), _p(out, f32p)))
        return out

    def compute(self, patches):
        p = np.ascontiguousarray(patches, np.uint8)
        assert p.ndim == 3 and p.shape[1:] == (64, 64)
        out = np.empty((p.shape[0], self.size), np.float32)
        self._ck(self.L.dlco_desc_compute(self.h, _p(p, u8p), p.shape[0], _p(out, f32p)))
        return out

    def compute_device(self, patches, dev_ptr, ld=None):
        p = np.ascontiguousarray(patches, np.uint8)
        assert p.ndim == 3 and p.shape[1:] == (64, 64)
        self._ck(self.L.dlco_desc_compute_device(self.h, _p(p, u8p), p.shape[0], C.c_void_p(dev_ptr), ld or self.size))

    def pair_dists(self, patches, pairs):
        p, q = np.ascontiguousarray(patches, np.uint8), _i32(pairs)
        assert p.ndim == 3 and p.shape[1:] == (64, 64) and q.ndim == 2 and q.shape[1] == 4
        dist = np.empty((q.shape[0], self.size), np.float32)
        lab = np.empty(q.shape[0], np.uint8)
        self._ck(self.L.dlco_desc_pair_dists(self.h, _p(p, u8p), p.shape[0], _p(q, i32p), q.shape[0], _p(dist, f32p), _p(lab, u8p)))
        return dist, lab

    def full_dists(self, patches, pairs):
        """comp-fulldists: per-region squared descriptor distances [n_pairs, rows/8] and labels (pr-learn's input)."""
        p, q = np.ascontiguousarray(patches, np.uint8), _i32(pairs)
        assert p.ndim == 3 and p.shape[1:] == (64, 64) and q.ndim == 2 and q.shape[1] == 4
        dist = np.empty((q.shape[0], max(1, self.size // 64)), np.float32)
        lab = np.empty(q.shape[0], np.uint8)
        self._ck(self.L.dlco_desc_full_dists(self.h, _p(p, u8p), p.shape[0], _p(q, i32p), q.shape[0], _p(dist, f32p), _p(lab, u8p)))
        return dist, lab

    # ---- the learnt descriptor y = W * min(sPRFilters * get_desc(patch), 1) ----
    def set_projection(self, W):
        """pj-learn's W [r, F] with F == size; replaces any earlier projection."""
        w = _f32(W)
        assert w.ndim == 2
        self._ck(self.L.dlco_desc_set_projection(self.h, _p(w, f32p), w.shape[0], w.shape[1]))

    @property
    def projected_size(self):
        return self.L.dlco_desc_projected_size(self.h)

    def describe(self, patches):
        """Learnt descriptors [n, r] of patches [n,64,64] u8."""
        p = np.ascontiguousarray(patches, np.uint8)
        assert p.ndim == 3 and p.shape[1:] == (64, 64)
        out = np.empty((p.shape[0], self.projected_size), np.float32)
        self._ck(self.L.dlco_desc_describe(self.h, _p(p, u8p), p.shape[0], _p(out, f32p)))
        return out

    def describe_device(self, patches, dev_ptr, ld=None):
        p = np.ascontiguousarray(patches, np.uint8)
        assert p.ndim == 3 and p.shape[1:] == (64, 64)
        self._ck(self.L.dlco_desc_describe_device(self.h, _p(p, u8p), p.shape[0], C.c_void_p(dev_ptr), ld or self.projected_size))

    # ---- keypoints of an image: patches sampled on the device (csrc/patch_rules.hpp states the rule) ----
    def set_image(self, img):
        """img [H, W] u8 (rows may be strided); copied to the device."""
        a = np.asarray(img)
        if a.dtype != np.uint8 or a.ndim != 2 or a.strides[1] != 1 or a.strides[0] < a.shape[1]:
            a = np.ascontiguousarray(a, np.uint8)
        assert a.ndim == 2
        self._ck(self.L.dlco_desc_set_image(self.h, C.cast(C.c_void_p(a.ctypes.data), u8p), a.shape[1], a.shape[0], a.strides[0]))

    def set_image_device(self, ptr, w, h, pitch=None):
        """An image [h][pitch] u8 already in device memory: adopted, the caller keeps it alive."""
        self._ck(self.L.dlco_desc_set_image_device(self.h, C.c_void_p(ptr), w, h, pitch or w))

    @staticmethod
    def _keypoints(kp):
        k = _f32(kp)
        assert k.ndim == 2 and k.shape[1] == 4, "keypoints are [n, 4] = (x, y, size, angle)"
        return k

    def extract_patches(self, kp, scale_factor=6.25, use_orientation=True):
        """(patches [n,64,64] u8, status [n] u8) of keypoints [n,4] = (x, y, size, angle) on the image set."""
        k = self._keypoints(kp)
        patches, status = np.empty((k.shape[0], 64, 64), np.uint8), np.empty(k.shape[0], np.uint8)
        self._ck(self.L.dlco_desc_extract_patches(self.h, _p(k, f32p), k.shape[0], scale_factor, 1 if use_orientation else 0, _p(patches, u8p),
                                                  _p(status, u8p)))
        return patches, status

    def describe_keypoints(self, kp, scale_factor=6.25, use_orientation=True):
        """(Y [n, r], status [n]): describe(extract_patches(kp)) without the patches leaving the device; status-0 rows are zero."""
        k = self._keypoints(kp)
        out, status = np.empty((k.shape[0], self.projected_size), np.float32), np.empty(k.shape[0], np.uint8)
        self._ck(self.L.dlco_desc_describe_keypoints(self.h, _p(k, f32p), k.shape[0], scale_factor, 1 if use_orientation else 0, _p(out, f32p),
                                                     _p(status, u8p)))
        return out, status

    def describe_keypoints_device(self, kp, dev_ptr, ld=None, scale_factor=6.25, use_orientation=True):
        """The same rows into device memory at dev_ptr, row pitch ld floats; returns status [n]."""
        k = self._keypoints(kp)
        status = np.empty(k.shape[0], np.uint8)
        self._ck(self.L.dlco_desc_describe_keypoints_device(self.h, _p(k, f32p), k.shape[0], scale_factor, 1 if use_orientation else 0,
                                                            C.c_void_p(dev_ptr), ld or self.projected_size, _p(status, u8p)))
        return status

    # ---- the keypoints themselves: a detector on the image set (csrc/detect_rules.hpp states the rule) ----
    def detect(self, n_octaves=3, threshold=DETECT_THRESHOLD, max_keypoints=100000):
        """(keypoints [n,4] f32 = (x, y, size, -1), response [n] i64, n_found) of the image set: the n = min(n_found,
        max_keypoints) strongest keypoints, strongest first.  The default threshold is a determinant of 100 squared grey levels."""
        kp, resp = np.empty((max(max_keypoints, 1), 4), np.float32), np.empty(max(max_keypoints, 1), np.int64)
        n, found = C.c_int64(), C.c_int64()
        self._ck(self.L.dlco_desc_detect(self.h, n_octaves, threshold, max_keypoints, _p(kp, f32p), _p(resp, C.POINTER(C.c_int64)),
                                         C.byref(n), C.byref(found)))
        return kp[:n.value].copy(), resp[:n.value].copy(), found.value

    def detect_oriented(self, n_octaves=3, threshold=DETECT_THRESHOLD, max_keypoints=100000):
        """detect with the fourth column filled by the orientation rule (csrc/orient_rules.hpp): (keypoints [n,4] f32 =
        (x, y, size, angle), response [n] i64, n_found).  The keypoints are oriented before they leave the device."""
        kp, resp = np.empty((max(max_keypoints, 1), 4), np.float32), np.empty(max(max_keypoints, 1), np.int64)
        n, found = C.c_int64(), C.c_int64()
        self._ck(self.L.dlco_desc_detect_oriented(self.h, n_octaves, threshold, max_keypoints, _p(kp, f32p), _p(resp, C.POINTER(C.c_int64)),
                                                  C.byref(n), C.byref(found)))
        return kp[:n.value].copy(), resp[:n.value].copy(), found.value

    def orient(self, kp):
        """(angles [n] f32, vectors [n,2] i64, status [n] u8) of keypoints [n,4] on the image set; the angle that comes in is
        ignored.  An angle is in [0, 360) or -1 (none); status 0 invalid, 1 some samples skipped at the border, 2 all used."""
        k = self._keypoints(kp)
        n = k.shape[0]
        angles, vectors, status = np.empty(n, np.float32), np.empty((n, 2), np.int64), np.empty(n, np.uint8)
        self._ck(self.L.dlco_desc_orient(self.h, _p(k, f32p), n, _p(angles, f32p), _p(vectors, C.POINTER(C.c_int64)), _p(status, u8p)))
        return angles, vectors, status

    def last_orient_ms(self):
        """Kernel milliseconds of the last orientation kernel (orient, detect_oriented)."""
        return self.L.dlco_desc_last_orient_ms(self.h)

    def detect_device(self, kp_ptr, resp_ptr, n_octaves=3, threshold=DETECT_THRESHOLD, max_keypoints=100000):
        """The same rows into device memory: kp_ptr [max_keypoints][4] f32 (16-byte aligned), resp_ptr [max_keypoints] i64 or
        None; returns (n, n_found).  Rows at and beyond n keep what they held."""
        n, found = C.c_int64(), C.c_int64()
        self._ck(self.L.dlco_desc_detect_device(self.h, n_octaves, threshold, max_keypoints, C.c_void_p(kp_ptr), C.c_void_p(resp_ptr),
                                                C.byref(n), C.byref(found)))
        return n.value, found.value

    def detect_stage_ms(self):
        """Kernel milliseconds of the last detect call: {"integral": (0 when cached), "octaves": [4], "selection":}."""
        ms = (C.c_double * 6)()
        self._ck(self.L.dlco_desc_detect_stage_ms(self.h, ms))
        return {"integral": ms[0], "octaves": [ms[1], ms[2], ms[3], ms[4]], "selection": ms[5]}

    def pair_sqdists(self, patches, pairs):
        """Per pair ||y_a - y_b||^2 [n_pairs] f32 and labels [n_pairs] u8; the descriptors stay on the device."""
        p, q = np.ascontiguousarray(patches, np.uint8), _i32(pairs)
        assert p.ndim == 3 and p.shape[1:] == (64, 64) and q.ndim == 2 and q.shape[1] == 4
        dist = np.empty(q.shape[0], np.float32)
        lab = np.empty(q.shape[0], np.uint8)
        self._ck(self.L.dlco_desc_pair_sqdists(self.h, _p(p, u8p), p.shape[0], _p(q, i32p), q.shape[0], _p(dist, f32p), _p(lab, u8p)))
        return dist, lab

    def pair_stats(self, patches, pairs):
        """(dim, fpr95, auc) of the projected distances of a raw patch-pair set (ComputePJStats semantics)."""
        p, q = np.ascontiguousarray(patches, np.uint8), _i32(pairs)
        assert p.ndim == 3 and p.shape[1:] == (64, 64) and q.ndim == 2 and q.shape[1] == 4
        dim, f, a = C.c_int32(), C.c_float(), C.c_double()
        self._ck(self.L.dlco_desc_pair_stats(self.h, _p(p, u8p), p.shape[0], _p(q, i32p), q.shape[0], C.byref(dim), C.byref(f), C.byref(a)))
        return dim.value, f.value, a.value

    # ---- matching two descriptor tables.  The matcher's call shapes, one helper each: `line` is _FLOAT or _BYTE, `name` the C
    # function without dlco_desc_ and without the line's suffix; the public methods below forward to them ----
    def _fn(self, line, name, device=False):
        return getattr(self.L, "dlco_desc_" + name + line.suffix + ("_device" if device else ""))

    @staticmethod
    def _tables(line, query, train):
        q, t = np.ascontiguousarray(query, line.dtype), np.ascontiguousarray(train, line.dtype)
        assert q.ndim == 2 and t.ndim == 2 and q.shape[1] == t.shape[1]
        return q, t

    def _top2(self, line, name, query, train):
        q, t = self._tables(line, query, train)
        idx, d = np.empty((q.shape[0], 2), np.int32), np.empty((q.shape[0], 2), line.dist)
        self._ck(self._fn(line, name)(self.h, _p(q, line.ptr), q.shape[0], _p(t, line.ptr), t.shape[0], q.shape[1], _p(idx, i32p), _p(d, line.dptr)))
        return idx, d

    def _matrix(self, line, name, query, train):
        q, t = self._tables(line, query, train)
        out = np.empty((q.shape[0], t.shape[0]), line.dist)
        self._ck(self._fn(line, name)(self.h, _p(q, line.ptr), q.shape[0], _p(t, line.ptr), t.shape[0], q.shape[1], _p(out, line.dptr)))
        return out

    def _on_device(self, line, name, q_ptr, nq, t_ptr, nt, r, idx_ptr, d_ptr, ldq, ldt):
        self._ck(self._fn(line, name, True)(self.h, C.c_void_p(q_ptr), ldq or r, nq, C.c_void_p(t_ptr), ldt or r, nt, r, C.c_void_p(idx_ptr),
                                            C.c_void_p(d_ptr)))

    def _guided_tables(self, line, query, query_xy, train, train_xy, M):
        q, t = self._tables(line, query, train)
        qxy, txy = _f32(query_xy), _f32(train_xy)
        assert qxy.shape == (q.shape[0], 2) and txy.shape == (t.shape[0], 2)
        return q, qxy, t, txy, self._model(M)

    @staticmethod
    def _model(M):
        m = np.ascontiguousarray(M, np.float64)
        assert m.size == 9
        return m

    def _top2_guided(self, line, name, query, query_xy, train, train_xy, M, radius, side):
        q, qxy, t, txy, m = self._guided_tables(line, query, query_xy, train, train_xy, M)
        idx, d = np.empty((q.shape[0], 2), np.int32), np.empty((q.shape[0], 2), line.dist)
        self._ck(self._fn(line, name)(self.h, _p(q, line.ptr), _p(qxy, f32p), q.shape[0], _p(t, line.ptr), _p(txy, f32p), t.shape[0], q.shape[1],
                                      _p(m, f64p), radius, side, _p(idx, i32p), _p(d, line.dptr)))
        return idx, d

    def _matrix_guided(self, line, name, query, query_xy, train, train_xy, M, radius, side):
        q, qxy, t, txy, m = self._guided_tables(line, query, query_xy, train, train_xy, M)
        out = np.empty((q.shape[0], t.shape[0]), line.dist)
        self._ck(self._fn(line, name)(self.h, _p(q, line.ptr), _p(qxy, f32p), q.shape[0], _p(t, line.ptr), _p(txy, f32p), t.shape[0], q.shape[1],
                                      _p(m, f64p), radius, side, _p(out, line.dptr)))
        return out

    def _on_device_guided(self, line, name, q_ptr, qxy_ptr, nq, t_ptr, txy_ptr, nt, r, M, idx_ptr, d_ptr, radius, side, ldq, ldt, ldxy_q, ldxy_t):
        self._ck(self._fn(line, name, True)(self.h, C.c_void_p(q_ptr), ldq or r, C.c_void_p(qxy_ptr), ldxy_q, nq, C.c_void_p(t_ptr), ldt or r,
                                            C.c_void_p(txy_ptr), ldxy_t, nt, r, _p(self._model(M), f64p), radius, side, C.c_void_p(idx_ptr),
                                            C.c_void_p(d_ptr)))

    def match(self, query, train):
        """For every row of query [nq, r] the nearest and second-nearest row of train [nt, r]: (idx [nq,2] int32,
        sqdist [nq,2] float32), ordered by (distance, index); nt == 1 gives -1 / +inf in column 1."""
        return self._top2(_FLOAT, "match", query, train)

    # ---- verifying a match list against a homography (csrc/verify_rules.hpp states the rule) ----
    @staticmethod
    def _match_points(src, dst):
        s, d = _f32(src), _f32(dst)
        assert s.ndim == 2 and s.shape[1] == 2 and d.shape == s.shape
        return s, d

    def _verify_model(self, call, src, dst, threshold, n_hyp, seed, refine):
        """call is dlco_desc_verify_homography or dlco_desc_verify_fundamental: (M [3,3], inlier [m] bool, best_hyp)."""
        s, d = self._match_points(src, dst)
        m = s.shape[0]
        M, mask = np.zeros((3, 3), np.float64), np.zeros(m, np.uint8)
        n, best = C.c_int64(), C.c_int32()
        self._ck(call(self.h, _p(s, f32p), _p(d, f32p), m, threshold, n_hyp, seed, refine, _p(M, C.POINTER(C.c_double)), _p(mask, u8p),
                      C.byref(n), C.byref(best)))
        assert n.value == int(mask.sum())
        return M, mask.astype(bool), best.value

    def _verify_hypotheses(self, call, src, dst, threshold, n_hyp, seed):
        """call is dlco_desc_verify_hypotheses or dlco_desc_verify_fundamental_hypotheses: (M_all [n_hyp,3,3], count [n_hyp])."""
        s, d = self._match_points(src, dst)
        M_all, count = np.zeros((n_hyp, 3, 3), np.float64), np.zeros(n_hyp, np.int32)
        self._ck(call(self.h, _p(s, f32p), _p(d, f32p), s.shape[0], threshold, n_hyp, seed, _p(M_all, C.POINTER(C.c_double)), _p(count, i32p)))
        return M_all, count

    def verify_homography(self, src, dst, threshold=3.0, n_hyp=2048, seed=0, refine=2):
        """The homography of the matches src [m,2] -> dst [m,2] by the library's deterministic RANSAC: (H [3,3] f64 with
        max |H| in [1, 2), inlier [m] bool, best_hyp).  No model: H and inlier all zero, best_hyp = -1."""
        return self._verify_model(self.L.dlco_desc_verify_homography, src, dst, threshold, n_hyp, seed, refine)

    def verify_hypotheses(self, src, dst, threshold=3.0, n_hyp=2048, seed=0):
        """Every hypothesis of verify_homography and its inlier count: (H_all [n_hyp,3,3] f64, all zero where invalid,
        count [n_hyp] int32)."""
        return self._verify_hypotheses(self.L.dlco_desc_verify_hypotheses, src, dst, threshold, n_hyp, seed)

    # ---- the same against a fundamental matrix (csrc/epipolar_rules.hpp states the rule) ----
    def verify_fundamental(self, src, dst, threshold=1.0, n_hyp=2048, seed=0, refine=2):
        """The fundamental matrix F, dst^T F src = 0, of the matches src [m,2] -> dst [m,2] (m >= 8) by the library's
        deterministic eight-point RANSAC: (F [3,3] f64 with max |F| in [1, 2), inlier [m] bool, best_hyp).  F is of rank 2 up to
        rounding once a refit round was accepted, the linear eight-point hypothesis otherwise.  No model: F and inlier all
        zero, best_hyp = -1."""
        return self._verify_model(self.L.dlco_desc_verify_fundamental, src, dst, threshold, n_hyp, seed, refine)

    def verify_fundamental_hypotheses(self, src, dst, threshold=1.0, n_hyp=2048, seed=0):
        """Every hypothesis of verify_fundamental and its inlier count: (F_all [n_hyp,3,3] f64, all zero where invalid,
        count [n_hyp] int32)."""
        return self._verify_hypotheses(self.L.dlco_desc_verify_fundamental_hypotheses, src, dst, threshold, n_hyp, seed)

    # ---- verifying many pairs in one call: the lists as one list (csrc/verify_batch.hpp states the plan) ----
    def _match_lists(self, lists):
        """lists of (src [m,2], dst [m,2]), m >= 0, as one list: (src, dst [M + 1,2] with a row of padding, so that an empty
        list still has an address, moff [n_pairs + 1] int64)"""
        pts = [self._match_points(np.reshape(_f32(s), (-1, 2)), np.reshape(_f32(d), (-1, 2))) for s, d in lists]
        assert pts, "verify_pairs: no pair"
        moff = np.concatenate([[0], np.cumsum([len(s) for s, _ in pts])]).astype(np.int64)
        pad = [np.zeros((1, 2), np.float32)]
        return np.concatenate([s for s, _ in pts] + pad), np.concatenate([d for _, d in pts] + pad), moff

    def _verify_pairs_model(self, call, lists, threshold, n_hyp, seed, refine):
        s, d, moff = self._match_lists(lists)
        P = moff.size - 1
        M, mask = np.zeros((P, 3, 3), np.float64), np.zeros(max(int(moff[-1]), 1), np.uint8)
        n, best = np.zeros(P, np.int64), np.zeros(P, np.int32)
        self._ck(call(self.h, _p(s, f32p), _p(d, f32p), _p(moff, i64p), P, threshold, n_hyp, seed, refine, _p(M, C.POINTER(C.c_double)), _p(mask, u8p),
                      _p(n, i64p), _p(best, i32p)))
        out = [(M[p], mask[moff[p]:moff[p + 1]].astype(bool), int(best[p])) for p in range(P)]
        assert all(int(o[1].sum()) == n[p] for p, o in enumerate(out))
        return out

    def _verify_pairs_hypotheses(self, call, lists, threshold, n_hyp, seed):
        s, d, moff = self._match_lists(lists)
        P = moff.size - 1
        M_all, count = np.zeros((P, n_hyp, 3, 3), np.float64), np.zeros((P, n_hyp), np.int32)
        self._ck(call(self.h, _p(s, f32p), _p(d, f32p), _p(moff, i64p), P, threshold, n_hyp, seed, _p(M_all, C.POINTER(C.c_double)), _p(count, i32p)))
        return M_all, count

    def verify_pairs_homography(self, lists, threshold=3.0, n_hyp=2048, seed=0, refine=2):
        """verify_homography for a list of (src [m,2], dst [m,2]) in one call: a list of (H [3,3], inlier [m] bool, best_hyp),
        each what verify_homography returns for its pair, byte for byte.  A pair of fewer than 4 matches (0 is allowed) gets
        "no model": zeros and best_hyp = -1."""
        return self._verify_pairs_model(self.L.dlco_desc_verify_pairs_homography, lists, threshold, n_hyp, seed, refine)

    def verify_pairs_fundamental(self, lists, threshold=1.0, n_hyp=2048, seed=0, refine=2):
        """verify_fundamental for a list of (src, dst) in one call; a pair of fewer than 8 matches gets "no model"."""
        return self._verify_pairs_model(self.L.dlco_desc_verify_pairs_fundamental, lists, threshold, n_hyp, seed, refine)

    def verify_pairs_hypotheses(self, lists, threshold=3.0, n_hyp=2048, seed=0):
        """Every hypothesis of verify_pairs_homography and its count: (H_all [n_pairs,n_hyp,3,3] f64, count [n_pairs,n_hyp]
        int32), all zero for a pair of fewer than 4 matches."""
        return self._verify_pairs_hypotheses(self.L.dlco_desc_verify_pairs_hypotheses, lists, threshold, n_hyp, seed)

    def verify_pairs_fundamental_hypotheses(self, lists, threshold=1.0, n_hyp=2048, seed=0):
        """Every hypothesis of verify_pairs_fundamental and its count, all zero for a pair of fewer than 8 matches."""
        return self._verify_pairs_hypotheses(self.L.dlco_desc_verify_pairs_fundamental_hypotheses, lists, threshold, n_hyp, seed)

    def _verify_pairs_device(self, call, src_ptr, dst_ptr, moff, threshold, n_hyp, seed, refine, inlier_ptr):
        o = np.ascontiguousarray(moff, np.int64)
        assert o.ndim == 1 and o.size >= 2
        P = o.size - 1
        M, n, best = np.zeros((P, 3, 3), np.float64), np.zeros(P, np.int64), np.zeros(P, np.int32)
        self._ck(call(self.h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), _p(o, i64p), P, threshold, n_hyp, seed, refine, _p(M, C.POINTER(C.c_double)),
                      None if inlier_ptr is None else C.c_void_p(inlier_ptr), _p(n, i64p), _p(best, i32p)))
        return M, n, best

    def verify_pairs_homography_device(self, src_ptr, dst_ptr, moff, threshold=3.0, n_hyp=2048, seed=0, refine=2, inlier_ptr=None):
        """verify_pairs_homography on lists in device memory, src / dst [moff[-1], 2] float32 (8-byte aligned) as
        select_pairs_device wrote them and moff [n_pairs + 1] as it returned it, with the refit rounds on the device:
        (H [n_pairs, 3, 3], n_inliers [n_pairs] int64, best_hyp [n_pairs] int32) on the host, the mask [moff[-1]] uint8 to the
        device pointer inlier_ptr (None: no mask).  Every pair is byte for byte what verify_pairs_homography returns."""
        return self._verify_pairs_device(self.L.dlco_desc_verify_pairs_homography_device, src_ptr, dst_ptr, moff, threshold, n_hyp, seed, refine, inlier_ptr)

    def verify_pairs_fundamental_device(self, src_ptr, dst_ptr, moff, threshold=1.0, n_hyp=2048, seed=0, refine=2, inlier_ptr=None):
        """verify_pairs_fundamental on lists in device memory, as verify_pairs_homography_device."""
        return self._verify_pairs_device(self.L.dlco_desc_verify_pairs_fundamental_device, src_ptr, dst_ptr, moff, threshold, n_hyp, seed, refine, inlier_ptr)

    def verify_pairs_refit_round(self, lists, masks, fundamental=False):
        """One round of the refit kernel for a list of (src [m,2], dst [m,2]) under the caller's masks, a list of [m] bool:
        (M [n_pairs, 3, 3] f64, ok [n_pairs] bool); a rejected round and a pair below the sample give ok = False and zeros.
        For tests and tools."""
        s, d, moff = self._match_lists(lists)
        assert len(masks) == len(lists) and all(len(k) == len(l[0]) for k, l in zip(masks, lists))
        mk = np.ascontiguousarray(np.concatenate([np.asarray(k, bool).astype(np.uint8) for k in masks] + [np.zeros(1, np.uint8)]))
        P = moff.size - 1
        M, ok = np.zeros((P, 3, 3), np.float64), np.zeros(P, np.uint8)
        self._ck(self.L.dlco_desc_verify_pairs_refit_round(self.h, _p(s, f32p), _p(d, f32p), _p(moff, i64p), P, _p(mk, u8p), 1 if fundamental else 0,
                                                           _p(M, C.POINTER(C.c_double)), _p(ok, u8p)))
        return M, ok.astype(bool)

    def match_device(self, q_ptr, nq, t_ptr, nt, r, idx_ptr, d_ptr, ldq=None, ldt=None):
        """match on tables in device memory (row pitches ldq, ldt: multiples of 4, default r); results to device memory."""
        self._on_device(_FLOAT, "match", q_ptr, nq, t_ptr, nt, r, idx_ptr, d_ptr, ldq, ldt)

    def cross_sqdists(self, query, train):
        """The whole matrix [nq, nt] float32 of the distances match orders (nq * nt <= 2^28)."""
        return self._matrix(_FLOAT, "cross_sqdists", query, train)

    # ---- guided matching: the nearest two among the rows a homography admits (csrc/guided_rules.hpp states the rule) ----
    def match_guided(self, query, query_xy, train, train_xy, H, radius=6.0, h_side=0):
        """match among the rows of train the homography H [3,3] admits for a query: those whose keypoint train_xy [nt,2] lies
        within radius pixels of H applied to the query's query_xy [nq,2] (h_side=0: H maps the query image to the train
        image; h_side=1: H maps the train image to the query image, the call of a mutual check with the tables swapped).
        (idx [nq,2] int32, sqdist [nq,2] float32); fewer than two admitted rows leave -1 / +inf."""
        return self._top2_guided(_FLOAT, "match_guided", query, query_xy, train, train_xy, H, radius, h_side)

    def match_guided_device(self, q_ptr, qxy_ptr, nq, t_ptr, txy_ptr, nt, r, H, idx_ptr, d_ptr, radius=6.0, h_side=0, ldq=None,
                            ldt=None, ldxy_q=2, ldxy_t=2):
        """match_guided on tables in device memory (row pitches ldq, ldt: multiples of 4, default r; coordinate pitches in
        floats, >= 2: 4 takes the keypoint rows detect_device wrote); results to device memory."""
        self._on_device_guided(_FLOAT, "match_guided", q_ptr, qxy_ptr, nq, t_ptr, txy_ptr, nt, r, H, idx_ptr, d_ptr, radius, h_side, ldq, ldt,
                               ldxy_q, ldxy_t)

    def cross_sqdists_guided(self, query, query_xy, train, train_xy, H, radius=6.0, h_side=0):
        """cross_sqdists with +inf where H does not admit the pair: match_guided is the top two of its finite entries."""
        return self._matrix_guided(_FLOAT, "cross_sqdists_guided", query, query_xy, train, train_xy, H, radius, h_side)

    # ---- guided matching under a fundamental matrix (csrc/guided_epipolar_rules.hpp states the rule) ----
    def match_guided_epipolar(self, query, query_xy, train, train_xy, F, threshold=3.0, f_side=0):
        """match among the rows of train the fundamental matrix F [3,3] admits for a query: those whose keypoint and the
        query's have a Sampson error within threshold pixels, the inlier test of verify_fundamental (f_side=0: the query image
        is src, F as verify_fundamental(query keypoints, train keypoints) returns it; f_side=1: the train image is src, the
        call of a mutual check with the tables swapped).  (idx [nq,2] int32, sqdist [nq,2] float32); fewer than two admitted
        rows leave -1 / +inf."""
        return self._top2_guided(_FLOAT, "match_guided_epipolar", query, query_xy, train, train_xy, F, threshold, f_side)

    def match_guided_epipolar_device(self, q_ptr, qxy_ptr, nq, t_ptr, txy_ptr, nt, r, F, idx_ptr, d_ptr, threshold=3.0, f_side=0,
                                     ldq=None, ldt=None, ldxy_q=2, ldxy_t=2):
        """match_guided_epipolar on tables in device memory, pitches as match_guided_device; results to device memory."""
        self._on_device_guided(_FLOAT, "match_guided_epipolar", q_ptr, qxy_ptr, nq, t_ptr, txy_ptr, nt, r, F, idx_ptr, d_ptr, threshold, f_side,
                               ldq, ldt, ldxy_q, ldxy_t)

    def cross_sqdists_guided_epipolar(self, query, query_xy, train, train_xy, F, threshold=3.0, f_side=0):
        """cross_sqdists with +inf where F does not admit the pair: match_guided_epipolar is the top two of its finite entries."""
        return self._matrix_guided(_FLOAT, "cross_sqdists_guided_epipolar", query, query_xy, train, train_xy, F, threshold, f_side)

    # ---- eight-bit descriptors: rows quantised on the device, byte tables matched with exact integer distances ----
    def set_quantizer(self, scale, offset=None, r=None):
        """The quantiser of the _u8 calls (quant_fit gives one); offset None = zeros, then r says how wide."""
        off = None if offset is None else _f32(offset).ravel()
        self._ck(self.L.dlco_desc_set_quantizer(self.h, scale, _p(off, f32p), off.size if off is not None else (r or self.projected_size)))

    def describe_u8(self, patches):
        """quantize(describe(patches)) [n, r] uint8, quantised on the device."""
        p = np.ascontiguousarray(patches, np.uint8)
        assert p.ndim == 3 and p.shape[1:] == (64, 64)
        out = np.empty((p.shape[0], self.projected_size), np.uint8)
        self._ck(self.L.dlco_desc_describe_u8(self.h, _p(p, u8p), p.shape[0], _p(out, u8p)))
        return out

    def describe_u8_device(self, patches, dev_ptr, ld=None):
        p = np.ascontiguousarray(patches, np.uint8)
        assert p.ndim == 3 and p.shape[1:] == (64, 64)
        self._ck(self.L.dlco_desc_describe_u8_device(self.h, _p(p, u8p), p.shape[0], C.c_void_p(dev_ptr), ld or self.projected_size))

    def describe_keypoints_u8(self, kp, scale_factor=6.25, use_orientation=True):
        """(bytes [n, r], status [n]): quantize(describe_keypoints(kp)); a status-0 row is the quantised zero vector."""
        k = self._keypoints(kp)
        out, status = np.empty((k.shape[0], self.projected_size), np.uint8), np.empty(k.shape[0], np.uint8)
        self._ck(self.L.dlco_desc_describe_keypoints_u8(self.h, _p(k, f32p), k.shape[0], scale_factor, 1 if use_orientation else 0,
                                                        _p(out, u8p), _p(status, u8p)))
        return out, status

    def describe_keypoints_u8_device(self, kp, dev_ptr, ld=None, scale_factor=6.25, use_orientation=True):
        """The same rows into device memory at dev_ptr, row pitch ld bytes; returns status [n]."""
        k = self._keypoints(kp)
        status = np.empty(k.shape[0], np.uint8)
        self._ck(self.L.dlco_desc_describe_keypoints_u8_device(self.h, _p(k, f32p), k.shape[0], scale_factor, 1 if use_orientation else 0,
                                                               C.c_void_p(dev_ptr), ld or self.projected_size, _p(status, u8p)))
        return status

    def match_u8(self, query, train):
        """match on byte tables [nq, r] / [nt, r] uint8: (idx [nq,2] int32, sqdist [nq,2] int32), exact integer distances
        ordered by (distance, index); nt == 1 gives -1 / INT32_MAX in column 1."""
        return self._top2(_BYTE, "match", query, train)

    def match_u8_device(self, q_ptr, nq, t_ptr, nt, r, idx_ptr, d_ptr, ldq=None, ldt=None):
        """match_u8 on tables in device memory (row pitches ldq, ldt in bytes: multiples of 16); results to device memory."""
        self._on_device(_BYTE, "match", q_ptr, nq, t_ptr, nt, r, idx_ptr, d_ptr, ldq, ldt)

    def cross_sqdists_u8(self, query, train):
        """The whole matrix [nq, nt] int32 of the distances match_u8 orders (nq * nt <= 2^28)."""
        return self._matrix(_BYTE, "cross_sqdists", query, train)

    # ---- guided matching on byte tables: the float guided calls argument for argument, integer distances ----
    def match_guided_u8(self, query, query_xy, train, train_xy, H, radius=6.0, h_side=0):
        """match_guided on byte tables [n, r] uint8: the first two rows of match_u8's (d, index) order among those the homography
        admits.  (idx [nq,2] int32, sqdist [nq,2] int32); fewer than two admitted rows leave -1 / INT32_MAX."""
        return self._top2_guided(_BYTE, "match_guided", query, query_xy, train, train_xy, H, radius, h_side)

    def match_guided_u8_device(self, q_ptr, qxy_ptr, nq, t_ptr, txy_ptr, nt, r, H, idx_ptr, d_ptr, radius=6.0, h_side=0, ldq=None,
                               ldt=None, ldxy_q=2, ldxy_t=2):
        """match_guided_u8 on tables in device memory (row pitches ldq, ldt in bytes: multiples of 16; coordinate pitches in
        floats, >= 2); results to device memory."""
        self._on_device_guided(_BYTE, "match_guided", q_ptr, qxy_ptr, nq, t_ptr, txy_ptr, nt, r, H, idx_ptr, d_ptr, radius, h_side, ldq, ldt,
                               ldxy_q, ldxy_t)

    def cross_sqdists_guided_u8(self, query, query_xy, train, train_xy, H, radius=6.0, h_side=0):
        """cross_sqdists_u8 with INT32_MAX where H does not admit the pair: match_guided_u8 is the top two of the entries below it."""
        return self._matrix_guided(_BYTE, "cross_sqdists_guided", query, query_xy, train, train_xy, H, radius, h_side)

    def match_guided_epipolar_u8(self, query, query_xy, train, train_xy, F, threshold=3.0, f_side=0):
        """match_guided_epipolar on byte tables: (idx [nq,2] int32, sqdist [nq,2] int32), -1 / INT32_MAX in free columns."""
        return self._top2_guided(_BYTE, "match_guided_epipolar", query, query_xy, train, train_xy, F, threshold, f_side)

    def match_guided_epipolar_u8_device(self, q_ptr, qxy_ptr, nq, t_ptr, txy_ptr, nt, r, F, idx_ptr, d_ptr, threshold=3.0, f_side=0,
                                        ldq=None, ldt=None, ldxy_q=2, ldxy_t=2):
        """match_guided_epipolar_u8 on tables in device memory, pitches as match_guided_u8_device."""
        self._on_device_guided(_BYTE, "match_guided_epipolar", q_ptr, qxy_ptr, nq, t_ptr, txy_ptr, nt, r, F, idx_ptr, d_ptr, threshold, f_side,
                               ldq, ldt, ldxy_q, ldxy_t)

    def cross_sqdists_guided_epipolar_u8(self, query, query_xy, train, train_xy, F, threshold=3.0, f_side=0):
        """cross_sqdists_u8 with INT32_MAX where F does not admit the pair."""
        return self._matrix_guided(_BYTE, "cross_sqdists_guided_epipolar", query, query_xy, train, train_xy, F, threshold, f_side)

    # ---- matching many pairs of images in one call (csrc/match_batch.hpp states the plan) ----
    @staticmethod
    def _batch(line, tables, pairs):
        """the images as one table: (table, seg, pairs, row0) as the match_pairs calls take them"""
        tabs = [np.ascontiguousarray(t, line.dtype) for t in tables]
        assert tabs and all(t.ndim == 2 and t.shape[1] == tabs[0].shape[1] for t in tabs)
        seg = np.concatenate([[0], np.cumsum([t.shape[0] for t in tabs])]).astype(np.int64)
        seg, q = _seg_pairs(seg, pairs)
        return np.ascontiguousarray(np.concatenate(tabs, axis=0)), seg, q, match_pairs_rows(seg, q)

    def _match_pairs(self, line, name, tables, pairs):
        table, seg, q, row0 = self._batch(line, tables, pairs)
        idx, d = np.empty((row0[-1], 2), np.int32), np.empty((row0[-1], 2), line.dist)
        self._ck(self._fn(line, name)(self.h, _p(table, line.ptr), _p(seg, i64p), seg.size - 1, _p(q, i32p), q.shape[0], table.shape[1],
                                      _p(idx, i32p), _p(d, line.dptr)))
        return [(idx[row0[p]:row0[p + 1]], d[row0[p]:row0[p + 1]]) for p in range(q.shape[0])]

    def _match_pairs_device(self, line, name, table_ptr, seg, pairs, r, idx_ptr, d_ptr, ld):
        s, q = _seg_pairs(seg, pairs)
        self._ck(self._fn(line, name, True)(self.h, C.c_void_p(table_ptr), ld or r, _p(s, i64p), s.size - 1, _p(q, i32p), q.shape[0], r,
                                            C.c_void_p(idx_ptr), C.c_void_p(d_ptr)))

    def match_pairs(self, tables, pairs):
        """Many pairs of images in one call: tables is a list of [n_s, r] arrays (an image may have no rows), pairs [n_pairs, 2]
        of (query image, train image).  Returns a list of (idx [n_a, 2] int32, sqdist [n_a, 2] float32), one per pair, each
        byte for byte what match(tables[a], tables[b]) returns; an empty train image gives -1 / +inf in both columns."""
        return self._match_pairs(_FLOAT, "match_pairs", tables, pairs)

    def match_pairs_u8(self, tables, pairs):
        """match_pairs on byte tables: every pair is what match_u8 returns for it; an empty train image gives -1 / INT32_MAX."""
        return self._match_pairs(_BYTE, "match_pairs", tables, pairs)

    def match_pairs_device(self, table_ptr, seg, pairs, r, idx_ptr, d_ptr, ld=None):
        """match_pairs on one table in device memory (row pitch ld floats, a multiple of 4, default r) whose segments seg
        [n_img + 1] are the images; results [match_pairs_rows(seg, pairs)[-1], 2] to device memory."""
        self._match_pairs_device(_FLOAT, "match_pairs", table_ptr, seg, pairs, r, idx_ptr, d_ptr, ld)

    def match_pairs_u8_device(self, table_ptr, seg, pairs, r, idx_ptr, d_ptr, ld=None):
        """match_pairs_u8 on one table in device memory (row pitch ld bytes, a multiple of 16)."""
        self._match_pairs_device(_BYTE, "match_pairs", table_ptr, seg, pairs, r, idx_ptr, d_ptr, ld)

    # ---- guided matching of many pairs in one call: a matrix per pair (csrc/match_batch.hpp states the plan) ----
    def _match_pairs_guided(self, line, name, tables, xys, pairs, M, radius, side):
        table, seg, q, row0 = self._batch(line, tables, pairs)
        cs = [_f32(x) for x in xys]
        assert len(cs) == seg.size - 1 and all(x.shape == (n, 2) for x, n in zip(cs, np.diff(seg)))
        m = np.ascontiguousarray(M, np.float64).reshape(-1, 9)
        assert m.shape[0] == q.shape[0]
        xy = np.ascontiguousarray(np.concatenate(cs, axis=0))
        idx, d = np.empty((row0[-1], 2), np.int32), np.empty((row0[-1], 2), line.dist)
        self._ck(self._fn(line, name)(self.h, _p(table, line.ptr), _p(xy, f32p), _p(seg, i64p), seg.size - 1, _p(q, i32p), q.shape[0],
                                      table.shape[1], _p(m, f64p), radius, side, _p(idx, i32p), _p(d, line.dptr)))
        return [(idx[row0[p]:row0[p + 1]], d[row0[p]:row0[p + 1]]) for p in range(q.shape[0])]

    def match_pairs_guided(self, tables, xys, pairs, H, radius=6.0, h_side=0):
        """match_pairs under a homography per pair: tables and pairs as match_pairs takes them, xys a list of [n_s, 2] keypoint
        coordinates, one per table, H [n_pairs, 3, 3] (or [n_pairs, 9]) as verify_pairs_homography returns it.  Returns a list of
        (idx, sqdist), one per pair, each byte for byte what match_guided(tables[a], xys[a], tables[b], xys[b], H[p], radius,
        h_side) returns; an all-zero H[p] ("no model") or an empty train image gives -1 / +inf in both columns."""
        return self._match_pairs_guided(_FLOAT, "match_pairs_guided", tables, xys, pairs, H, radius, h_side)

    def match_pairs_guided_epipolar(self, tables, xys, pairs, F, threshold=3.0, f_side=0):
        """match_pairs under a fundamental matrix per pair: every pair is what match_guided_epipolar returns for it."""
        return self._match_pairs_guided(_FLOAT, "match_pairs_guided_epipolar", tables, xys, pairs, F, threshold, f_side)

    def _match_pairs_guided_device(self, line, name, table_ptr, xy_ptr, seg, pairs, r, M, idx_ptr, d_ptr, radius, side, ld, ldxy):
        s, q = _seg_pairs(seg, pairs)
        m = np.ascontiguousarray(M, np.float64).reshape(-1, 9)
        assert m.shape[0] == q.shape[0]
        self._ck(self._fn(line, name, True)(self.h, C.c_void_p(table_ptr), ld or r, C.c_void_p(xy_ptr), ldxy, _p(s, i64p), s.size - 1, _p(q, i32p),
                                            q.shape[0], r, _p(m, f64p), radius, side, C.c_void_p(idx_ptr), C.c_void_p(d_ptr)))

    def match_pairs_guided_device(self, table_ptr, xy_ptr, seg, pairs, r, H, idx_ptr, d_ptr, radius=6.0, h_side=0, ld=None, ldxy=2):
        """match_pairs_guided on one table in device memory (row pitch ld floats, default r) and one coordinate table with the
        same rows (pitch ldxy floats >= 2: 4 takes the keypoint rows detect_device wrote); H on the host; results
        [match_pairs_rows(seg, pairs)[-1], 2] to device memory."""
        self._match_pairs_guided_device(_FLOAT, "match_pairs_guided", table_ptr, xy_ptr, seg, pairs, r, H, idx_ptr, d_ptr, radius, h_side, ld, ldxy)

    def match_pairs_guided_epipolar_device(self, table_ptr, xy_ptr, seg, pairs, r, F, idx_ptr, d_ptr, threshold=3.0, f_side=0, ld=None, ldxy=2):
        """match_pairs_guided_epipolar on tables in device memory, pitches as match_pairs_guided_device."""
        self._match_pairs_guided_device(_FLOAT, "match_pairs_guided_epipolar", table_ptr, xy_ptr, seg, pairs, r, F, idx_ptr, d_ptr, threshold, f_side,
                                        ld, ldxy)

    def match_pairs_guided_u8(self, tables, xys, pairs, H, radius=6.0, h_side=0):
        """match_pairs_guided on byte tables: every pair is byte for byte what match_guided_u8 returns for it with H[p]; an
        all-zero H[p] or an empty train image gives -1 / INT32_MAX in both columns."""
        return self._match_pairs_guided(_BYTE, "match_pairs_guided", tables, xys, pairs, H, radius, h_side)

    def match_pairs_guided_epipolar_u8(self, tables, xys, pairs, F, threshold=3.0, f_side=0):
        """match_pairs_guided_epipolar on byte tables: every pair is what match_guided_epipolar_u8 returns for it."""
        return self._match_pairs_guided(_BYTE, "match_pairs_guided_epipolar", tables, xys, pairs, F, threshold, f_side)

    def match_pairs_guided_u8_device(self, table_ptr, xy_ptr, seg, pairs, r, H, idx_ptr, d_ptr, radius=6.0, h_side=0, ld=None, ldxy=2):
        """match_pairs_guided_u8 on one table in device memory (row pitch ld bytes, a multiple of 16) and one coordinate table
        (pitch ldxy floats >= 2); H on the host; results to device memory."""
        self._match_pairs_guided_device(_BYTE, "match_pairs_guided", table_ptr, xy_ptr, seg, pairs, r, H, idx_ptr, d_ptr, radius, h_side, ld, ldxy)

    def match_pairs_guided_epipolar_u8_device(self, table_ptr, xy_ptr, seg, pairs, r, F, idx_ptr, d_ptr, threshold=3.0, f_side=0, ld=None,
                                              ldxy=2):
        """match_pairs_guided_epipolar_u8 on tables in device memory, pitches as match_pairs_guided_u8_device."""
        self._match_pairs_guided_device(_BYTE, "match_pairs_guided_epipolar", table_ptr, xy_ptr, seg, pairs, r, F, idx_ptr, d_ptr, threshold, f_side,
                                        ld, ldxy)

    # ---- selecting matches: from the answer of match_pairs to the lists of verify_pairs (csrc/select_rules.hpp states the rule) ----
    @staticmethod
    def _select_seg(answers, sizes_or_seg, q):
        """seg [n_img + 1] from the row counts of the images [n_img] or from seg itself, whichever fits the answers: pair
        (a, b)'s answer has as many rows as image a.  Row counts are tried first."""
        s = np.ascontiguousarray(sizes_or_seg, np.int64)
        assert s.ndim == 1 and s.size >= 1 and len(answers) == q.shape[0]
        rows = np.array([len(a[0]) for a in answers], np.int64)
        fits = lambda n: q.size > 0 and q.min() >= 0 and q.max() < n.size and np.array_equal(n[q[:, 0]], rows)
        if fits(s):
            return np.concatenate([[0], np.cumsum(s)]).astype(np.int64)
        assert s.size >= 2 and s[0] == 0 and fits(np.diff(s)), "select_pairs: neither the row counts nor seg of these answers"
        return s

    def _select_pairs(self, line, answers, sizes_or_seg, pairs, ratio, back, xys):
        q = np.ascontiguousarray(pairs, np.int32)
        assert q.ndim == 2 and q.shape[1] == 2
        seg = self._select_seg(answers, sizes_or_seg, q)
        P, dist, dp = q.shape[0], line.dist, line.dptr
        stack = lambda ans, k, t: np.ascontiguousarray(np.concatenate([np.reshape(np.asarray(a[k], t), (-1, 2)) for a in ans] + [np.zeros((1, 2), t)]))
        idx, d = stack(answers, 0, np.int32), stack(answers, 1, dist)       # a row of padding: an empty answer still has an address
        row0 = match_pairs_rows(seg, q)
        R = int(row0[-1])
        bidx, brow0, nback = None, None, 0
        if back is not None:
            assert len(back) == P
            if all(b is None or isinstance(b, (int, np.integer)) for b in back):    # the same batch: back[p] names the pair that reverses p
                bidx, nback = idx, R
                brow0 = np.array([-1 if b is None or b < 0 else row0[int(b)] for b in back], np.int64)
            else:                                                           # a second answer list, None where a pair has none
                n = [0 if b is None else len(b[0]) for b in back]
                brow0 = np.concatenate([[0], np.cumsum(n)])[:-1].astype(np.int64)
                brow0[[b is None for b in back]] = -1
                bidx, nback = stack([b for b in back if b is not None], 0, np.int32), int(sum(n))
        xy = src = dst = None
        if xys is not None:
            assert len(xys) == seg.size - 1 and all(np.shape(x) == (seg[k + 1] - seg[k], 2) for k, x in enumerate(xys))
            xy = np.ascontiguousarray(np.concatenate([_f32(x).reshape(-1, 2) for x in xys] + [np.zeros((1, 2), np.float32)]))
            src, dst = np.empty((R + 1, 2), np.float32), np.empty((R + 1, 2), np.float32)
        moff, m, dd = np.empty(P + 1, np.int64), np.empty((R + 1, 2), np.int32), np.empty(R + 1, dist)
        self._ck(self._fn(line, "select_pairs")(self.h, _p(seg, i64p), seg.size - 1, _p(q, i32p), P, _p(idx, i32p), _p(d, dp), 0.0 if ratio is None else ratio,
                                                _p(bidx, i32p), _p(brow0, i64p), nback, _p(xy, f32p), _p(moff, i64p), _p(m, i32p), _p(dd, dp), _p(src, f32p),
                                                _p(dst, f32p)))
        sel = [(m[moff[p]:moff[p + 1]], dd[moff[p]:moff[p + 1]]) for p in range(P)]
        if xys is None:
            return sel
        return sel, [(src[moff[p]:moff[p + 1]], dst[moff[p]:moff[p + 1]]) for p in range(P)]

    def select_pairs(self, answers, sizes_or_seg, pairs, ratio=None, back=None, xys=None):
        """The matches of every pair of a match_pairs / match_pairs_guided* answer, selected on the device: answers is the list
        those calls return, sizes_or_seg the row counts of the images [n_img] (or seg [n_img + 1]), pairs as they took them.
        ratio (None: no ratio test, else in (0, 1]) is Lowe's test, idx2 == -1 or d1 < ratio^2 d2 in double; back asks for the
        mutual check: either a list of pair indices, back[p] the pair of this batch that reverses p (None or -1: no check for p),
        or a second answer list, back[p] the answer of (b, a) (None: no check for p).  Returns per pair (matches [m, 2] int32 of
        (query row, train row), dist [m] float32), rows ascending.  With xys, the list of [n_s, 2] keypoint coordinates of the
        images, returns (that list, lists), lists the per-pair (src [m, 2], dst [m, 2]) that verify_pairs_* take."""
        return self._select_pairs(_FLOAT, answers, sizes_or_seg, pairs, ratio, back, xys)

    def select_pairs_u8(self, answers, sizes_or_seg, pairs, ratio=None, back=None, xys=None):
        """select_pairs on the answers of the byte line (match_pairs_u8, match_pairs_guided*_u8): dist [m] int32."""
        return self._select_pairs(_BYTE, answers, sizes_or_seg, pairs, ratio, back, xys)

    def _select_pairs_device(self, line, idx_ptr, d_ptr, seg, pairs, matches_ptr, dist_ptr, ratio, back_idx_ptr, back_row0, n_back_rows, xy_ptr, ldxy,
                             src_ptr, dst_ptr):
        s, q = _seg_pairs(seg, pairs)
        b = None if back_row0 is None else np.ascontiguousarray(back_row0, np.int64)
        assert b is None or b.shape == (q.shape[0],)
        moff = np.empty(q.shape[0] + 1, np.int64)
        ptr = lambda a: None if a is None else C.c_void_p(a)
        self._ck(self._fn(line, "select_pairs", True)(self.h, _p(s, i64p), s.size - 1, _p(q, i32p), q.shape[0], ptr(idx_ptr), ptr(d_ptr),
                                                      0.0 if ratio is None else ratio, ptr(back_idx_ptr), _p(b, i64p), n_back_rows, ptr(xy_ptr), ldxy,
                                                      _p(moff, i64p), ptr(matches_ptr), ptr(dist_ptr), ptr(src_ptr), ptr(dst_ptr)))
        return moff

    def select_pairs_device(self, idx_ptr, d_ptr, seg, pairs, matches_ptr, dist_ptr, ratio=None, back_idx_ptr=None, back_row0=None, n_back_rows=0,
                            xy_ptr=None, ldxy=2, src_ptr=None, dst_ptr=None):
        """select_pairs on an answer in device memory, idx / sqdist [R, 2] as match_pairs_device wrote them for seg and pairs
        (R = match_pairs_rows(seg, pairs)[-1]).  back_idx_ptr [n_back_rows, 2] holds the reverse answers and back_row0 [n_pairs]
        the first row of every pair's (-1: no check); it may be idx_ptr itself.  xy_ptr is the coordinate table (pitch ldxy
        floats).  The lists go to device memory of R entries each: matches [., 2] int32, dist [.] float32, and with xy_ptr src,
        dst [., 2] float32.  Returns moff [n_pairs + 1] int64; the first moff[-1] entries are written."""
        return self._select_pairs_device(_FLOAT, idx_ptr, d_ptr, seg, pairs, matches_ptr, dist_ptr, ratio, back_idx_ptr,
                                         back_row0, n_back_rows, xy_ptr, ldxy, src_ptr, dst_ptr)

    def select_pairs_u8_device(self, idx_ptr, d_ptr, seg, pairs, matches_ptr, dist_ptr, ratio=None, back_idx_ptr=None, back_row0=None, n_back_rows=0,
                               xy_ptr=None, ldxy=2, src_ptr=None, dst_ptr=None):
        """select_pairs_device on the answer of match_pairs_u8_device: int32 distances in and out."""
        return self._select_pairs_device(_BYTE, idx_ptr, d_ptr, seg, pairs, matches_ptr, dist_ptr, ratio,
                                         back_idx_ptr, back_row0, n_back_rows, xy_ptr, ldxy, src_ptr, dst_ptr)

    # ---- building tracks: from the match lists and masks of many pairs to the keypoints that are one scene point (csrc/track_rules.hpp) ----
    @staticmethod
    def _tracks_seg(sizes_or_seg, q):
        """seg [n_img + 1] from seg itself or from the row counts of the images [n_img]: the array is seg when it starts at 0,
        never decreases and has an entry more than the images the pairs name need; pass seg where that could be in doubt."""
        s = np.ascontiguousarray(sizes_or_seg, np.int64)
        assert s.ndim == 1 and s.size >= 1
        n_named = int(q.max()) + 1 if q.size else 1
        if s.size >= n_named + 1 and s[0] == 0 and (np.diff(s) >= 0).all():
            return s
        return np.concatenate([[0], np.cumsum(s)]).astype(np.int64)

    def build_tracks(self, matches, moff, sizes_or_seg, pairs, keep=None, min_len=2, unique=True):
        """The tracks across the images of a batch: matches [M, 2] int32 of (query row, train row) and moff [n_pairs + 1] as
        select_pairs_device wrote them (or the per-pair lists select_pairs returns, concatenated), sizes_or_seg the row counts of
        the images [n_img] or seg [n_img + 1], pairs [n_pairs, 2], keep [M] the inlier mask of verify_pairs_* (None: every match
        counts).  A node is a row of the batch's table, seg[a] + i; a track is a connected component of at least min_len nodes
        and, with unique, without two nodes in one image.  Returns Tracks(toff, obs, track_of, label, counts, seg): tracks
        ascend in their smallest node, nodes ascend inside a track."""
        q = np.ascontiguousarray(pairs, np.int32)
        assert q.ndim == 2 and q.shape[1] == 2
        seg = self._tracks_seg(sizes_or_seg, q)
        o = np.ascontiguousarray(moff, np.int64)
        assert o.shape == (q.shape[0] + 1,)
        M, N = int(o[-1]) if o.size else 0, int(seg[-1])
        m = np.ascontiguousarray(np.concatenate([np.reshape(np.asarray(matches, np.int32), (-1, 2)), np.zeros((1, 2), np.int32)]))
        assert m.shape[0] == M + 1, "build_tracks: matches and moff disagree"
        k = None
        if keep is not None:
            k = np.ascontiguousarray(np.concatenate([np.reshape(np.asarray(keep), -1) != 0, [False]]).astype(np.uint8))
            assert k.size == M + 1, "build_tracks: keep and moff disagree"
        nt, counts = np.zeros(1, np.int64), np.zeros(3, np.int64)
        toff, obs, track_of, label = np.empty(N // 2 + 1, np.int64), np.empty(N + 1, np.int32), np.full(N + 1, -1, np.int32), np.empty(N + 1, np.int32)
        self._ck(self.L.dlco_desc_build_tracks(self.h, _p(seg, i64p), seg.size - 1, _p(q, i32p), q.shape[0], _p(o, i64p), _p(m, i32p), _p(k, u8p), min_len,
                                               1 if unique else 0, _p(nt, i64p), _p(toff, i64p), _p(obs, i32p), _p(track_of, i32p), _p(label, i32p),
                                               _p(counts, i64p)))
        T = int(nt[0])
        return Tracks(toff[:T + 1].copy(), obs[:toff[T]].copy(), track_of[:N], label[:N], counts, seg)

    def build_tracks_device(self, matches_ptr, moff, seg, pairs, toff_ptr, obs_ptr, track_of_ptr, keep_ptr=None, label_ptr=None, min_len=2, unique=True):
        """build_tracks on lists in device memory: matches [M, 2] int32 as select_pairs_device wrote them for seg and pairs, moff
        [n_pairs + 1] as it returned it, keep [M] uint8 as verify_pairs_*_device wrote inlier_ptr (None: every match counts).
        The outputs go to device memory: toff [N // 2 + 1] int64, obs [N] int32, track_of [N] int32 and, if asked for, label [N]
        int32, N = seg[-1].  Returns (n_tracks, counts [3] int64); toff[:n_tracks + 1] and obs[:toff[n_tracks]] are written."""
        s, q = _seg_pairs(seg, pairs)
        o = np.ascontiguousarray(moff, np.int64)
        assert o.shape == (q.shape[0] + 1,)
        nt, counts = np.zeros(1, np.int64), np.zeros(3, np.int64)
        ptr = lambda a: None if a is None else C.c_void_p(a)
        self._ck(self.L.dlco_desc_build_tracks_device(self.h, _p(s, i64p), s.size - 1, _p(q, i32p), q.shape[0], _p(o, i64p), ptr(matches_ptr), ptr(keep_ptr),
                                                      min_len, 1 if unique else 0, _p(nt, i64p), ptr(toff_ptr), ptr(obs_ptr), ptr(track_of_ptr),
                                                      ptr(label_ptr), _p(counts, i64p)))
        return int(nt[0]), counts

    def match_pairs_slices(self, seg, pairs, u8=False):
        """The plan only: slices [n_pairs] int32 of train that each pair is cut into in such a call on this context's device
        (0: the pair launches nothing); more than one means partials and a merge.  Nothing is launched."""
        s, q = _seg_pairs(seg, pairs)
        out = np.empty(q.shape[0], np.int32)
        self._ck(self.L.dlco_desc_match_pairs_slices(self.h, _p(s, i64p), s.size - 1, _p(q, i32p), q.shape[0], 1 if u8 else 0, _p(out, i32p)))
        return out

    def last_kernel_ms(self):
        return self.L.dlco_desc_last_kernel_ms(self.h)
