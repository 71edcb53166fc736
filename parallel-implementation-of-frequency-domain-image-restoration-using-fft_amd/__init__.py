"""MI355X-native frequency-domain image restoration (Wiener deconvolution) -- Python host mirror.

Thin ctypes binding over libfdr.so (HIP kernels + C ABI, include/fdr.h) plus functions carrying
the reference's own names (utils.hpp / fft/fft.hpp of the reference) so parity tests read like
the reference's drivers.  The product path is HIP only: importing this module fails loudly when
libfdr.so is missing, and nothing here falls back to numpy or to oracle/.

The directory name contains hyphens, so import it with importlib:
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
"""
import collections
import ctypes
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FDR_LIB_PATH selects an alternative build of the same library (timing-only debug builds)
LIB_PATH = os.environ.get("FDR_LIB_PATH") or os.path.join(_HERE, "libfdr.so")

MODE_PARITY = 0
MODE_FAST = 1
FLAG_SIMPLE_PATH = 1
FLAG_FULL_SPECTRUM = 32
FLAG_ANY_SIZE = 512
FLAG_TABLES_ONLY = 1024
FLAG_MIXED_RADIX = 2048
NORM_PADDED = 1
NORM_CROPPED = 0
NORM_NONE = 2  # Richardson-Lucy only: the raw estimate
RL_SIGMA = 1e-2  # FDR_RL_SIGMA: the usual coverage threshold of free-boundary Richardson-Lucy
RLTV_MAX_LAMBDA = 0.125  # FDR_RLTV_MAX_LAMBDA: the largest weight of Richardson-Lucy's total-variation prior
RLTV_EPS = 1e-3  # FDR_RLTV_EPS: the smoothing of |grad u| that eps = 0 selects
RL_STOP_NONE, RL_STOP_RESIDUAL, RL_STOP_KL = 0, 1, 2  # FDR_RL_STOP_*: the stopping rules of Plan.richardson_lucy_auto
TV_COUPLE_NONE = 0      # FDR_TV_COUPLE_NONE: every image of a TV batch on its own
TV_COUPLE_CHANNELS = 1  # FDR_TV_COUPLE_CHANNELS: vectorial TV, one shrinkage by the joint gradient norm of the channels
RL_ACCEL_MAX = 0.9990234375  # FDR_RL_ACCEL_MAX = 1 - 2^-10: the upper bound of accelerated Richardson-Lucy's extrapolation factor
MAX_PASSES = 16
OPT_TWO_SWEEP_NORM = 2
OPT_BATCH_GRAPH = 3
OPT_CE_CHUNK_MB = 4
OPT_PAD_MODE = 5  # Plan.set_option: what the Wiener / CLS calls put outside the picture (fast-mode power-of-two plans)
PAD_ZERO = 0      # zeros, as the reference pads (default)
PAD_SMOOTH = 1    # a smooth periodic continuation of the picture (include/fdr.h, FDR_OPT_PAD_MODE)
PHASES = ("alloc", "h2d", "pre", "compute", "d2h", "post")  # the reference Profiler's buckets, fft/fft_gpu.cu:17-57
BATCH_MAX_DEVICES = 16
REG_DISCREPANCY = 0  # Plan.choose_regularisation: residual energy = tau rows cols sigma^2 (Morozov; Gonzalez & Woods 5.9)
REG_GCV = 1          # ... or the minimum of M N rho / trace^2 (generalised cross-validation): needs no noise level
REG_PARAM_K = 0      # the weight that is searched: K ...
REG_PARAM_GAMMA = 1  # ... or the CLS gamma
REG_AT_LOW = 1       # RegChoice.flags: the search range's lower / upper end was taken
REG_AT_HIGH = 2

_f32p = ctypes.POINTER(ctypes.c_float)


class BatchDesc(ctypes.Structure):
    """fdr_batch_desc of include/fdr.h"""
    _fields_ = [("n_devices", ctypes.c_int), ("devices", ctypes.POINTER(ctypes.c_int)),
                ("M", ctypes.c_int), ("N", ctypes.c_int), ("mode", ctypes.c_int), ("flags", ctypes.c_uint),
                ("psf_host", ctypes.c_void_p), ("psf_rows", ctypes.c_int), ("psf_cols", ctypes.c_int), ("psf_stride", ctypes.c_int),
                ("psf_size", ctypes.c_int), ("psf_angle_deg", ctypes.c_double), ("K", ctypes.c_float),
                ("count", ctypes.c_int), ("rows", ctypes.c_int), ("cols", ctypes.c_int), ("stride", ctypes.c_int), ("out_stride", ctypes.c_int),
                ("imgs_host", ctypes.POINTER(ctypes.c_void_p)), ("outs_host", ctypes.POINTER(ctypes.c_void_p)),
                ("synth_seed", ctypes.c_uint64), ("steps", ctypes.c_int), ("warmup", ctypes.c_int),
                ("nstreams", ctypes.c_int), ("group", ctypes.c_int), ("norm_area", ctypes.c_int), ("bcast_filter", ctypes.c_int)]


class BatchStats(ctypes.Structure):
    """fdr_batch_stats of include/fdr.h"""
    _fields_ = [("n_devices", ctypes.c_int), ("first", ctypes.c_int * 16), ("images", ctypes.c_int * 16),
                ("elapsed_ms", ctypes.c_double * 16), ("checksum", ctypes.c_double * 16), ("status", ctypes.c_int * 16),
                ("wall_ms", ctypes.c_double), ("images_done", ctypes.c_longlong), ("mpixels_per_s", ctypes.c_double), ("filter_path", ctypes.c_int)]


class TvParams(ctypes.Structure):
    """fdr_tv_params of include/fdr.h"""
    _fields_ = [("mu", ctypes.c_float), ("rho", ctypes.c_float), ("iterations", ctypes.c_int), ("anisotropic", ctypes.c_int),
                ("nonneg", ctypes.c_int), ("norm_area", ctypes.c_int)]


class TvBatchParams(ctypes.Structure):
    """fdr_tv_batch_params of include/fdr.h"""
    _fields_ = [("mu", ctypes.c_float), ("rho", ctypes.c_float), ("iterations", ctypes.c_int), ("anisotropic", ctypes.c_int),
                ("nonneg", ctypes.c_int), ("norm_area", ctypes.c_int), ("coupling", ctypes.c_int)]


class TvFreeParams(ctypes.Structure):
    """fdr_tv_free_params of include/fdr.h"""
    _fields_ = [("mu", ctypes.c_float), ("rho", ctypes.c_float), ("nu", ctypes.c_float), ("iterations", ctypes.c_int),
                ("anisotropic", ctypes.c_int), ("nonneg", ctypes.c_int), ("norm_area", ctypes.c_int), ("out_rows", ctypes.c_int),
                ("out_cols", ctypes.c_int)]


class TvAutoParams(ctypes.Structure):
    """fdr_tv_auto_params of include/fdr.h"""
    _fields_ = [("sigma", ctypes.c_float), ("tau", ctypes.c_float), ("rho", ctypes.c_float), ("nu", ctypes.c_float),
                ("iterations", ctypes.c_int), ("anisotropic", ctypes.c_int), ("nonneg", ctypes.c_int), ("norm_area", ctypes.c_int),
                ("out_rows", ctypes.c_int), ("out_cols", ctypes.c_int)]


class TvFreeBatchParams(ctypes.Structure):
    """fdr_tv_free_batch_params of include/fdr.h"""
    _fields_ = [("mu", ctypes.c_float), ("rho", ctypes.c_float), ("nu", ctypes.c_float), ("iterations", ctypes.c_int),
                ("anisotropic", ctypes.c_int), ("nonneg", ctypes.c_int), ("norm_area", ctypes.c_int), ("out_rows", ctypes.c_int),
                ("out_cols", ctypes.c_int), ("coupling", ctypes.c_int)]


class TvPoissonParams(ctypes.Structure):
    """fdr_tv_poisson_params of include/fdr.h"""
    _fields_ = [("mu", ctypes.c_float), ("rho", ctypes.c_float), ("nu", ctypes.c_float), ("background", ctypes.c_float),
                ("iterations", ctypes.c_int), ("anisotropic", ctypes.c_int), ("nonneg", ctypes.c_int), ("norm_area", ctypes.c_int),
                ("out_rows", ctypes.c_int), ("out_cols", ctypes.c_int)]


class TvPoissonBatchParams(ctypes.Structure):
    """fdr_tv_poisson_batch_params of include/fdr.h"""
    _fields_ = [("mu", ctypes.c_float), ("rho", ctypes.c_float), ("nu", ctypes.c_float), ("background", ctypes.c_float),
                ("iterations", ctypes.c_int), ("anisotropic", ctypes.c_int), ("nonneg", ctypes.c_int), ("norm_area", ctypes.c_int),
                ("out_rows", ctypes.c_int), ("out_cols", ctypes.c_int), ("coupling", ctypes.c_int)]


class TvAutoBatchParams(ctypes.Structure):
    """fdr_tv_auto_batch_params of include/fdr.h"""
    _fields_ = [("sigma", ctypes.c_float), ("tau", ctypes.c_float), ("rho", ctypes.c_float), ("nu", ctypes.c_float),
                ("iterations", ctypes.c_int), ("anisotropic", ctypes.c_int), ("nonneg", ctypes.c_int), ("norm_area", ctypes.c_int),
                ("out_rows", ctypes.c_int), ("out_cols", ctypes.c_int), ("coupling", ctypes.c_int)]


class TvAutoResultC(ctypes.Structure):
    """fdr_tv_auto_result of include/fdr.h"""
    _fields_ = [("sigma", ctypes.c_double), ("target", ctypes.c_double), ("mu", ctypes.c_double), ("discrepancy", ctypes.c_double),
                ("S", ctypes.c_double)]


# the result of Plan.tv_deconv_auto / tvDeblurAuto_myfft beside the image: the noise level used, the target tau sigma^2 S, the last
# mu_k (the mu of the equivalent tv_deconv_free call), the last discrepancy sum m (blur(x) - d)^2 and S = sum m
TvAutoResult = collections.namedtuple("TvAutoResult", "sigma target mu discrepancy S")
TV_AUTO_MAX_RATIO = 1e6
TV_AUTO_NU_RATIO = 25.0


class RlFreeParams(ctypes.Structure):
    """fdr_rlfree_params of include/fdr.h"""
    _fields_ = [("iterations", ctypes.c_int), ("sigma", ctypes.c_float), ("norm_area", ctypes.c_int), ("out_rows", ctypes.c_int),
                ("out_cols", ctypes.c_int)]


TILED_RL_FREE = 0  # FDR_TILED_RL_FREE: the tiles by free-boundary Richardson-Lucy
TILED_TV_FREE = 1  # FDR_TILED_TV_FREE: the tiles by free-boundary TV deconvolution


class TiledParams(ctypes.Structure):
    """fdr_tiled_params of include/fdr.h"""
    _fields_ = [("method", ctypes.c_int), ("tile_rows", ctypes.c_int), ("tile_cols", ctypes.c_int), ("overlap_rows", ctypes.c_int),
                ("overlap_cols", ctypes.c_int), ("iterations", ctypes.c_int), ("sigma", ctypes.c_float), ("mu", ctypes.c_float),
                ("rho", ctypes.c_float), ("nu", ctypes.c_float), ("anisotropic", ctypes.c_int), ("nonneg", ctypes.c_int),
                ("norm_area", ctypes.c_int)]

    @classmethod
    def make(cls, method, tile, overlap=0, iterations=30, sigma=RL_SIGMA, mu=1.0, rho=2.0, nu=0.0, anisotropic=False, nonneg=False,
             norm_area=NORM_NONE):
        """tile and overlap: one number for both axes or (rows, cols)"""
        tr, tc = (tile, tile) if np.isscalar(tile) else tile
        orr, oc = (overlap, overlap) if np.isscalar(overlap) else overlap
        return cls(int(method), int(tr), int(tc), int(orr), int(oc), int(iterations), float(sigma), float(mu), float(rho), float(nu),
                   int(bool(anisotropic)), int(bool(nonneg)), int(norm_area))


class TiledLayoutC(ctypes.Structure):
    """fdr_tiled_layout of include/fdr.h"""
    _fields_ = [("tiles_r", ctypes.c_int), ("tiles_c", ctypes.c_int), ("win_rows", ctypes.c_int), ("win_cols", ctypes.c_int),
                ("min_M", ctypes.c_int), ("min_N", ctypes.c_int), ("work_bytes", ctypes.c_size_t)]


# what tiled_layout returns: tiles per axis, the window of every tile, the smallest tile plan and the workspace of the _dev call on it
TiledLayout = collections.namedtuple("TiledLayout", "tiles_r tiles_c win_rows win_cols min_M min_N work_bytes")


class RlTvParams(ctypes.Structure):
    """fdr_rl_tv_params of include/fdr.h"""
    _fields_ = [("iterations", ctypes.c_int), ("free_boundary", ctypes.c_int), ("lambda", ctypes.c_float), ("eps", ctypes.c_float),
                ("norm_area", ctypes.c_int), ("cov_sigma", ctypes.c_float), ("out_rows", ctypes.c_int), ("out_cols", ctypes.c_int)]


MAX_FRAMES = 8  # FDR_MAX_FRAMES


class RlFramesParams(ctypes.Structure):
    """fdr_rl_frames_params of include/fdr.h"""
    _fields_ = [("iterations", ctypes.c_int), ("sigma", ctypes.c_float), ("norm_area", ctypes.c_int), ("out_rows", ctypes.c_int),
                ("out_cols", ctypes.c_int), ("tv_lambda", ctypes.c_float), ("tv_eps", ctypes.c_float)]


TV_FRAMES_LEAST_SQUARES = 0  # FDR_TV_FRAMES_LEAST_SQUARES
TV_FRAMES_POISSON = 1        # FDR_TV_FRAMES_POISSON


class TvFramesParams(ctypes.Structure):
    """fdr_tv_frames_params of include/fdr.h (the stream of the _dev form travels in the struct)"""
    _fields_ = [("mu", ctypes.c_float), ("rho", ctypes.c_float), ("nu", ctypes.c_float), ("background", ctypes.c_float),
                ("data_term", ctypes.c_int), ("iterations", ctypes.c_int), ("anisotropic", ctypes.c_int), ("nonneg", ctypes.c_int),
                ("norm_area", ctypes.c_int), ("out_rows", ctypes.c_int), ("out_cols", ctypes.c_int), ("stream", ctypes.c_void_p)]


class FrameShiftC(ctypes.Structure):
    """fdr_frame_shift of include/fdr.h"""
    _fields_ = [("dy", ctypes.c_double), ("dx", ctypes.c_double), ("peak", ctypes.c_float), ("confidence", ctypes.c_float)]


class RegisterParams(ctypes.Structure):
    """fdr_register_params of include/fdr.h (the stream of the _dev form travels in the struct)"""
    _fields_ = [("reference", ctypes.c_int), ("max_shift_rows", ctypes.c_int), ("max_shift_cols", ctypes.c_int), ("eps_rel", ctypes.c_float),
                ("stream", ctypes.c_void_p)]


class PsfShiftParams(ctypes.Structure):
    """fdr_psf_shift_params of include/fdr.h (the stream of the _dev form travels in the struct)"""
    _fields_ = [("pad_rows", ctypes.c_int), ("pad_cols", ctypes.c_int), ("stream", ctypes.c_void_p)]


REGISTER_EPS_REL = 1e-3  # FDR_REGISTER_EPS_REL: the whitening floor that eps_rel = 0 selects
# the result of Plan.register_frames / registerFrames per frame: the translation (rows down, columns right) that belongs in the frame's
# PSF, the correlation peak and its confidence (peak - mean) / std over the correlation plane
FrameShift = collections.namedtuple("FrameShift", "dy dx peak confidence")


class RlTvBatchParams(ctypes.Structure):
    """fdr_rl_tv_batch_params of include/fdr.h"""
    _fields_ = RlTvParams._fields_ + [("couple", ctypes.c_int)]


class RlBatchParams(ctypes.Structure):
    """fdr_rl_batch_params of include/fdr.h"""
    _fields_ = [("iterations", ctypes.c_int), ("norm_area", ctypes.c_int), ("free_boundary", ctypes.c_int), ("sigma", ctypes.c_float),
                ("out_rows", ctypes.c_int), ("out_cols", ctypes.c_int)]


class BlindParams(ctypes.Structure):
    """fdr_blind_params of include/fdr.h"""
    _fields_ = [("iterations", ctypes.c_int), ("free_boundary", ctypes.c_int), ("psf_hold", ctypes.c_int), ("norm_area", ctypes.c_int),
                ("cov_sigma", ctypes.c_float), ("out_rows", ctypes.c_int), ("out_cols", ctypes.c_int)]


class RlAutoParams(ctypes.Structure):
    """fdr_rl_auto_params of include/fdr.h"""
    _fields_ = [("iterations", ctypes.c_int), ("free_boundary", ctypes.c_int), ("accelerate", ctypes.c_int), ("rule", ctypes.c_int),
                ("sigma", ctypes.c_float), ("gain", ctypes.c_float), ("tau", ctypes.c_float), ("check_every", ctypes.c_int),
                ("norm_area", ctypes.c_int), ("cov_sigma", ctypes.c_float), ("out_rows", ctypes.c_int), ("out_cols", ctypes.c_int)]


class RlAutoResultC(ctypes.Structure):
    """fdr_rl_auto_result of include/fdr.h"""
    _fields_ = [("iterations_done", ctypes.c_int), ("stopped", ctypes.c_int), ("sigma", ctypes.c_double), ("target", ctypes.c_double),
                ("statistic", ctypes.c_double)]


# the result of Plan.richardson_lucy_auto* / richardsonLucyAuto_myfft beside the image: the steps taken, whether the rule fired, the
# noise level used, the target and the last statistic the decision saw (in the rule's units)
RlAutoResult = collections.namedtuple("RlAutoResult", "iterations_done stopped sigma target statistic")


class MotionEstimateC(ctypes.Structure):
    """fdr_motion_estimate of include/fdr.h"""
    _fields_ = [("length", ctypes.c_int), ("angle_deg", ctypes.c_double), ("score", ctypes.c_float), ("confidence", ctypes.c_float),
                ("n_angles", ctypes.c_int), ("n_lengths", ctypes.c_int)]


class DefocusEstimateC(ctypes.Structure):
    """fdr_defocus_estimate of include/fdr.h"""
    _fields_ = [("diameter", ctypes.c_int), ("ring", ctypes.c_double), ("radius", ctypes.c_double), ("score", ctypes.c_float),
                ("confidence", ctypes.c_float), ("n_angles", ctypes.c_int), ("n_diameters", ctypes.c_int)]


class RegParams(ctypes.Structure):
    """fdr_reg_params of include/fdr.h"""
    _fields_ = [("method", ctypes.c_int), ("param", ctypes.c_int), ("fixed", ctypes.c_float), ("sigma", ctypes.c_float),
                ("tau", ctypes.c_float), ("lo", ctypes.c_double), ("hi", ctypes.c_double), ("n_grid", ctypes.c_int), ("refine", ctypes.c_int)]


class RegChoiceC(ctypes.Structure):
    """fdr_reg_choice of include/fdr.h"""
    _fields_ = [("value", ctypes.c_double), ("sigma", ctypes.c_double), ("residual", ctypes.c_double), ("trace", ctypes.c_double),
                ("gcv", ctypes.c_double), ("flags", ctypes.c_int), ("evaluations", ctypes.c_int)]


# the result of Plan.choose_regularisation* / chooseRegularisation: the chosen weight (K or gamma, whichever was searched), the noise
# level used, residual energy, trace and GCV score at the candidate nearest to it, REG_AT_* flags, candidates evaluated
RegChoice = collections.namedtuple("RegChoice", "value sigma residual trace gcv flags evaluations")


# the result of Plan.estimate_motion* / estimateMotionBlur: blur length (px) and angle (deg, motionBlurKernel convention), the
# table minimum and the confidence (median - min) / (1.4826 MAD) of the score table, and the table's shape
MotionEstimate = collections.namedtuple("MotionEstimate", "length angle score confidence n_angles n_lengths")


# the result of Plan.estimate_defocus* / estimateDefocusBlur: the ring's diameter (px, whole and sub-pixel), the disk radius it stands
# for (goes straight into psf_disk / Plan.set_psf_disk), the profile minimum, its confidence and the shape of the search
DefocusEstimate = collections.namedtuple("DefocusEstimate", "diameter ring radius score confidence n_angles n_diameters")
# the result of Plan.estimate_blur* / estimateBlur: both estimates of one cepstrum and the blur kind they point to (BLUR_*)
BlurEstimate = collections.namedtuple("BlurEstimate", "kind motion defocus")
BLUR_NONE, BLUR_MOTION, BLUR_DEFOCUS = 0, 1, 2


def _motion_table_shape(rows, cols, min_length, max_length, angle_step):
    """(n_angles, n_lengths) of the estimate's table, with fdr.h's defaults for arguments of 0"""
    lo = int(min_length) or 3
    hi = int(max_length) or min(100, min(int(rows), int(cols)) // 4)
    step = float(angle_step) or 0.5
    if not (0 < step <= 90) or hi < lo or math.ceil(180.0 / step) * (hi - lo + 1) > 1 << 26:
        return 1, 1  # refused by the library before it writes anything
    return int(math.ceil(180.0 / step)), hi - lo + 1


def _defocus_estimate(est):
    return DefocusEstimate(est.diameter, est.ring, est.radius, est.score, est.confidence, est.n_angles, est.n_diameters)


class FdrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libfdr error %d: %s" % (code, msg))
        self.code = code


def build(force=False):
    """Compile libfdr.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs.append(os.path.join(_HERE, "..", "include", "fdr.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", _HERE, "-j4", "-s"])
    return LIB_PATH


def _signatures():
    """Every function of include/fdr.h, once: name -> (restype, argtypes; None = not declared).  _load applies it and
    EXPORTED_SYMBOLS is its keys, so an entry point cannot have its argument types without its return type."""
    vp, ci, cf, cd, cu, sz, u64, P = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_uint, ctypes.c_size_t,
                                      ctypes.c_uint64, ctypes.POINTER)
    return {
        "fdr_version": (ci, None),
        "fdr_last_error": (ctypes.c_char_p, None),
        "fdr_device_count": (ci, [P(ci)]),
        "fdr_next_pow2": (ci, [ci]),
        "fdr_is_pow2": (ci, [ci]),
        "fdr_optimal_dft_size": (ci, [ci]),
        "fdr_plan_set_option": (ci, [vp, ci, ctypes.c_longlong]),
        "fdr_plan_phase_times": (ci, [vp, _f32p, ci]),
        "fdr_batch_run": (ci, [P(BatchDesc), P(BatchStats)]),
        "fdr_slab_pad_dev": (ci, [vp, ci, ci, ci, vp, ci, ci, vp]),
        "fdr_slab_rows_fft_dev": (ci, [vp, vp, ci, ci, ci, vp]),
        "fdr_slab_pack_dev": (ci, [vp, ci, ci, ci, P(ci), ci, vp, vp]),
        "fdr_slab_transpose_dev": (ci, [vp, vp, ci, ci, ci, vp]),
        "fdr_slab_wiener_dev": (ci, [vp, vp, vp, sz, cf, vp]),
        "fdr_slab_real_dev": (ci, [vp, vp, sz, vp]),
        "fdr_slab_minmax_dev": (ci, [vp, vp, ci, ci, ci, ci, vp, vp]),
        "fdr_slab_normalize_dev": (ci, [vp, ci, vp, vp, ci, ci, ci, vp]),
        "fdr_plan_create": (ci, [ci, ci, ci, ci, cu, P(vp)]),
        "fdr_plan_destroy": (ci, [vp]),
        "fdr_plan_dims": (ci, [vp, P(ci), P(ci), P(ci)]),
        "fdr_psf_motion": (ci, [ci, cd, vp]),
        "fdr_psf_motion_dev": (ci, [ci, ci, cd, vp, vp]),
        "fdr_warp_affine_f32": (ci, [vp, ci, ci, ci, P(cd), vp, ci, ci, ci]),
        "fdr_plan_filter_bytes": (ci, [vp, P(sz)]),
        "fdr_plan_export_filter_dev": (ci, [vp, vp, sz, vp]),
        "fdr_plan_import_filter_dev": (ci, [vp, vp, sz, cf, vp]),
        "fdr_set_psf": (ci, [vp, vp, ci, ci, ci, cf]),
        "fdr_set_psf_dev": (ci, [vp, vp, ci, ci, ci, cf, vp]),
        "fdr_set_psf_motion": (ci, [vp, ci, cd, cf, vp]),
        "fdr_set_psf_cls": (ci, [vp, vp, ci, ci, ci, cf, cf]),
        "fdr_set_psf_cls_dev": (ci, [vp, vp, ci, ci, ci, cf, cf, vp]),
        "fdr_set_psf_motion_cls": (ci, [vp, ci, cd, cf, cf, vp]),
        "fdr_wiener_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, ci]),
        "fdr_wiener_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, ci, vp]),
        "fdr_wiener_batch_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, ci, vp]),
        "fdr_wiener_batch_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, ci]),
        "fdr_wiener_batch_ptrs_f32": (ci, [vp, P(vp), P(vp), ci, ci, ci, ci, ci, ci]),
        "fdr_host_alloc": (ci, [sz, P(vp)]),
        "fdr_host_free": (ci, [vp]),
        "fdr_white_balance_u8": (ci, [ci, P(vp), P(vp), ci, ci, ci, vp, ci]),
        "fdr_white_balance_u8_dev": (ci, [ci, P(vp), P(vp), ci, ci, ci, vp, ci, vp]),
        "fdr_plan_set_concurrency": (ci, [vp, ci]),
        "fdr_plan_set_batching": (ci, [vp, ci, ci]),
        "fdr_fft2d_c2c": (ci, [vp, vp, ci]),
        "fdr_fft2d_c2c_dev": (ci, [vp, vp, ci, vp]),
        "fdr_fft1d_c2c": (ci, [vp, ci, ci, ci]),
        "fdr_dft_naive_c2c": (ci, [vp, ci, ci]),
        "fdr_synth_image_dev": (ci, [ci, u64, u64, sz, vp, vp]),
        "fdr_plan_profile": (ci, [vp, ci]),
        "fdr_set_operator_psf": (ci, [vp, vp, ci, ci, ci]),
        "fdr_set_operator_psf_dev": (ci, [vp, vp, ci, ci, ci, vp]),
        "fdr_set_operator_psf_motion": (ci, [vp, ci, cd, vp]),
        "fdr_blur_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, ci]),
        "fdr_blur_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, ci, vp]),
        "fdr_richardson_lucy_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, ci, ci]),
        "fdr_richardson_lucy_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, ci, ci, vp]),
        "fdr_richardson_lucy_free_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(RlFreeParams)]),
        "fdr_richardson_lucy_free_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(RlFreeParams), vp]),
        "fdr_richardson_lucy_tv_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(RlTvParams)]),
        "fdr_richardson_lucy_tv_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(RlTvParams), vp]),
        "fdr_rl_tv_factor_f32_dev": (ci, [ci, vp, ci, ci, ci, vp, cf, cf, vp, ci, vp]),
        "fdr_richardson_lucy_tv_batch_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(RlTvBatchParams)]),
        "fdr_richardson_lucy_tv_batch_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(RlTvBatchParams), vp]),
        "fdr_rl_tv_factor_group_f32_dev": (ci, [ci, vp, sz, ci, ci, ci, ci, vp, cf, cf, ci, vp, sz, ci, vp]),
        "fdr_set_frame_psfs": (ci, [vp, vp, sz, ci, ci, ci, ci]),
        "fdr_set_frame_psfs_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp]),
        "fdr_frame_count": (ci, [vp, P(ci)]),
        "fdr_spectrum_sum_f32_dev": (ci, [ci, vp, P(vp), ci, sz, ci, vp]),
        "fdr_blur_frames_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, vp, sz, ci, ci, ci, vp]),
        "fdr_richardson_lucy_frames_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, vp, ci, P(RlFramesParams)]),
        "fdr_richardson_lucy_frames_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, vp, ci, P(RlFramesParams), vp]),
        "fdr_tv_deconv_frames_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, vp, ci, P(TvFramesParams)]),
        "fdr_tv_deconv_frames_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, vp, ci, P(TvFramesParams)]),
        "fdr_blur_batch_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, ci, vp]),
        "fdr_richardson_lucy_batch_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(RlBatchParams)]),
        "fdr_richardson_lucy_batch_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(RlBatchParams), vp]),
        "fdr_richardson_lucy_batch_accel_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(RlBatchParams), vp, sz]),
        "fdr_richardson_lucy_batch_accel_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(RlBatchParams), vp, sz, vp]),
        "fdr_richardson_lucy_accel_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, ci, ci, vp]),
        "fdr_richardson_lucy_accel_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, ci, ci, vp, vp]),
        "fdr_richardson_lucy_free_accel_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(RlFreeParams), vp]),
        "fdr_richardson_lucy_free_accel_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(RlFreeParams), vp, vp]),
        "fdr_richardson_lucy_blind_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, ci, ci, vp, ci, P(BlindParams)]),
        "fdr_richardson_lucy_blind_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, ci, ci, vp, ci, P(BlindParams), vp]),
        "fdr_richardson_lucy_blind_status": (ci, [vp, P(ci)]),
        "fdr_psf_gaussian": (ci, [ci, cd, vp]),
        "fdr_psf_gaussian_dev": (ci, [ci, ci, cd, vp, vp]),
        "fdr_tv_deconv_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, P(TvParams)]),
        "fdr_tv_deconv_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, P(TvParams), vp]),
        "fdr_tv_deconv_batch_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, P(TvBatchParams)]),
        "fdr_tv_deconv_batch_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, P(TvBatchParams), vp]),
        "fdr_tv_deconv_free_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(TvFreeParams)]),
        "fdr_tv_deconv_free_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(TvFreeParams), vp]),
        "fdr_tv_deconv_auto_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(TvAutoParams), P(TvAutoResultC), vp]),
        "fdr_tv_deconv_auto_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(TvAutoParams), vp, vp]),
        "fdr_tv_deconv_free_batch_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(TvFreeBatchParams)]),
        "fdr_tv_deconv_free_batch_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(TvFreeBatchParams), vp]),
        "fdr_tv_deconv_auto_batch_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(TvAutoBatchParams), vp, vp, vp, sz]),
        "fdr_tv_deconv_auto_batch_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(TvAutoBatchParams), vp, vp, sz, vp]),
        "fdr_tv_deconv_poisson_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(TvPoissonParams)]),
        "fdr_tv_deconv_poisson_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(TvPoissonParams), vp]),
        "fdr_tv_deconv_poisson_batch_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(TvPoissonBatchParams)]),
        "fdr_tv_deconv_poisson_batch_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, ci, vp, sz, ci, P(TvPoissonBatchParams), vp]),
        "fdr_tv_poisson_step_f32_dev": (ci, [vp, vp, vp, vp, ci, ci, ci, vp, ci, cf, cf, cf, vp]),
        "fdr_tv_poisson_step_group_f32_dev": (ci, [vp, vp, sz, vp, sz, vp, sz, ci, ci, ci, ci, vp, ci, cf, cf, cf, vp]),
        "fdr_tiled_layout_get": (ci, [ci, ci, ci, ci, P(TiledParams), P(TiledLayoutC)]),
        "fdr_tiled_tile_origin": (ci, [ci, ci, P(TiledParams), ci, ci, P(ci), P(ci)]),
        "fdr_restore_tiled_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, sz, ci, ci, ci, ci, vp, ci, P(TiledParams), vp, sz, vp]),
        "fdr_restore_tiled_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, sz, ci, ci, ci, ci, vp, ci, P(TiledParams)]),
        "fdr_cepstrum_f32": (ci, [vp, vp, ci, ci, ci, vp]),
        "fdr_cepstrum_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, vp]),
        "fdr_estimate_motion_f32": (ci, [vp, vp, ci, ci, ci, ci, ci, cd, P(MotionEstimateC), vp]),
        "fdr_estimate_motion_f32_dev": (ci, [vp, vp, ci, ci, ci, ci, ci, cd, P(MotionEstimateC), vp, vp]),
        "fdr_register_frames_f32": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, ci, ci, P(RegisterParams), vp]),
        "fdr_register_frames_f32_dev": (ci, [vp, vp, sz, ci, ci, ci, ci, vp, sz, ci, ci, ci, P(RegisterParams), vp, vp]),
        "fdr_psf_shift_f32": (ci, [ci, vp, sz, ci, ci, ci, ci, vp, P(PsfShiftParams), vp, sz, ci]),
        "fdr_psf_shift_f32_dev": (ci, [ci, vp, sz, ci, ci, ci, ci, vp, P(PsfShiftParams), vp, sz, ci]),
        "fdr_psf_disk": (ci, [ci, cd, vp]),
        "fdr_psf_disk_dev": (ci, [ci, ci, cd, vp, vp]),
        "fdr_set_psf_disk": (ci, [vp, cd, cf, vp]),
        "fdr_set_psf_disk_cls": (ci, [vp, cd, cf, cf, vp]),
        "fdr_set_operator_psf_disk": (ci, [vp, cd, vp]),
        "fdr_estimate_defocus_f32": (ci, [vp, vp, ci, ci, ci, ci, ci, cd, P(DefocusEstimateC), vp]),
        "fdr_estimate_defocus_f32_dev": (ci, [vp, vp, ci, ci, ci, ci, ci, cd, P(DefocusEstimateC), vp, vp]),
        "fdr_estimate_blur_f32": (ci, [vp, vp, ci, ci, ci, ci, ci, cd, ci, ci, cd, P(MotionEstimateC), P(DefocusEstimateC), P(ci)]),
        "fdr_estimate_blur_f32_dev": (ci, [vp, vp, ci, ci, ci, ci, ci, cd, ci, ci, cd, P(MotionEstimateC), P(DefocusEstimateC), P(ci), vp]),
        "fdr_blur_kind": (ci, [cd, cd]),
        "fdr_richardson_lucy_auto_f32": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(RlAutoParams), P(RlAutoResultC), vp]),
        "fdr_richardson_lucy_auto_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, ci, P(RlAutoParams), P(RlAutoResultC), vp, vp]),
        "fdr_noise_sigma_f32": (ci, [ci, vp, ci, ci, ci, P(cd)]),
        "fdr_noise_sigma_f32_dev": (ci, [ci, vp, ci, ci, ci, P(cd), vp]),
        "fdr_reg_curve_f32": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, vp, vp]),
        "fdr_reg_curve_f32_dev": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, vp, vp, vp]),
        "fdr_choose_reg_f32": (ci, [vp, vp, ci, ci, ci, P(RegParams), P(RegChoiceC)]),
        "fdr_choose_reg_f32_dev": (ci, [vp, vp, ci, ci, ci, P(RegParams), P(RegChoiceC), vp]),
        "fdr_plan_pass_times": (ci, [vp, P(ci), _f32p, P(ctypes.c_char_p), P(ci)]),
    }


_SIGNATURES = _signatures()
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libfdr.so not found at %s: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64 and publishes
    # them in the global symbol scope.  Loaded first, libfdr.so binds to that same runtime, so device
    # pointers and hipStream_t handles can be shared with torch; loaded second, torch's runtime would
    # find the GPU already claimed ("No HIP GPUs are available").  Without torch (C++ callers, the CLI)
    # libfdr.so simply uses /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for this binding
        pass
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    return L


lib = _load()


def _alphas_array(iterations, accelerate, return_alphas):
    """room for the extrapolation factors of an accelerated Richardson-Lucy call (None when they are not asked for)"""
    if not return_alphas:
        return None
    if not accelerate:
        raise ValueError("return_alphas needs accelerate=True")
    return np.zeros(max(int(iterations), 0), dtype=np.float32)


def _check(rc):
    if rc != 0:
        raise FdrError(rc, lib.fdr_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _stream(stream):
    return ctypes.c_void_p(int(stream) if stream else 0)


# ---- utils.hpp mirrors ---------------------------------------------------------------------
def csrc_fingerprint():
    """sha256 (first 16 hex digits) over names and contents of csrc/*: which kernel sources a build, a profile or a bench
    line belongs to.  tools/collect_profiles.sh records it beside the PMC passes, tools/summarize_profiles.py writes it into
    profiles/traffic.json, and bench.py reports `roofline.traffic_stale` when the tree it runs from has another one."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".hpp", ".h")):
            h.update(name.encode() + b"\0")
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


def traffic_entry(tj, key, pass_name, images, fingerprint, P, spectrum):
    """Looks a pass up in profiles/traffic.json (PMC bytes per launch, tools/summarize_profiles.py) for bench.py's roofline.
    Returns a dict: `traffic` (bytes per launch of `images` images, or None), `stale` (the counters were collected on other
    kernel sources than `fingerprint`, or the entry carries no fingerprint: the bytes are then NOT reported), `note`."""
    out = {"traffic": None, "stale": False, "note": None, "kernel": None}
    ent = tj.get(key, {}).get(pass_name)
    if ent is None:
        out["note"] = "no PMC entry for %s / %s" % (key, pass_name)
        return out
    if not isinstance(ent, dict):
        ent = {"per_launch": float(ent), "images": 1}
    out["kernel"] = ent.get("kernel")
    if ent.get("csrc") != fingerprint:
        out["stale"] = True
        out["note"] = "counters collected on csrc %s, this tree is %s" % (ent.get("csrc"), fingerprint)
        return out
    if ent["images"] == images:
        out["traffic"] = ent["per_launch"]
    else:  # a launch of another size was profiled: scale the per-image part, keep W once (pass B')
        w_once = (4 if spectrum == "half" else 8) * P if pass_name.startswith("B' cols") else 0
        out["traffic"] = (ent["per_launch"] - w_once) * images / ent["images"] + w_once
        out["note"] = "scaled from a %d-image launch" % ent["images"]
    return out


def nextPowerOfTwo(n):
    """utils.hpp:27-31"""
    return lib.fdr_next_pow2(int(n))


getNextPowerOf2 = nextPowerOfTwo  # utils.hpp:33-37


def isPowerOfTwo(n):
    """utils.hpp:50-52"""
    return bool(lib.fdr_is_pow2(int(n)))


def getOptimalDFTSize(n):
    """cv::getOptimalDFTSize as fft/fft_serial.cpp:153-154 uses it: smallest 2^a 3^b 5^c >= n"""
    return lib.fdr_optimal_dft_size(int(n))


def motionBlurKernel(size, angle):
    """utils.hpp:15-24 -- generated by the device PSF kernel, returned as a size x size float32 array."""
    out = np.empty((int(size), int(size)), dtype=np.float32)
    _check(lib.fdr_psf_motion(int(size), float(angle), _ptr(out)))
    return out


def warpAffine(src, M, dsize):
    """cv::warpAffine(src, dst, M, dsize) with its defaults (bilinear, constant 0 border) on the device: src float32
    [rows, cols], M the 2 x 3 forward matrix, dsize = (width, height) as cv::Size."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    m = (ctypes.c_double * 6)(*[float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)])
    out = np.empty((int(dsize[1]), int(dsize[0])), dtype=np.float32)
    _check(lib.fdr_warp_affine_f32(_ptr(src), src.shape[0], src.shape[1], src.shape[1], m, _ptr(out), out.shape[0], out.shape[1], out.shape[1]))
    return out


def getRotationMatrix2D(center, angle, scale):
    """cv::getRotationMatrix2D (utils.hpp:20): center = (x, y) rounded to float as cv::Point2f, angle in degrees."""
    a = float(angle) * np.pi / 180.0
    alpha, beta = np.cos(a) * scale, np.sin(a) * scale
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def autoPadToPowerOfTwo(src):
    """utils.hpp:40-47 (host helper; the device path pads on load instead)."""
    src = np.asarray(src, dtype=np.float32)
    out = np.zeros((nextPowerOfTwo(src.shape[0]), nextPowerOfTwo(src.shape[1])), dtype=np.float32)
    out[:src.shape[0], :src.shape[1]] = src
    return out


# ---- plan -----------------------------------------------------------------------------------
class Plan:
    """One (device, M, N, mode) workspace: twiddles, spectrum buffers, filter spectrum."""

    def __init__(self, M, N, mode=MODE_PARITY, device=0, flags=0):
        h = ctypes.c_void_p()
        _check(lib.fdr_plan_create(int(device), int(M), int(N), int(mode), int(flags), ctypes.byref(h)))
        self._h = h
        self.M, self.N, self.mode, self.device = int(M), int(N), int(mode), int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib.fdr_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # PSF.  gamma > 0: the constrained least-squares filter W = conj(H) / (|H|^2 + K + gamma L^2) (fdr_set_psf_cls*, fast mode
    # only); gamma == 0: the Wiener filter of fdr_set_psf*
    def set_psf(self, psf, K=0.01, gamma=0.0):
        psf = np.ascontiguousarray(psf, dtype=np.float32)
        if gamma == 0:
            _check(lib.fdr_set_psf(self._h, _ptr(psf), psf.shape[0], psf.shape[1], psf.shape[1], ctypes.c_float(K)))
        else:
            _check(lib.fdr_set_psf_cls(self._h, _ptr(psf), psf.shape[0], psf.shape[1], psf.shape[1], ctypes.c_float(K),
                                       ctypes.c_float(gamma)))

    def set_psf_dev(self, d_ptr, prows, pcols, pstride, K=0.01, stream=None, gamma=0.0):
        if gamma == 0:
            _check(lib.fdr_set_psf_dev(self._h, ctypes.c_void_p(int(d_ptr)), prows, pcols, pstride, ctypes.c_float(K),
                                       _stream(stream)))
        else:
            _check(lib.fdr_set_psf_cls_dev(self._h, ctypes.c_void_p(int(d_ptr)), prows, pcols, pstride, ctypes.c_float(K),
                                           ctypes.c_float(gamma), _stream(stream)))

    def set_psf_motion(self, size, angle, K=0.01, stream=None, gamma=0.0):
        if gamma == 0:
            _check(lib.fdr_set_psf_motion(self._h, int(size), float(angle), ctypes.c_float(K), _stream(stream)))
        else:
            _check(lib.fdr_set_psf_motion_cls(self._h, int(size), float(angle), ctypes.c_float(K), ctypes.c_float(gamma),
                                              _stream(stream)))

    def set_psf_disk(self, radius, K=0.01, gamma=0.0, stream=None):
        """the Wiener (gamma = 0) or CLS filter of the disk of `radius` px, size 2 ceil(radius) + 1, generated on the device"""
        if gamma == 0:
            _check(lib.fdr_set_psf_disk(self._h, float(radius), ctypes.c_float(K), _stream(stream)))
        else:
            _check(lib.fdr_set_psf_disk_cls(self._h, float(radius), ctypes.c_float(K), ctypes.c_float(gamma), _stream(stream)))

    # the prepared filter as an opaque block (one rank's PSF spectrum handed to the others: fft/fft_mpi.cpp:334-378)
    def filter_bytes(self):
        n = ctypes.c_size_t(0)
        _check(lib.fdr_plan_filter_bytes(self._h, ctypes.byref(n)))
        return int(n.value)

    def export_filter_dev(self, d_dst, nbytes, stream=None):
        _check(lib.fdr_plan_export_filter_dev(self._h, ctypes.c_void_p(int(d_dst)), int(nbytes), _stream(stream)))

    def import_filter_dev(self, d_src, nbytes, K=0.01, stream=None):
        _check(lib.fdr_plan_import_filter_dev(self._h, ctypes.c_void_p(int(d_src)), int(nbytes), ctypes.c_float(K), _stream(stream)))

    # operator
    def wiener(self, img, norm_area=NORM_PADDED):
        """One channel, host arrays; serial.cpp:34-39 semantics (pad -> restore -> crop)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        out = np.empty_like(img)
        _check(lib.fdr_wiener_f32(self._h, _ptr(img), img.shape[0], img.shape[1], img.shape[1], _ptr(out), img.shape[1],
                                  int(norm_area)))
        return out

    def wiener_dev(self, d_img, rows, cols, stride, d_out, out_stride, norm_area=NORM_PADDED, stream=None):
        _check(lib.fdr_wiener_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride, ctypes.c_void_p(int(d_out)),
                                      out_stride, int(norm_area), _stream(stream)))

    def wiener_batch_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride,
                         norm_area=NORM_PADDED, stream=None):
        _check(lib.fdr_wiener_batch_f32_dev(self._h, ctypes.c_void_p(int(d_imgs)), img_pitch, count, rows, cols, stride,
                                            ctypes.c_void_p(int(d_out)), out_pitch, out_stride, int(norm_area),
                                            _stream(stream)))

    def prepared_batch_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride,
                           norm_area=NORM_PADDED, stream=None):
        """The same call as wiener_batch_dev with its arguments converted ONCE: returns a zero-argument callable.  For callers
        that repeat one call many times (a single small image per step is a 20 us call: the per-call ctypes conversions of
        twelve arguments are then a measurable part of it)."""
        fn = lib.fdr_wiener_batch_f32_dev
        args = (self._h, ctypes.c_void_p(int(d_imgs)), ctypes.c_size_t(img_pitch), ctypes.c_int(count), ctypes.c_int(rows), ctypes.c_int(cols),
                ctypes.c_int(stride), ctypes.c_void_p(int(d_out)), ctypes.c_size_t(out_pitch), ctypes.c_int(out_stride), ctypes.c_int(int(norm_area)),
                _stream(stream))

        def call():
            rc = fn(*args)
            if rc != 0:
                _check(rc)
        return call

    def wiener_batch(self, imgs, out=None, norm_area=NORM_PADDED):
        """Host arrays [count, rows, cols] in, restored planes out; H2D / compute / D2H of consecutive images
        overlap (pinned arrays from host_alloc() are copied by DMA in place)."""
        imgs = np.ascontiguousarray(imgs, dtype=np.float32)  # (no copy when it already is: pinned arrays stay pinned)
        if out is None:
            out = np.empty_like(imgs)
        cnt, rows, cols = imgs.shape
        _check(lib.fdr_wiener_batch_f32(self._h, _ptr(imgs), rows * cols, cnt, rows, cols, cols, _ptr(out), rows * cols, cols, int(norm_area)))
        return out

    # the blur operator and Richardson-Lucy (include/fdr.h): an operator PSF of its own, apart from the Wiener / CLS filter
    def set_operator_psf(self, psf):
        psf = np.ascontiguousarray(psf, dtype=np.float32)
        _check(lib.fdr_set_operator_psf(self._h, _ptr(psf), psf.shape[0], psf.shape[1], psf.shape[1]))

    def set_operator_psf_dev(self, d_ptr, prows, pcols, pstride, stream=None):
        _check(lib.fdr_set_operator_psf_dev(self._h, ctypes.c_void_p(int(d_ptr)), prows, pcols, pstride, _stream(stream)))

    def set_operator_psf_motion(self, size, angle, stream=None):
        _check(lib.fdr_set_operator_psf_motion(self._h, int(size), float(angle), _stream(stream)))

    def set_operator_psf_disk(self, radius, stream=None):
        _check(lib.fdr_set_operator_psf_disk(self._h, float(radius), _stream(stream)))

    def blur(self, img, adjoint=False):
        """blur(img) = window(IDFT2(H . DFT2(pad(img)))), or the adjoint with conj(H); host arrays."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        out = np.empty_like(img)
        _check(lib.fdr_blur_f32(self._h, _ptr(img), img.shape[0], img.shape[1], img.shape[1], _ptr(out), img.shape[1], int(bool(adjoint))))
        return out

    def blur_dev(self, d_img, rows, cols, stride, d_out, out_stride, adjoint=False, stream=None):
        _check(lib.fdr_blur_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride, ctypes.c_void_p(int(d_out)), out_stride,
                                    int(bool(adjoint)), _stream(stream)))

    def richardson_lucy(self, img, iterations, norm_area=NORM_NONE, accelerate=False, return_alphas=False):
        """`iterations` Richardson-Lucy steps on the window img (host arrays), normalised by norm_area.  accelerate: with Biggs &
        Andrews' vector extrapolation (fdr_richardson_lucy_accel_f32); return_alphas (accelerated only): (result, the
        `iterations` extrapolation factors)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        out = np.empty_like(img)
        alphas = _alphas_array(iterations, accelerate, return_alphas)
        if accelerate:
            _check(lib.fdr_richardson_lucy_accel_f32(self._h, _ptr(img), img.shape[0], img.shape[1], img.shape[1], _ptr(out), img.shape[1],
                                                     int(iterations), int(norm_area), _ptr(alphas) if return_alphas else None))
        else:
            _check(lib.fdr_richardson_lucy_f32(self._h, _ptr(img), img.shape[0], img.shape[1], img.shape[1], _ptr(out), img.shape[1],
                                               int(iterations), int(norm_area)))
        return (out, alphas) if return_alphas else out

    def richardson_lucy_dev(self, d_img, rows, cols, stride, d_out, out_stride, iterations, norm_area=NORM_NONE, stream=None,
                            accelerate=False, d_alphas=None):
        """the same on device pointers, asynchronous; d_alphas (accelerated only): device room for `iterations` floats"""
        if accelerate:
            _check(lib.fdr_richardson_lucy_accel_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride,
                                                         ctypes.c_void_p(int(d_out)), out_stride, int(iterations), int(norm_area),
                                                         ctypes.c_void_p(int(d_alphas)) if d_alphas else None, _stream(stream)))
            return
        if d_alphas:
            raise ValueError("d_alphas needs accelerate=True")
        _check(lib.fdr_richardson_lucy_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride, ctypes.c_void_p(int(d_out)),
                                               out_stride, int(iterations), int(norm_area), _stream(stream)))

    # free-boundary, weighted Richardson-Lucy (include/fdr.h); uses the operator PSF
    def richardson_lucy_free(self, img, iterations, weights=None, sigma=RL_SIGMA, norm_area=NORM_NONE, full_plane=False, accelerate=False,
                             return_alphas=False):
        """`iterations` free-boundary Richardson-Lucy steps on the window img (host arrays): the estimate lives on the whole plan,
        the data constrain it inside the window only.  weights (img.shape, in [0, 1]; None = all ones) say how much each pixel
        counts: 0 excludes it.  Returns the window, or with full_plane the whole M x N estimate; normalised over what is returned.
        accelerate and return_alphas as Plan.richardson_lucy (fdr_richardson_lucy_free_accel_f32)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        rows, cols = img.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != img.shape:
                raise ValueError("weights must have the shape of img")
        orows, ocols = (self.M, self.N) if full_plane else (rows, cols)
        out = np.empty((orows, ocols), dtype=np.float32)
        prm = RlFreeParams(int(iterations), float(sigma), int(norm_area), orows, ocols)
        alphas = _alphas_array(iterations, accelerate, return_alphas)
        if accelerate:
            _check(lib.fdr_richardson_lucy_free_accel_f32(self._h, _ptr(img), rows, cols, cols, _ptr(w) if w is not None else None, cols,
                                                          _ptr(out), ocols, ctypes.byref(prm), _ptr(alphas) if return_alphas else None))
        else:
            _check(lib.fdr_richardson_lucy_free_f32(self._h, _ptr(img), rows, cols, cols, _ptr(w) if w is not None else None, cols, _ptr(out),
                                                    ocols, ctypes.byref(prm)))
        return (out, alphas) if return_alphas else out

    def richardson_lucy_free_dev(self, d_img, rows, cols, stride, d_out, out_stride, iterations, d_weights=None, wstride=0, sigma=RL_SIGMA,
                                 norm_area=NORM_NONE, out_rows=None, out_cols=None, stream=None, accelerate=False, d_alphas=None):
        """the same on device pointers; out_rows x out_cols (default rows x cols, up to M x N) is the output window.  Asynchronous.
        d_alphas (accelerated only): device room for `iterations` floats."""
        prm = RlFreeParams(int(iterations), float(sigma), int(norm_area), int(rows if out_rows is None else out_rows),
                           int(cols if out_cols is None else out_cols))
        if accelerate:
            _check(lib.fdr_richardson_lucy_free_accel_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride,
                                                              ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                                              ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(prm),
                                                              ctypes.c_void_p(int(d_alphas)) if d_alphas else None, _stream(stream)))
            return
        if d_alphas:
            raise ValueError("d_alphas needs accelerate=True")
        _check(lib.fdr_richardson_lucy_free_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride,
                                                    ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                                    ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(prm), _stream(stream)))

    # multi-frame Richardson-Lucy (include/fdr.h): several exposures of one scene, one PSF each, in frame tables of their own
    def set_frame_psfs(self, psfs):
        """the frame tables from K (1 .. MAX_FRAMES) host PSFs of one shape, each top-left in the plan as set_operator_psf takes it;
        sums are not normalised (a frame's PSF sum is its relative exposure).  Apart from every other table of the plan."""
        psfs = np.ascontiguousarray(np.stack([np.asarray(q, dtype=np.float32) for q in psfs]), dtype=np.float32)
        k, pr, pc = psfs.shape
        _check(lib.fdr_set_frame_psfs(self._h, _ptr(psfs), pr * pc, k, pr, pc, pc))

    def set_frame_psfs_dev(self, d_psfs, psf_pitch, count, prows, pcols, pstride, stream=None):
        """the same from device memory: PSF k at d_psfs + k psf_pitch (elements).  Asynchronous."""
        _check(lib.fdr_set_frame_psfs_dev(self._h, ctypes.c_void_p(int(d_psfs)), int(psf_pitch), int(count), prows, pcols, pstride,
                                          _stream(stream)))

    def frame_count(self):
        """frames of the last set_frame_psfs (0 before the first)"""
        n = ctypes.c_int(0)
        _check(lib.fdr_frame_count(self._h, ctypes.byref(n)))
        return n.value

    def blur_frames_dev(self, d_in, in_pitch, rows, cols, stride, d_out, out_pitch, out_stride, count, adjoint=False, stream=None):
        """adjoint=False: the one window d_in through every frame's PSF, window k to d_out + k out_pitch (the bits of blur_dev under
        PSF k).  adjoint=True: the `count` windows at d_in + k in_pitch to the ONE window sum_k blur_k^T(y_k) at d_out, added in the
        spectrum in a fixed order.  Pitches in elements.  Asynchronous."""
        _check(lib.fdr_blur_frames_f32_dev(self._h, ctypes.c_void_p(int(d_in)), int(in_pitch), rows, cols, stride, ctypes.c_void_p(int(d_out)),
                                           int(out_pitch), out_stride, int(count), int(bool(adjoint)), _stream(stream)))

    def richardson_lucy_frames(self, frames, iterations, weights=None, tv_lambda=0.0, tv_eps=0.0, sigma=RL_SIGMA, norm_area=NORM_NONE,
                               full_plane=False):
        """`iterations` joint free-boundary Richardson-Lucy steps on the K frames (host arrays of one shape, K = frame_count()):
        u <- u / alpha . sum_k H_k^T(w_k d_k / (H_k u)).  weights: None, one plane for all frames, or K planes (one per frame).
        tv_lambda > 0 adds the TV prior of richardson_lucy_tv (tv_eps 0 = RLTV_EPS).  Returns the window, or with full_plane the
        whole M x N estimate; normalised over what is returned."""
        frames = np.ascontiguousarray(np.stack([np.asarray(f, dtype=np.float32) for f in frames]), dtype=np.float32)
        k, rows, cols = frames.shape
        w, wpitch = None, 0
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape == (rows, cols):
                wpitch = 0
            elif w.shape == (k, rows, cols):
                wpitch = rows * cols
            else:
                raise ValueError("weights must have the shape of one frame or of all frames")
        orows, ocols = (self.M, self.N) if full_plane else (rows, cols)
        out = np.empty((orows, ocols), dtype=np.float32)
        prm = RlFramesParams(int(iterations), float(sigma), int(norm_area), orows, ocols, float(tv_lambda), float(tv_eps))
        _check(lib.fdr_richardson_lucy_frames_f32(self._h, _ptr(frames), rows * cols, k, rows, cols, cols, _ptr(w) if w is not None else None,
                                                  wpitch, cols, _ptr(out), ocols, ctypes.byref(prm)))
        return out

    def richardson_lucy_frames_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_stride, iterations, d_weights=None,
                                   weight_pitch=0, wstride=0, tv_lambda=0.0, tv_eps=0.0, sigma=RL_SIGMA, norm_area=NORM_NONE, out_rows=None,
                                   out_cols=None, stream=None):
        """the same on device pointers: frame k at d_imgs + k img_pitch, weights None, one plane (weight_pitch 0) or one per frame;
        out_rows x out_cols (default rows x cols, up to M x N) is the output window.  Asynchronous."""
        prm = RlFramesParams(int(iterations), float(sigma), int(norm_area), int(rows if out_rows is None else out_rows),
                             int(cols if out_cols is None else out_cols), float(tv_lambda), float(tv_eps))
        _check(lib.fdr_richardson_lucy_frames_f32_dev(self._h, ctypes.c_void_p(int(d_imgs)), int(img_pitch), int(count), rows, cols, stride,
                                                      ctypes.c_void_p(int(d_weights)) if d_weights else None, int(weight_pitch), int(wstride),
                                                      ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(prm), _stream(stream)))

    # multi-frame TV deconvolution (include/fdr.h): the frames of set_frame_psfs under one TV prior
    def tv_deconv_frames(self, frames, mu, iterations, weights=None, data_term=TV_FRAMES_LEAST_SQUARES, background=0.0, rho=2.0, nu=0.0,
                         anisotropic=False, nonneg=False, norm_area=NORM_NONE, full_plane=False):
        """`iterations` ADMM steps of  min mu sum_k Phi_k(blur_k(x)) + TV(x)  on the K frames (host arrays of one shape, K =
        frame_count()); Phi_k least squares or (TV_FRAMES_POISSON, with the known background) the Poisson likelihood.  weights: None,
        one plane for all frames, or K planes (one per frame).  Returns the window, or with full_plane the whole M x N estimate."""
        frames = np.ascontiguousarray(np.stack([np.asarray(f, dtype=np.float32) for f in frames]), dtype=np.float32)
        k, rows, cols = frames.shape
        w, wpitch = None, 0
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape == (rows, cols):
                wpitch = 0
            elif w.shape == (k, rows, cols):
                wpitch = rows * cols
            else:
                raise ValueError("weights must have the shape of one frame or of all frames")
        orows, ocols = (self.M, self.N) if full_plane else (rows, cols)
        out = np.empty((orows, ocols), dtype=np.float32)
        prm = TvFramesParams(float(mu), float(rho), float(nu), float(background), int(data_term), int(iterations), int(bool(anisotropic)),
                             int(bool(nonneg)), int(norm_area), orows, ocols, None)
        _check(lib.fdr_tv_deconv_frames_f32(self._h, _ptr(frames), rows * cols, k, rows, cols, cols, _ptr(w) if w is not None else None,
                                            wpitch, cols, _ptr(out), ocols, ctypes.byref(prm)))
        return out

    def tv_deconv_frames_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_stride, mu, iterations, d_weights=None,
                             weight_pitch=0, wstride=0, data_term=TV_FRAMES_LEAST_SQUARES, background=0.0, rho=2.0, nu=0.0, anisotropic=False,
                             nonneg=False, norm_area=NORM_NONE, out_rows=None, out_cols=None, stream=None):
        """the same on device pointers: frame k at d_imgs + k img_pitch, weights None, one plane (weight_pitch 0) or one per frame;
        out_rows x out_cols (default rows x cols, up to M x N) is the output window.  Asynchronous on `stream`, which travels in the
        parameter struct."""
        prm = TvFramesParams(float(mu), float(rho), float(nu), float(background), int(data_term), int(iterations), int(bool(anisotropic)),
                             int(bool(nonneg)), int(norm_area), int(rows if out_rows is None else out_rows),
                             int(cols if out_cols is None else out_cols), int(stream) if stream else None)
        _check(lib.fdr_tv_deconv_frames_f32_dev(self._h, ctypes.c_void_p(int(d_imgs)), int(img_pitch), int(count), rows, cols, stride,
                                                ctypes.c_void_p(int(d_weights)) if d_weights else None, int(weight_pitch), int(wstride),
                                                ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(prm)))

    # Richardson-Lucy with a total-variation prior, both forms (include/fdr.h); uses the operator PSF
    def richardson_lucy_tv(self, img, iterations, lam, eps=0.0, free_boundary=False, weights=None, cov_sigma=RL_SIGMA, norm_area=NORM_NONE,
                           full_plane=False):
        """`iterations` Richardson-Lucy steps with a total-variation prior of weight lam (0 .. RLTV_MAX_LAMBDA; 0 is the call of the
        form) on the window img (host arrays); eps (in the units of img; 0 = RLTV_EPS) smooths |grad u|.  free_boundary: the
        free-boundary, weighted form with weights, cov_sigma and full_plane as Plan.richardson_lucy_free; the plain form takes none."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        rows, cols = img.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != img.shape:
                raise ValueError("weights must have the shape of img")
        if full_plane and not free_boundary:
            raise ValueError("full_plane needs free_boundary=True")
        orows, ocols = (self.M, self.N) if full_plane else (rows, cols)
        out = np.empty((orows, ocols), dtype=np.float32)
        prm = RlTvParams(int(iterations), int(bool(free_boundary)), float(lam), float(eps), int(norm_area), float(cov_sigma), orows, ocols)
        _check(lib.fdr_richardson_lucy_tv_f32(self._h, _ptr(img), rows, cols, cols, _ptr(w) if w is not None else None, cols, _ptr(out), ocols,
                                              ctypes.byref(prm)))
        return out

    def richardson_lucy_tv_dev(self, d_img, rows, cols, stride, d_out, out_stride, iterations, lam, eps=0.0, free_boundary=False, d_weights=None,
                               wstride=0, cov_sigma=RL_SIGMA, norm_area=NORM_NONE, out_rows=None, out_cols=None, stream=None):
        """the same on device pointers; out_rows x out_cols (default rows x cols; free_boundary: up to M x N) is the output window.
        Asynchronous."""
        prm = RlTvParams(int(iterations), int(bool(free_boundary)), float(lam), float(eps), int(norm_area), float(cov_sigma),
                         int(rows if out_rows is None else out_rows), int(cols if out_cols is None else out_cols))
        _check(lib.fdr_richardson_lucy_tv_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride,
                                                  ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                                  ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(prm), _stream(stream)))

    def rl_tv_factor_dev(self, d_u, rows, cols, stride, d_out, out_stride, lam, eps=0.0, d_w=None, stream=None):
        """the factor w / (1 - lam div(grad u / |grad u|)) of one such step on a device window, on the plan's device (rl_tv_factor_dev)"""
        rl_tv_factor_dev(d_u, rows, cols, stride, d_out, out_stride, lam, eps, d_w, self.device, stream)

    def rl_tv_factor_group_dev(self, d_u, u_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, lam, eps=0.0, d_w=None,
                               couple=TV_COUPLE_NONE, stream=None):
        """the factors of `count` (1 .. 8) device windows in one launch, window k at d_u + k u_pitch -> d_out + k out_pitch (elements),
        one d_w (or None) for all, on the plan's device.  couple=TV_COUPLE_NONE: window k gets the bits of rl_tv_factor_dev on it;
        TV_COUPLE_CHANNELS: the windows are the channels of one picture and share the norm sqrt(eps^2 + sum_c |grad u_c|^2).
        Asynchronous."""
        _check(lib.fdr_rl_tv_factor_group_f32_dev(int(self.device), ctypes.c_void_p(int(d_u)), int(u_pitch), int(count), rows, cols, stride,
                                                  ctypes.c_void_p(int(d_w)) if d_w else None, float(lam), float(eps), int(couple),
                                                  ctypes.c_void_p(int(d_out)), int(out_pitch), out_stride, _stream(stream)))

    def richardson_lucy_tv_batch_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, iterations, lam, eps=0.0,
                                     free_boundary=False, d_weights=None, wstride=0, cov_sigma=RL_SIGMA, norm_area=NORM_NONE, out_rows=None,
                                     out_cols=None, couple=TV_COUPLE_NONE, stream=None):
        """richardson_lucy_tv_dev on `count` windows, image i at d_imgs + i img_pitch / d_out + i out_pitch (elements), in launch
        groups of set_batching's `group` images: one factor launch and one launch per pass for a group.  couple=TV_COUPLE_NONE: every
        image has the bits of richardson_lucy_tv_dev; TV_COUPLE_CHANNELS: the images are the channels of one picture under one
        vectorial TV prior (count <= group).  free_boundary: one weights plane (or None) for all images.  Asynchronous."""
        prm = RlTvBatchParams(int(iterations), int(bool(free_boundary)), float(lam), float(eps), int(norm_area), float(cov_sigma),
                              int((rows if free_boundary else 0) if out_rows is None else out_rows),
                              int((cols if free_boundary else 0) if out_cols is None else out_cols), int(couple))
        _check(lib.fdr_richardson_lucy_tv_batch_f32_dev(self._h, ctypes.c_void_p(int(d_imgs)), int(img_pitch), int(count), rows, cols, stride,
                                                        ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                                        ctypes.c_void_p(int(d_out)), int(out_pitch), out_stride, ctypes.byref(prm),
                                                        _stream(stream)))

    def richardson_lucy_tv_batch(self, imgs, iterations, lam, eps=0.0, free_boundary=False, weights=None, cov_sigma=RL_SIGMA,
                                 norm_area=NORM_NONE, full_plane=False, couple=TV_COUPLE_NONE):
        """Host arrays [count, rows, cols] in, [count, rows, cols] out (free_boundary with full_plane: [count, M, N]); weights
        ([rows, cols], free_boundary only) serve every image.  couple as richardson_lucy_tv_batch_dev."""
        imgs = np.ascontiguousarray(imgs, dtype=np.float32)
        cnt, rows, cols = imgs.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != (rows, cols):
                raise ValueError("weights must have the shape of one image")
        if full_plane and not free_boundary:
            raise ValueError("full_plane needs free_boundary=True")
        orows, ocols = (self.M, self.N) if full_plane else (rows, cols)
        out = np.empty((cnt, orows, ocols), dtype=np.float32)
        prm = RlTvBatchParams(int(iterations), int(bool(free_boundary)), float(lam), float(eps), int(norm_area), float(cov_sigma),
                              orows if free_boundary else 0, ocols if free_boundary else 0, int(couple))
        _check(lib.fdr_richardson_lucy_tv_batch_f32(self._h, _ptr(imgs), rows * cols, cnt, rows, cols, cols, _ptr(w) if w is not None else None,
                                                    cols, _ptr(out), orows * ocols, ocols, ctypes.byref(prm)))
        return out

    # several images per launch (include/fdr.h, "batched blur and Richardson-Lucy"): groups of set_batching's `group` images, every
    # image with the bits of its single-image call
    def blur_batch_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, adjoint=False, stream=None):
        """blur (or blur^T) of `count` windows, image i at d_imgs + i img_pitch / d_out + i out_pitch (elements); asynchronous"""
        _check(lib.fdr_blur_batch_f32_dev(self._h, ctypes.c_void_p(int(d_imgs)), img_pitch, count, rows, cols, stride,
                                          ctypes.c_void_p(int(d_out)), out_pitch, out_stride, int(bool(adjoint)), _stream(stream)))

    def richardson_lucy_batch_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, iterations,
                                  norm_area=NORM_NONE, free_boundary=False, d_weights=None, wstride=0, sigma=RL_SIGMA, out_rows=None,
                                  out_cols=None, stream=None, accelerate=False, d_alphas=None, alpha_pitch=None):
        """`iterations` Richardson-Lucy steps on `count` windows with the plan's operator PSF: the iteration of richardson_lucy_dev,
        or with free_boundary that of richardson_lucy_free_dev (one weights plane, or None, for all images; out_rows x out_cols the
        output window).  accelerate: the accelerated iteration on the group (fdr_richardson_lucy_batch_accel_f32_dev); d_alphas
        (accelerated only): device room for image i's `iterations` floats at d_alphas + i alpha_pitch (default pitch: iterations).
        Asynchronous."""
        prm = RlBatchParams(int(iterations), int(norm_area), int(bool(free_boundary)), float(sigma),
                            int((rows if free_boundary else 0) if out_rows is None else out_rows),
                            int((cols if free_boundary else 0) if out_cols is None else out_cols))
        args = (self._h, ctypes.c_void_p(int(d_imgs)), img_pitch, count, rows, cols, stride, ctypes.c_void_p(int(d_weights)) if d_weights else None,
                int(wstride), ctypes.c_void_p(int(d_out)), out_pitch, out_stride, ctypes.byref(prm))
        if accelerate:
            _check(lib.fdr_richardson_lucy_batch_accel_f32_dev(*args, ctypes.c_void_p(int(d_alphas)) if d_alphas else None,
                                                               int(max(int(iterations), 0) if alpha_pitch is None else alpha_pitch), _stream(stream)))
            return
        if d_alphas:
            raise ValueError("d_alphas needs accelerate=True")
        _check(lib.fdr_richardson_lucy_batch_f32_dev(*args, _stream(stream)))

    def richardson_lucy_batch(self, imgs, iterations, free_boundary=False, weights=None, sigma=RL_SIGMA, norm_area=NORM_NONE,
                              full_plane=False, accelerate=False, return_alphas=False):
        """Host arrays [count, rows, cols] in, [count, rows, cols] out (free_boundary with full_plane: [count, M, N]); weights
        ([rows, cols], free_boundary only) serve every image.  accelerate: the accelerated iteration
        (fdr_richardson_lucy_batch_accel_f32); return_alphas (accelerated only): (results, alphas [count, iterations])."""
        imgs = np.ascontiguousarray(imgs, dtype=np.float32)
        cnt, rows, cols = imgs.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != (rows, cols):
                raise ValueError("weights must have the shape of one image")
        orows, ocols = (self.M, self.N) if (free_boundary and full_plane) else (rows, cols)
        out = np.empty((cnt, orows, ocols), dtype=np.float32)
        prm = RlBatchParams(int(iterations), int(norm_area), int(bool(free_boundary)), float(sigma), orows if free_boundary else 0,
                            ocols if free_boundary else 0)
        args = (self._h, _ptr(imgs), rows * cols, cnt, rows, cols, cols, _ptr(w) if w is not None else None, cols, _ptr(out), orows * ocols, ocols,
                ctypes.byref(prm))
        if return_alphas and not accelerate:
            raise ValueError("return_alphas needs accelerate=True")
        if not accelerate:
            _check(lib.fdr_richardson_lucy_batch_f32(*args))
            return out
        n = max(int(iterations), 0)
        alphas = np.zeros((cnt, n), dtype=np.float32) if return_alphas else None
        _check(lib.fdr_richardson_lucy_batch_accel_f32(*args, _ptr(alphas) if return_alphas and alphas.size else None, n))
        return (out, alphas) if return_alphas else out

    # blind Richardson-Lucy (include/fdr.h): refines the PSF with the picture and leaves the operator tables of the refined PSF
    def richardson_lucy_blind(self, img, psf_start, iterations, free_boundary=False, weights=None, psf_hold=0, cov_sigma=RL_SIGMA,
                              norm_area=NORM_NONE, full_plane=False):
        """`iterations` blind Richardson-Lucy steps on the window img (host arrays) from the start PSF psf_start: the plain form, or
        with free_boundary the free-boundary, weighted one (weights, cov_sigma and full_plane as Plan.richardson_lucy_free).  The
        PSF is kept for the first psf_hold steps.  Returns (image, psf); the plan's operator PSF is then the returned one.  The call
        refines a PSF: a flat start does not move and zeros of the start stay zeros.  The free-boundary form needs a window of at
        least the PSF's size (rows >= prows, cols >= pcols): a smaller one is refused (FdrError, FDR_ERR_ARG; include/fdr.h)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        psf = np.array(psf_start, dtype=np.float32, order="C", ndmin=2)
        rows, cols = img.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != img.shape:
                raise ValueError("weights must have the shape of img")
        orows, ocols = (self.M, self.N) if (full_plane and free_boundary) else (rows, cols)
        out = np.empty((orows, ocols), dtype=np.float32)
        prm = BlindParams(int(iterations), int(bool(free_boundary)), int(psf_hold), int(norm_area), float(cov_sigma), orows, ocols)
        _check(lib.fdr_richardson_lucy_blind_f32(self._h, _ptr(img), rows, cols, cols, _ptr(w) if w is not None else None, cols, _ptr(psf),
                                                 psf.shape[0], psf.shape[1], psf.shape[1], _ptr(out), ocols, ctypes.byref(prm)))
        return out, psf

    def richardson_lucy_blind_dev(self, d_img, rows, cols, stride, d_psf, prows, pcols, pstride, d_out, out_stride, iterations,
                                  free_boundary=False, d_weights=None, wstride=0, psf_hold=0, cov_sigma=RL_SIGMA, norm_area=NORM_NONE,
                                  out_rows=None, out_cols=None, stream=None):
        """the same on device pointers, asynchronous: d_psf holds the start PSF and receives the refined one; out_rows x out_cols
        (free form; default rows x cols, up to M x N) is the output window.  A bad start PSF shows in blind_status().  A
        free-boundary window smaller than the PSF (rows < prows or cols < pcols) is refused before any device work (FDR_ERR_ARG)."""
        prm = BlindParams(int(iterations), int(bool(free_boundary)), int(psf_hold), int(norm_area), float(cov_sigma),
                          int(rows if out_rows is None else out_rows), int(cols if out_cols is None else out_cols))
        _check(lib.fdr_richardson_lucy_blind_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride,
                                                     ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                                     ctypes.c_void_p(int(d_psf)) if d_psf else None, int(prows), int(pcols), int(pstride),
                                                     ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(prm), _stream(stream)))

    def blind_status(self):
        """the status word of the last blind call on this plan (synchronises the device): 0 = its start PSF was good, 1 = it had a
        negative entry or a sum that is not finite and > 0 (the PSF was then left alone)"""
        st = ctypes.c_int(-1)
        _check(lib.fdr_richardson_lucy_blind_status(self._h, ctypes.byref(st)))
        return st.value

    # Richardson-Lucy that stops from the data (include/fdr.h); uses the operator PSF
    def richardson_lucy_auto(self, img, max_iterations, rule=RL_STOP_RESIDUAL, sigma=0.0, gain=0.0, tau=0.0, check_every=0,
                             free_boundary=False, accelerate=False, weights=None, cov_sigma=RL_SIGMA, norm_area=NORM_NONE, full_plane=False):
        """At most max_iterations Richardson-Lucy steps of the chosen form (free_boundary, accelerate) on the window img (host
        arrays), stopped by `rule` (RL_STOP_NONE: never; RL_STOP_RESIDUAL: Gaussian noise of standard deviation sigma, 0 = estimated;
        RL_STOP_KL: Poisson noise with `gain` photons per unit) looked at every check_every steps.  weights, cov_sigma and full_plane
        as Plan.richardson_lucy_free.  Returns (image, RlAutoResult, trace): trace[k] = (res_k, kl_k) of the point step k started
        from, iterations_done rows."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        rows, cols = img.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != img.shape:
                raise ValueError("weights must have the shape of img")
        orows, ocols = (self.M, self.N) if full_plane and free_boundary else (rows, cols)
        out = np.empty((orows, ocols), dtype=np.float32)
        prm = RlAutoParams(int(max_iterations), int(bool(free_boundary)), int(bool(accelerate)), int(rule), float(sigma), float(gain),
                           float(tau), int(check_every), int(norm_area), float(cov_sigma), orows, ocols)
        res = RlAutoResultC()
        trace = np.zeros((max(int(max_iterations), 0), 2), dtype=np.float64)
        _check(lib.fdr_richardson_lucy_auto_f32(self._h, _ptr(img), rows, cols, cols, _ptr(w) if w is not None else None, cols, _ptr(out),
                                                ocols, ctypes.byref(prm), ctypes.byref(res), _ptr(trace) if trace.size else None))
        return out, RlAutoResult(res.iterations_done, res.stopped, res.sigma, res.target, res.statistic), trace[:res.iterations_done]

    def richardson_lucy_auto_dev(self, d_img, rows, cols, stride, d_out, out_stride, max_iterations, rule=RL_STOP_RESIDUAL, sigma=0.0,
                                 gain=0.0, tau=0.0, check_every=0, free_boundary=False, accelerate=False, d_weights=None, wstride=0,
                                 cov_sigma=RL_SIGMA, norm_area=NORM_NONE, out_rows=None, out_cols=None, d_trace=None, stream=None):
        """the same on device pointers; d_trace: device room for 2 max_iterations doubles (or None).  Asynchronous with RL_STOP_NONE,
        synchronous with a rule.  Returns the RlAutoResult."""
        prm = RlAutoParams(int(max_iterations), int(bool(free_boundary)), int(bool(accelerate)), int(rule), float(sigma), float(gain),
                           float(tau), int(check_every), int(norm_area), float(cov_sigma), int(rows if out_rows is None else out_rows),
                           int(cols if out_cols is None else out_cols))
        res = RlAutoResultC()
        _check(lib.fdr_richardson_lucy_auto_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride,
                                                    ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                                    ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(prm), ctypes.byref(res),
                                                    ctypes.c_void_p(int(d_trace)) if d_trace else None, _stream(stream)))
        return RlAutoResult(res.iterations_done, res.stopped, res.sigma, res.target, res.statistic)

    # total-variation deconvolution by ADMM (include/fdr.h); uses the operator PSF
    def tv_deconv(self, img, mu, rho=2.0, iterations=50, anisotropic=False, nonneg=False, norm_area=NORM_NONE):
        """`iterations` ADMM steps of mu / 2 ||blur(x) - img||^2 + TV(x) on the window img (host arrays), normalised by norm_area."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        out = np.empty_like(img)
        prm = TvParams(float(mu), float(rho), int(iterations), int(bool(anisotropic)), int(bool(nonneg)), int(norm_area))
        _check(lib.fdr_tv_deconv_f32(self._h, _ptr(img), img.shape[0], img.shape[1], img.shape[1], _ptr(out), img.shape[1], ctypes.byref(prm)))
        return out

    def tv_deconv_dev(self, d_img, rows, cols, stride, d_out, out_stride, mu, rho=2.0, iterations=50, anisotropic=False, nonneg=False,
                      norm_area=NORM_NONE, stream=None):
        prm = TvParams(float(mu), float(rho), int(iterations), int(bool(anisotropic)), int(bool(nonneg)), int(norm_area))
        _check(lib.fdr_tv_deconv_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride, ctypes.c_void_p(int(d_out)), out_stride,
                                         ctypes.byref(prm), _stream(stream)))

    # free-boundary, weighted TV deconvolution (include/fdr.h); uses the operator PSF
    def tv_deconv_free(self, img, mu, rho=2.0, iterations=50, weights=None, nu=0.0, anisotropic=False, nonneg=False, norm_area=NORM_NONE,
                       full_plane=False):
        """`iterations` ADMM steps of mu / 2 sum m (blur(x) - img)^2 + TV(x) on the window img (host arrays) that is a crop of a larger
        scene: x lives on the whole plan, the data constrain it inside the window only.  weights (img.shape, in [0, 1]; None = all
        ones) say how much each pixel counts: 0 excludes it.  nu is the penalty of the splitting s = blur(x) (0 = rho).  Returns the
        window, or with full_plane the whole M x N estimate; normalised over what is returned (fdr_tv_deconv_free_f32)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        rows, cols = img.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != img.shape:
                raise ValueError("weights must have the shape of img")
        orows, ocols = (self.M, self.N) if full_plane else (rows, cols)
        out = np.empty((orows, ocols), dtype=np.float32)
        prm = TvFreeParams(float(mu), float(rho), float(nu), int(iterations), int(bool(anisotropic)), int(bool(nonneg)), int(norm_area), orows, ocols)
        _check(lib.fdr_tv_deconv_free_f32(self._h, _ptr(img), rows, cols, cols, _ptr(w) if w is not None else None, cols, _ptr(out), ocols,
                                          ctypes.byref(prm)))
        return out

    def tv_deconv_free_dev(self, d_img, rows, cols, stride, d_out, out_stride, mu, rho=2.0, iterations=50, d_weights=None, wstride=0, nu=0.0,
                           anisotropic=False, nonneg=False, norm_area=NORM_NONE, out_rows=None, out_cols=None, stream=None):
        """the same on device pointers; out_rows x out_cols (default rows x cols, up to M x N) is the output window.  Asynchronous."""
        prm = TvFreeParams(float(mu), float(rho), float(nu), int(iterations), int(bool(anisotropic)), int(bool(nonneg)), int(norm_area),
                           int(rows if out_rows is None else out_rows), int(cols if out_cols is None else out_cols))
        _check(lib.fdr_tv_deconv_free_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride,
                                              ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                              ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(prm), _stream(stream)))

    # Poisson-likelihood TV deconvolution (include/fdr.h): the free-boundary call with the data step of the Poisson term
    def tv_deconv_poisson(self, img, mu, rho=2.0, iterations=50, weights=None, nu=0.0, background=0.0, anisotropic=False, nonneg=False,
                          norm_area=NORM_NONE, full_plane=False):
        """tv_deconv_free for photon-limited pictures: `iterations` ADMM steps of mu sum m [(blur(x) + b) - img+ log(blur(x) + b)] +
        TV(x), b = background >= 0 in the units of img, mu = photons per unit times the weight wanted on the likelihood.  weights, nu,
        nonneg, norm_area and full_plane as tv_deconv_free (fdr_tv_deconv_poisson_f32)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        rows, cols = img.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != img.shape:
                raise ValueError("weights must have the shape of img")
        orows, ocols = (self.M, self.N) if full_plane else (rows, cols)
        out = np.empty((orows, ocols), dtype=np.float32)
        prm = TvPoissonParams(float(mu), float(rho), float(nu), float(background), int(iterations), int(bool(anisotropic)), int(bool(nonneg)),
                              int(norm_area), orows, ocols)
        _check(lib.fdr_tv_deconv_poisson_f32(self._h, _ptr(img), rows, cols, cols, _ptr(w) if w is not None else None, cols, _ptr(out), ocols,
                                             ctypes.byref(prm)))
        return out

    def tv_deconv_poisson_dev(self, d_img, rows, cols, stride, d_out, out_stride, mu, rho=2.0, iterations=50, d_weights=None, wstride=0, nu=0.0,
                              background=0.0, anisotropic=False, nonneg=False, norm_area=NORM_NONE, out_rows=None, out_cols=None, stream=None):
        """the same on device pointers; out_rows x out_cols (default rows x cols, up to M x N) is the output window.  Asynchronous."""
        prm = TvPoissonParams(float(mu), float(rho), float(nu), float(background), int(iterations), int(bool(anisotropic)), int(bool(nonneg)),
                              int(norm_area), int(rows if out_rows is None else out_rows), int(cols if out_cols is None else out_cols))
        _check(lib.fdr_tv_deconv_poisson_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride,
                                                 ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                                 ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(prm), _stream(stream)))

    def tv_poisson_step_dev(self, d_c, d_q, d_img, rows, cols, stride, mu, nu, background=0.0, d_weights=None, wstride=0, stream=None):
        """fdr_tv_poisson_step_f32_dev: the data step of tv_deconv_poisson alone, in place on the rows x cols window of the dense M x N
        device planes d_c (blur(x) in, r out) and d_q; d_img and d_weights (None = 1) are device windows.  Asynchronous."""
        _check(lib.fdr_tv_poisson_step_f32_dev(self._h, ctypes.c_void_p(int(d_c)), ctypes.c_void_p(int(d_q)), ctypes.c_void_p(int(d_img)), rows,
                                               cols, stride, ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride), float(mu),
                                               float(nu), float(background), _stream(stream)))

    def tv_poisson_step_group_dev(self, d_c, c_pitch, d_q, q_pitch, d_imgs, img_pitch, count, rows, cols, stride, mu, nu, background=0.0,
                                  d_weights=None, wstride=0, stream=None):
        """fdr_tv_poisson_step_group_f32_dev: tv_poisson_step_dev on `count` (1 .. 8) images in one launch, image k's planes at d_c + k
        c_pitch and d_q + k q_pitch, its data at d_imgs + k img_pitch (elements), one weights window for all.  Asynchronous."""
        _check(lib.fdr_tv_poisson_step_group_f32_dev(self._h, ctypes.c_void_p(int(d_c)), int(c_pitch), ctypes.c_void_p(int(d_q)), int(q_pitch),
                                                     ctypes.c_void_p(int(d_imgs)), int(img_pitch), int(count), rows, cols, stride,
                                                     ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride), float(mu), float(nu),
                                                     float(background), _stream(stream)))

    # sectioned restoration (include/fdr.h): overlapping tiles on this plan, blended; one PSF for all tiles or one per tile
    def restore_tiled(self, img, psfs, params, weights=None):
        """The picture img (host array, any size) restored in overlapping tiles on this tile plan by the free-boundary iteration of
        params.method (a TiledParams) and blended.  psfs: one PSF (2-D) for all tiles, or tiles_r x tiles_c PSFs of one shape (3-D, tile
        (a, b) at a tiles_c + b); a PSF is taken as centred, so the result is registered with img.  weights (img.shape; None = ones)
        as Plan.richardson_lucy_free.  The plan's operator tables are those of the last tile's PSF afterwards (fdr_restore_tiled_f32)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        rows, cols = img.shape
        psfs = np.ascontiguousarray(psfs, dtype=np.float32)
        if psfs.ndim == 2:
            psfs = psfs[None]
        if psfs.ndim != 3:
            raise ValueError("psfs must be one PSF (2-D) or a stack of PSFs (3-D)")
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != img.shape:
                raise ValueError("weights must have the shape of img")
        count, prows, pcols = psfs.shape
        out = np.empty((rows, cols), dtype=np.float32)
        _check(lib.fdr_restore_tiled_f32(self._h, _ptr(img), rows, cols, cols, _ptr(w) if w is not None else None, cols, _ptr(psfs),
                                         prows * pcols, count, prows, pcols, pcols, _ptr(out), cols, ctypes.byref(params)))
        return out

    def restore_tiled_dev(self, d_img, rows, cols, stride, d_psfs, psf_pitch, psf_count, prows, pcols, pstride, d_out, out_stride, params,
                          d_work, work_bytes, d_weights=None, wstride=0, stream=None):
        """the same on device pointers, with the caller's workspace (tiled_layout(...).work_bytes for the smallest tile plan).
        Allocates nothing after the plan's first-use workspaces; asynchronous."""
        _check(lib.fdr_restore_tiled_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride,
                                             ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                             ctypes.c_void_p(int(d_psfs)), int(psf_pitch), int(psf_count), prows, pcols, pstride,
                                             ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(params), ctypes.c_void_p(int(d_work)),
                                             int(work_bytes), _stream(stream)))

    # noise-constrained TV deconvolution (include/fdr.h): the free-boundary call with mu chosen from the noise level
    def tv_deconv_auto(self, img, sigma=0.0, rho=2.0, iterations=100, weights=None, tau=0.0, nu=0.0, anisotropic=False, nonneg=False,
                       norm_area=NORM_NONE, full_plane=False):
        """tv_deconv_free without mu: minimises TV(x) subject to sum m (blur(x) - img)^2 <= tau sigma^2 sum m, sigma the noise standard
        deviation of img (0: estimated from img as noise_sigma does), tau = 0 selecting 1 and nu = 0 selecting TV_AUTO_NU_RATIO rho.
        Returns (image, TvAutoResult, trace): trace[k] = (res_c, res_e, mu_k) of iteration k (fdr_tv_deconv_auto_f32)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        rows, cols = img.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != img.shape:
                raise ValueError("weights must have the shape of img")
        orows, ocols = (self.M, self.N) if full_plane else (rows, cols)
        out = np.empty((orows, ocols), dtype=np.float32)
        trace = np.zeros((max(int(iterations), 0), 3), dtype=np.float64)
        prm = TvAutoParams(float(sigma), float(tau), float(rho), float(nu), int(iterations), int(bool(anisotropic)), int(bool(nonneg)),
                           int(norm_area), orows, ocols)
        res = TvAutoResultC()
        _check(lib.fdr_tv_deconv_auto_f32(self._h, _ptr(img), rows, cols, cols, _ptr(w) if w is not None else None, cols, _ptr(out), ocols,
                                          ctypes.byref(prm), ctypes.byref(res), _ptr(trace) if trace.size else None))
        return out, TvAutoResult(res.sigma, res.target, res.mu, res.discrepancy, res.S), trace

    def tv_deconv_auto_dev(self, d_img, rows, cols, stride, d_out, out_stride, sigma=0.0, rho=2.0, iterations=100, d_weights=None, wstride=0,
                           tau=0.0, nu=0.0, anisotropic=False, nonneg=False, norm_area=NORM_NONE, out_rows=None, out_cols=None, d_trace=None,
                           stream=None):
        """the same on device pointers; out_rows x out_cols (default rows x cols, up to M x N) is the output window, d_trace room for
        3 * iterations doubles or None.  Asynchronous with sigma > 0; with sigma = 0 the stream is waited for once, before the first
        iteration, for the noise estimate."""
        prm = TvAutoParams(float(sigma), float(tau), float(rho), float(nu), int(iterations), int(bool(anisotropic)), int(bool(nonneg)),
                           int(norm_area), int(rows if out_rows is None else out_rows), int(cols if out_cols is None else out_cols))
        _check(lib.fdr_tv_deconv_auto_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride,
                                              ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                              ctypes.c_void_p(int(d_out)), out_stride, ctypes.byref(prm),
                                              ctypes.c_void_p(int(d_trace)) if d_trace else None, _stream(stream)))

    def tv_deconv_batch_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, mu, rho=2.0, iterations=50,
                            anisotropic=False, nonneg=False, norm_area=NORM_NONE, coupled=False, stream=None):
        """fdr_tv_deconv_batch_f32_dev: tv_deconv_dev on `count` windows, image i at d_imgs + i img_pitch / d_out + i out_pitch
        (elements), in launch groups of the plan's `group` (set_batching).  coupled: the images are the channels of one picture
        and share one shrinkage by their joint gradient norm (vectorial TV; count <= group, isotropic).  Asynchronous."""
        prm = TvBatchParams(float(mu), float(rho), int(iterations), int(bool(anisotropic)), int(bool(nonneg)), int(norm_area),
                            TV_COUPLE_CHANNELS if coupled else TV_COUPLE_NONE)
        _check(lib.fdr_tv_deconv_batch_f32_dev(self._h, ctypes.c_void_p(int(d_imgs)), img_pitch, count, rows, cols, stride,
                                               ctypes.c_void_p(int(d_out)), out_pitch, out_stride, ctypes.byref(prm), _stream(stream)))

    def tv_deconv_batch(self, imgs, mu, rho=2.0, iterations=50, anisotropic=False, nonneg=False, norm_area=NORM_NONE, coupled=False):
        """Host arrays [count, rows, cols] in, [count, rows, cols] out: tv_deconv per image, several per launch; coupled: vectorial
        TV on the images as the channels of one picture (fdr_tv_deconv_batch_f32)."""
        imgs = np.ascontiguousarray(imgs, dtype=np.float32)
        cnt, rows, cols = imgs.shape
        out = np.empty((cnt, rows, cols), dtype=np.float32)
        prm = TvBatchParams(float(mu), float(rho), int(iterations), int(bool(anisotropic)), int(bool(nonneg)), int(norm_area),
                            TV_COUPLE_CHANNELS if coupled else TV_COUPLE_NONE)
        _check(lib.fdr_tv_deconv_batch_f32(self._h, _ptr(imgs), rows * cols, cnt, rows, cols, cols, _ptr(out), rows * cols, cols, ctypes.byref(prm)))
        return out

    # free-boundary and noise-constrained TV deconvolution in groups (include/fdr.h): several crops per launch, or the channels of
    # one picture under vectorial TV
    def _crop_batch_args(self, imgs, weights, full_plane):
        imgs = np.ascontiguousarray(imgs, dtype=np.float32)
        cnt, rows, cols = imgs.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != (rows, cols):
                raise ValueError("weights must have the shape of one image")
        orows, ocols = (self.M, self.N) if full_plane else (rows, cols)
        return imgs, cnt, rows, cols, w, orows, ocols, np.empty((cnt, orows, ocols), dtype=np.float32)

    def tv_deconv_free_batch(self, imgs, mu, rho=2.0, iterations=50, weights=None, nu=0.0, anisotropic=False, nonneg=False,
                             norm_area=NORM_NONE, full_plane=False, coupled=False):
        """Host arrays [count, rows, cols] in, [count, rows, cols] (full_plane: [count, M, N]) out: tv_deconv_free per image with one
        weights plane for all, several per launch (set_batching); coupled: vectorial TV on the images as the channels of one picture
        (fdr_tv_deconv_free_batch_f32)."""
        imgs, cnt, rows, cols, w, orows, ocols, out = self._crop_batch_args(imgs, weights, full_plane)
        prm = TvFreeBatchParams(float(mu), float(rho), float(nu), int(iterations), int(bool(anisotropic)), int(bool(nonneg)), int(norm_area),
                                orows, ocols, TV_COUPLE_CHANNELS if coupled else TV_COUPLE_NONE)
        _check(lib.fdr_tv_deconv_free_batch_f32(self._h, _ptr(imgs), rows * cols, cnt, rows, cols, cols, _ptr(w) if w is not None else None, cols,
                                                _ptr(out), orows * ocols, ocols, ctypes.byref(prm)))
        return out

    def tv_deconv_free_batch_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, mu, rho=2.0, iterations=50,
                                 d_weights=None, wstride=0, nu=0.0, anisotropic=False, nonneg=False, norm_area=NORM_NONE, out_rows=None,
                                 out_cols=None, coupled=False, stream=None):
        """fdr_tv_deconv_free_batch_f32_dev: tv_deconv_free_dev on `count` windows, image i at d_imgs + i img_pitch / d_out + i
        out_pitch (elements), one weights window for all, in launch groups of the plan's `group` (set_batching).  coupled: the images
        are the channels of one picture and share one shrinkage (count <= group, isotropic).  Asynchronous."""
        prm = TvFreeBatchParams(float(mu), float(rho), float(nu), int(iterations), int(bool(anisotropic)), int(bool(nonneg)), int(norm_area),
                                int(rows if out_rows is None else out_rows), int(cols if out_cols is None else out_cols),
                                TV_COUPLE_CHANNELS if coupled else TV_COUPLE_NONE)
        _check(lib.fdr_tv_deconv_free_batch_f32_dev(self._h, ctypes.c_void_p(int(d_imgs)), img_pitch, count, rows, cols, stride,
                                                    ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                                    ctypes.c_void_p(int(d_out)), out_pitch, out_stride, ctypes.byref(prm), _stream(stream)))

    def tv_deconv_poisson_batch(self, imgs, mu, rho=2.0, iterations=50, weights=None, nu=0.0, background=0.0, anisotropic=False, nonneg=False,
                                norm_area=NORM_NONE, full_plane=False, coupled=False):
        """Host arrays [count, rows, cols] in, [count, rows, cols] (full_plane: [count, M, N]) out: tv_deconv_poisson per image with one
        weights plane and one background for all, several per launch (set_batching); coupled: vectorial TV on the images as the
        channels of one picture, the data step per channel (fdr_tv_deconv_poisson_batch_f32)."""
        imgs, cnt, rows, cols, w, orows, ocols, out = self._crop_batch_args(imgs, weights, full_plane)
        prm = TvPoissonBatchParams(float(mu), float(rho), float(nu), float(background), int(iterations), int(bool(anisotropic)),
                                   int(bool(nonneg)), int(norm_area), orows, ocols, TV_COUPLE_CHANNELS if coupled else TV_COUPLE_NONE)
        _check(lib.fdr_tv_deconv_poisson_batch_f32(self._h, _ptr(imgs), rows * cols, cnt, rows, cols, cols, _ptr(w) if w is not None else None,
                                                   cols, _ptr(out), orows * ocols, ocols, ctypes.byref(prm)))
        return out

    def tv_deconv_poisson_batch_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, mu, rho=2.0,
                                    iterations=50, d_weights=None, wstride=0, nu=0.0, background=0.0, anisotropic=False, nonneg=False,
                                    norm_area=NORM_NONE, out_rows=None, out_cols=None, coupled=False, stream=None):
        """fdr_tv_deconv_poisson_batch_f32_dev: tv_deconv_poisson_dev on `count` windows laid out as in tv_deconv_free_batch_dev, in
        launch groups of the plan's `group`; coupled: one shrinkage for the channels of one picture (count <= group, isotropic).
        Asynchronous."""
        prm = TvPoissonBatchParams(float(mu), float(rho), float(nu), float(background), int(iterations), int(bool(anisotropic)),
                                   int(bool(nonneg)), int(norm_area), int(rows if out_rows is None else out_rows),
                                   int(cols if out_cols is None else out_cols), TV_COUPLE_CHANNELS if coupled else TV_COUPLE_NONE)
        _check(lib.fdr_tv_deconv_poisson_batch_f32_dev(self._h, ctypes.c_void_p(int(d_imgs)), img_pitch, count, rows, cols, stride,
                                                       ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                                       ctypes.c_void_p(int(d_out)), out_pitch, out_stride, ctypes.byref(prm), _stream(stream)))

    def tv_deconv_auto_batch(self, imgs, sigma=0.0, rho=2.0, iterations=100, weights=None, tau=0.0, nu=0.0, anisotropic=False, nonneg=False,
                             norm_area=NORM_NONE, full_plane=False, sigmas=None, coupled=False):
        """tv_deconv_auto on host arrays [count, rows, cols], several per launch: sigmas (count entries; None: sigma for all) gives a
        noise level per image, 0 = estimated from that image; every image has its own ball and its own mu_k, also with coupled
        (vectorial TV on the images as the channels of one picture).  Returns (images, [TvAutoResult], traces [count, iterations, 3])
        (fdr_tv_deconv_auto_batch_f32)."""
        imgs, cnt, rows, cols, w, orows, ocols, out = self._crop_batch_args(imgs, weights, full_plane)
        n = max(int(iterations), 0)
        traces = np.zeros((cnt, n, 3), dtype=np.float64)
        sg = None
        if sigmas is not None:
            sg = np.ascontiguousarray(sigmas, dtype=np.float64)
            if sg.shape != (cnt,):
                raise ValueError("sigmas must have one entry per image")
        prm = TvAutoBatchParams(float(sigma), float(tau), float(rho), float(nu), int(iterations), int(bool(anisotropic)), int(bool(nonneg)),
                                int(norm_area), orows, ocols, TV_COUPLE_CHANNELS if coupled else TV_COUPLE_NONE)
        res = (TvAutoResultC * max(cnt, 1))()
        _check(lib.fdr_tv_deconv_auto_batch_f32(self._h, _ptr(imgs), rows * cols, cnt, rows, cols, cols, _ptr(w) if w is not None else None, cols,
                                                _ptr(out), orows * ocols, ocols, ctypes.byref(prm), _ptr(sg) if sg is not None else None, res,
                                                _ptr(traces) if traces.size else None, 3 * n))
        return out, [TvAutoResult(r.sigma, r.target, r.mu, r.discrepancy, r.S) for r in res[:cnt]], traces

    def tv_deconv_auto_batch_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, sigma=0.0, rho=2.0,
                                 iterations=100, d_weights=None, wstride=0, tau=0.0, nu=0.0, anisotropic=False, nonneg=False, norm_area=NORM_NONE,
                                 out_rows=None, out_cols=None, sigmas=None, d_trace=None, trace_pitch=0, coupled=False, stream=None):
        """fdr_tv_deconv_auto_batch_f32_dev: tv_deconv_auto_dev on `count` windows laid out as in tv_deconv_free_batch_dev; sigmas is a
        host sequence of count noise levels or None, image i's trace (3 * iterations doubles) goes to d_trace + i trace_pitch
        (elements) when d_trace is given.  Asynchronous when every noise level is given; an estimated one waits for the stream once."""
        prm = TvAutoBatchParams(float(sigma), float(tau), float(rho), float(nu), int(iterations), int(bool(anisotropic)), int(bool(nonneg)),
                                int(norm_area), int(rows if out_rows is None else out_rows), int(cols if out_cols is None else out_cols),
                                TV_COUPLE_CHANNELS if coupled else TV_COUPLE_NONE)
        sg = None
        if sigmas is not None:
            sg = np.ascontiguousarray(sigmas, dtype=np.float64)
            if sg.shape != (count,):
                raise ValueError("sigmas must have one entry per image")
        _check(lib.fdr_tv_deconv_auto_batch_f32_dev(self._h, ctypes.c_void_p(int(d_imgs)), img_pitch, count, rows, cols, stride,
                                                    ctypes.c_void_p(int(d_weights)) if d_weights else None, int(wstride),
                                                    ctypes.c_void_p(int(d_out)), out_pitch, out_stride, ctypes.byref(prm),
                                                    _ptr(sg) if sg is not None else None, ctypes.c_void_p(int(d_trace)) if d_trace else None,
                                                    int(trace_pitch), _stream(stream)))

    # the motion-blur estimate (include/fdr.h): the power cepstrum of the windowed picture and the blur it shows
    def cepstrum(self, img):
        """c = Re IDFT2(log(|DFT2(hann . img)| + eps)) on the plan (M x N float32); img is the window at the top-left (host array)"""
        img = np.ascontiguousarray(img, dtype=np.float32)
        out = np.empty((self.M, self.N), dtype=np.float32)
        _check(lib.fdr_cepstrum_f32(self._h, _ptr(img), img.shape[0], img.shape[1], img.shape[1], _ptr(out)))
        return out

    def cepstrum_dev(self, d_img, rows, cols, stride, d_out, stream=None):
        """the same on device pointers: d_out is M x N floats (row stride N); asynchronous on `stream`"""
        _check(lib.fdr_cepstrum_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride, ctypes.c_void_p(int(d_out)), _stream(stream)))

    def estimate_motion(self, img, min_length=0, max_length=0, angle_step=0.0, scores=False):
        """the blur length and angle of the window img (host array): a MotionEstimate, and with scores=True also the
        (n_angles, n_lengths) float32 score table.  0 selects an argument's default (3, min(100, min(rows, cols) // 4), 0.5 deg)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        rows, cols = img.shape
        est = MotionEstimateC()
        table = np.empty(_motion_table_shape(rows, cols, min_length, max_length, angle_step), dtype=np.float32) if scores else None
        _check(lib.fdr_estimate_motion_f32(self._h, _ptr(img), rows, cols, cols, int(min_length), int(max_length), float(angle_step),
                                           ctypes.byref(est), _ptr(table) if scores else None))
        res = MotionEstimate(est.length, est.angle_deg, est.score, est.confidence, est.n_angles, est.n_lengths)
        if scores:
            assert table.shape == (est.n_angles, est.n_lengths)
            return res, table
        return res

    def estimate_motion_dev(self, d_img, rows, cols, stride, min_length=0, max_length=0, angle_step=0.0, d_scores=None, stream=None):
        """the same on a device window; d_scores (n_angles x n_lengths floats) may be None.  Returns after the work on `stream`."""
        est = MotionEstimateC()
        _check(lib.fdr_estimate_motion_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride, int(min_length), int(max_length),
                                               float(angle_step), ctypes.byref(est), ctypes.c_void_p(int(d_scores)) if d_scores else None,
                                               _stream(stream)))
        return MotionEstimate(est.length, est.angle_deg, est.score, est.confidence, est.n_angles, est.n_lengths)

    # registering the frames of a burst (include/fdr.h): the translation of every frame against the reference, PSFs accounted for
    def register_frames(self, frames, psfs=None, reference=0, max_shift=0, eps_rel=0.0):
        """the shift of each of the K frames (host arrays of one shape, the window at the plan's top-left) against frames[reference]: a list
        of K FrameShift, the one that belongs in frame k's PSF.  psfs: the K PSFs (one shape, as set_frame_psfs takes them), or None for
        plain phase correlation.  max_shift: the search range in pixels, one number or (rows, cols); 0 selects min(rows, cols) // 4."""
        frames = np.ascontiguousarray(np.stack([np.asarray(f, dtype=np.float32) for f in frames]), dtype=np.float32)
        k, rows, cols = frames.shape
        q, pr, pc = None, 0, 0
        if psfs is not None:
            q = np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.float32) for a in psfs]), dtype=np.float32)
            if q.shape[0] != k:
                raise ValueError("one PSF per frame")
            pr, pc = q.shape[1:]
        mr, mc = (max_shift if isinstance(max_shift, (tuple, list)) else (max_shift, max_shift))
        prm = RegisterParams(int(reference), int(mr), int(mc), float(eps_rel), None)
        out = (FrameShiftC * k)()
        _check(lib.fdr_register_frames_f32(self._h, _ptr(frames), rows * cols, k, rows, cols, cols, _ptr(q) if q is not None else None, pr * pc,
                                           pr, pc, pc, ctypes.byref(prm), out))
        return [FrameShift(o.dy, o.dx, o.peak, o.confidence) for o in out]

    def register_frames_dev(self, d_imgs, img_pitch, count, rows, cols, stride, d_shifts, d_psfs=None, psf_pitch=0, prows=0, pcols=0, pstride=0,
                            reference=0, max_shift=0, eps_rel=0.0, d_corr=None, stream=None):
        """the same on device pointers: frame k at d_imgs + k img_pitch, PSF k at d_psfs + k psf_pitch (None: plain phase correlation),
        the K results (24 bytes each: two doubles, two floats) to the device array d_shifts; d_corr (K planes of M x N floats) receives
        the correlation planes when it is not None.  Reads nothing back.  Asynchronous on `stream`, which travels in the parameter struct."""
        mr, mc = (max_shift if isinstance(max_shift, (tuple, list)) else (max_shift, max_shift))
        prm = RegisterParams(int(reference), int(mr), int(mc), float(eps_rel), int(stream) if stream else None)
        _check(lib.fdr_register_frames_f32_dev(self._h, ctypes.c_void_p(int(d_imgs)), int(img_pitch), int(count), rows, cols, stride,
                                               ctypes.c_void_p(int(d_psfs)) if d_psfs else None, int(psf_pitch), int(prows), int(pcols),
                                               int(pstride), ctypes.byref(prm), ctypes.c_void_p(int(d_shifts)) if d_shifts else None,
                                               ctypes.c_void_p(int(d_corr)) if d_corr else None))

    # the defocus estimate (include/fdr.h): the ring of a disk blur in the same cepstrum, and both estimates from one cepstrum
    def estimate_defocus(self, img, min_diameter=0, max_diameter=0, angle_step=0.0, return_profile=False):
        """the disk radius of the window img (host array): a DefocusEstimate, and with return_profile=True also the profile T
        (n_diameters float32).  0 selects an argument's default, as in estimate_motion."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        rows, cols = img.shape
        est = DefocusEstimateC()
        prof = np.empty(_motion_table_shape(rows, cols, min_diameter, max_diameter, angle_step)[1], dtype=np.float32) if return_profile else None
        _check(lib.fdr_estimate_defocus_f32(self._h, _ptr(img), rows, cols, cols, int(min_diameter), int(max_diameter), float(angle_step),
                                            ctypes.byref(est), _ptr(prof) if return_profile else None))
        res = _defocus_estimate(est)
        if return_profile:
            assert prof.shape == (est.n_diameters,)
            return res, prof
        return res

    def estimate_defocus_dev(self, d_img, rows, cols, stride, min_diameter=0, max_diameter=0, angle_step=0.0, d_profile=None, stream=None):
        """the same on a device window; d_profile (n_diameters floats) may be None.  Returns after the work on `stream`."""
        est = DefocusEstimateC()
        _check(lib.fdr_estimate_defocus_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride, int(min_diameter), int(max_diameter),
                                                float(angle_step), ctypes.byref(est), ctypes.c_void_p(int(d_profile)) if d_profile else None,
                                                _stream(stream)))
        return _defocus_estimate(est)

    def estimate_blur(self, img, min_length=0, max_length=0, motion_step=0.0, min_diameter=0, max_diameter=0, defocus_step=0.0):
        """both estimates of the window img (host array) from one cepstrum: BlurEstimate(kind, MotionEstimate, DefocusEstimate), each
        part what estimate_motion / estimate_defocus return, kind one of BLUR_NONE, BLUR_MOTION, BLUR_DEFOCUS"""
        img = np.ascontiguousarray(img, dtype=np.float32)
        mo, de, kind = MotionEstimateC(), DefocusEstimateC(), ctypes.c_int(0)
        _check(lib.fdr_estimate_blur_f32(self._h, _ptr(img), img.shape[0], img.shape[1], img.shape[1], int(min_length), int(max_length),
                                         float(motion_step), int(min_diameter), int(max_diameter), float(defocus_step), ctypes.byref(mo),
                                         ctypes.byref(de), ctypes.byref(kind)))
        return BlurEstimate(kind.value, MotionEstimate(mo.length, mo.angle_deg, mo.score, mo.confidence, mo.n_angles, mo.n_lengths),
                            _defocus_estimate(de))

    def estimate_blur_dev(self, d_img, rows, cols, stride, min_length=0, max_length=0, motion_step=0.0, min_diameter=0, max_diameter=0,
                          defocus_step=0.0, stream=None):
        """the same on a device window.  Returns after the work on `stream`."""
        mo, de, kind = MotionEstimateC(), DefocusEstimateC(), ctypes.c_int(0)
        _check(lib.fdr_estimate_blur_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride, int(min_length), int(max_length),
                                             float(motion_step), int(min_diameter), int(max_diameter), float(defocus_step), ctypes.byref(mo),
                                             ctypes.byref(de), ctypes.byref(kind), _stream(stream)))
        return BlurEstimate(kind.value, MotionEstimate(mo.length, mo.angle_deg, mo.score, mo.confidence, mo.n_angles, mo.n_lengths),
                            _defocus_estimate(de))

    # choosing the regularisation weight (include/fdr.h): noise estimate, residual / trace curve, discrepancy principle and GCV
    def noise_sigma(self, img):
        """Immerkaer's estimate of the noise standard deviation of img (host array, at least 3 x 3), on the plan's device"""
        img = np.ascontiguousarray(img, dtype=np.float32)
        sigma = ctypes.c_double()
        _check(lib.fdr_noise_sigma_f32(self.device, _ptr(img), img.shape[0], img.shape[1], img.shape[1], ctypes.byref(sigma)))
        return sigma.value

    def noise_sigma_dev(self, d_img, rows, cols, stride, stream=None):
        """the same on a device window.  Returns after the work on `stream`."""
        sigma = ctypes.c_double()
        _check(lib.fdr_noise_sigma_f32_dev(self.device, ctypes.c_void_p(int(d_img)), rows, cols, stride, ctypes.byref(sigma), _stream(stream)))
        return sigma.value

    def reg_curve(self, img, K, gamma):
        """(residual, trace) as float64 arrays: rho and trace of the CLS filter with each pair (K[i], gamma[i]) on the window img
        (host array), with the operator PSF of set_operator_psf*; K and gamma broadcast against each other"""
        img = np.ascontiguousarray(img, dtype=np.float32)
        K, gamma = np.broadcast_arrays(np.asarray(K, dtype=np.float64), np.asarray(gamma, dtype=np.float64))
        shape = K.shape
        K, gamma = np.ascontiguousarray(K).ravel(), np.ascontiguousarray(gamma).ravel()
        rho, tr = np.empty(K.size, dtype=np.float64), np.empty(K.size, dtype=np.float64)
        _check(lib.fdr_reg_curve_f32(self._h, _ptr(img), img.shape[0], img.shape[1], img.shape[1], _ptr(K), _ptr(gamma), K.size, _ptr(rho),
                                     _ptr(tr)))
        return rho.reshape(shape), tr.reshape(shape)

    def reg_curve_dev(self, d_img, rows, cols, stride, K, gamma, stream=None):
        """the same on a device window (K, gamma: equally long host sequences).  Returns after the work on `stream`."""
        K, gamma = np.ascontiguousarray(K, dtype=np.float64).ravel(), np.ascontiguousarray(gamma, dtype=np.float64).ravel()
        rho, tr = np.empty(K.size, dtype=np.float64), np.empty(K.size, dtype=np.float64)
        _check(lib.fdr_reg_curve_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride, _ptr(K), _ptr(gamma), min(K.size, gamma.size),
                                         _ptr(rho), _ptr(tr), _stream(stream)))
        return rho, tr

    @staticmethod
    def _reg_params(method, param, fixed, sigma, tau, lo, hi, n_grid, refine):
        return RegParams(int(method), int(param), float(fixed), float(sigma), float(tau), float(lo), float(hi), int(n_grid), int(refine))

    def choose_regularisation(self, img, method=REG_GCV, param=REG_PARAM_GAMMA, fixed=0.0, sigma=0.0, tau=0.0, lo=0.0, hi=0.0, n_grid=0,
                              refine=-1):
        """K or gamma (param) of the CLS filter for the window img (host array), by the discrepancy principle or GCV (method), with
        the other weight at `fixed`: a RegChoice.  0 selects an argument's default (sigma: estimated, tau 1, range 1e-8 .. 1e2, 32
        candidates per round; refine -1: 2 rounds).  The value goes into set_psf(psf, K, gamma)."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        prm = self._reg_params(method, param, fixed, sigma, tau, lo, hi, n_grid, refine)
        c = RegChoiceC()
        _check(lib.fdr_choose_reg_f32(self._h, _ptr(img), img.shape[0], img.shape[1], img.shape[1], ctypes.byref(prm), ctypes.byref(c)))
        return RegChoice(c.value, c.sigma, c.residual, c.trace, c.gcv, c.flags, c.evaluations)

    def choose_regularisation_dev(self, d_img, rows, cols, stride, method=REG_GCV, param=REG_PARAM_GAMMA, fixed=0.0, sigma=0.0, tau=0.0,
                                  lo=0.0, hi=0.0, n_grid=0, refine=-1, stream=None):
        """the same on a device window.  Returns after the work on `stream`."""
        prm = self._reg_params(method, param, fixed, sigma, tau, lo, hi, n_grid, refine)
        c = RegChoiceC()
        _check(lib.fdr_choose_reg_f32_dev(self._h, ctypes.c_void_p(int(d_img)), rows, cols, stride, ctypes.byref(prm), ctypes.byref(c),
                                          _stream(stream)))
        return RegChoice(c.value, c.sigma, c.residual, c.trace, c.gcv, c.flags, c.evaluations)

    def set_concurrency(self, nstreams):
        """Batched mode: alternate images over `nstreams` private workspaces / internal streams."""
        _check(lib.fdr_plan_set_concurrency(self._h, int(nstreams)))

    def set_batching(self, nstreams, group):
        """Batched mode: `nstreams` internal streams, `group` images per pass-B' launch (fast mode)."""
        _check(lib.fdr_plan_set_batching(self._h, int(nstreams), int(group)))

    # transforms
    def fft2d(self, x, inverse=False):
        """fft_gpu::my_dft2D(Mat&, bool): unscaled, complex64 [M, N]."""
        a = np.ascontiguousarray(x, dtype=np.complex64).copy()
        assert a.shape == (self.M, self.N)
        _check(lib.fdr_fft2d_c2c(self._h, _ptr(a), int(inverse)))
        return a

    def fft2d_dev(self, d_ptr, inverse=False, stream=None):
        _check(lib.fdr_fft2d_c2c_dev(self._h, ctypes.c_void_p(int(d_ptr)), int(inverse), _stream(stream)))

    def set_option(self, option, value):
        _check(lib.fdr_plan_set_option(self._h, int(option), int(value)))

    def phase_times(self, reset=False):
        """The reference Profiler's six buckets (ms) accumulated on this plan: dict alloc/h2d/pre/compute/d2h/post."""
        ms = (ctypes.c_float * len(PHASES))()
        _check(lib.fdr_plan_phase_times(self._h, ms, int(reset)))
        return {k: float(ms[i]) for i, k in enumerate(PHASES)}

    # profiling
    def profile(self, enable=True):
        _check(lib.fdr_plan_profile(self._h, int(enable)))

    def pass_times(self):
        n = ctypes.c_int(0)
        ms = (ctypes.c_float * MAX_PASSES)()
        names = (ctypes.c_char_p * MAX_PASSES)()
        cnt = (ctypes.c_int * MAX_PASSES)()
        _check(lib.fdr_plan_pass_times(self._h, ctypes.byref(n), ms, names, cnt))
        return [(names[i].decode(), float(ms[i]), int(cnt[i])) for i in range(n.value)]


def fft1d(x, inverse=False, mode=MODE_PARITY):
    """fft_gpu::fft_radix2_kernel / transform_row_kernel: unscaled 1-D transform of a host array."""
    a = np.ascontiguousarray(x, dtype=np.complex64).copy()
    _check(lib.fdr_fft1d_c2c(_ptr(a), a.size, int(inverse), int(mode)))
    return a


def dft_naive(x, inverse=False):
    """fft_gpu::dft_naive_kernel"""
    a = np.ascontiguousarray(x, dtype=np.complex64).copy()
    _check(lib.fdr_dft_naive_c2c(_ptr(a), a.size, int(inverse)))
    return a


def synth_image_dev(d_out, count, seed, first_index=0, device=0, stream=None):
    _check(lib.fdr_synth_image_dev(int(device), ctypes.c_uint64(seed), ctypes.c_uint64(first_index), count,
                                   ctypes.c_void_p(int(d_out)), _stream(stream)))


# ---- fft/fft.hpp mirrors (fft_gpu namespace) --------------------------------------------------
def applyWhiteBalance_u8(orig_bgr, restored_bgr, device=0):
    """The drivers' colour epilogue (serial.cpp:43-54 / gpu.cpp:123-137 with utils.hpp:55-71) on the device:
    two lists of three float planes (B, G, R in [0,1]) -> uint8 [rows, cols, 3] BGR."""
    o = [np.ascontiguousarray(c, dtype=np.float32) for c in orig_bgr]
    r = [np.ascontiguousarray(c, dtype=np.float32) for c in restored_bgr]
    rows, cols = o[0].shape
    out = np.empty((rows, cols, 3), dtype=np.uint8)
    po = (ctypes.c_void_p * 3)(*[c.ctypes.data for c in o])
    pr = (ctypes.c_void_p * 3)(*[c.ctypes.data for c in r])
    _check(lib.fdr_white_balance_u8(int(device), po, pr, rows, cols, cols, ctypes.c_void_p(out.ctypes.data), 3 * cols))
    return out


def host_alloc(shape, dtype=np.float32):
    """numpy array in pinned host memory (fdr_host_alloc; the reference's cudaMallocHost buffers,
    fft/fft_gpu.cu:306-308).  Freed when the array (and every view of it) is garbage collected."""
    import weakref
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = ctypes.c_void_p()
    _check(lib.fdr_host_alloc(n, ctypes.byref(p)))
    buf = (ctypes.c_char * n).from_address(p.value)
    weakref.finalize(buf, lib.fdr_host_free, ctypes.c_void_p(p.value))
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def _pad_plan_size(rows, cols, prows, pcols):
    """the plan of the Wiener entry points with pad=PAD_SMOOTH: the next powers of two of rows + prows - 1 and cols + pcols - 1, as
    _rlfree_plan_size -- the margin is then at least the PSF's reach.  A picture whose sides are powers of two already gets a plan of
    4x the area (and about 4x the time) of its PAD_ZERO plan."""
    return _rlfree_plan_size(rows, cols, prows, pcols)


def _wiener_plan(rows, cols, psf, mode, device, pad):
    """the plan of wienerDeblur_myfft / _RGB_optimized for one picture size, its padding mode set"""
    if pad == PAD_ZERO:
        return Plan(nextPowerOfTwo(rows), nextPowerOfTwo(cols), mode, device)
    if pad != PAD_SMOOTH:
        raise ValueError("pad must be PAD_ZERO or PAD_SMOOTH")
    if mode != MODE_FAST:
        raise ValueError("pad=PAD_SMOOTH needs mode=MODE_FAST (parity mode is bit-identical to ./serial, which pads with zeros)")
    prows, pcols = np.shape(psf)
    p = Plan(*_pad_plan_size(rows, cols, prows, pcols), mode, device)
    try:
        p.set_option(OPT_PAD_MODE, PAD_SMOOTH)
    except Exception:
        p.close()
        raise
    return p


def wienerDeblur_myfft(img, psf, K, mode=MODE_PARITY, device=0, norm_area=NORM_PADDED, cls_gamma=0.0, pad=PAD_ZERO):
    """One channel the way the DRIVERS call the operator: pad to powers of two (serial.cpp:36 / fft_gpu.cu:287-288, on the
    device), restore, normalise (default: over the padded area, serial.cpp:34-39), crop.  cls_gamma > 0 (MODE_FAST): the
    constrained least-squares filter instead of the Wiener filter (Plan.set_psf).  pad=PAD_SMOOTH (MODE_FAST): the picture is
    continued smoothly into the padding (OPT_PAD_MODE) of a plan of _pad_plan_size -- for a crop of a larger scene."""
    img = np.asarray(img, dtype=np.float32)
    with _wiener_plan(img.shape[0], img.shape[1], psf, mode, device, pad) as p:
        p.set_psf(psf, K, gamma=cls_gamma)
        return p.wiener(img, norm_area)


def wienerDeblur_myfft_unpadded(img, psf, K, mode=MODE_PARITY, device=0, mixed_radix=False, cls_gamma=0.0):
    """fft_serial::wienerDeblur_myfft called DIRECTLY on a channel of any size (fft/fft_serial.cpp:141-261): pad to
    getOptimalDFTSize (2^a 3^b 5^c; a non-power-of-two dimension is transformed by the naive DFT, :100-101), restore,
    crop to the input size, normalise over the cropped plane (:243-246).  mixed_radix=True with MODE_FAST: the
    mixed-radix FFTs of FLAG_MIXED_RADIX instead of the naive DFT (dimensions up to 8192).  cls_gamma > 0: the constrained
    least-squares filter (fast-mode plans only: a naive-DFT plan is a parity plan and refuses it)."""
    img = np.asarray(img, dtype=np.float32)
    M, N = getOptimalDFTSize(img.shape[0]), getOptimalDFTSize(img.shape[1])
    flags = 0 if (isPowerOfTwo(M) and isPowerOfTwo(N)) else FLAG_ANY_SIZE
    if mixed_radix and mode == MODE_FAST:
        flags |= FLAG_MIXED_RADIX
    with Plan(M, N, mode, device, flags=flags) as p:
        p.set_psf(psf, K, gamma=cls_gamma)
        return p.wiener(img, NORM_CROPPED)


def _rl_plan_size(rows, cols):
    """the plan richardsonLucy_myfft pads to: the next power of two, at least 8 rows and 32 columns"""
    return max(8, nextPowerOfTwo(rows)), max(32, nextPowerOfTwo(cols))


def richardsonLucy_myfft(img, psf, iterations, device=0, norm_area=NORM_NONE, accelerate=False):
    """Richardson-Lucy deconvolution of one channel: pad each dimension to the next power of two (at least 8 rows and 32
    columns; the padding is zero and stays zero), `iterations` steps on the device, crop.  psf lies top-left in the plan, as
    for the Wiener calls.  accelerate: the accelerated iteration of Plan.richardson_lucy."""
    img = np.asarray(img, dtype=np.float32)
    M, N = _rl_plan_size(img.shape[0], img.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        return p.richardson_lucy(img, iterations, norm_area, accelerate=accelerate)


def _rlfree_plan_size(rows, cols, prows, pcols):
    """the plan richardsonLucyFree_myfft uses: the next powers of two of rows + prows - 1 and cols + pcols - 1 (the far borders of the
    window then do not couple through the wrap), at least 8 rows and 32 columns"""
    return max(8, nextPowerOfTwo(rows + prows - 1)), max(32, nextPowerOfTwo(cols + pcols - 1))


def richardsonLucyFree_myfft(img, psf, iterations, weights=None, sigma=RL_SIGMA, device=0, norm_area=NORM_NONE, full_plane=False,
                             accelerate=False):
    """Free-boundary, weighted Richardson-Lucy of one channel that is a crop of a larger scene: a plan with room for the PSF's
    reach beyond the window, `iterations` steps on the device, the window (or with full_plane the whole plan) back.  psf lies
    top-left in the plan, as for the Wiener calls; weights and accelerate as Plan.richardson_lucy_free."""
    img = np.asarray(img, dtype=np.float32)
    psf = np.asarray(psf, dtype=np.float32)
    M, N = _rlfree_plan_size(img.shape[0], img.shape[1], psf.shape[0], psf.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        return p.richardson_lucy_free(img, iterations, weights, sigma, norm_area, full_plane, accelerate=accelerate)


def spectrum_sum_dev(d_dst, d_srcs, n_floats, accumulate=False, device=0, stream=None):
    """fdr_spectrum_sum_f32_dev: dst[i] = (accumulate ? dst[i] : src_0[i]) + the remaining sources in ascending order, plain float32
    adds, i < n_floats (even).  d_srcs: 1 .. 8 device pointers, 16-byte aligned as d_dst; d_dst may be one of them.  Asynchronous."""
    arr = (ctypes.c_void_p * len(d_srcs))(*[int(q) for q in d_srcs])
    _check(lib.fdr_spectrum_sum_f32_dev(int(device), ctypes.c_void_p(int(d_dst)), arr, len(d_srcs), int(n_floats), int(bool(accumulate)),
                                        _stream(stream)))


def _frames_plan_size(rows, cols, psfs, pad=0):
    """the plan of richardsonLucyFree_myfft for the largest of the PSFs (with `pad` more on every side: the room of a registration)"""
    return _rlfree_plan_size(rows, cols, max(q.shape[0] for q in psfs) + 2 * pad, max(q.shape[1] for q in psfs) + 2 * pad)


def psf_shift(psfs, shifts, pad_rows, pad_cols=None, device=0):
    """fdr_psf_shift_f32: the K PSFs (one shape prows x pcols) shifted by the K shifts (FrameShift or (dy, dx) pairs) into K planes of
    (prows + 2 pad_rows) x (pcols + 2 pad_cols): PSF k at offset (pad_rows + dy, pad_cols + dx) by bilinear weights, the sum kept.  A
    shift outside [-pad, pad - 1] is clamped, a NaN is taken as 0."""
    q = np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.float32) for a in psfs]), dtype=np.float32)
    k, pr, pc = q.shape
    pad_cols = pad_rows if pad_cols is None else pad_cols
    if len(shifts) != k:
        raise ValueError("one shift per PSF")
    sh = (FrameShiftC * k)(*[FrameShiftC(float(t[0]), float(t[1]), 0.0, 0.0) for t in shifts])
    orows, ocols = pr + 2 * int(pad_rows), pc + 2 * int(pad_cols)
    out = np.empty((k, max(orows, 1), max(ocols, 1)), dtype=np.float32)
    prm = PsfShiftParams(int(pad_rows), int(pad_cols), None)
    _check(lib.fdr_psf_shift_f32(int(device), _ptr(q), pr * pc, k, pr, pc, pc, sh, ctypes.byref(prm), _ptr(out), out.shape[1] * out.shape[2],
                                 out.shape[2]))
    return out


def psf_shift_dev(d_psfs, psf_pitch, count, prows, pcols, pstride, d_shifts, pad_rows, pad_cols, d_out, out_pitch, out_stride, device=0,
                  stream=None):
    """the same on device pointers, the shifts read from device memory (straight from Plan.register_frames_dev): PSF k at d_psfs + k
    psf_pitch to d_out + k out_pitch.  Asynchronous on `stream`, which travels in the parameter struct."""
    prm = PsfShiftParams(int(pad_rows), int(pad_cols), int(stream) if stream else None)
    _check(lib.fdr_psf_shift_f32_dev(int(device), ctypes.c_void_p(int(d_psfs)) if d_psfs else None, int(psf_pitch), int(count), prows, pcols,
                                     pstride, ctypes.c_void_p(int(d_shifts)) if d_shifts else None, ctypes.byref(prm),
                                     ctypes.c_void_p(int(d_out)) if d_out else None, int(out_pitch), out_stride))


def registerFrames(imgs, psfs=None, reference=0, max_shift=0, eps_rel=0.0, device=0):
    """the translation of every frame of a burst against imgs[reference] (fdr_register_frames_f32): a list of FrameShift, frame k's the
    shift that belongs in its PSF (psf_shift).  imgs: K pictures of one size, one channel or rows x cols x channels (the per-pixel mean
    is used); psfs: the K known PSFs, whose phases the estimate undoes, or None for plain phase correlation (right only for frames of one
    common PSF).  The plan is the smallest 2^a 3^b 5^c size of each dimension (at least 32), FLAG_MIXED_RADIX."""
    frames = [np.asarray(f, dtype=np.float32) for f in imgs]
    frames = [f.mean(axis=2, dtype=np.float32) if f.ndim == 3 else f for f in frames]
    rows, cols = frames[0].shape
    if psfs is not None:
        psfs = _frame_psfs(psfs)
        rows, cols = max(rows, psfs.shape[1]), max(cols, psfs.shape[2])
    M, N = _motion_plan_size(rows, cols)
    with Plan(M, N, MODE_FAST, device, flags=FLAG_MIXED_RADIX) as p:
        return p.register_frames(frames, psfs, reference, max_shift, eps_rel)


def _register_pad(rows, cols, max_shift):
    """the padding that holds every result of a registration with this range: max_shift + 2"""
    return (int(max_shift) or min(rows, cols) // 4) + 2


def _registered_psfs(p, frames, psfs, max_shift):
    """register=True of the multi-frame calls on the plan p: the frames registered against frame 0 with their PSFs, every PSF shifted
    by its frame's estimate (psf_shift) and laid into an M x N plane rolled back by the padding, so that the PSFs keep the origin the
    caller gave them and the restoration stays where frame 0 is.  Returns the K planes."""
    k, pr, pc = psfs.shape
    pad = _register_pad(frames[0].shape[0], frames[0].shape[1], max_shift)
    if pr + 2 * pad > p.M or pc + 2 * pad > p.N:
        raise ValueError("register=True needs compact PSFs: PSF + 2 (max_shift + 2) must fit the plan")
    shifts = p.register_frames(frames, psfs, 0, max_shift)
    shifted = psf_shift(psfs, shifts, pad, pad, device=p.device)
    planes = np.zeros((k, p.M, p.N), dtype=np.float32)
    planes[:, :pr + 2 * pad, :pc + 2 * pad] = shifted
    return np.roll(planes, (-pad, -pad), axis=(1, 2))


def _frame_psfs(psfs):
    """K PSFs padded with zeros (bottom, right) to one shape: a PSF lies top-left in the plan, so the padding changes nothing"""
    psfs = [np.asarray(q, dtype=np.float32) for q in psfs]
    pr, pc = max(q.shape[0] for q in psfs), max(q.shape[1] for q in psfs)
    out = np.zeros((len(psfs), pr, pc), dtype=np.float32)
    for k, q in enumerate(psfs):
        out[k, :q.shape[0], :q.shape[1]] = q
    return out


def richardsonLucyFrames_myfft(frames, psfs, iterations, weights=None, tv_lambda=0.0, tv_eps=0.0, sigma=RL_SIGMA, device=0,
                               norm_area=NORM_NONE, full_plane=False, register=False, max_shift=0):
    """Joint free-boundary Richardson-Lucy of K (1 .. MAX_FRAMES) exposures of one scene, frame k blurred by psfs[k] (top-left in
    the plan, as for richardsonLucyFree_myfft; sums not normalised: a PSF's sum is its frame's relative exposure): the plan of
    richardsonLucyFree_myfft, the frame tables, `iterations` steps, the window back.  weights: None, one plane, or one per frame;
    tv_lambda > 0 adds the TV prior (without it the joint iteration fits the noise within a few steps, as plain RL does).
    register=True: the frames are not registered to each other (hand shake): each frame's translation against frame 0 is estimated
    with the PSFs (Plan.register_frames, search range max_shift) and folded into its PSF before the restoration."""
    frames = [np.asarray(f, dtype=np.float32) for f in frames]
    psfs = _frame_psfs(psfs)
    pad = _register_pad(frames[0].shape[0], frames[0].shape[1], max_shift) if register else 0
    M, N = _frames_plan_size(frames[0].shape[0], frames[0].shape[1], psfs, pad)
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_frame_psfs(_registered_psfs(p, frames, psfs, max_shift) if register else psfs)
        p.set_batching(1, min(len(frames), 8))
        return p.richardson_lucy_frames(frames, iterations, weights, tv_lambda, tv_eps, sigma, norm_area, full_plane)


def richardsonLucyFrames_RGB(frames, psfs, iterations, weights=None, tv_lambda=0.0, tv_eps=0.0, sigma=RL_SIGMA, device=0, norm_area=NORM_NONE,
                             register=False, max_shift=0):
    """fft_gpu::richardsonLucyFrames_RGB: frames[k] is the list of channel planes of exposure k (every exposure the same channels
    and size).  Returns the list of restored channels: the frame tables are set once, then one joint call per channel (the bits of
    richardsonLucyFrames_myfft on that channel).  register=True: as there, the shifts estimated once on the mean of the channels."""
    if not frames or not frames[0]:
        return []
    psfs = _frame_psfs(psfs)
    r, c = np.asarray(frames[0][0]).shape
    M, N = _frames_plan_size(r, c, psfs, _register_pad(r, c, max_shift) if register else 0)
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_frame_psfs(_registered_psfs(p, _channel_means(frames), psfs, max_shift) if register else psfs)
        p.set_batching(1, min(len(frames), 8))
        return [p.richardson_lucy_frames([f[ch] for f in frames], iterations, weights, tv_lambda, tv_eps, sigma, norm_area)
                for ch in range(len(frames[0]))]


def _channel_means(frames):
    """per exposure the per-pixel mean of its channel planes: what register=True of the _RGB calls registers"""
    return [np.mean(np.stack([np.asarray(ch, dtype=np.float32) for ch in f]), axis=0, dtype=np.float32) for f in frames]


def tvDeblurFrames_myfft(frames, psfs, mu, iterations, weights=None, data_term=TV_FRAMES_LEAST_SQUARES, background=0.0, rho=2.0, nu=0.0,
                         anisotropic=False, nonneg=False, device=0, norm_area=NORM_NONE, full_plane=False, register=False, max_shift=0):
    """Joint TV deconvolution of K (1 .. MAX_FRAMES) exposures of one scene, frame k blurred by psfs[k] (top-left in the plan; sums
    not normalised: a PSF's sum is its frame's relative exposure): the plan of richardsonLucyFrames_myfft, the frame tables,
    `iterations` ADMM steps of  min mu sum_k Phi_k(blur_k(x)) + TV(x),  the window back.  weights: None, one plane, or one per frame.
    register=True: as richardsonLucyFrames_myfft, every frame's translation against frame 0 estimated and folded into its PSF."""
    frames = [np.asarray(f, dtype=np.float32) for f in frames]
    psfs = _frame_psfs(psfs)
    pad = _register_pad(frames[0].shape[0], frames[0].shape[1], max_shift) if register else 0
    M, N = _frames_plan_size(frames[0].shape[0], frames[0].shape[1], psfs, pad)
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_frame_psfs(_registered_psfs(p, frames, psfs, max_shift) if register else psfs)
        p.set_batching(1, min(len(frames), 8))
        return p.tv_deconv_frames(frames, mu, iterations, weights, data_term, background, rho, nu, anisotropic, nonneg, norm_area, full_plane)


def tvDeblurFrames_RGB(frames, psfs, mu, iterations, weights=None, data_term=TV_FRAMES_LEAST_SQUARES, background=0.0, rho=2.0, nu=0.0,
                       anisotropic=False, nonneg=False, device=0, norm_area=NORM_NONE, register=False, max_shift=0):
    """fft_gpu::tvDeblurFrames_RGB: frames[k] is the list of channel planes of exposure k (every exposure the same channels and
    size).  Returns the list of restored channels: the frame tables are set once, then one joint call per channel (the bits of
    tvDeblurFrames_myfft on that channel).  register=True: as there, the shifts estimated once on the mean of the channels."""
    if not frames or not frames[0]:
        return []
    psfs = _frame_psfs(psfs)
    r, c = np.asarray(frames[0][0]).shape
    M, N = _frames_plan_size(r, c, psfs, _register_pad(r, c, max_shift) if register else 0)
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_frame_psfs(_registered_psfs(p, _channel_means(frames), psfs, max_shift) if register else psfs)
        p.set_batching(1, min(len(frames), 8))
        return [p.tv_deconv_frames([f[ch] for f in frames], mu, iterations, weights, data_term, background, rho, nu, anisotropic, nonneg,
                                   norm_area)
                for ch in range(len(frames[0]))]


def rl_tv_factor_dev(d_u, rows, cols, stride, d_out, out_stride, lam, eps=0.0, d_w=None, device=0, stream=None):
    """fdr_rl_tv_factor_f32_dev: d_out = w / (1 - lam div(grad u / sqrt(|grad u|^2 + eps^2))) on the rows x cols device window d_u (row
    stride `stride`; d_w, same stride, None = 1), forward differences replicated at the far edges.  Any size, stride and alignment;
    needs no plan.  Asynchronous."""
    _check(lib.fdr_rl_tv_factor_f32_dev(int(device), ctypes.c_void_p(int(d_u)), rows, cols, stride, ctypes.c_void_p(int(d_w)) if d_w else None,
                                        float(lam), float(eps), ctypes.c_void_p(int(d_out)), out_stride, _stream(stream)))


def richardsonLucyTV_myfft(img, psf, iterations, lam, eps=0.0, free_boundary=False, weights=None, cov_sigma=RL_SIGMA, device=0,
                           norm_area=NORM_NONE, full_plane=False):
    """Richardson-Lucy with a total-variation prior of one channel: the plan of richardsonLucy_myfft, or with free_boundary (the form
    for a crop of a larger scene; weights as richardsonLucyFree_myfft) that of richardsonLucyFree_myfft, `iterations` steps, crop.
    lam in 0 .. RLTV_MAX_LAMBDA (0.01 is a usual value for a picture scaled to 1); eps in the units of img, 0 = RLTV_EPS."""
    img = np.asarray(img, dtype=np.float32)
    psf = np.asarray(psf, dtype=np.float32)
    if free_boundary:
        M, N = _rlfree_plan_size(img.shape[0], img.shape[1], psf.shape[0], psf.shape[1])
    else:
        M, N = _rl_plan_size(img.shape[0], img.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        return p.richardson_lucy_tv(img, iterations, lam, eps, free_boundary, weights, cov_sigma, norm_area, full_plane)


def richardsonLucyTV_RGB(channels, psf, iterations, lam, eps=0.0, free_boundary=False, weights=None, coupled=False, cov_sigma=RL_SIGMA,
                         device=0, norm_area=NORM_NONE):
    """fft_gpu::richardsonLucyTV_RGB: replaces every element of `channels` (float32 planes of one size, at most 8) in place with its
    Richardson-Lucy estimate under the TV prior, from one plan and one batched call: the bits of richardsonLucyTV_myfft per channel,
    or with coupled=True the channels under one vectorial TV prior (one norm for all, so an edge falls in the same place in every
    channel).  free_boundary and weights as richardsonLucyTV_myfft; one weights plane serves every channel."""
    if not channels:
        return
    psf = np.asarray(psf, dtype=np.float32)
    r, c = np.asarray(channels[0]).shape
    if free_boundary:
        M, N = _rlfree_plan_size(r, c, psf.shape[0], psf.shape[1])
    else:
        M, N = _rl_plan_size(r, c)
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        p.set_batching(1, min(len(channels), 8))
        out = p.richardson_lucy_tv_batch(np.stack([np.asarray(ch, dtype=np.float32) for ch in channels]), iterations, lam, eps, free_boundary,
                                         weights, cov_sigma, norm_area, couple=TV_COUPLE_CHANNELS if coupled else TV_COUPLE_NONE)
    for i in range(len(channels)):
        channels[i] = out[i]


def psf_gaussian(size, sigma=0.0):
    """fdr_psf_gaussian: the size x size Gaussian PSF centred at size // 2 (the centre of motionBlurKernel), sum 1; sigma = 0 selects
    size / 4.  The usual start of richardsonLucyBlind_myfft.  Computed on the host: needs no device."""
    out = np.empty((int(size), int(size)), dtype=np.float32) if size > 0 else np.empty((1, 1), dtype=np.float32)
    _check(lib.fdr_psf_gaussian(int(size), float(sigma), _ptr(out)))
    return out


def richardsonLucyBlind_myfft(img, psf_start=None, psf_size=9, iterations=30, free_boundary=False, mask=None, psf_hold=0, psf_sigma=0.0,
                              cov_sigma=RL_SIGMA, device=0, norm_area=NORM_NONE):
    """Blind Richardson-Lucy of one channel: refines the PSF together with the picture and returns (image, psf).  psf_start: the
    start PSF (None: psf_gaussian(psf_size, psf_sigma)); zeros in it stay zeros, so it also masks the support.  The plan is that of
    richardsonLucy_myfft, or with free_boundary (the form for a crop of a larger scene) of richardsonLucyFree_myfft; mask (img.shape,
    in [0, 1]; free_boundary only) are the pixel weights.  This refines a PSF, it does not find one from nothing."""
    img = np.asarray(img, dtype=np.float32)
    psf = psf_gaussian(psf_size, psf_sigma) if psf_start is None else np.asarray(psf_start, dtype=np.float32)
    if mask is not None and not free_boundary:
        raise ValueError("mask needs free_boundary=True")
    if free_boundary:
        M, N = _rlfree_plan_size(img.shape[0], img.shape[1], psf.shape[0], psf.shape[1])
    else:
        M, N = _rl_plan_size(img.shape[0], img.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        return p.richardson_lucy_blind(img, psf, iterations, free_boundary, mask, psf_hold, cov_sigma, norm_area)


def richardsonLucyAuto_myfft(img, psf, max_iterations, rule=RL_STOP_RESIDUAL, sigma=0.0, gain=0.0, tau=0.0, check_every=0, free_boundary=False,
                             accelerate=False, weights=None, cov_sigma=RL_SIGMA, device=0, norm_area=NORM_NONE):
    """Richardson-Lucy of one channel that chooses its own iteration count: the plan of richardsonLucy_myfft (free_boundary: of
    richardsonLucyFree_myfft), at most max_iterations steps stopped by `rule` as Plan.richardson_lucy_auto describes, crop.  Returns
    (image, RlAutoResult, trace)."""
    img = np.asarray(img, dtype=np.float32)
    psf = np.asarray(psf, dtype=np.float32)
    if free_boundary:
        M, N = _rlfree_plan_size(img.shape[0], img.shape[1], psf.shape[0], psf.shape[1])
    else:
        M, N = _rl_plan_size(img.shape[0], img.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        return p.richardson_lucy_auto(img, max_iterations, rule, sigma, gain, tau, check_every, free_boundary, accelerate, weights, cov_sigma,
                                      norm_area)


def tvDeblur_myfft(img, psf, mu, rho=2.0, iterations=50, anisotropic=False, nonneg=False, device=0, norm_area=NORM_NONE):
    """Total-variation deconvolution of one channel: the plan of richardsonLucy_myfft (each dimension padded to the next power of
    two, at least 8 rows and 32 columns), `iterations` ADMM steps on the device, crop.  psf lies top-left in the plan."""
    img = np.asarray(img, dtype=np.float32)
    M, N = _rl_plan_size(img.shape[0], img.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        return p.tv_deconv(img, mu, rho, iterations, anisotropic, nonneg, norm_area)


def tvDeblur_RGB(channels, psf, mu, rho=2.0, iterations=50, nonneg=False, device=0, norm_area=NORM_NONE, coupled=False):
    """fft_gpu::tvDeblur_RGB: replaces every element of `channels` (float32 planes of one size, at most 8 when coupled) in place with
    its total-variation estimate, from one plan (that of richardsonLucy_RGB) and one launch per pass -- the bits of tvDeblur_myfft per
    channel, or with coupled the vectorial TV of the picture: one shrinkage by the joint gradient norm of the channels."""
    if not channels:
        return
    r, c = np.asarray(channels[0]).shape
    M, N = _rl_plan_size(r, c)
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        p.set_batching(1, min(len(channels), 8))
        out = p.tv_deconv_batch(np.stack([np.asarray(c, dtype=np.float32) for c in channels]), mu, rho, iterations, False, nonneg, norm_area, coupled)
    for i in range(len(channels)):
        channels[i] = out[i]


def tvDeblurFree_myfft(img, psf, mu, rho=2.0, iterations=50, weights=None, nu=0.0, anisotropic=False, nonneg=False, device=0,
                       norm_area=NORM_NONE, full_plane=False):
    """Free-boundary, weighted total-variation deconvolution of one channel that is a crop of a larger scene: the plan of
    richardsonLucyFree_myfft (room for the PSF's reach beyond the window), `iterations` ADMM steps on the device, the window (or with
    full_plane the whole plan) back.  psf lies top-left in the plan; weights as Plan.tv_deconv_free."""
    img = np.asarray(img, dtype=np.float32)
    psf = np.asarray(psf, dtype=np.float32)
    M, N = _rlfree_plan_size(img.shape[0], img.shape[1], psf.shape[0], psf.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        return p.tv_deconv_free(img, mu, rho, iterations, weights, nu, anisotropic, nonneg, norm_area, full_plane)


def tvDeblurFree_RGB(channels, psf, mu, rho=2.0, iterations=50, nonneg=False, device=0, norm_area=NORM_NONE, weights=None, nu=0.0,
                     coupled=False):
    """fft_gpu::tvDeblurFree_RGB: replaces every element of `channels` (float32 planes of one size, at most 8 when coupled) in place
    with its free-boundary total-variation estimate, from one plan (that of tvDeblurFree_myfft), one weights plane for all channels
    and one launch per pass -- the bits of tvDeblurFree_myfft per channel, or with coupled the vectorial TV of the picture: one
    shrinkage by the joint gradient norm of the channels."""
    if not channels:
        return
    psf = np.asarray(psf, dtype=np.float32)
    r, c = np.asarray(channels[0]).shape
    M, N = _rlfree_plan_size(r, c, psf.shape[0], psf.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        p.set_batching(1, min(len(channels), 8))
        out = p.tv_deconv_free_batch(np.stack([np.asarray(c, dtype=np.float32) for c in channels]), mu, rho, iterations, weights, nu, False,
                                     nonneg, norm_area, False, coupled)
    for i in range(len(channels)):
        channels[i] = out[i]


def tvDeblurPoisson_myfft(img, psf, mu, rho=2.0, iterations=50, weights=None, nu=0.0, background=0.0, anisotropic=False, nonneg=False,
                          device=0, norm_area=NORM_NONE, full_plane=False):
    """Poisson-likelihood total-variation deconvolution of one photon-limited channel that is a crop of a larger scene: the plan of
    tvDeblurFree_myfft, `iterations` ADMM steps on the device, the window (or with full_plane the whole plan) back.  psf lies top-left
    in the plan; mu, background and weights as Plan.tv_deconv_poisson."""
    img = np.asarray(img, dtype=np.float32)
    psf = np.asarray(psf, dtype=np.float32)
    M, N = _rlfree_plan_size(img.shape[0], img.shape[1], psf.shape[0], psf.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        return p.tv_deconv_poisson(img, mu, rho, iterations, weights, nu, background, anisotropic, nonneg, norm_area, full_plane)


def tvDeblurPoisson_RGB(channels, psf, mu, rho=2.0, iterations=50, nonneg=False, device=0, norm_area=NORM_NONE, weights=None, nu=0.0,
                        background=0.0, coupled=False):
    """fft_gpu::tvDeblurPoisson_RGB: replaces every element of `channels` (float32 planes of one size, at most 8 when coupled) in place
    with its Poisson-likelihood total-variation estimate, from one plan (that of tvDeblurPoisson_myfft), one weights plane and one
    background for all channels and one launch per pass -- the bits of tvDeblurPoisson_myfft per channel, or with coupled the
    vectorial TV of the picture."""
    if not channels:
        return
    psf = np.asarray(psf, dtype=np.float32)
    r, c = np.asarray(channels[0]).shape
    M, N = _rlfree_plan_size(r, c, psf.shape[0], psf.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        p.set_batching(1, min(len(channels), 8))
        out = p.tv_deconv_poisson_batch(np.stack([np.asarray(c, dtype=np.float32) for c in channels]), mu, rho, iterations, weights, nu,
                                        background, False, nonneg, norm_area, False, coupled)
    for i in range(len(channels)):
        channels[i] = out[i]


def tiled_layout(rows, cols, prows, pcols, params):
    """fdr_tiled_layout_get: how a rows x cols picture is tiled by params (a TiledParams) for a prows x pcols PSF.  Pure host."""
    lay = TiledLayoutC()
    _check(lib.fdr_tiled_layout_get(int(rows), int(cols), int(prows), int(pcols), ctypes.byref(params), ctypes.byref(lay)))
    return TiledLayout(lay.tiles_r, lay.tiles_c, lay.win_rows, lay.win_cols, lay.min_M, lay.min_N, lay.work_bytes)


def tiled_tile_origin(rows, cols, params, a, b):
    """fdr_tiled_tile_origin: (y, x) of tile (a, b).  Pure host."""
    y, x = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib.fdr_tiled_tile_origin(int(rows), int(cols), ctypes.byref(params), int(a), int(b), ctypes.byref(y), ctypes.byref(x)))
    return y.value, x.value


def _tiled_psf_shape(psf_or_psfs):
    psfs = np.asarray(psf_or_psfs, dtype=np.float32)
    if psfs.ndim not in (2, 3):
        raise ValueError("psfs must be one PSF (2-D) or a stack of PSFs (3-D)")
    return psfs, psfs.shape[-2], psfs.shape[-1]


def restoreTiled_myfft(img, psf_or_psfs, params, weights=None, device=0):
    """Sectioned restoration of one channel of any size: the smallest tile plan of tiled_layout, the tiles by params.method on the
    device, the blended picture back.  psf_or_psfs and weights as Plan.restore_tiled."""
    img = np.asarray(img, dtype=np.float32)
    psfs, prows, pcols = _tiled_psf_shape(psf_or_psfs)
    lay = tiled_layout(img.shape[0], img.shape[1], prows, pcols, params)
    with Plan(lay.min_M, lay.min_N, MODE_FAST, device) as p:
        return p.restore_tiled(img, psfs, params, weights)


def restoreTiled_RGB(channels, psf_or_psfs, params, weights=None, device=0):
    """fft_gpu::restoreTiled_RGB: replaces every element of `channels` (float32 planes of one size) in place with its sectioned
    restoration, one tiled call per channel on one tile plan -- the bits of restoreTiled_myfft per channel."""
    if not channels:
        return
    psfs, prows, pcols = _tiled_psf_shape(psf_or_psfs)
    r, c = np.asarray(channels[0]).shape
    lay = tiled_layout(r, c, prows, pcols, params)
    with Plan(lay.min_M, lay.min_N, MODE_FAST, device) as p:
        for i in range(len(channels)):
            channels[i] = p.restore_tiled(channels[i], psfs, params, weights)


def tvDeblurAuto_myfft(img, psf, sigma=0.0, rho=2.0, iterations=100, weights=None, tau=0.0, nu=0.0, anisotropic=False, nonneg=False, device=0,
                       norm_area=NORM_NONE, full_plane=False):
    """Noise-constrained total-variation deconvolution of one channel that is a crop of a larger scene: tvDeblurFree_myfft with the
    noise level sigma (0: estimated from img) in the place of mu, on the same plan.  Returns (image, TvAutoResult, trace) as
    Plan.tv_deconv_auto."""
    img = np.asarray(img, dtype=np.float32)
    psf = np.asarray(psf, dtype=np.float32)
    M, N = _rlfree_plan_size(img.shape[0], img.shape[1], psf.shape[0], psf.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        return p.tv_deconv_auto(img, sigma, rho, iterations, weights, tau, nu, anisotropic, nonneg, norm_area, full_plane)


def tvDeblurAuto_RGB(channels, psf, sigma=0.0, rho=2.0, iterations=100, nonneg=False, device=0, norm_area=NORM_NONE, weights=None, tau=0.0,
                     nu=0.0, coupled=False):
    """fft_gpu::tvDeblurAuto_RGB: replaces every element of `channels` (float32 planes of one size, at most 8 when coupled) in place
    with its noise-constrained total-variation estimate, from one plan (that of tvDeblurAuto_myfft), one weights plane for all
    channels and one launch per pass, sigma given or (0) estimated per channel -- the bits of tvDeblurAuto_myfft per channel, or with
    coupled the vectorial TV of the picture with a ball and a mu_k per channel.  Returns the TvAutoResult of every channel."""
    results = []
    if not channels:
        return results
    psf = np.asarray(psf, dtype=np.float32)
    r, c = np.asarray(channels[0]).shape
    M, N = _rlfree_plan_size(r, c, psf.shape[0], psf.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        p.set_batching(1, min(len(channels), 8))
        out, results, _ = p.tv_deconv_auto_batch(np.stack([np.asarray(c, dtype=np.float32) for c in channels]), sigma, rho, iterations, weights,
                                                 tau, nu, False, nonneg, norm_area, False, None, coupled)
    for i in range(len(channels)):
        channels[i] = out[i]
    return results


def _motion_plan_size(rows, cols):
    """the plan estimateMotionBlur uses: fdr_optimal_dft_size of each dimension, at least 32"""
    return max(32, getOptimalDFTSize(rows)), max(32, getOptimalDFTSize(cols))


def estimateMotionBlur(img, device=0, min_length=0, max_length=0, angle_step=0.0, scores=False):
    """the motion blur (length, angle) of a picture of unknown blur, by the power cepstrum on the device (fdr_estimate_motion_f32).
    img: one channel, or rows x cols x channels (their per-pixel mean is used).  The plan is the smallest 2^a 3^b 5^c size of
    each dimension (at least 32), FLAG_MIXED_RADIX.  Returns a MotionEstimate (and the score table with scores=True); the
    length and angle go straight into motionBlurKernel / Plan.set_psf_motion."""
    img = np.asarray(img, dtype=np.float32)
    if img.ndim == 3:
        img = img.mean(axis=2, dtype=np.float32)
    M, N = _motion_plan_size(img.shape[0], img.shape[1])
    with Plan(M, N, MODE_FAST, device, flags=FLAG_MIXED_RADIX) as p:
        return p.estimate_motion(img, min_length, max_length, angle_step, scores)


def psf_disk(size, radius):
    """fdr_psf_disk: the size x size uniform disk of `radius` px centred at size // 2, each pixel the share of its square inside the
    disk (16 x 16 sub-samples), sum 1; generated by the device PSF kernel"""
    out = np.empty((int(size), int(size)), dtype=np.float32) if size > 0 else np.empty((1, 1), dtype=np.float32)
    _check(lib.fdr_psf_disk(int(size), float(radius), _ptr(out)))
    return out


def estimateDefocusBlur(img, device=0, min_diameter=0, max_diameter=0, angle_step=0.0, return_profile=False):
    """the disk radius of an out-of-focus picture, by the ring in its power cepstrum on the device (fdr_estimate_defocus_f32).  img
    and plan as estimateMotionBlur.  Returns a DefocusEstimate (and the profile with return_profile=True); the radius goes
    straight into psf_disk / Plan.set_psf_disk."""
    img = np.asarray(img, dtype=np.float32)
    if img.ndim == 3:
        img = img.mean(axis=2, dtype=np.float32)
    M, N = _motion_plan_size(img.shape[0], img.shape[1])
    with Plan(M, N, MODE_FAST, device, flags=FLAG_MIXED_RADIX) as p:
        return p.estimate_defocus(img, min_diameter, max_diameter, angle_step, return_profile)


def estimateBlur(img, device=0):
    """the kind of blur of a picture and both estimates, from one cepstrum (fdr_estimate_blur_f32): a BlurEstimate.  img and plan as
    estimateMotionBlur."""
    img = np.asarray(img, dtype=np.float32)
    if img.ndim == 3:
        img = img.mean(axis=2, dtype=np.float32)
    M, N = _motion_plan_size(img.shape[0], img.shape[1])
    with Plan(M, N, MODE_FAST, device, flags=FLAG_MIXED_RADIX) as p:
        return p.estimate_blur(img)


def chooseRegularisation(img, psf, method=REG_GCV, param=REG_PARAM_GAMMA, fixed=0.0, sigma=0.0, tau=0.0, lo=0.0, hi=0.0, n_grid=0, refine=-1,
                         device=0):
    """K or gamma of the Wiener / CLS filter for a blurred picture and its PSF, chosen on the device (fdr_choose_reg_f32).
    img: one channel, or rows x cols x channels (their per-pixel mean is used).  The plan is that of richardsonLucy_myfft (each
    dimension padded to the next power of two, at least 8 rows and 32 columns); psf lies top-left in it.  Returns a RegChoice;
    arguments as Plan.choose_regularisation."""
    img = np.asarray(img, dtype=np.float32)
    if img.ndim == 3:
        img = img.mean(axis=2, dtype=np.float32)
    M, N = _rl_plan_size(img.shape[0], img.shape[1])
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        return p.choose_regularisation(img, method, param, fixed, sigma, tau, lo, hi, n_grid, refine)


def batch_run(devices, M, N, count, rows=None, cols=None, mode=MODE_FAST, flags=0, psf=None, psf_size=50, psf_angle=30.0, K=0.01,
              imgs=None, seed=0x5EED0005, steps=1, warmup=0, nstreams=0, group=0, norm_area=NORM_PADDED, bcast_filter=False):
    """fdr_batch_run: `count` independent images sharded over `devices` (ordinals, may repeat) by the reference's
    calculate_distribution rule, one host thread + plan per entry.  imgs = float32 [count, rows, cols] host array (results
    returned) or None for the device-resident synthetic run.  Returns (stats dict, outputs or None)."""
    rows = rows or M
    cols = cols or N
    d = BatchDesc()
    devs = (ctypes.c_int * len(devices))(*[int(x) for x in devices])
    d.n_devices, d.devices = len(devices), devs
    d.M, d.N, d.mode, d.flags = int(M), int(N), int(mode), int(flags)
    keep = []
    if psf is not None:
        psf = np.ascontiguousarray(psf, dtype=np.float32)
        keep.append(psf)
        d.psf_host, d.psf_rows, d.psf_cols, d.psf_stride = psf.ctypes.data, psf.shape[0], psf.shape[1], psf.shape[1]
    d.psf_size, d.psf_angle_deg, d.K = int(psf_size), float(psf_angle), float(K)
    d.count, d.rows, d.cols, d.stride, d.out_stride = int(count), int(rows), int(cols), int(cols), int(cols)
    outs = None
    if imgs is not None:
        imgs = np.ascontiguousarray(imgs, dtype=np.float32)
        assert imgs.shape == (count, rows, cols)
        outs = np.empty_like(imgs)
        pin = (ctypes.c_void_p * max(count, 1))(*[imgs[i].ctypes.data for i in range(count)])
        pout = (ctypes.c_void_p * max(count, 1))(*[outs[i].ctypes.data for i in range(count)])
        keep += [imgs, pin, pout]
        d.imgs_host, d.outs_host = pin, pout
    d.synth_seed, d.steps, d.warmup = int(seed), int(steps), int(warmup)
    d.nstreams, d.group, d.norm_area = int(nstreams), int(group), int(norm_area)
    d.bcast_filter = int(bcast_filter)  # False / True / 2 (RCCL even for one device entry)
    st = BatchStats()
    _check(lib.fdr_batch_run(ctypes.byref(d), ctypes.byref(st)))
    n = st.n_devices
    stats = {"first": list(st.first[:n]), "images": list(st.images[:n]), "elapsed_ms": list(st.elapsed_ms[:n]),
             "checksum": list(st.checksum[:n]), "status": list(st.status[:n]), "wall_ms": st.wall_ms,
             "images_done": st.images_done, "mpixels_per_s": st.mpixels_per_s,
             "filter_path": ("local", "rccl_broadcast", "peer_copy")[st.filter_path] if 0 <= st.filter_path <= 2 else st.filter_path}
    return stats, outs


def wienerDeblur_RGB_optimized(channels, psf, K, mode=MODE_PARITY, device=0, norm_area=NORM_PADDED, cls_gamma=0.0, pad=PAD_ZERO):
    """fft_gpu::wienerDeblur_RGB_optimized (fft/fft_gpu.cu:279-394): replaces every element of
    `channels` (unpadded float32 planes of one size) in place with its restored [0,1] plane.
    One plan and one PSF spectrum serve all channels.  cls_gamma > 0: the constrained least-squares filter.  pad: as
    wienerDeblur_myfft."""
    if not channels:
        return
    r, c = np.asarray(channels[0]).shape
    with _wiener_plan(r, c, psf, mode, device, pad) as p:
        p.set_psf(psf, K, gamma=cls_gamma)
        for i in range(len(channels)):
            channels[i] = p.wiener(channels[i], norm_area)


def _rl_rgb(channels, M, N, psf, iterations, device, **kw):
    """the channels of one picture as ONE batched call on a group of len(channels) (at most 8) images"""
    with Plan(M, N, MODE_FAST, device) as p:
        p.set_operator_psf(psf)
        p.set_batching(1, min(len(channels), 8))
        out = p.richardson_lucy_batch(np.stack([np.asarray(c, dtype=np.float32) for c in channels]), iterations, **kw)
    for i in range(len(channels)):
        channels[i] = out[i]


def richardsonLucy_RGB(channels, psf, iterations, device=0, norm_area=NORM_NONE, accelerate=False):
    """fft_gpu::richardsonLucy_RGB: replaces every element of `channels` (float32 planes of one size) in place with its
    Richardson-Lucy estimate -- the bits of richardsonLucy_myfft per channel, from one plan and one launch per pass.  accelerate:
    the accelerated iteration, batched as well (the bits of richardsonLucy_myfft(..., accelerate=True) per channel)."""
    if not channels:
        return
    r, c = np.asarray(channels[0]).shape
    M, N = _rl_plan_size(r, c)
    _rl_rgb(channels, M, N, psf, iterations, device, norm_area=norm_area, accelerate=accelerate)


def richardsonLucyFree_RGB(channels, psf, iterations, weights=None, sigma=RL_SIGMA, device=0, norm_area=NORM_NONE, accelerate=False):
    """fft_gpu::richardsonLucyFree_RGB: the free-boundary form of richardsonLucy_RGB (richardsonLucyFree_myfft per channel); one
    weights plane (or None) serves every channel, and its coverage is computed once.  accelerate as richardsonLucy_RGB."""
    if not channels:
        return
    r, c = np.asarray(channels[0]).shape
    psf = np.asarray(psf, dtype=np.float32)
    M, N = _rlfree_plan_size(r, c, psf.shape[0], psf.shape[1])
    _rl_rgb(channels, M, N, psf, iterations, device, free_boundary=True, weights=weights, sigma=sigma, norm_area=norm_area,
            accelerate=accelerate)


def wienerDeblur_RGB_naive(channels, psf, K, mode=MODE_PARITY, device=0, norm_area=NORM_PADDED, cls_gamma=0.0, pad=PAD_ZERO):
    """fft_gpu::wienerDeblur_RGB_naive (fft/fft_gpu.cu:400-512): same results, but every channel
    builds and frees its own plan and PSF spectrum, as the reference's allocation-in-loop variant."""
    for i in range(len(channels)):
        channels[i] = wienerDeblur_myfft(channels[i], psf, K, mode, device, norm_area, cls_gamma, pad)
