"""The smallest windows of every windowed call: the tables test_edge_windows_host.py and test_edge_windows_gpu.py share.

Every image entry point takes a rows x cols window from 1 x 1 up to the plan's M x N.  The other files of the suite judge the
features at every transform length, group size and pitch; this one judges them where the masks, tails and sums of a window
degenerate: one pixel, one row, one column, less than one 4-row group, narrower than one 4-column lane request, one short of the
plan -- and at PSFs of 1, 2, 4 and M - 1 rows, the heights around nvalid = (prows + 3) & ~3.

    PLANS       chosen by the kernels they select (the comment beside each)
    windows()   small, line and near-full windows of a plan
    psfs()      the PSFs of a family on a plan
    picture()   seeded, in [0.2, 1], one negative pixel where there is more than one
    FAMILIES    one entry per call: its float64 model, its threshold and error measure (those of its own model file, unchanged), the
                _dev call and the host call
    Guarded     device buffers: every window lies behind a NaN guard band of four buffer rows plus 64 floats on each side, so that
                an access one line off lands inside the allocation and fails an assertion

MEASURED below: for every family the largest error one run of test_edge_windows_gpu.py gave on an MI355X and the case it occurred
at (DESIGN.md section 43 holds the same table).  No case needed a bound of its own (CASE_TOL is empty): every case stays below
its family's threshold."""
import numpy as np

from _blind_model import blind_model, gpu_tol
from _cls_model import cls_raw
from _frames_model import FRAMES_ADJ_TOL, FRAMES_TOL, blur_frames, blur_frames_adjoint, frames_model
from _mixed_model import wiener_raw
from _pad_model import DEVICE_TOL, PAD_SMOOTH, PAD_ZERO, pad_plane
from _rl_model import (BLUR_TOL, NORM_CROPPED, NORM_NONE, NORM_PADDED, RL_TOL, blur_model, centred_psf, dense_psf, normalize, rel_err,
                       rl_model)
from _rlaccel_model import RLA_FREE_TOL, RLA_TOL, rl_accel_model, rlfree_accel_model
from _rlfree_model import RLFREE_TOL, rlfree_model
from _rlstop_model import STOP_RESIDUAL, TRACE_TOL, run_model, stop_model, trace_error
from _rltv_model import RLTV_FREE_TOL, RLTV_TOL, rltv_free_model, rltv_model
from _tv_model import TV_TOL, tv_model
from _tvauto_model import TVA_TOL, TVA_TRACE_TOL, trace_err, tvauto_model
from _tvframes_model import TVFR_TOL, tvframes_model
from _tvfree_model import TVF_TOL, tvfree_model
from _tvpoisson_model import TVP_TOL, tvpoisson_model

# MEASURED on an MI355X by test_edge_windows_gpu.py -s: family -> (largest error over its plans, windows, PSFs, iteration counts,
# norm_area values, weights and both alignments, the family's threshold, the case: plan, window, PSF, weights, n, norm_area).
# Traces: rl_auto 5.18e-7 (TRACE_TOL 2e-5), tv_auto 1.2e-5 (TVA_TRACE_TOL 5e-5); rl_auto_res: 204 stops, every count and flag the
# model's; PSF {1}: 1.13e-6 (DELTA_TOL 2.5e-6, 4096 x 32); the blind forms' threshold is gpu_tol of the float32 replay (1e-5 here).
# The blind forms' refined PSF against the model's: 5.48e-7 plain (256 x 64), 7.91e-7 free (64 x 256), same bound; at the minimum
# window 5 x 5 of the free form: image 4.74e-7, PSF 2.1e-7.
# A record for the reader (nothing reads it): the thresholds stay those of the model files.
MEASURED = {
    "blur_fwd": (6.31e-07, BLUR_TOL, "4096x32 win 4095x31 rows4 norm=none"),
    "blur_adj": (6.6e-07, BLUR_TOL, "4096x32 win 4095x31 rows4 norm=none"),
    "rl": (1.17e-06, RL_TOL, "4096x32 win 4096x1 rows1 n=3 norm=padded"),
    "rl_accel": (1.17e-06, RLA_TOL, "4096x32 win 4096x1 rows1 n=3 norm=padded"),
    "rl_free": (2.14e-06, RLFREE_TOL, "4096x32 win 4095x31 dense5c n=3 norm=cropped"),
    "rl_free_accel": (5.73e-06, RLA_FREE_TOL, "64x256 win 1x2 dense5c w=frac n=3 norm=none"),
    "rl_auto": (1.17e-06, RL_TOL, "4096x32 win 4096x1 rows1 n=3 norm=padded"),
    "rl_auto_res": (1.17e-06, RL_TOL, "4096x32 win 4096x1 rows1 n=3 norm=padded"),
    "rl_tv": (6.04e-06, RLTV_TOL, "4096x32 win 4095x31 rows2 n=3 norm=padded"),
    "rl_tv_free": (1.51e-05, RLTV_FREE_TOL, "16x4096 win 15x4095 dense5c w=frac n=3 norm=none"),
    "blind_hold0": (9.06e-07, 1e-5, "4096x32 win 4095x31 rows1 n=1 norm=none"),
    "blind_hold1": (9.06e-07, 1e-5, "4096x32 win 4095x31 rows1 n=1 norm=none"),
    "blind_free_hold0": (1.98e-06, 1e-5, "8x32 win 5x15 dense5 n=1 norm=cropped"),
    "blind_free_hold1": (3.09e-06, 1e-5, "64x256 win 5x127 dense5 w=frac n=3 norm=padded"),
    "tv": (2.69e-06, TV_TOL, "256x64 win 255x64 dense5 n=3 norm=cropped"),
    "tv_free": (2.44e-06, TVF_TOL, "64x256 win 64x255 dense5c n=3 norm=cropped"),
    "tv_auto": (2.16e-06, TVA_TOL, "16x4096 win 1x4096 dense5c n=3 norm=none"),
    "tv_poisson": (5.78e-06, TVP_TOL, "8x32 win 5x2 dense5c n=3 norm=cropped"),
    "rl_frames": (1.77e-06, FRAMES_TOL, "16x4096 win 1x4096 dense5c w=frac n=3 norm=none"),
    "tv_frames": (3.51e-06, TVFR_TOL, "8x32 win 5x2 dense5c n=3 norm=cropped"),
    "blur_frames_fwd": (6.68e-07, BLUR_TOL, "4096x32 win 4095x31 dense5 norm=none"),
    "blur_frames_adj": (6.27e-07, FRAMES_ADJ_TOL, "16x4096 win 15x4095 rows1 norm=none"),
    "wiener_zero": (8.29e-07, DEVICE_TOL, "4096x32 win 4096x1 rows1 norm=cropped"),
    "cls_zero": (6.95e-07, DEVICE_TOL, "256x64 win 256x63 dense5 norm=padded"),
    "wiener_smooth": (1.37e-06, DEVICE_TOL, "16x4096 win 16x1 rows1 norm=padded"),
    "cls_smooth": (9.9e-07, DEVICE_TOL, "4096x32 win 4095x31 rows2 norm=cropped"),
}

# (family, plan, window, psf) -> (bound, device error, float32 model's distance): a bound of its own only where the float32 run of
# the MODEL is itself past a quarter of the family's threshold; then 4x that distance.  None needed.
CASE_TOL = {}

PLANS = ((8, 32),      # the smallest operator plan
         (64, 256),    # split row kernels (rows4_use_split), persistent radix-8 columns
         (256, 64),    # the split column kernel
         (16, 4096),   # 16-value packed row kernels
         (4096, 32))   # fused16 columns; 1023 of 1024 row groups empty under a one-row window
PLAN_IDS = ["%dx%d" % p for p in PLANS]
AREAS = (NORM_NONE, NORM_CROPPED, NORM_PADDED)
ITERATIONS = (0, 1, 3)


def windows(M, N):
    """the windows of a plan, unique, in the order of the issue's table"""
    if max(M, N) >= 4096:
        return [(1, 1), (3, 3), (1, N), (M, 1), (M - 1, N - 1)]
    small = [(1, 1), (1, 2), (2, 1), (3, 3), (4, 4), (2, 5), (5, 2)]
    lines = [(1, N), (M, 1), (1, N - 1), (M - 1, 1)]
    near = [(M - 1, N), (M, N - 1), (M - 1, N - 1), (4, N // 2 + 1), (5, N // 2 - 1)]
    return list(dict.fromkeys(small + lines + near))


def core_windows(M, N):
    """the windows every family meets under every PSF, and the group tests use"""
    return [(1, 1), (3, 3), (1, N), (M, 1), (M - 1, N - 1)]


def tall_psf(prows, seed=3):
    """a dense positive prows x 3 PSF, sum 1, a quarter of it at (0, 0): under a cropped window the first pixel's reblurred value
    c = blur(u) is carried by that tap alone (the others reach the zeros beyond the window), and Richardson-Lucy divides by c.  The
    other taps lie within 10 % of each other: the coverage of a free-boundary form under a small window is a sum of k taps, and
    with 63 x 3 taps of 0.0036 .. 0.0044 two of them stay below FDR_RL_SIGMA = 0.01 and three above it, each by more than the
    margin the host file asserts (with 255 x 3 taps nine stay below)."""
    p = 0.9 + 0.2 * np.random.default_rng(seed + prows).random((prows, 3))
    p[0, 0] = 0.0
    p[0, 0] = p.sum() / 3.0
    return (p / p.sum()).astype(np.float32)


DENSE5 = dense_psf(5, 5)
ONE = np.ones((1, 1), dtype=np.float32)


def psfs(M, N, centred):
    """[(name, PSF, main)]: the dense 5 x 5 PSF (top-left for the periodic forms, its centred plane for the free-boundary ones: every
    window, iteration count and norm_area), then the PSFs of 1, 2, 4 and M - 1 rows (core windows; M - 1 on the three small plans).
    The PSF {1} is not here: under it a blur is the identity and no window fault shows against the model; it serves the exact
    tests.  No top-left motion PSF: it has no weight at (0, 0) (test_rl_gpu.py::_rl_cases)."""
    out = [("dense5c", centred_psf(DENSE5, M, N), True) if centred else ("dense5", DENSE5, True)]
    heights = [1, 2, 4] + ([M - 1] if M * N <= 64 * 256 else [])
    return out + [("rows%d" % h, tall_psf(h), False) for h in heights]


def picture(rows, cols, seed=0, grow=0):
    """float32 (rows + grow) x (cols + grow) picture whose top-left rows x cols is the picture of the case: seeded, in [0.2, 1], one
    negative pixel where the window has more than one (grow: the pixels a window fault one line long would read).  The negative
    pixel lies at (rows / 2, cols / 2), never at (0, 0): Richardson-Lucy starts from d+ = 0 there, and in a 1 x 2 window with the
    zero first nothing would reach the first pixel's c = blur(u)."""
    rng = np.random.default_rng(1000003 * rows + 1009 * cols + seed)
    img = (0.2 + 0.8 * rng.random((rows + 1, cols + 1))).astype(np.float32)
    if rows * cols > 1:
        img[rows // 2, cols // 2] = np.float32(-0.3)
    return np.ascontiguousarray(img[:rows + grow, :cols + grow])


WEIGHT_KINDS = ("none", "frac", "hole")
WEIGHT_SEED = 2  # chosen so that no coverage of a free-boundary form lies at its threshold (test_edge_windows_host.py asserts the margin)


def weights(kind, rows, cols, grow=0):
    """None, fractional weights in [0.25, 1], or ones with a hole (a zero) at the last pixel; `hole` needs more than one pixel"""
    if kind == "none":
        return None
    rng = np.random.default_rng(WEIGHT_SEED + 7 * rows + cols)
    w = (0.25 + 0.75 * rng.random((rows + 1, cols + 1))).astype(np.float32)
    if kind == "hole":
        w[:] = 1
        w[rows - 1, cols - 1] = 0
    return np.ascontiguousarray(w[:rows + grow, :cols + grow])


# ---- the parameters of the calls that take some ----
LAM, EPS = 0.01, 1e-3                       # RL-TV (the quality pair of _rltv_model.py)
MU, RHO, NU = 50.0, 2.0, 3.0                # the TV forms (the dense-PSF combination of their short cases)
SIGMA_N = 0.02                              # noise level given to the auto TV call
SIGMA_STOP = 0.27                           # noise level given to the residual rule: about a third of the cases stop within 3 steps; the
                                            # host file asserts DECISION_MARGIN (1 %) between every model statistic and its target (the
                                            # closest measured lies 4.4 % off)
BACKGROUND = 0.01                           # Poisson TV
KW, GAMMA = float(np.float32(0.01)), float(np.float32(0.05))  # Wiener K and CLS gamma (test_pad_gpu.py)


def second_psf(psf):
    """the second frame's PSF: the first with half the tap at (0, 0), so a shorter exposure.  The other taps stay: where a small
    window leaves a pixel of the plan little coverage, the tap at (0, 0) is not among those that reach it, the two frames'
    coverages are equal there and their sum keeps the distance from its threshold that the single PSF's has (tall_psf)."""
    p = np.array(psf, dtype=np.float32)
    p[0, 0] *= np.float32(0.5)
    return p


class Family:
    """one call.  model(img, psf, M, N, n, w, dtype) -> the raw (FDR_NORM_NONE) rows x cols float window (count windows for
    out_count > 1); finish(raw, area, M, N, rows, cols) normalises it as the call does
    (the Wiener families' raw output is the whole M x N plane, which FDR_NORM_PADDED counts).  dev(p, a) runs the _dev form on the Guarded buffers of `a`,
    host(p, img, n, area, w, psf) the host form.  setup(p, psf) sets the PSF the call uses.  frames: the call takes this many pictures."""

    def __init__(self, name, tol, model, dev, host, free=False, weighted=False, iters=ITERATIONS, areas=AREAS, setup=None, frames=1,
                 out_count=1, finish=None, err32_tol=None, rl=False, centred=None, trace=None, psf_model=None):
        self.name, self.tol, self.model, self.dev, self.host = name, tol, model, dev, host
        self.free, self.weighted, self.iters, self.areas, self.frames, self.out_count = free, weighted, iters, areas, frames, out_count
        self.setup = setup or (lambda p, psf: p.set_operator_psf(psf))
        self.finish = finish or (lambda raw, area, M, N, rows, cols: normalize(raw, area, M, N))
        self.err32_tol = err32_tol  # blind RL: the bound comes from the float32 replay of the same case (gpu_tol)
        self.centred = free if centred is None else centred  # the dense PSF as its centred plane
        self.trace = trace          # (doubles per step, model(img, psf, M, N, n, w) -> [n, doubles], error(got, want), threshold)
        self.psf_model = psf_model  # blind RL: the refined PSF the call writes back, judged beside the image
        self.rl = rl                # divides by c = blur(u): the host file asserts c >= 1e-2 max c

    def kinds(self):
        return WEIGHT_KINDS if self.weighted else ("none",)

    def error(self, got, want, area):
        """the measure of every model file: max |got - want| / max |want| of a raw output, max-abs of a normalised one"""
        if area == NORM_NONE:
            return rel_err(got, want)
        return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)))


def frames_of(img):
    """the two pictures of a multi-frame case from the first: frame 1 is frame 0 at 0.6 of the exposure with a mild texture of its
    own (a zero picture stays zero, the negative pixel negative)"""
    img = np.asarray(img, dtype=np.float32)
    i, j = np.indices(img.shape)
    return [img, np.ascontiguousarray(img * (0.6 + 0.05 * ((i + j) % 3)).astype(np.float32))]


def _wiener_model(pad, gamma):
    def model(img, psf, M, N, n, w, dtype):
        e = pad_plane(np.asarray(img, dtype=np.float64), M, N, pad)
        return cls_raw(e, psf, KW, gamma, M, N) if gamma > 0 else wiener_raw(e, psf, KW, M, N)  # the whole M x N raw plane
    return model


def _wiener_finish(raw, area, M, N, rows, cols):
    """min-max over the window (CROPPED) or the whole raw plane (PADDED) of the M x N raw plane"""
    plane = np.asarray(raw)
    win = plane[:rows, :cols]
    src = plane if area == NORM_PADDED else win
    lo, hi = float(src.min()), float(src.max())
    return (win - lo) / (hi - lo) if hi - lo > 2.2204460492503131e-16 else np.zeros_like(win)


def _wiener(pad, gamma):
    model = _wiener_model(pad, gamma)

    def setup(p, psf):
        import importlib
        fdr = importlib.import_module(type(p).__module__)
        p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH if pad == PAD_SMOOTH else fdr.PAD_ZERO)
        p.set_psf(psf, KW, gamma=gamma)

    return dict(model=model, setup=setup, finish=_wiener_finish, iters=(None,), areas=(NORM_CROPPED, NORM_PADDED),
                dev=lambda p, a: p.wiener_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, a.area),
                host=lambda p, img, n, area, w, psf: p.wiener(img, area))


def _auto_model(img, psf, M, N, n, w, dtype):
    return rl_model(img, psf, M, N, n, dtype=dtype)  # rule none runs n plain steps; the trace is judged beside it


def stop_decision(img, psf, M, N, n):
    """the residual rule with sigma = SIGMA_STOP on n plain steps at most: stop_model's dict"""
    return stop_model(run_model(img, psf, M, N, n), STOP_RESIDUAL, sigma=SIGMA_STOP)


def _blind(free, hold):
    def model(img, psf, M, N, n, w, dtype):
        return blind_model(img, psf, M, N, n, free, w, hold, dtype=dtype)[0]

    def psf_model(img, psf, M, N, n, w, dtype):
        return blind_model(img, psf, M, N, n, free, w, hold, dtype=dtype)[1]

    def dev(p, a):
        p.richardson_lucy_blind_dev(a.img, a.rows, a.cols, a.stride, a.psf, a.prows, a.pcols, a.pstride, a.out, a.ostride, a.n, free, a.w,
                                    a.wstride, hold, norm_area=a.area)

    def host(p, img, n, area, w, psf):
        return p.richardson_lucy_blind(img, psf, n, free, w, hold, norm_area=area)[0]

    # the start PSF stays top-left in both forms: a centred plane has M N entries (FDR_BLIND_MAX_PSF is 65536) and zeros that a
    # multiplicative PSF step never leaves
    return dict(model=model, dev=dev, host=host, free=free, weighted=free, setup=lambda p, psf: None, psf_model=psf_model,
                err32_tol=gpu_tol, rl=True, centred=False)


def _families():
    F = []

    def add(name, tol, **kw):
        F.append(Family(name, tol, **kw))

    one = dict(iters=(None,), areas=(NORM_NONE,))
    add("blur_fwd", BLUR_TOL, model=lambda img, psf, M, N, n, w, dt: blur_model(img, psf, M, N, dtype=dt),
        dev=lambda p, a: p.blur_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, False),
        host=lambda p, img, n, area, w, psf: p.blur(img), **one)
    add("blur_adj", BLUR_TOL, model=lambda img, psf, M, N, n, w, dt: blur_model(img, psf, M, N, adjoint=True, dtype=dt),
        dev=lambda p, a: p.blur_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, True),
        host=lambda p, img, n, area, w, psf: p.blur(img, adjoint=True), **one)
    add("rl", RL_TOL, rl=True, model=lambda img, psf, M, N, n, w, dt: rl_model(img, psf, M, N, n, dtype=dt),
        dev=lambda p, a: p.richardson_lucy_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, a.n, a.area),
        host=lambda p, img, n, area, w, psf: p.richardson_lucy(img, n, area))
    add("rl_accel", RLA_TOL, rl=True, model=lambda img, psf, M, N, n, w, dt: rl_accel_model(img, psf, M, N, n, dtype=dt)[0],
        dev=lambda p, a: p.richardson_lucy_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, a.n, a.area, accelerate=True),
        host=lambda p, img, n, area, w, psf: p.richardson_lucy(img, n, area, accelerate=True))
    add("rl_free", RLFREE_TOL, rl=True, free=True, weighted=True,
        model=lambda img, psf, M, N, n, w, dt: rlfree_model(img, psf, M, N, n, w, dtype=dt),
        dev=lambda p, a: p.richardson_lucy_free_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, a.n, a.w, a.wstride, norm_area=a.area),
        host=lambda p, img, n, area, w, psf: p.richardson_lucy_free(img, n, w, norm_area=area))
    add("rl_free_accel", RLA_FREE_TOL, rl=True, free=True, weighted=True,
        model=lambda img, psf, M, N, n, w, dt: rlfree_accel_model(img, psf, M, N, n, w, dtype=dt)[0],
        dev=lambda p, a: p.richardson_lucy_free_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, a.n, a.w, a.wstride, norm_area=a.area,
                                                    accelerate=True),
        host=lambda p, img, n, area, w, psf: p.richardson_lucy_free(img, n, w, norm_area=area, accelerate=True))
    add("rl_auto", RL_TOL, rl=True, model=_auto_model,
        trace=(2, lambda img, psf, M, N, n, w: run_model(img, psf, M, N, n)["trace"], trace_error, TRACE_TOL),
        dev=lambda p, a: p.richardson_lucy_auto_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, a.n, 0, norm_area=a.area, d_trace=a.trace),
        host=lambda p, img, n, area, w, psf: p.richardson_lucy_auto(img, n, 0, norm_area=area)[0])
    add("rl_auto_res", RL_TOL, rl=True, model=lambda img, psf, M, N, n, w, dt: stop_decision(img, psf, M, N, n)["u"],
        dev=lambda p, a: p.richardson_lucy_auto_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, a.n, STOP_RESIDUAL, SIGMA_STOP, norm_area=a.area),
        host=lambda p, img, n, area, w, psf: p.richardson_lucy_auto(img, n, STOP_RESIDUAL, SIGMA_STOP, norm_area=area)[0])
    add("rl_tv", RLTV_TOL, rl=True, model=lambda img, psf, M, N, n, w, dt: rltv_model(img, psf, M, N, n, LAM, EPS, dtype=dt),
        dev=lambda p, a: p.richardson_lucy_tv_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, a.n, LAM, EPS, norm_area=a.area),
        host=lambda p, img, n, area, w, psf: p.richardson_lucy_tv(img, n, LAM, EPS, norm_area=area))
    add("rl_tv_free", RLTV_FREE_TOL, rl=True, free=True, weighted=True,
        model=lambda img, psf, M, N, n, w, dt: rltv_free_model(img, psf, M, N, n, LAM, EPS, w, dtype=dt),
        dev=lambda p, a: p.richardson_lucy_tv_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, a.n, LAM, EPS, True, a.w, a.wstride,
                                                  norm_area=a.area),
        host=lambda p, img, n, area, w, psf: p.richardson_lucy_tv(img, n, LAM, EPS, True, w, norm_area=area))
    for free in (False, True):
        for hold in (0, 1):
            add("blind%s_hold%d" % ("_free" if free else "", hold), None, **_blind(free, hold))
    add("tv", TV_TOL, model=lambda img, psf, M, N, n, w, dt: tv_model(img, psf, M, N, MU, RHO, n, dtype=dt),
        dev=lambda p, a: p.tv_deconv_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, MU, RHO, a.n, norm_area=a.area),
        host=lambda p, img, n, area, w, psf: p.tv_deconv(img, MU, RHO, n, norm_area=area))
    add("tv_free", TVF_TOL, free=True, weighted=True,
        model=lambda img, psf, M, N, n, w, dt: tvfree_model(img, psf, M, N, MU, RHO, n, w, NU, dtype=dt),
        dev=lambda p, a: p.tv_deconv_free_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, MU, RHO, a.n, a.w, a.wstride, NU, norm_area=a.area),
        host=lambda p, img, n, area, w, psf: p.tv_deconv_free(img, MU, RHO, n, w, NU, norm_area=area))
    add("tv_auto", TVA_TOL, free=True, weighted=True,
        model=lambda img, psf, M, N, n, w, dt: tvauto_model(img, psf, M, N, SIGMA_N, RHO, n, w, dtype=dt)[0],
        trace=(3, lambda img, psf, M, N, n, w: tvauto_model(img, psf, M, N, SIGMA_N, RHO, n, w)[1], trace_err, TVA_TRACE_TOL),
        dev=lambda p, a: p.tv_deconv_auto_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, SIGMA_N, RHO, a.n, a.w, a.wstride, norm_area=a.area,
                                              d_trace=a.trace),
        host=lambda p, img, n, area, w, psf: p.tv_deconv_auto(img, SIGMA_N, RHO, n, w, norm_area=area)[0])
    add("tv_poisson", TVP_TOL, free=True, weighted=True,
        model=lambda img, psf, M, N, n, w, dt: tvpoisson_model(img, psf, M, N, MU, RHO, n, w, NU, BACKGROUND, dtype=dt),
        dev=lambda p, a: p.tv_deconv_poisson_dev(a.img, a.rows, a.cols, a.stride, a.out, a.ostride, MU, RHO, a.n, a.w, a.wstride, NU, BACKGROUND,
                                                 norm_area=a.area),
        host=lambda p, img, n, area, w, psf: p.tv_deconv_poisson(img, MU, RHO, n, w, NU, BACKGROUND, norm_area=area))
    # two frames, PSFs (psf, second_psf(psf))
    fr = dict(frames=2, free=True, setup=lambda p, psf: p.set_frame_psfs([psf, second_psf(psf)]))
    add("rl_frames", FRAMES_TOL, rl=True, weighted=True,
        model=lambda img, psf, M, N, n, w, dt: frames_model(frames_of(img), [psf, second_psf(psf)], M, N, n, w, dtype=dt),
        dev=lambda p, a: p.richardson_lucy_frames_dev(a.img, a.pitch, 2, a.rows, a.cols, a.stride, a.out, a.ostride, a.n, a.w, 0, a.wstride,
                                                      norm_area=a.area),
        host=lambda p, img, n, area, w, psf: p.richardson_lucy_frames(frames_of(img), n, w, norm_area=area), **fr)
    add("tv_frames", TVFR_TOL, weighted=True,
        model=lambda img, psf, M, N, n, w, dt: tvframes_model(frames_of(img), [psf, second_psf(psf)], M, N, MU, RHO, n, w, NU, dtype=dt),
        dev=lambda p, a: p.tv_deconv_frames_dev(a.img, a.pitch, 2, a.rows, a.cols, a.stride, a.out, a.ostride, MU, a.n, a.w, 0, a.wstride, rho=RHO, nu=NU,
                                                norm_area=a.area),
        host=lambda p, img, n, area, w, psf: p.tv_deconv_frames(frames_of(img), MU, n, w, rho=RHO, nu=NU, norm_area=area), **fr)
    add("blur_frames_fwd", BLUR_TOL, out_count=2, host=None, iters=(None,), areas=(NORM_NONE,),
        model=lambda img, psf, M, N, n, w, dt: np.stack(blur_frames(img, [psf, second_psf(psf)], M, N, dt)),
        dev=lambda p, a: p.blur_frames_dev(a.img, 0, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, 2, False),
        frames=1, free=False, setup=fr["setup"])
    add("blur_frames_adj", FRAMES_ADJ_TOL, host=None, iters=(None,), areas=(NORM_NONE,),
        model=lambda img, psf, M, N, n, w, dt: blur_frames_adjoint(frames_of(img), [psf, second_psf(psf)], M, N, dt),
        dev=lambda p, a: p.blur_frames_dev(a.img, a.pitch, a.rows, a.cols, a.stride, a.out, 0, a.ostride, 2, True),
        frames=2, free=False, setup=fr["setup"])
    for name, pad, gamma in (("wiener_zero", PAD_ZERO, 0.0), ("cls_zero", PAD_ZERO, GAMMA), ("wiener_smooth", PAD_SMOOTH, 0.0),
                             ("cls_smooth", PAD_SMOOTH, GAMMA)):
        add(name, DEVICE_TOL, **_wiener(pad, gamma))
    return F


FAMILIES = _families()
FAMILY = {f.name: f for f in FAMILIES}


def cases(fam, M, N):
    """[(rows, cols, psf name, psf, main)] of a family on a plan: every window under the main PSF, the core windows under the others"""
    out = []
    for name, psf, main in psfs(M, N, fam.centred):
        for rows, cols in (windows(M, N) if main else core_windows(M, N)):
            if defined(fam, rows, cols, psf):
                out.append((rows, cols, name, psf, main))
    return out


def tolerance(fam, M, N, rows, cols, psf_name):
    return CASE_TOL.get((fam.name, (M, N), (rows, cols), psf_name), (fam.tol,))[0]


# ---- window and PSF faults (test_edge_windows_host.py): what a kernel whose mask or tail is one line off would compute ----
FAULTS = ("row_short", "col_short", "row_long", "col_long", "psf_row_short")


def fault_model(fam, fault, rows, cols, psf, M, N, n, kind):
    """the raw output on the rows x cols window of the family's model under `fault`, or None where the fault does not exist (a window
    of one row cannot be a row short, a full window not a row long, a one-row PSF not a row short).  *_short: the input window ends
    one line early (the line reads as padding); *_long: it ends one line late (the call reads one line of the caller's buffer beyond
    the window); the output window is the true one."""
    dr = {"row_short": -1, "row_long": 1}.get(fault, 0)
    dc = {"col_short": -1, "col_long": 1}.get(fault, 0)
    r2, c2 = rows + dr, cols + dc
    if r2 < 1 or c2 < 1 or r2 > M or c2 > N:
        return None
    if fault == "psf_row_short":
        if psf.shape[0] < 2:
            return None
        psf = psf[:-1]
    big = picture(rows, cols, grow=1)
    img = np.ascontiguousarray(big[:r2, :c2])
    w = weights(kind, rows, cols, grow=1)
    w = None if w is None else np.ascontiguousarray(w[:r2, :c2])
    raw = np.asarray(fam.model(img, psf, M, N, n, w, np.float64))
    if raw.shape[-2:] == (M, N):  # the Wiener families return the plane
        return raw[..., :rows, :cols]
    out = np.zeros(raw.shape[:-2] + (rows, cols))
    out[..., :min(rows, r2), :min(cols, c2)] = raw[..., :min(rows, r2), :min(cols, c2)]
    return out


# ---- device buffers ----
class Guarded:
    """`count` windows of rows x cols floats at `pitch` in one device allocation, each row `stride` apart; NaN everywhere outside
    the windows: in the stride padding, between the images and in a guard band of four buffer rows plus 64 floats before the
    first and after the last window.  misaligned: the base lies one float off a 16-byte boundary and the stride is odd (the scalar
    forms); else the base is 16-byte aligned and the stride a multiple of 4 (the vector forms).  `odd_pitch` puts image 1 off image
    0's alignment."""

    def __init__(self, rows, cols, misaligned, fill=None, count=1, extra=0, odd_pitch=False):
        import torch
        self.rows, self.cols, self.count = rows, cols, count
        self.stride = (cols + 3) // 4 * 4 + 4 + 4 * extra + (1 if misaligned else 0)
        span = rows * self.stride
        self.pitch = span + 8 if count > 1 else span
        if odd_pitch:
            self.pitch += (1 - self.pitch) % 4
        self.guard = (4 * self.stride + 64 + 3) // 4 * 4  # a multiple of 4 floats: the base stays aligned
        self.offset = self.guard + (1 if misaligned else 0)
        total = self.offset + (count - 1) * self.pitch + span + self.guard
        host = np.full(total, np.nan, dtype=np.float32)
        if fill is not None:
            fill = np.asarray(fill, dtype=np.float32).reshape(count, rows, cols)
            for k in range(count):
                self._window(host, k)[:] = fill[k]
        self.host = host
        self.dev = torch.from_numpy(host).cuda()
        self.ptr = self.dev.data_ptr() + 4 * self.offset
        assert (self.ptr % 16 == 0) == (not misaligned)

    def _window(self, flat, k):
        a = self.offset + k * self.pitch
        return flat[a:a + self.rows * self.stride].reshape(self.rows, self.stride)[:, :self.cols]

    def unchanged(self):
        """an input buffer after the call: every byte as uploaded"""
        return np.array_equal(self.dev.cpu().numpy().view(np.uint32), self.host.view(np.uint32))

    def result(self):
        """(the count x rows x cols windows of an output buffer, whether everything outside them is still NaN)"""
        flat = self.dev.cpu().numpy()
        out = np.stack([self._window(flat, k).copy() for k in range(self.count)])
        for k in range(self.count):
            self._window(flat, k)[:] = np.nan
        return out, bool(np.all(np.isnan(flat)))


class Args:
    """what a Family.dev reads: pointers, strides and pitches of the Guarded buffers of one call"""
    trace = None
    w = None
    wstride = 0
    psf = None


def stage(fam, imgs, w, psf, n, area, misaligned, out_count=1, odd_pitch=False):
    """(Args, the Guarded buffers by name) of one _dev call of the family: inputs filled, the output NaN.  odd_pitch (the group
    calls): image 1 lies off image 0's 16-byte alignment in both buffers."""
    import torch
    imgs = np.asarray(imgs, dtype=np.float32)
    imgs = imgs[None] if imgs.ndim == 2 else imgs
    count, rows, cols = imgs.shape
    a, bufs = Args(), {}
    bufs["img"] = Guarded(rows, cols, misaligned, imgs, count, odd_pitch=odd_pitch)
    bufs["out"] = Guarded(rows, cols, misaligned, None, out_count, extra=1, odd_pitch=odd_pitch)
    a.img, a.stride, a.pitch = bufs["img"].ptr, bufs["img"].stride, bufs["img"].pitch
    a.out, a.ostride, a.opitch = bufs["out"].ptr, bufs["out"].stride, bufs["out"].pitch
    a.rows, a.cols, a.n, a.area, a.count = rows, cols, n, area, count
    if w is not None:
        bufs["w"] = Guarded(rows, cols, misaligned, w, 1, extra=2)
        a.w, a.wstride = bufs["w"].ptr, bufs["w"].stride
    if fam.err32_tol is not None:  # blind RL: the start PSF goes in and the refined one comes out of a device buffer
        bufs["psf"] = Guarded(psf.shape[0], psf.shape[1], misaligned, psf, 1)
        a.psf, a.prows, a.pcols, a.pstride = bufs["psf"].ptr, psf.shape[0], psf.shape[1], bufs["psf"].stride
    if fam.trace is not None and n:  # a trace of n steps behind 8 NaN doubles on each side
        a.keep = torch.full((fam.trace[0] * n + 16,), float("nan"), dtype=torch.float64, device="cuda")
        a.trace = a.keep.data_ptr() + 64
    return a, bufs


def run_dev(fam, p, imgs, w, psf, n, area, misaligned, call=None, out_count=None, odd_pitch=False):
    """one fenced _dev call (or `call`, a group call of BATCH): the output windows [count, rows, cols] (the window alone for one) and
    the Args.  Raises if a store landed outside an output window, an input changed, or a guard band was touched."""
    import torch
    a, bufs = stage(fam, imgs, w, psf, n, area, misaligned, fam.out_count if out_count is None else out_count, odd_pitch)
    a.returned = (call or fam.dev)(p, a)
    torch.cuda.synchronize()
    out, clean = bufs["out"].result()
    assert clean, "%s: a store landed outside the output window" % fam.name
    for k, b in bufs.items():
        if k == "psf":
            got_psf, clean = b.result()
            assert clean, "%s: a store landed outside the PSF window" % fam.name
            a.psf_out = got_psf[0]
        elif k != "out":
            assert b.unchanged(), "%s: the call wrote to its input `%s`" % (fam.name, k)
    if a.trace is not None:
        t, k = a.keep.cpu().numpy(), fam.trace[0]
        assert np.all(np.isnan(t[:8])) and np.all(np.isnan(t[8 + k * n:])), "%s: a store landed outside the trace" % fam.name
        a.trace_out = t[8:8 + k * n].reshape(n, k)
    return (out[0] if out.shape[0] == 1 else out), a


def defined(fam, rows, cols, psf):
    """whether the call has a defined answer on the window.  The free-boundary blind form divides the PSF step by den = corr_u(W)
    tap by tap; on a window smaller than the PSF a tap's den can be exactly 0 in exact arithmetic (every pixel it reaches lies
    where the coverage is below FDR_RL_SIGMA, so u = 0 there), and its sign is then rounding noise in any precision: the float64
    and float32 runs of the MODEL part by up to 4.2 (3 x 3 window, 255 x 3 PSF).  fdr_richardson_lucy_blind_f32* refuse such a
    window (include/fdr.h); test_edge_windows_gpu.py::test_blind_free_refuses_windows_below_the_psf holds the refusal."""
    if fam.err32_tol is not None and fam.free:
        return rows >= psf.shape[0] and cols >= psf.shape[1]
    return True


def _rlb(**kw):
    return lambda p, a: p.richardson_lucy_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, a.n, a.area,
                                                    d_weights=a.w, wstride=a.wstride, **kw)


# the group call of a family: (p, a) -> `a.count` windows at a.pitch / a.opitch.  Every image has the bytes of its single call.
BATCH = {
    "blur_fwd": lambda p, a: p.blur_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, False),
    "blur_adj": lambda p, a: p.blur_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, True),
    "rl": _rlb(), "rl_accel": _rlb(accelerate=True), "rl_free": _rlb(free_boundary=True), "rl_free_accel": _rlb(free_boundary=True, accelerate=True),
    "rl_tv": lambda p, a: p.richardson_lucy_tv_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, a.n, LAM, EPS,
                                                         norm_area=a.area),
    "rl_tv_free": lambda p, a: p.richardson_lucy_tv_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, a.n, LAM,
                                                              EPS, True, a.w, a.wstride, norm_area=a.area),
    "tv": lambda p, a: p.tv_deconv_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, MU, RHO, a.n, norm_area=a.area),
    "tv_free": lambda p, a: p.tv_deconv_free_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, MU, RHO, a.n, a.w,
                                                       a.wstride, NU, norm_area=a.area),
    "tv_auto": lambda p, a: p.tv_deconv_auto_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, SIGMA_N, RHO, a.n,
                                                       a.w, a.wstride, norm_area=a.area),
    "tv_poisson": lambda p, a: p.tv_deconv_poisson_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, MU, RHO, a.n,
                                                             a.w, a.wstride, NU, BACKGROUND, norm_area=a.area),
    "wiener_zero": lambda p, a: p.wiener_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, a.area),
    "wiener_smooth": lambda p, a: p.wiener_batch_dev(a.img, a.pitch, a.count, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, a.area),
}
