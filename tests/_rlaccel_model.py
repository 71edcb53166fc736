"""float64 model of accelerated Richardson-Lucy (fdr_richardson_lucy_accel_f32*, fdr_richardson_lucy_free_accel_f32*; include/fdr.h):
Biggs & Andrews' vector extrapolation around the iteration of _rl_model.py / _rlfree_model.py.

With step(y) one iteration of either form applied to y, and u_0 the start of the plain call:

    k = 0, 1 :  alpha_k = 0;  y_k = u_k
    k >= 2   :  alpha_k = clamp( sum(g_(k-1) . g_(k-2)) / sum(g_(k-2) . g_(k-2)), 0, ACCEL_MAX )   (0 for a zero denominator or a
                quotient that is not finite);  y_k = max(u_k + alpha_k (u_k - u_(k-1)), 0)
    every k  :  u_(k+1) = step(y_k);   g_k = u_(k+1) - y_k

The sums run over the window (plain form) or the whole plan (free-boundary form).  Pinned against the plain models, the flux
identities, fixed points and injected faults in test_rlaccel_host.py before it judges the GPU (test_rlaccel_gpu.py)."""
import numpy as np

from _rl_model import NORM_NONE, TAU, blur_model, centred_psf, normalize, op_spectrum, smooth_image
from _rlfree_model import SIGMA, fullblur, rlfree_state

ACCEL_MAX = 0.9990234375  # FDR_RL_ACCEL_MAX = 1 - 2^-10

# Thresholds from one run of test_rlaccel_gpu.py on an MI355X, each at most 4x the largest value measured there and none above 1e-4.
# RLA_TOL, the plain form against this model, max |got - model| / max |model| (FDR_NORM_NONE) or max-abs (normalised outputs) over
# n in {0, 1, 2, 3, 5, 30} and the three norm_area: measured 3.66e-6 (1024 x 512, window 999 x 345, n = 30; 1.4e-6 at 2048 x 1024, n = 4).
# RLA_FREE_TOL, the free-boundary form likewise over both output windows: measured 1.58e-5 (512^2, window 480 x 470, dense 5 x 5 PSF;
# 6.4e-6 on the masked 64 x 128 case).  RLA_ALPHA_TOL, max |alpha_k - model| over k, both forms: measured 6.37e-5 (masked 64 x 128
# case, n = 30; plain form 2.48e-5; at most 8.7e-7 up to n = 5) -- alpha is a ratio of two sums that shrink as the iteration
# converges, so it carries the estimate's relative error amplified.  The free-boundary case with the thin motion PSF is held to
# 10x the float32 CPU run of this model instead (test_rlaccel_gpu.py says why): measured 1.89e-4 in u on the whole plan against
# 4.5e-5 for the float32 CPU run, 1.1e-5 on the window, 2.31e-4 against 1.19e-4 in alpha.
RLA_TOL = 1.2e-5
RLA_FREE_TOL = 6e-5
RLA_ALPHA_TOL = 1e-4

FAULTS = ("alpha_early", "no_clip", "stale_g", "swap_u")


def accelerate(u0, step, iterations, dtype=np.float64, fault=None, keep=None):
    """the recursion around `step` from the start u0: (u_n, alphas[n]).  fault (for the CPU pins only): 'alpha_early' (alpha applied
    from k = 1), 'no_clip' (y not clipped at 0), 'stale_g' (g_(k-2) in both factors), 'swap_u' (u_(k-1) - u_k).  keep: a dict that
    receives u_k for every k <= iterations it has as a key (the run to n is the run to any k <= n, stopped there)."""
    assert fault is None or fault in FAULTS
    u = np.asarray(u0, dtype=dtype)
    if keep is not None and 0 in keep:
        keep[0] = u
    u_prev, g1, g2 = None, None, None  # u_(k-1), g_(k-1), g_(k-2)
    alphas = np.zeros(iterations, dtype=np.float64)
    for k in range(iterations):
        alpha = 0.0
        if k >= (1 if fault == "alpha_early" else 2):
            b = g2 if g2 is not None else g1  # g_(k-2); at k = 1 (alpha_early) only g_0 exists
            a = b if fault == "stale_g" else g1
            num = float(np.sum(a.astype(np.float64) * b.astype(np.float64)))
            den = float(np.sum(b.astype(np.float64) * b.astype(np.float64)))
            q = num / den if den != 0.0 else 0.0
            alpha = min(max(q, 0.0), ACCEL_MAX) if np.isfinite(q) else 0.0
            alpha = float(np.float32(alpha)) if dtype == np.float32 else alpha
        alphas[k] = alpha
        if alpha != 0.0:
            diff = (u_prev - u) if fault == "swap_u" else (u - u_prev)
            y = u + dtype(alpha) * diff
            y = (y if fault == "no_clip" else np.maximum(y, 0)).astype(dtype)
        else:
            y = u
        u_next = step(y)
        g2, g1 = g1, (u_next - y).astype(dtype)
        u_prev, u = u, u_next
        if keep is not None and k + 1 in keep:
            keep[k + 1] = u
    return u, alphas


def rl_step_fn(d, psf, M, N, dtype=np.float64, tau=TAU):
    """(u_0, step) of the plain form on the window d"""
    d = np.asarray(d, dtype=dtype)
    H = op_spectrum(psf, M, N)
    dp = np.maximum(d, 0)

    def step(y):
        c = blur_model(y, psf, M, N, H=H, dtype=dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(c > tau, dp / np.where(c > tau, c, 1), 0).astype(dtype)
        g = blur_model(r, psf, M, N, adjoint=True, H=H, dtype=dtype)
        return np.maximum(y * g, 0).astype(dtype)

    return dp.copy(), step


def rl_accel_model(d, psf, M, N, iterations, norm_area=NORM_NONE, dtype=np.float64, fault=None):
    """fdr_richardson_lucy_accel_f32 on the window d: (output, alphas)"""
    u0, step = rl_step_fn(d, psf, M, N, dtype)
    u, alphas = accelerate(u0, step, iterations, dtype, fault)
    return normalize(u, norm_area, M, N), alphas


def rlfree_step_fn(d, psf, M, N, weights=None, sigma=SIGMA, dtype=np.float64, tau=TAU):
    """(state of the start, step) of the free-boundary form; the state is rlfree_state(..., 0)"""
    st = rlfree_state(d, psf, M, N, 0, weights, sigma, dtype, tau)
    rows, cols = np.asarray(d).shape
    H = op_spectrum(psf, M, N)
    win = np.zeros((M, N), dtype=bool)
    win[:rows, :cols] = True
    dw, wgt = st["dw"], st["wgt"]

    def step(y):
        c = fullblur(y, H, dtype=dtype)
        ok = win & (c > tau)
        r = np.where(ok, dw / np.where(ok, c, 1), 0).astype(dtype)
        g = fullblur(r, H, adjoint=True, dtype=dtype)
        return np.maximum(y * wgt * g, 0).astype(dtype)

    return st, step


def rl_accel_path(d, psf, M, N, counts, dtype=np.float64):
    """({n: raw u_n on the window for n in counts}, the alphas of max(counts) iterations) of the plain form, in one run"""
    u0, step = rl_step_fn(d, psf, M, N, dtype)
    keep = dict.fromkeys(counts)
    _, alphas = accelerate(u0, step, max(counts), dtype, keep=keep)
    return keep, alphas


def rlfree_accel_path(d, psf, M, N, counts, weights=None, sigma=SIGMA, dtype=np.float64):
    """(the start's state, {n: u_n on the whole plan}, alphas) of the free-boundary form, in one run"""
    st, step = rlfree_step_fn(d, psf, M, N, weights, sigma, dtype)
    keep = dict.fromkeys(counts)
    _, alphas = accelerate(st["u"], step, max(counts), dtype, keep=keep)
    return st, keep, alphas


def rlfree_accel_state(d, psf, M, N, iterations, weights=None, sigma=SIGMA, dtype=np.float64, fault=None):
    """(state with u = u_n, alphas): the state of rlfree_state after `iterations` accelerated steps"""
    st, step = rlfree_step_fn(d, psf, M, N, weights, sigma, dtype)
    u, alphas = accelerate(st["u"], step, iterations, dtype, fault)
    st = dict(st)
    st["u"] = u
    return st, alphas


def rlfree_accel_model(d, psf, M, N, iterations, weights=None, sigma=SIGMA, out_shape=None, norm_area=NORM_NONE, dtype=np.float64,
                       fault=None):
    """fdr_richardson_lucy_free_accel_f32: (the top-left out_shape (default d.shape) of u_n normalised by norm_area, alphas)"""
    st, alphas = rlfree_accel_state(d, psf, M, N, iterations, weights, sigma, dtype, fault)
    orows, ocols = np.asarray(d).shape if out_shape is None else out_shape
    return normalize(st["u"][:orows, :ocols], norm_area, M, N), alphas


def i_divergence(dp, c):
    """sum(dp log(dp / c) - dp + c) in float64 over pixels with c > 0 (0 log 0 = 0): the functional Richardson-Lucy descends"""
    dp = np.asarray(dp, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    ok = c > 0
    t = np.where(ok & (dp > 0), dp * np.log(np.where(ok & (dp > 0), dp / np.where(ok, c, 1), 1)), 0.0)
    return float(np.sum(t[ok] - dp[ok] + c[ok]))


# ---- the scenes of the convergence claim (test_rlaccel_host.py on the model, test_rlaccel_gpu.py on the device) ----
def unit_psf(psf):
    """psf normalised to sum 1 (float32)"""
    psf = np.asarray(psf, dtype=np.float64)
    return (psf / psf.sum()).astype(np.float32)


def plain_scene(psf, M=512, N=512):
    """smooth_image blurred circularly on the plan, noise sigma 2e-3 (a full-plane window)"""
    truth = smooth_image(M, N, 7).astype(np.float64)
    return (blur_model(truth, psf, M, N) + np.random.default_rng(1).normal(0, 2e-3, (M, N))).astype(np.float32)


def free_scene(psf, M=256, N=512, rows=200, cols=400):
    """(centred PSF plane, window): smooth_image blurred circularly on the plan with the centred PSF, cropped, noise sigma 2e-3"""
    cp = centred_psf(psf, M, N)
    blurred = fullblur(smooth_image(M, N, 7).astype(np.float64), np.fft.rfft2(cp.astype(np.float64)))
    return cp, (blurred[:rows, :cols] + np.random.default_rng(2).normal(0, 2e-3, (rows, cols))).astype(np.float32)


def plain_divergence(d, psf, M, N, u):
    """I-divergence of blur(u) against d+ on the window"""
    return i_divergence(np.maximum(d, 0), blur_model(u, psf, M, N))


def free_divergence(d, cp, M, N, u_plan):
    """I-divergence of window(fullblur(u)) against d+ for an estimate on the whole plan"""
    rows, cols = np.asarray(d).shape
    return i_divergence(np.maximum(d, 0), fullblur(u_plan, op_spectrum(cp, M, N))[:rows, :cols])
