"""float64 model of Richardson-Lucy with a total-variation prior, plain and free-boundary (fdr_richardson_lucy_tv_f32*,
fdr_rl_tv_factor_f32_dev; include/fdr.h): the specification.

The domain of the estimate u is R x C: the window rows x cols in the plain form, the whole M x N plan in the free-boundary form.
Differences are forward and replicate at the domain's far edges:

    gx[i, j] = j < C-1 ? u[i, j+1] - u[i, j] : 0
    gy[i, j] = i < R-1 ? u[i+1, j] - u[i, j] : 0
    m  = sqrt(gx^2 + gy^2 + eps^2);  px = gx / m;  py = gy / m
    div[i, j] = (px[i, j] - (j > 0 ? px[i, j-1] : 0)) + (py[i, j] - (i > 0 ? py[i-1, j] : 0))            (div = -D^T)
    g = 1 - lambda div
    factor = w / g        w = 1 (plain form) or wgt = 1 / alpha (free form; 0 stays 0)

    plain form:  u <- max(u . factor . blur^T(r), 0)
    free form:   u <- max(u . factor . fullblur^T(pad(r)), 0)

Starts, c, r, tau, coverage, output windows and normalisation are those of _rl_model.py and _rlfree_model.py; the factor is taken
from the u that enters the step.  lambda and eps are rounded to float32 first, as the C ABI takes them.  lambda lies in [0,
MAX_LAMBDA]: |div| <= 2 + sqrt 2, so g >= 0.57, and the model asserts g >= 0.5.  Pinned in test_rltv_host.py before it judges the
GPU (test_rltv_gpu.py).

The explicit step is not a contraction in flat areas once eps is well below 4 lambda max(u): it oscillates there at the scale of
eps, and a float32 and a float64 run of these formulas drift apart (eps = 1e-3, lambda = 0.01, the 256^2 scene below: 9.2e-6 at
n = 3, 9.5e-4 at n = 10, 2.8e-2 in max-norm at n = 30, rms 6.4e-4, 0.0001 dB of PSNR; 0.004 dB at n = 100), while with eps = 0.05
they agree to 7.7e-7 through 100 steps.  The device is therefore compared step for step only for n <= 3 at eps = 1e-3 and for longer runs at eps = 0.05; at
eps = 1e-3 and n = 100 it is compared by PSNR."""
import numpy as np

from _rl_model import NORM_NONE, TAU, blur_model, centred_psf, normalize, op_spectrum, psnr
from _rlfree_model import SIGMA, fullblur

MAX_LAMBDA = 0.125  # FDR_RLTV_MAX_LAMBDA
EPS = float(np.float32(1e-3))  # FDR_RLTV_EPS
FAULTS = ("lambda_sign", "forward_div", "no_eps", "periodic", "factor_new_u")

# Device against this model.  RLTV_FACTOR_TOL: max |got - model| of the factor with w = 1 or, with w, relative to max(w) (the
# factor is w / g with g in [0.57, 1.6]).  RLTV_TOL, RLTV_FREE_TOL: max |got - model| / max |model| (FDR_NORM_NONE) or max-abs
# (normalised outputs) of the two calls.  Each is at most 4x the largest value one run of test_rltv_gpu.py measured on an MI355X, and
# the test also holds every case within 10x of the float32 CPU run of this model (dtype=np.float32).  Measured on the MI355X (in
# brackets the float32 CPU run of the same case):
#   factor: 2.3e-7 (2.4e-7), the largest over every shape, layout, input and parameter pair (at 129 x 129 and 65 x 127); the kernel
#           forms p with a reciprocal square root where the model divides by a square root, otherwise it rounds as numpy's float32
#   plain form, largest over n and norm_area: 64x128 win 37x101 6.2e-7 (2.4e-7), 256 win 200x151 1.0e-5 (1.0e-6: the border rows of
#           a top-left PSF, where c is small), 512 full plane 1.5e-6 (7.3e-7), 2048x512 win 2000x500 n = 3 1.5e-6 (6.4e-7)
#   free form: 64x128 masked 4.5e-6 (2.6e-6), 256 win 200x151 1.0e-5 (4.5e-6), 512 full plane 1.7e-5 (3.1e-6; n = 3 at eps = 1e-3),
#           2048x512 n = 3 1.9e-5 (2.6e-6)
# Case by case the device is within a factor of 9.7 of the float32 CPU run (256 win 200x151, plain form, n = 1).  At eps = 1e-3 an
# error delta of u moves the factor by up to lambda delta / eps = 10 delta, so the transforms' own error (larger on the device than
# in numpy's float32 transforms) is what these figures show.
RLTV_FACTOR_TOL = 9e-7
RLTV_TOL = 3e-5
RLTV_FREE_TOL = 6e-5


def _f32(x):
    return float(np.float32(x))


def tv_grad(u, periodic=False):
    """(gx, gy): forward differences of u, 0 at the far edges (periodic: wrapped)"""
    u = np.asarray(u)
    if periodic:
        return np.roll(u, -1, axis=1) - u, np.roll(u, -1, axis=0) - u
    gx = np.zeros_like(u)
    gy = np.zeros_like(u)
    gx[:, :-1] = u[:, 1:] - u[:, :-1]
    gy[:-1, :] = u[1:, :] - u[:-1, :]
    return gx, gy


def tv_div(px, py, periodic=False, forward=False):
    """div = -D^T: backward differences of (px, py) with 0 before the first row / column (periodic: wrapped; forward: the fault
    that takes forward differences, 0 beyond the last)"""
    if periodic:
        s = -1 if forward else 1
        nx, ny = np.roll(px, s, axis=1), np.roll(py, s, axis=0)
    else:
        nx, ny = np.zeros_like(px), np.zeros_like(py)
        if forward:
            nx[:, :-1] = px[:, 1:]
            ny[:-1, :] = py[1:, :]
        else:
            nx[:, 1:] = px[:, :-1]
            ny[1:, :] = py[:-1, :]
    return ((nx - px) + (ny - py)) if forward else ((px - nx) + (py - ny))


def tv_g(u, lam, eps=EPS, dtype=np.float64, fault=None):
    """g = 1 - lambda div(grad u / sqrt(|grad u|^2 + eps^2)) on the domain u.shape, every operation in `dtype`"""
    u = np.asarray(u, dtype=dtype)
    lam, eps = dtype(_f32(lam)), dtype(_f32(eps))
    periodic = fault == "periodic"
    gx, gy = tv_grad(u, periodic)
    e2 = dtype(0) if fault == "no_eps" else max(eps * eps, dtype(np.finfo(np.float32).tiny))  # (the launcher keeps eps^2 a normal float)
    m = np.sqrt(gx * gx + gy * gy + e2)
    ok = m > 0
    m = np.where(ok, m, 1)
    px, py = np.where(ok, gx / m, 0).astype(dtype), np.where(ok, gy / m, 0).astype(dtype)
    div = tv_div(px, py, periodic, forward=fault == "forward_div")
    g = (1 + lam * div) if fault == "lambda_sign" else (1 - lam * div)
    assert g.dtype == dtype
    if fault is None:
        assert float(g.min()) >= 0.5, "g = %g < 0.5" % float(g.min())
    return g


def tv_factor(u, lam, eps=EPS, w=None, dtype=np.float64, fault=None):
    """factor = w / g (w = 1 for None)"""
    g = tv_g(u, lam, EPS if eps == 0 else eps, dtype, fault)
    return ((dtype(1) if w is None else np.asarray(w, dtype=dtype)) / g).astype(dtype)


def rltv_model(d, psf, M, N, iterations, lam, eps=EPS, norm_area=NORM_NONE, dtype=np.float64, tau=TAU, fault=None):
    """the plain form on the window d: rl_model of _rl_model.py with the factor in the update"""
    d = np.asarray(d, dtype=dtype)
    H = op_spectrum(psf, M, N)
    dp = np.maximum(d, 0)
    u = dp.copy()
    for _ in range(iterations):
        c = blur_model(u, psf, M, N, H=H, dtype=dtype)
        r = np.where(c > tau, dp / np.where(c > tau, c, 1), 0).astype(dtype)
        g = blur_model(r, psf, M, N, adjoint=True, H=H, dtype=dtype)
        if fault == "factor_new_u":
            un = np.maximum(u * g, 0).astype(dtype)
            u = np.maximum(un * tv_factor(un, lam, eps, dtype=dtype), 0).astype(dtype)
        else:
            u = np.maximum(u * tv_factor(u, lam, eps, dtype=dtype, fault=fault) * g, 0).astype(dtype)
    return normalize(u, norm_area, M, N)


def rltv_free_state(d, psf, M, N, iterations, lam, eps=EPS, weights=None, sigma=SIGMA, dtype=np.float64, tau=TAU, fault=None):
    """the free-boundary form: rlfree_state of _rlfree_model.py with factor = wgt / g in the place of wgt; dict(u, alpha, wgt)"""
    d = np.asarray(d, dtype=dtype)
    rows, cols = d.shape
    m = np.ones((rows, cols), dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)
    H = op_spectrum(psf, M, N)
    W = np.zeros((M, N), dtype=dtype)
    W[:rows, :cols] = m
    dw = np.zeros((M, N), dtype=dtype)
    dw[:rows, :cols] = m * np.maximum(d, 0)
    alpha = fullblur(W, H, adjoint=True, dtype=dtype)
    seen = alpha > sigma
    wgt = np.where(seen, 1 / np.where(seen, alpha, 1), 0).astype(dtype)
    sw = float(np.sum(W, dtype=np.float64))
    mean = float(np.sum(dw, dtype=np.float64)) / sw if sw > 0 else 0.0
    u = np.where(seen, mean, 0).astype(dtype)
    win = np.zeros((M, N), dtype=bool)
    win[:rows, :cols] = True
    for _ in range(iterations):
        c = fullblur(u, H, dtype=dtype)
        ok = win & (c > tau)
        r = np.where(ok, dw / np.where(ok, c, 1), 0).astype(dtype)
        g = fullblur(r, H, adjoint=True, dtype=dtype)
        if fault == "factor_new_u":
            un = np.maximum(u * wgt * g, 0).astype(dtype)
            u = np.maximum(un * tv_factor(un, lam, eps, dtype=dtype), 0).astype(dtype)
        else:
            u = np.maximum(u * tv_factor(u, lam, eps, w=wgt, dtype=dtype, fault=fault) * g, 0).astype(dtype)
    return dict(u=u, alpha=alpha, wgt=wgt)


def rltv_free_model(d, psf, M, N, iterations, lam, eps=EPS, weights=None, sigma=SIGMA, out_shape=None, norm_area=NORM_NONE, dtype=np.float64,
                    fault=None):
    """the output of fdr_richardson_lucy_tv_f32 with free_boundary: the top-left out_shape (default d.shape) of u, normalised"""
    st = rltv_free_state(d, psf, M, N, iterations, lam, eps, weights, sigma, dtype, fault=fault)
    orows, ocols = np.asarray(d).shape if out_shape is None else out_shape
    return normalize(st["u"][:orows, :ocols], norm_area, M, N)


# ---- the two quality scenes -------------------------------------------------------------------------------------------------------
# A piecewise-constant S x S scene: 12 rectangles (sides S/16 .. S/3, levels uniform in 0.2 .. 1, later ones cover earlier ones) on a
# 0.1 pedestal, default_rng(3), scaled to max 1.  It is blurred circularly on S x S with the 15 px / 30 degree line PSF centred at
# (0, 0) and given Poisson noise at 1000 photons per unit (default_rng(4)).
#   "full": S = 256, restored by the plain form on the 256^2 plan.
#   "crop": S = 512, the 200 x 200 crop at (150, 170), restored by the free-boundary form on a 256^2 plan.
# Measured with this model in float64, PSNR against the truth in dB (lambda = 0.01, eps = 1e-3):
#   "full": blurred 20.13; unregularised best iterate 23.41 at k = 21, 19.98 at n = 100; with the prior 30.87 at n = 100, 32.37 at 200
#   "crop": blurred 21.70; unregularised (free-boundary) best 24.68 at k = 14, 19.34 at n = 100; with the prior 32.35 at n = 100,
#           33.49 at 200; the plain form on that crop, with the prior, 10.29
#   flux of "full" at n = 100: sum(u) / sum(d+) = 0.99962
# The float32 run of the model gives the same PSNR to 0.004 dB at n = 100; the MI355X gave 30.861 and 32.351.
PHOTONS = 1000.0
QUALITY_LAMBDA, QUALITY_EPS, QUALITY_N = 0.01, 1e-3, 100


def line_psf(size=15, angle=30.0):
    """a motion-like line PSF made on the CPU (test_rlfree_host.py makes the same), sum 1"""
    k = np.zeros((size, size))
    c = size // 2
    for t in np.linspace(-c, c, 4 * size):
        k[int(round(c - t * np.sin(np.deg2rad(angle)))), int(round(c + t * np.cos(np.deg2rad(angle))))] = 1
    return (k / k.sum()).astype(np.float32)


def rect_scene(S, seed=3):
    rng = np.random.default_rng(seed)
    img = np.full((S, S), 0.1)
    for _ in range(12):
        h, w = rng.integers(S // 16, S // 3, 2)
        y, x = rng.integers(0, S - h), rng.integers(0, S - w)
        img[y:y + h, x:x + w] = rng.uniform(0.2, 1.0)
    return img / img.max()


def quality_case(which):
    """dict(truth, d (float32), psf (the centred PSF plane of the plan), M, N, free): the scene `which` in ("full", "crop")"""
    S = 256 if which == "full" else 512
    scene = rect_scene(S)
    psf = line_psf()
    blurred = np.fft.irfft2(np.fft.rfft2(scene) * np.fft.rfft2(centred_psf(psf, S, S).astype(np.float64)), s=scene.shape)
    noisy = np.random.default_rng(4).poisson(np.maximum(blurred, 0) * PHOTONS) / PHOTONS
    if which == "full":
        truth, d = scene, noisy
    else:
        truth, d = scene[150:350, 170:370], noisy[150:350, 170:370]
    return dict(truth=truth, d=d.astype(np.float32), psf=centred_psf(psf, 256, 256), M=256, N=256, free=which == "crop")


def quality_run(case, iterations, lam, eps=QUALITY_EPS, dtype=np.float64):
    """the form's model on a quality case (lam = 0: the unregularised form)"""
    if case["free"]:
        return rltv_free_model(case["d"], case["psf"], case["M"], case["N"], iterations, lam, eps, dtype=dtype)
    return rltv_model(case["d"], case["psf"], case["M"], case["N"], iterations, lam, eps, dtype=dtype)


def best_plain_iterate(case, upto=100):
    """(k, PSNR) of the unregularised form's best iterate over k <= upto"""
    from _rl_model import rl_model  # noqa: F401  (the same arithmetic: lam = 0 is that model)
    best = (0, -np.inf)
    d, psf, M, N = case["d"].astype(np.float64), case["psf"], case["M"], case["N"]
    H = op_spectrum(psf, M, N)
    if case["free"]:
        rows, cols = d.shape
        W = np.zeros((M, N))
        W[:rows, :cols] = 1
        dw = np.zeros((M, N))
        dw[:rows, :cols] = np.maximum(d, 0)
        alpha = fullblur(W, H, adjoint=True)
        seen = alpha > SIGMA
        wgt = np.where(seen, 1 / np.where(seen, alpha, 1), 0)
        u = np.where(seen, dw.sum() / W.sum(), 0.0)
        win = W > 0
        for k in range(1, upto + 1):
            c = fullblur(u, H)
            ok = win & (c > TAU)
            r = np.where(ok, dw / np.where(ok, c, 1), 0)
            u = np.maximum(u * wgt * fullblur(r, H, adjoint=True), 0)
            q = psnr(u[:rows, :cols], case["truth"])
            if q > best[1]:
                best = (k, q)
    else:
        dp = np.maximum(d, 0)
        u = dp.copy()
        for k in range(1, upto + 1):
            c = blur_model(u, psf, M, N, H=H)
            r = np.where(c > TAU, dp / np.where(c > TAU, c, 1), 0)
            u = np.maximum(u * blur_model(r, psf, M, N, adjoint=True, H=H), 0)
            q = psnr(u, case["truth"])
            if q > best[1]:
                best = (k, q)
    return best
