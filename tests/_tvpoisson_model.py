"""float64 / float32 model of Poisson-likelihood total-variation deconvolution (fdr_tv_deconv_poisson_f32*; include/fdr.h, DESIGN.md
section 36): the free-boundary iteration of _tvfree_model.py with its data step replaced.

    minimise over x on the whole plan  mu sum m [ (blur(x) + b) - d+ log(blur(x) + b) ] + TV(x)

d+ = max(d, 0), m = pad(weights) (None: 1 on the window, 0 elsewhere), b >= 0 the background.  Per window pixel with m > 0

    e = c + q;  k = mu m / nu;  a = e + b - k;  y = the root >= 0 of y^2 - a y - k d+ = 0;  s = y - b;  q = e - s;  r = s - q

and s = e where m = 0 and outside the window; everything else is tvfree_iterates.  step_f32 repeats the device's float operations in
the device's order (tvpoisson_data_pixel of csrc/fdr_kernels.hpp) and must give its bits.

Pinned in test_tvpoisson_host.py (the optimality of the s-update, the branches of the root, the objective, convergence, injected
faults, quality against the least-squares model) before it judges the GPU (test_tvpoisson_gpu.py)."""
import numpy as np

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, normalize, op_spectrum, psnr  # noqa: F401
from _rltv_model import line_psf, rect_scene
from _tv_model import blur_plane, dx, dxT, dy, dyT, shrink, solve_table, tv_value
from _tvfree_model import SHORT, SHORT_IDS, WEIGHT_KINDS, finish, pad_to, short_combos, tvf_image, tvf_weights, tvfree_model  # noqa: F401

# Threshold from one run of test_tvpoisson_gpu.py on an MI355X, at most 4x the largest value measured there: max |got - model| / max
# |model| (FDR_NORM_NONE) or max-abs (normalised outputs) of the device against this model in float64.  Measured maxima: 2.42e-6 over
# n = 1, 2, 3 (16 x 32, window 9 x 30, delta(2,3), mu 5, rho 10, nu 4, b 0.3, fractional weights, n = 2; 5.4e-7 at 8 x 32, 2.14e-6 at
# 64 x 128, 2.10e-6 and 2.36e-6 at 256^2, 1.33e-6 at 2048 x 512) and 3.59e-6 over n = 30 and 100 (512 x 256, window 500 x 250, motion
# 15/30, mu 500, rho 2, b 0, masked, n = 100; 2.92e-6 at 64 x 64, window 60 x 50, n = 100); 1.84e-6 and 2.97e-6 on the quality scenes
# (100 and 1000 photons, n = 100).  The same model in float32 / complex64 on the CPU gives, on the same cases, 1.49e-6 at 16 x 32
# (4.1e-7 at 8 x 32, 7.0e-7 at 64 x 128, 6.8e-7 and 8.1e-7 at 256^2, 7.1e-7 at 2048 x 512), 1.28e-6 at 64 x 64 and 1.02e-6 at 512 x
# 256: the device stays within 10x of its arithmetic class everywhere (3.5x at the maximum, 1.6x .. 3.1x elsewhere).  As for TVF_TOL the
# error does not grow with mu.  The step alone has no tolerance: the device gives the bits of step_f32.
TVP_TOL = 1.4e-5

FAULTS = ("gauss_step", "no_background", "k_without_m", "minus_root", "q_sign", "no_clamp_d")


def s_update(e, d, m, mu, nu, b, fault=None):
    """the minimiser over s of mu m [(s + b) - d+ log(s + b)] + nu / 2 (s - e)^2, pointwise, in the dtype of e; s = e where m is not
    above 0.  The root is formed as the device forms it: without cancellation."""
    dt = e.dtype.type
    mu, nu, b = dt(mu), dt(nu), dt(0.0 if fault == "no_background" else b)
    with np.errstate(invalid="ignore", divide="ignore"):
        if fault == "gauss_step":
            a = mu * m
            return np.where(m > 0, (a * d + nu * e) / (a + nu), e).astype(dt)
        k = (mu * m) / nu
        if fault == "k_without_m":
            k = np.where(m > 0, mu / nu, dt(0)).astype(dt)
        dp = d if fault == "no_clamp_d" else np.where(d < 0, dt(0), d)
        a = (e + b) - k
        t = k * dp
        disc = a * a + dt(4) * t
        rt = np.sqrt(np.maximum(disc, 0) if fault == "no_clamp_d" else disc)
        pos = a >= 0
        if fault == "minus_root":
            y = dt(0.5) * (a - rt)
        else:
            y = np.where(pos, dt(0.5) * (a + rt), (dt(2) * t) / np.where(pos, dt(1), rt - a))
        return np.where(m > 0, y - b, e).astype(dt)


def step_f32(c, q, d, weights, mu, nu, b):
    """the device's data step on the rows x cols window of the float32 planes c and q (copies returned): every operation one float32
    operation, in the order of tvpoisson_data_pixel"""
    c = np.array(c, dtype=np.float32)
    q = np.array(q, dtype=np.float32)
    d = np.asarray(d, dtype=np.float32)
    rows, cols = d.shape
    m = np.ones((rows, cols), dtype=np.float32) if weights is None else np.asarray(weights, dtype=np.float32)
    e = c[:rows, :cols] + q[:rows, :cols]
    s = s_update(e, d, m, mu, nu, b)
    assert s.dtype == np.float32
    qn = e - s
    q[:rows, :cols] = qn
    c[:rows, :cols] = s - qn
    return c, q


def tvpoisson_iterates(d, psf, M, N, mu, rho=2.0, iterations=50, weights=None, nu=0.0, background=0.0, anisotropic=False, dtype=np.float64,
                       fault=None):
    """yields dict(x, s, c, r, q, ...) after the start (x alone) and after every iteration, all M x N planes; dtype float32 runs the
    same formulas in single precision (complex64 spectra).  fault (for the CPU pins only): see FAULTS."""
    assert fault is None or fault in FAULTS, fault
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    d = np.asarray(d, dtype=dtype)
    rows, cols = d.shape
    nu = float(nu) if nu else float(rho)
    H = op_spectrum(psf, M, N)
    T = solve_table(H, M, N, nu, rho).astype(dtype)
    Hf, Hb = H.astype(cdt), np.conj(H).astype(cdt)
    pad = pad_to(d, M, N, dtype)
    m = np.zeros((M, N), dtype=dtype)
    m[:rows, :cols] = 1 if weights is None else np.asarray(weights, dtype=dtype)
    nu_, rho_ = dtype(nu), dtype(rho)
    x = pad.copy()
    wx = np.zeros((M, N), dtype=dtype)
    wy = np.zeros((M, N), dtype=dtype)
    q = np.zeros((M, N), dtype=dtype)
    t = dtype(1.0) / rho_
    yield dict(x=x)
    for _ in range(iterations):
        c = np.fft.irfft2(np.fft.rfft2(x).astype(cdt) * Hf, s=(M, N)).astype(dtype)
        e = c + q
        s = s_update(e, pad, m, mu, nu, background, fault)
        q = ((s - e) if fault == "q_sign" else (e - s)).astype(dtype)
        r = (s - q).astype(dtype)
        b = np.fft.irfft2(np.fft.rfft2(r).astype(cdt) * Hb, s=(M, N)).astype(dtype)
        gx, gy = dx(x) + wx, dy(x) + wy
        zx, zy = shrink(gx, gy, t, bool(anisotropic))
        wx, wy = gx - zx, gy - zy
        vx, vy = zx - wx, zy - wy
        rhs = (nu_ * b + rho_ * (dxT(vx) + dyT(vy))).astype(dtype)
        x = np.fft.irfft2(np.fft.rfft2(rhs).astype(cdt) * T, s=(M, N)).astype(dtype)
        yield dict(x=x, z=(zx, zy), s=s, c=c, r=r, v=(vx, vy), q=q)


def tvpoisson_model(d, psf, M, N, mu, rho=2.0, iterations=50, weights=None, nu=0.0, background=0.0, anisotropic=False, nonneg=False,
                    norm_area=NORM_NONE, out_shape=None, dtype=np.float64, fault=None):
    """the output of fdr_tv_deconv_poisson_f32 on the window d: the top-left out_shape (default d.shape) of x"""
    st = None
    for st in tvpoisson_iterates(d, psf, M, N, mu, rho, iterations, weights, nu, background, anisotropic, dtype, fault):
        pass
    return finish(st["x"], out_shape or np.asarray(d).shape, nonneg, norm_area, M, N)


def poisson_objective(x, d_pad, m, H, mu, background=0.0, anisotropic=False):
    """mu sum m [(blur(x) + b) - d+ log(blur(x) + b)] + TV(x); +inf where a pixel with m d+ > 0 has blur(x) + b <= 0"""
    u = blur_plane(x, H) + background
    dp = np.maximum(d_pad, 0)
    need = (m > 0) & (dp > 0)
    if np.any(u[need] <= 0) or np.any(u[m > 0] < 0):
        return float("inf")
    term = u - np.where(need, dp * np.log(np.where(need, u, 1.0)), 0.0)
    return mu * float(np.sum(m * term)) + tv_value(x, anisotropic)


def tvp_image(M, N, rows, cols, seed):
    """tvf_image lowered by 0.2, so that a good share of its pixels is negative (they are clamped), with 3 % of the pixels exactly 0"""
    img = tvf_image(M, N, rows, cols, seed) - np.float32(0.2)
    img[np.random.default_rng(seed + 200).random((rows, cols)) < 0.03] = 0
    return img


# ---- the quality scenes: a 200 x 200 crop of a blurred 512^2 scene with Poisson noise, restored on a 256^2 plan ----
QUALITY = dict(S=512, at=(150, 170), rows=200, cols=200, M=256, N=256, rho=2.0, nu=2.0, n=100, photons=(100, 1000), floor=0.02,
               mu_poisson=tuple(2.0 ** k for k in range(0, 8)), mu_gauss=tuple(2.0 ** k for k in range(3, 12)))

_quality = {}


def quality_case(photons):
    """dict(truth, d (float32 crop of the noisy counts / photons), psf (the centred PSF plane of the plan)) at `photons` per unit;
    computed once per level.  Scene 0.02 + rect_scene(512)^3, 15 px / 30 deg line PSF, Poisson noise from default_rng(4)."""
    if photons not in _quality:
        q = QUALITY
        S = q["S"]
        scene = q["floor"] + rect_scene(S) ** 3
        psf = line_psf()
        blurred = np.fft.irfft2(np.fft.rfft2(scene) * np.fft.rfft2(centred_psf(psf, S, S).astype(np.float64)), s=scene.shape)
        noisy = np.random.default_rng(4).poisson(np.maximum(blurred, 0) * photons) / float(photons)
        i, j = q["at"]
        _quality[photons] = dict(truth=scene[i:i + q["rows"], j:j + q["cols"]], d=noisy[i:i + q["rows"], j:j + q["cols"]].astype(np.float32),
                                 psf=centred_psf(psf, q["M"], q["N"]))
    return _quality[photons]


def quality_psnr(photons, mu, poisson=True):
    """PSNR against the truth of the float64 model's restoration (Poisson step, or the least-squares free model) at mu"""
    q, k = QUALITY, quality_case(photons)
    if poisson:
        out = tvpoisson_model(k["d"], k["psf"], q["M"], q["N"], mu, q["rho"], q["n"], None, q["nu"], 0.0, False, True)
    else:
        out = tvfree_model(k["d"], k["psf"], q["M"], q["N"], mu, q["rho"], q["n"], None, q["nu"], False, True)
    return psnr(out, k["truth"])
