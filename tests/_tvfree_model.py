"""float64 model of free-boundary, weighted total-variation deconvolution (fdr_tv_deconv_free_f32*; include/fdr.h).

The plan is M x N, the window rows x cols at its top-left corner; m = pad(weights) is the weights on the window and 0 elsewhere
(None: 1 on the window); pad(d), H, D, L and shrink are those of _tv_model.py:

    minimise over x on the whole plan  mu / 2 sum m (blur(x) - pad(d))^2 + TV(x)

by ADMM with two splittings, z = D x (scaled dual w, penalty rho) and s = blur(x) (scaled dual q, penalty nu; nu = 0 selects rho):

    x = pad(d);  w = 0;  q = 0;  t = 1 / rho;  T = 1 / (nu |H|^2 + rho L);  n times:
        c = blur(x)
        e = c + q;  s = (mu m pad(d) + nu e) / (mu m + nu);  q = e - s;  r = s - q        outside the window: s = e, q = 0, r = c
        b = blur^T(r)
        g = D x + w;  z = shrink(g, t);  w = g - z;  v = z - w
        x = IDFT2( DFT2(nu b + rho (Dx^T vx + Dy^T vy)) . T )

Pinned in test_tvfree_host.py (the s-update, the normal equations, convergence, the periodic limit, quality, injected faults) before
it judges the GPU (test_tvfree_gpu.py)."""
import numpy as np

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, normalize, op_spectrum  # noqa: F401
from _rltv_model import line_psf, rect_scene
from _tv_model import blur_plane, dx, dxT, dy, dyT, objective, shrink, solve_table, tv_value  # noqa: F401

# Threshold from one run of test_tvfree_gpu.py on an MI355X, at most 4x the largest value measured there: max |got - model| / max
# |model| (FDR_NORM_NONE) or max-abs (normalised outputs) of the device against this model in float64.  Measured maxima: 1.53e-6 over
# n = 1, 2, 3 (64 x 128, window 37 x 101, dense 5 x 5, mu 50, rho 1, nu 3, anisotropic, fractional weights, n = 3; 4.9e-7 at 8 x 32,
# 7.6e-7 at 16 x 32, 1.18e-6 and 1.02e-6 at 256^2, 1.27e-6 at 2048 x 512) and 3.46e-6 over n = 30 and 100 (64 x 64, window 60 x 50,
# motion 15/30, mu 500, rho 2, isotropic, n = 100; 3.05e-6 at 512 x 256, window 500 x 250, masked, n = 100); 1.29e-6 and 1.84e-6 on
# the quality scene (n = 30; masked, n = 100).  The same model in float32 / complex64 on the CPU gives 4.3e-7 and 5.5e-7 on the two
# maxima (7.0e-7 at 512 x 256; 3.1e-7 .. 5.6e-7 on the cases of test_tvfree_host.py): the device stays within 10x of its arithmetic
# class everywhere (3.6x and 6.2x at the two maxima).  Unlike TV_TOL the error does not grow with mu: the solve divides by
# nu |H|^2 + rho L with nu of the order of rho.
TVF_TOL = 1.3e-5

FAULTS = ("no_mask", "q_sign", "r_is_s", "no_conj", "table_mu", "weights_ignored")


def pad_to(a, M, N, dtype):
    out = np.zeros((M, N), dtype=dtype)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def s_update(e, d_pad, m, mu, nu):
    """the minimiser over s of mu / 2 m (s - d)^2 + nu / 2 (s - e)^2, pointwise"""
    return (mu * m * d_pad + nu * e) / (mu * m + nu)


def tvfree_iterates(d, psf, M, N, mu, rho=2.0, iterations=50, weights=None, nu=0.0, anisotropic=False, dtype=np.float64, fault=None):
    """yields dict(x, z=(zx, zy), s, c, r, v=(vx, vy), q) after the start (x alone) and after every iteration, all M x N planes.
    dtype float32 runs the same formulas in single precision (float32 planes and table, complex64 spectra): the arithmetic class of
    the device.  fault (for the CPU pins only): 'no_mask' (m = 1 on the whole plan), 'q_sign' (q = s - e), 'r_is_s' (r = s),
    'no_conj' (b without the conjugate), 'table_mu' (T built with mu in place of nu), 'weights_ignored' (weights = None)."""
    assert fault is None or fault in FAULTS, fault
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    d = np.asarray(d, dtype=dtype)
    rows, cols = d.shape
    nu = float(nu) if nu else float(rho)
    H = op_spectrum(psf, M, N)
    T = solve_table(H, M, N, mu if fault == "table_mu" else nu, rho).astype(dtype)
    Hf, Hb = H.astype(cdt), (H if fault == "no_conj" else np.conj(H)).astype(cdt)
    pad = pad_to(d, M, N, dtype)
    m = np.zeros((M, N), dtype=dtype)
    m[:rows, :cols] = 1 if weights is None or fault == "weights_ignored" else np.asarray(weights, dtype=dtype)
    if fault == "no_mask":
        m[:] = 1
    inside = np.zeros((M, N), dtype=bool)
    inside[:rows, :cols] = True
    if fault == "no_mask":
        inside[:] = True
    mu_, nu_, rho_ = dtype(mu), dtype(nu), dtype(rho)
    x = pad.copy()
    wx = np.zeros((M, N), dtype=dtype)
    wy = np.zeros((M, N), dtype=dtype)
    q = np.zeros((M, N), dtype=dtype)
    t = dtype(1.0) / rho_
    yield dict(x=x)
    for _ in range(iterations):
        c = np.fft.irfft2(np.fft.rfft2(x).astype(cdt) * Hf, s=(M, N)).astype(dtype)
        e = c + q
        a = mu_ * m
        s = np.where(inside, (a * pad + nu_ * e) / (a + nu_), e).astype(dtype)
        q = np.where(inside, (s - e) if fault == "q_sign" else (e - s), 0).astype(dtype)
        r = np.where(inside, s if fault == "r_is_s" else s - q, c).astype(dtype)
        b = np.fft.irfft2(np.fft.rfft2(r).astype(cdt) * Hb, s=(M, N)).astype(dtype)
        gx, gy = dx(x) + wx, dy(x) + wy
        zx, zy = shrink(gx, gy, t, bool(anisotropic))
        wx, wy = gx - zx, gy - zy
        vx, vy = zx - wx, zy - wy
        rhs = (nu_ * b + rho_ * (dxT(vx) + dyT(vy))).astype(dtype)
        x = np.fft.irfft2(np.fft.rfft2(rhs).astype(cdt) * T, s=(M, N)).astype(dtype)
        yield dict(x=x, z=(zx, zy), s=s, c=c, r=r, v=(vx, vy), q=q)


def finish(x, out_shape, nonneg, norm_area, M, N):
    """the output of the call from the plane x: the window out_shape, max(x, 0) with nonneg, normalised over what is returned"""
    out = np.asarray(x[:out_shape[0], :out_shape[1]], dtype=np.float64)
    if nonneg:
        out = np.maximum(out, 0)
    return normalize(out, norm_area, M, N)


def tvfree_model(d, psf, M, N, mu, rho=2.0, iterations=50, weights=None, nu=0.0, anisotropic=False, nonneg=False, norm_area=NORM_NONE,
                 out_shape=None, dtype=np.float64, fault=None):
    """the output of fdr_tv_deconv_free_f32 on the window d: the top-left out_shape (default d.shape) of x"""
    st = None
    for st in tvfree_iterates(d, psf, M, N, mu, rho, iterations, weights, nu, anisotropic, dtype, fault):
        pass
    return finish(st["x"], out_shape or np.asarray(d).shape, nonneg, norm_area, M, N)


def free_objective(x, d_pad, m, H, mu, anisotropic=False):
    r = blur_plane(x, H) - d_pad
    return 0.5 * mu * float(np.sum(m * r * r)) + tv_value(x, anisotropic)


# ---- the short cases of test_tvfree_gpu.py (n = 1, 2, 3 against this model), shared with the fault pins of test_tvfree_host.py ----
# (M, N, rows, cols, stride, wstride, out_stride, output windows): cols of every residue mod 4, odd strides (no row of the caller's
# windows is 16-byte aligned), a window one row and three columns short of the plan, the window equal to the plan, and the M x N
# output with its zero-data surround
SHORT = [(8, 32, 8, 32, 32, 32, 32, ((8, 32),)),
         (16, 32, 9, 30, 31, 33, 35, ((9, 30), (16, 32))),
         (64, 128, 37, 101, 103, 101, 131, ((37, 101), (64, 128))),
         (256, 256, 200, 151, 163, 152, 256, ((200, 151), (256, 256))),
         (256, 256, 255, 253, 253, 256, 253, ((255, 253),)),
         (2048, 512, 2000, 333, 347, 336, 512, ((2000, 333),))]
SHORT_IDS = ["%dx%d-win%dx%d" % c[:4] for c in SHORT]
WEIGHT_KINDS = ("none", "mask", "fractional")


def tvf_image(M, N, rows, cols, seed):
    """float32 window with edges, texture above the thresholds used here (1 / rho >= 0.1) and negative pixels"""
    from _tv_model import blocks_scene
    rng = np.random.default_rng(seed)
    return (blocks_scene(M, N, seed)[:rows, :cols] + 0.2 * rng.random((rows, cols)) - 0.15).astype(np.float32)


def tvf_weights(kind, rows, cols, seed):
    """None, a 0 / 1 mask with 2 % zeros, or fractional weights in [0, 1]"""
    rng = np.random.default_rng(seed + 100)
    if kind == "none":
        return None
    if kind == "mask":
        return (rng.random((rows, cols)) > 0.02).astype(np.float32)
    return rng.random((rows, cols)).astype(np.float32)


def short_combos(motion, M, N, rows, cols):
    """(name, psf, mu, rho, nu, anisotropic, nonneg): motion (centred where the window is cropped) / dense 5 x 5 / delta PSFs, mu 5 ..
    500, rho 1, 2, 10, nu = rho and not, both shrinkages; the plans of a megapixel keep the first two (float64 model time)"""
    from _rl_model import dense_psf
    from _spectral import delta_psf
    full = (rows, cols) == (M, N)
    out = [("motion15/30 mu500 rho2 iso", motion if full else centred_psf(motion, M, N), 500.0, 2.0, 0.0, False, False),
           ("dense5 mu50 rho1 nu3 aniso nonneg", dense_psf(5, 5), 50.0, 1.0, 3.0, True, True),
           ("delta(2,3) mu5 rho10 nu4 iso nonneg", delta_psf(2, 3), 5.0, 10.0, 4.0, False, True)]
    out = [c for c in out if c[1].shape[0] <= M and c[1].shape[1] <= N]
    return out[:2] if M * N >= 1 << 20 else out


# ---- the quality scene: a 200 x 200 crop of a blurred, noisy piecewise-constant 512^2 scene, restored on a 256^2 plan ----
QUALITY = dict(S=512, at=(150, 170), rows=200, cols=200, M=256, N=256, noise=0.01, mu=500.0, rho=2.0, n=30, n_masked=100, stuck=0.02)


_quality = {}


def quality_case():
    """dict(truth, d (float32), stuck (d with 2 % of its pixels stuck at 1), keep (float32 weights: 0 at the stuck pixels), psf (the
    centred PSF plane of the plan)); computed once"""
    if not _quality:
        q = QUALITY
        S = q["S"]
        scene = rect_scene(S)
        psf = line_psf()
        blurred = np.fft.irfft2(np.fft.rfft2(scene) * np.fft.rfft2(centred_psf(psf, S, S).astype(np.float64)), s=scene.shape)
        noisy = blurred + q["noise"] * np.random.default_rng(4).standard_normal(blurred.shape)
        i, j = q["at"]
        d = noisy[i:i + q["rows"], j:j + q["cols"]].astype(np.float32)
        keep = np.random.default_rng(5).random((q["rows"], q["cols"])) > q["stuck"]
        _quality.update(truth=scene[i:i + q["rows"], j:j + q["cols"]], d=d, stuck=np.where(keep, d, np.float32(1.0)).astype(np.float32),
                        keep=keep.astype(np.float32), psf=centred_psf(psf, q["M"], q["N"]))
    return _quality
