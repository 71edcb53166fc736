"""float64 model of total-variation deconvolution by ADMM (fdr_tv_deconv_f32*; include/fdr.h).

The plan is M x N, the image window rows x cols at its top-left corner, pad(d) is d on the window and 0 elsewhere; the PSF lies
top-left in an M x N zero plane and H = DFT2 of that plane (op_spectrum of _rl_model.py).  Differences are forward and periodic:

    Dx x[i, j] = x[i, (j+1) % N] - x[i, j]     Dy x[i, j] = x[(i+1) % M, j] - x[i, j]     Dx^T v[i, j] = v[i, (j-1) % N] - v[i, j]
    L(u, v) = 4 sin^2(pi u / M) + 4 sin^2(pi v / N) = |DFT(Dx)|^2 + |DFT(Dy)|^2

    minimise  mu / 2 ||blur(x) - pad(d)||^2 + TV(x)
    b = mu blur^T(pad(d));  x = pad(d);  wx = wy = 0;  t = 1 / rho;  n times:
        gx = Dx x + wx;  gy = Dy x + wy;  z = shrink(g, t);  w = g - z;  v = z - w
        x = IDFT2( DFT2(b + rho (Dx^T vx + Dy^T vy)) / (mu |H|^2 + rho L) )

Built on numpy's rfft2 / irfft2.  Pinned in test_tv_host.py (symbol, adjointness, normal equations, proximal map, convergence,
invariants, injected faults) before it judges the GPU (test_tv_gpu.py)."""
import numpy as np

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, normalize, op_spectrum  # noqa: F401

# Threshold from one run of test_tv_gpu.py on an MI355X, at most 4x the largest value measured there: max |got - model| / max |model|
# (FDR_NORM_NONE) or max-abs (normalised outputs) of the device against this model in float64.  Measured maxima: 3.6e-5 over
# n = 1, 2, 3 (8192^2, motion 15/30, mu 500, rho 2, isotropic, n = 3; 2.1e-5 at 4096^2, 1.4e-5 at 1024^2, 7.6e-6 at 256^2) and 2.7e-5
# over n = 30 and 100 (2048 x 512, window 2000 x 500, mu 50, rho 10, anisotropic, n = 100).  The same model in float32 / complex64 on
# the CPU gives 7.9e-6 and 3.3e-6 on those two cases (5.9e-6 at 1024^2, 4.9e-6 at 4096^2; 1.7e-6 .. 7.5e-6 on the cases of
# test_tv_host.py): the device stays within 10x of its arithmetic class everywhere (4.5x and 8.3x at the two maxima).  The error
# grows with mu and with the plan because the solve divides by mu |H|^2 + rho L, which is small where the PSF's spectrum has its
# zeros at low frequencies.
TV_TOL = 1.2e-4


def lap_symbol(M, N):
    """L on the half spectrum, M x (N/2 + 1)"""
    a = 4.0 * np.sin(np.pi * np.arange(M) / M) ** 2
    b = 4.0 * np.sin(np.pi * np.arange(N // 2 + 1) / N) ** 2
    return a[:, None] + b[None, :]


def dx(x):
    return np.roll(x, -1, axis=1) - x


def dy(x):
    return np.roll(x, -1, axis=0) - x


def dxT(v):
    return np.roll(v, 1, axis=1) - v


def dyT(v):
    return np.roll(v, 1, axis=0) - v


def shrink(gx, gy, t, anisotropic):
    """the proximal map of t * TV at g: isotropic (the vector (gx, gy) shortened by t) or anisotropic (each component)"""
    if anisotropic:
        return np.sign(gx) * np.maximum(np.abs(gx) - t, 0), np.sign(gy) * np.maximum(np.abs(gy) - t, 0)
    m = np.sqrt(gx * gx + gy * gy)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(m > t, 1 - t / np.where(m > t, m, 1), 0).astype(gx.dtype)
    return s * gx, s * gy


def tv_value(x, anisotropic):
    gx, gy = dx(x), dy(x)
    return float(np.sum(np.abs(gx) + np.abs(gy))) if anisotropic else float(np.sum(np.sqrt(gx * gx + gy * gy)))


def blur_plane(x, H, adjoint=False):
    """circular blur of the whole M x N plane x (float64)"""
    return np.fft.irfft2(np.fft.rfft2(x) * (np.conj(H) if adjoint else H), s=x.shape)


def objective(x, d_pad, H, mu, anisotropic):
    r = blur_plane(x, H) - d_pad
    return 0.5 * mu * float(np.sum(r * r)) + tv_value(x, anisotropic)


def solve_table(H, M, N, mu, rho):
    """1 / (mu |H|^2 + rho L); 0 where the denominator is 0"""
    den = mu * np.abs(H) ** 2 + rho * lap_symbol(M, N)
    return np.where(den > 0, 1.0 / np.where(den > 0, den, 1), 0.0)


def tv_iterates(d, psf, M, N, mu, rho=2.0, iterations=50, anisotropic=False, dtype=np.float64, fault=None):
    """yields (x, zx, zy, rhs) of every iteration, x the M x N plane.  dtype float32 runs the same formulas in single precision
    (float32 planes and table, complex64 spectra): the arithmetic class of the device.  fault (for the CPU pins only): 'no_conj' (b
    without the conjugate), 'dxT_sign' (Dx^T with the wrong sign), 'thr_rho' (threshold rho instead of 1 / rho), 'swap_shrink'
    (the other shrinkage)."""
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    d = np.asarray(d, dtype=dtype)
    rows, cols = d.shape
    H = op_spectrum(psf, M, N)
    T = solve_table(H, M, N, mu, rho).astype(dtype)
    pad = np.zeros((M, N), dtype=dtype)
    pad[:rows, :cols] = d
    Hb = (H if fault == "no_conj" else np.conj(H)).astype(cdt)
    b = (dtype(mu) * np.fft.irfft2(np.fft.rfft2(pad).astype(cdt) * Hb, s=(M, N)).astype(dtype)).astype(dtype)
    x = pad.copy()
    wx = np.zeros((M, N), dtype=dtype)
    wy = np.zeros((M, N), dtype=dtype)
    t = dtype(rho) if fault == "thr_rho" else dtype(1.0) / dtype(rho)
    aniso = bool(anisotropic) != (fault == "swap_shrink")
    yield x, None, None, None
    for _ in range(iterations):
        gx, gy = dx(x) + wx, dy(x) + wy
        zx, zy = shrink(gx, gy, t, aniso)
        wx, wy = gx - zx, gy - zy
        vx, vy = zx - wx, zy - wy
        div = (-dxT(vx) if fault == "dxT_sign" else dxT(vx)) + dyT(vy)
        rhs = (b + dtype(rho) * div).astype(dtype)
        x = np.fft.irfft2(np.fft.rfft2(rhs).astype(cdt) * T, s=(M, N)).astype(dtype)
        yield x, zx, zy, rhs


def tv_model(d, psf, M, N, mu, rho=2.0, iterations=50, anisotropic=False, nonneg=False, norm_area=NORM_NONE, dtype=np.float64, fault=None):
    """the output of fdr_tv_deconv_f32 on the window d: x on the window, max(x, 0) with nonneg, normalised by norm_area"""
    rows, cols = np.asarray(d).shape
    x = None
    for x, _, _, _ in tv_iterates(d, psf, M, N, mu, rho, iterations, anisotropic, dtype, fault):
        pass
    out = np.asarray(x[:rows, :cols], dtype=np.float64)
    if nonneg:
        out = np.maximum(out, 0)
    return normalize(out, norm_area, M, N)


def blocks_scene(M, N, seed=0):
    """float64 piecewise-constant picture: rectangles of random level on a pedestal of 0.2, values in [0.1, 1]"""
    rng = np.random.default_rng(seed)
    img = np.full((M, N), 0.2)
    for _ in range(12):
        h, w = int(rng.uniform(0.08, 0.3) * M), int(rng.uniform(0.08, 0.3) * N)
        r, c = int(rng.uniform(0.05, 0.9) * (M - h)), int(rng.uniform(0.05, 0.9) * (N - w))
        img[r:r + h, c:c + w] = rng.uniform(0.1, 1.0)
    return img
