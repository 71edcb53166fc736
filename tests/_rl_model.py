"""float64 model of the blur operator and of Richardson-Lucy deconvolution (fdr_blur_f32*, fdr_richardson_lucy_f32*; include/fdr.h).

The plan is M x N, the image window rows x cols at its top-left corner.  pad(x) is x on the window and 0 elsewhere; the PSF lies
top-left in an M x N zero plane (as fdr_set_psf places it) and H = DFT2 of that plane:

    blur(x)   = window( IDFT2( H       . DFT2(pad(x)) ) )
    blur^T(y) = window( IDFT2( conj(H) . DFT2(pad(y)) ) )
    d+ = max(d, 0);  u = d+;  n times:  c = blur(u);  r = c > TAU ? d+ / c : 0;  u = max(u . blur^T(r), 0)

Built on numpy's rfft2 / irfft2, so an 8192^2 blur stays affordable.  Pinned against direct summation, adjointness, a delta PSF,
flux conservation and injected faults in test_rl_host.py before it judges the GPU (test_rl_gpu.py)."""
import numpy as np

TAU = float(np.float32(1e-7))  # FDR_RL_TAU
NORM_CROPPED, NORM_PADDED, NORM_NONE = 0, 1, 2

# Thresholds from one run of test_rl_gpu.py on an MI355X, each at most 4x the largest value measured there (in the comments).
# BLUR_TOL bounds max |got - model| / max |model| of a blur (measured 1.5e-6, 8192^2 dense 9 x 9 PSF), BLUR_BIN_TOL bin_error()
# of a full-plane blur of a tone image (a blur is linear, so the affine fit is the identity up to rounding; 3.5e-4 at 8192^2),
# ADJ_TOL the relative adjointness defect <blur x, y> - <x, blur^T y> on the device (2.1e-8).
BLUR_TOL = 5e-6
BLUR_BIN_TOL = 1.2e-3
ADJ_TOL = 8e-8
# RL against the float64 model: max |got - model| / max |model| (FDR_NORM_NONE) or max-abs (normalised outputs), n <= 30 on
# planes up to 2048 x 512, n <= 3 at 4096^2 and 8192^2 (measured 3.3e-6: 2048 x 512, window 2000 x 512, n = 30).  DELTA_TOL: a delta PSF against d+
# (6.5e-7).  FLUX_TOL is the bound the feature promises (measured 1.2e-8 after 30 iterations at 512^2).
RL_TOL = 8e-6
DELTA_TOL = 2.5e-6
FLUX_TOL = 1e-5


def centred_psf(psf, M, N):
    """the M x N plane of `psf` rolled so that its centre tap lies at (0, 0): the blur then keeps each pixel in place instead of
    shifting it by half the PSF"""
    plane = np.zeros((M, N), dtype=np.float32)
    plane[:psf.shape[0], :psf.shape[1]] = psf
    return np.roll(plane, (-(psf.shape[0] // 2), -(psf.shape[1] // 2)), axis=(0, 1))


def op_spectrum(psf, M, N, dtype=np.float64):
    """rfft2 of the PSF placed top-left in an M x N zero plane (M x (N/2 + 1))"""
    psf = np.asarray(psf, dtype=np.float64)
    plane = np.zeros((M, N), dtype=dtype)
    plane[:psf.shape[0], :psf.shape[1]] = psf
    return np.fft.rfft2(plane)


def blur_model(x, psf, M, N, adjoint=False, H=None, dtype=np.float64):
    """blur(x) (or blur^T(x)) on the window x.shape; H: op_spectrum(psf, M, N), computed when None.  dtype float32 runs the same
    formula in single precision (complex64 spectra), the arithmetic class of the device."""
    x = np.asarray(x)
    rows, cols = x.shape
    if H is None:
        H = op_spectrum(psf, M, N)
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    plane = np.zeros((M, N), dtype=dtype)
    plane[:rows, :cols] = x
    X = np.fft.rfft2(plane).astype(cdt)
    Hc = H.astype(cdt)
    Y = X * (np.conj(Hc) if adjoint else Hc)
    return np.fft.irfft2(Y, s=(M, N))[:rows, :cols].astype(dtype)


def normalize(u, norm_area, M, N):
    """FDR_NORM_* of the RL calls: NONE the raw estimate, CROPPED min-max over the window, PADDED min-max over the plan (u = 0 outside
    the window); a flat result becomes 0 (minmax_to_scale_shift of the device)"""
    u = np.asarray(u, dtype=np.float64)
    if norm_area == NORM_NONE:
        return u
    lo, hi = float(u.min()), float(u.max())
    if norm_area == NORM_PADDED and u.shape != (M, N):
        lo, hi = min(lo, 0.0), max(hi, 0.0)
    if hi - lo <= 2.2204460492503131e-16:
        return np.zeros_like(u)
    return (u - lo) / (hi - lo)


def rl_model(d, psf, M, N, iterations, norm_area=NORM_NONE, dtype=np.float64, tau=TAU, fault=None):
    """Richardson-Lucy on the window d.  fault (for the CPU pins only): 'no_conj' (the adjoint without the conjugate), 'raw_d'
    (d in place of d+ in the ratio and the start)"""
    d = np.asarray(d, dtype=dtype)
    H = op_spectrum(psf, M, N)
    dp = d if fault == "raw_d" else np.maximum(d, 0)
    u = dp.copy()
    for _ in range(iterations):
        c = blur_model(u, psf, M, N, H=H, dtype=dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(c > tau, dp / np.where(c > tau, c, 1), 0).astype(dtype)
        g = blur_model(r, psf, M, N, adjoint=fault != "no_conj", H=H, dtype=dtype)
        u = np.maximum(u * g, 0).astype(dtype)
    return normalize(u, norm_area, M, N)


def rel_err(got, want):
    """max |got - want| / max |want| in float64 (NaN when either holds a NaN)"""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1e-30))


def psnr(x, ref):
    """PSNR in dB of x against ref, peak = max(ref) - min(ref)"""
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    peak = float(ref.max() - ref.min())
    return 10.0 * np.log10(peak * peak / float(np.mean((x - ref) ** 2)))


def smooth_image(M, N, seed):
    """float32 M x N positive test picture: a few Gaussian blobs and a soft-edged bar on a pedestal, values in (0, 1]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:M, 0:N].astype(np.float64)
    img = np.full((M, N), 0.1)
    for _ in range(6):
        cy, cx = rng.uniform(0.15, 0.85) * M, rng.uniform(0.15, 0.85) * N
        s = rng.uniform(0.02, 0.08) * min(M, N)
        img += rng.uniform(0.3, 0.7) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    # a bar with soft (logistic, 1.5 px) edges
    inside = np.minimum(0.04 * M - np.abs(yy - 0.3 * M), 0.3 * N - np.abs(xx - 0.5 * N))
    img += 0.3 / (1 + np.exp(-inside / 1.5))
    return (img / img.max()).astype(np.float32)


def dense_psf(seed, size=9):
    """a dense random non-negative size x size PSF, normalised to sum 1"""
    p = np.random.default_rng(seed).random((size, size))
    return (p / p.sum()).astype(np.float32)
