"""float64 model of free-boundary, weighted Richardson-Lucy (fdr_richardson_lucy_free_f32*; include/fdr.h): the specification.

The plan is M x N, the data window d rows x cols at its top-left corner, the weights m rows x cols in [0, 1] (None = all ones).
H = DFT2 of the PSF placed top-left in the plan (op_spectrum of _rl_model.py); fullblur works on the whole plan:

    fullblur(x) = IDFT2(H . DFT2(x));  fullblur^T(y) = IDFT2(conj(H) . DFT2(y))
    W = pad(m);  dw = pad(m . max(d, 0))
    alpha = fullblur^T(W);  wgt = alpha > sigma ? 1 / alpha : 0;  u = alpha > sigma ? sum(dw) / sum(W) : 0
    n times:  c = window(fullblur(u));  r = c > TAU ? dw / c : 0 (0 outside the window);  u = max(u . wgt . fullblur^T(pad(r)), 0)

The output is the top-left out_rows x out_cols of u, normalised over that window as the RL calls normalise theirs.  Pinned against
direct summation, plain RL, the flux invariant, a delta PSF and injected faults in test_rlfree_host.py before it judges the GPU
(test_rlfree_gpu.py)."""
import numpy as np

from _rl_model import NORM_NONE, TAU, normalize, op_spectrum, smooth_image

SIGMA = float(np.float32(1e-2))  # FDR_RL_SIGMA

# Device against this model: max |got - model| / max |model| over the compared window (FDR_NORM_NONE) or max-abs (normalised
# outputs).  RLFREE_TOL is at most 4x the largest value one run of test_rlfree_gpu.py measured on an MI355X, and the test also holds
# every case within 10x of the float32 / complex64 CPU run of this model (dtype=np.float32 below).  Measured on the MI355X (largest
# over n, both output windows and the three norm_area; in brackets the float32 CPU run of the same case):
#   sigma 1e-2:  512^2 win 480^2 1.2e-5 (4.3e-6), 256^2 win 200x151 1.2e-5 (4.5e-6), 1024x512 win 1000x333 masked 2.8e-5 (1.6e-5),
#                64x128 win 37x101 masked 4.7e-6 (2.3e-6), 2048x512 win 2000x500 1.2e-5 (4.8e-6), 256^2 full plane 1.4e-6 (5.7e-7),
#                4096^2 win 4000x3900 n <= 3 2.9e-5 (7.0e-6), 8192^2 win 8000x8100 n = 1 2.5e-5 (5.9e-6)
#   sigma 1e-3:  the same cases 2.0e-4 (1.4e-4), 1.1e-4 (4.0e-5), 3.9e-4 (2.4e-4), 1.1e-4 (2.8e-5), 1.9e-4 (9.5e-5), 1.4e-6 (5.7e-7),
#                3.7e-4 (1.0e-4), 3.4e-4 (7.3e-5)
# The errors sit where the coverage is small: wgt = 1 / alpha turns the 5e-7 absolute error of a float32 alpha into 3e-4 relative
# at alpha = 1.7e-3, the smallest coverage above sigma = 1e-3 with the 15 px motion PSF; with a centred PSF that rim lies outside
# the data window, whose output then stays below 2.0e-5.  Case by case the device is within a factor of 7.4 of the float32 CPU run (64 x 128, sigma 1e-3).
RLFREE_TOL = 1e-3
SIGMA_MARGIN = 1e-4  # no model alpha may lie this close to sigma: a rounding flip of the threshold would void the comparison


def fullblur(x, H, adjoint=False, dtype=np.float64):
    """circular blur of the whole M x N plane x; dtype float32 runs it in single precision (complex64 spectra)"""
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    X = np.fft.rfft2(np.asarray(x, dtype=dtype)).astype(cdt)
    Hc = H.astype(cdt)
    return np.fft.irfft2(X * (np.conj(Hc) if adjoint else Hc), s=x.shape).astype(dtype)


def rlfree_state(d, psf, M, N, iterations, weights=None, sigma=SIGMA, dtype=np.float64, tau=TAU, fault=None):
    """the whole state after `iterations` steps: dict(u, alpha, wgt, dw, W), all M x N.  fault (for the CPU pins only): 'no_wgt'
    (the update without 1 / alpha), 'alpha_blur' (the coverage from fullblur instead of fullblur^T), 'mask_d_only' (the weights
    applied to d but not to W)"""
    d = np.asarray(d, dtype=dtype)
    rows, cols = d.shape
    m = np.ones((rows, cols), dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)
    H = op_spectrum(psf, M, N)
    W = np.zeros((M, N), dtype=dtype)
    W[:rows, :cols] = 1 if fault == "mask_d_only" else m
    dw = np.zeros((M, N), dtype=dtype)
    dw[:rows, :cols] = m * np.maximum(d, 0)
    alpha = fullblur(W, H, adjoint=fault != "alpha_blur", dtype=dtype)
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
        u = np.maximum(u * (1 if fault == "no_wgt" else wgt) * g, 0).astype(dtype)
    return dict(u=u, alpha=alpha, wgt=wgt, dw=dw, W=W)


def rlfree_model(d, psf, M, N, iterations, weights=None, sigma=SIGMA, out_shape=None, norm_area=NORM_NONE, dtype=np.float64, fault=None):
    """the output of fdr_richardson_lucy_free_f32: the top-left out_shape (default d.shape) of u, normalised by norm_area"""
    st = rlfree_state(d, psf, M, N, iterations, weights, sigma, dtype, fault=fault)
    orows, ocols = np.asarray(d).shape if out_shape is None else out_shape
    return normalize(st["u"][:orows, :ocols], norm_area, M, N)


def flux_defect(st):
    """|sum(alpha u) / sum(dw) - 1| in float64: 0 after every iteration wherever c > tau"""
    a = float(np.sum(st["alpha"].astype(np.float64) * st["u"].astype(np.float64)))
    b = float(np.sum(st["dw"], dtype=np.float64))
    return abs(a / b - 1.0)


def sigma_margin(alpha, sigma):
    """min |alpha - sigma| over the plan"""
    return float(np.min(np.abs(np.asarray(alpha, dtype=np.float64) - sigma)))


def crop_scene(S=1024, seed=5):
    """float64 S x S picture a crop is taken from: the smooth picture of _rl_model.py with sharp rectangles on it, in [0, 1]"""
    rng = np.random.default_rng(seed)
    img = 0.6 * smooth_image(S, S, seed).astype(np.float64)
    for _ in range(24):
        h, w = rng.integers(S // 40, S // 6, 2)
        y, x = rng.integers(0, S - h), rng.integers(0, S - w)
        img[y:y + h, x:x + w] += rng.uniform(-0.25, 0.4)
    img = np.clip(img, 0.02, None)
    return img / img.max()


QUALITY = dict(S=1024, at=(200, 200), rows=480, cols=480, M=512, N=512, noise=0.002, n=30, stuck=0.02, psf=(15, 30.0))


def quality_case(centred_psf_plane_of, seed=5):
    """truth window, blurred window (float32), the 2 % stuck-pixel variant and its weights.  centred_psf_plane_of(M, N) gives the
    15 / 30 line PSF rolled to put its centre at (0, 0) in an M x N plane: the scene is blurred circularly on S x S with it, the
    window restored on M x N with it."""
    q = QUALITY
    scene = crop_scene(q["S"], seed)
    Hs = np.fft.rfft2(centred_psf_plane_of(q["S"], q["S"]).astype(np.float64))
    blurred = np.fft.irfft2(np.fft.rfft2(scene) * Hs, s=scene.shape)
    y, x = q["at"]
    rng = np.random.default_rng(seed + 1)
    truth = scene[y:y + q["rows"], x:x + q["cols"]]
    d = (blurred[y:y + q["rows"], x:x + q["cols"]] + rng.normal(0, q["noise"], truth.shape)).astype(np.float32)
    stuck = rng.random(truth.shape) < q["stuck"]
    d_stuck = d.copy()
    d_stuck[stuck] = 1.0
    return truth, d, d_stuck, (~stuck).astype(np.float32)
