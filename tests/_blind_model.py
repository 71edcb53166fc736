"""float64 model of blind Richardson-Lucy, both forms (fdr_richardson_lucy_blind_f32*; include/fdr.h): the specification.

The plan is M x N, the window rows x cols at its top-left corner, p_k the prows x pcols PSF top-left in the plan, H_k = DFT2(pad(p_k)),
corr_u(y) = IDFT2(conj(DFT2(u)) . DFT2(y)) cropped to the top-left prows x pcols.

    plain form:  u_0 = d+;  every k:  c = blur_k(u_k);  r = c > TAU ? d+ / c : 0;  u_(k+1) = max(u_k . blur_k^T(r), 0)
                 k >= psf_hold:  q = max(p_k . corr_(u_k)(pad(r)), 0);  s = sum(q);  p_(k+1) = s > 0 and finite ? q / s : p_k
    free form:   W, dw, alpha_k = fullblur_k^T(W), wgt_k from p_k (recomputed with every new PSF), u_0 the free form's start under p_0,
                 the step of _rlfree_model.py with p_k, and q = den > 0 ? max(p_k . num / den, 0) : 0 with
                 num = corr_(u_k)(pad(r)), den = corr_(u_k)(W)

dtype=np.float32 replays the same formulas in single precision with torch.fft (complex64 spectra): the arithmetic class of the
device and the yardstick of the GPU tolerance.  Also here: the scene, the curved shake PSF, the Gaussian start and the
shift-tolerant correlation of the quality tests.  Pinned in test_blind_host.py before it judges the GPU (test_blind_gpu.py)."""
import numpy as np

from _rl_model import NORM_NONE, TAU, normalize
from _rlfree_model import SIGMA

FAULTS = ("no_conj", "psf_from_next", "no_renorm", "no_den", "alpha_fixed")


def _rfft2(x, dtype):
    if dtype == np.float32:
        import torch
        return torch.fft.rfft2(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()
    return np.fft.rfft2(np.asarray(x, dtype=np.float64))


def _irfft2(X, shape, dtype):
    if dtype == np.float32:
        import torch
        return torch.fft.irfft2(torch.from_numpy(np.ascontiguousarray(X, dtype=np.complex64)), s=shape).numpy()
    return np.fft.irfft2(X, s=shape)


def _pad(x, M, N, dtype):
    plane = np.zeros((M, N), dtype=dtype)
    plane[:x.shape[0], :x.shape[1]] = x
    return plane


def blind_state(d, p0, M, N, iterations, free_boundary=False, weights=None, psf_hold=0, sigma=SIGMA, dtype=np.float64, tau=TAU, fault=None,
                info=None):
    """(u, p) after `iterations` steps: u on the window (plain form) or on the whole plan (free form), p the PSF.  fault (for the
    CPU pins only): one of FAULTS -- U in place of conj(U); the PSF step from u_(k+1); q not divided by its sum; the free form's
    den dropped; the coverage kept from p_0."""
    assert fault is None or fault in FAULTS
    d = np.asarray(d, dtype=dtype)
    rows, cols = d.shape
    p = np.asarray(p0, dtype=dtype).copy()
    prows, pcols = p.shape
    dp = np.maximum(d, 0)
    win = np.zeros((M, N), dtype=bool)
    win[:rows, :cols] = True

    def coverage(H):
        alpha = _irfft2(Wspec * np.conj(H), (M, N), dtype).astype(dtype)
        if info is not None:
            info["margin"] = min(info.get("margin", np.inf), float(np.min(np.abs(alpha.astype(np.float64) - sigma))))
        seen = alpha > sigma
        return seen, np.where(seen, 1 / np.where(seen, alpha, 1), 0).astype(dtype)

    H = _rfft2(_pad(p, M, N, dtype), dtype)
    if free_boundary:
        m = np.ones((rows, cols), dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)
        W = _pad(m, M, N, dtype)
        dw = _pad((m * dp).astype(dtype), M, N, dtype)
        Wspec = _rfft2(W, dtype)
        seen, wgt = coverage(H)
        sw = float(np.sum(W, dtype=np.float64))
        mean = float(np.sum(dw, dtype=np.float64)) / sw if sw > 0 else 0.0
        u = np.where(seen, mean, 0).astype(dtype)
    else:
        dw = _pad(dp, M, N, dtype)
        u = _pad(dp, M, N, dtype)  # the estimate is 0 outside the window: every update is cropped
    for k in range(iterations):
        U = _rfft2(u, dtype)
        c = _irfft2(U * H, (M, N), dtype).astype(dtype)
        ok = win & (c > tau)
        r = np.where(ok, dw / np.where(ok, c, 1), 0).astype(dtype)
        R = _rfft2(r, dtype)
        g = _irfft2(R * np.conj(H), (M, N), dtype).astype(dtype)
        if free_boundary:
            u_next = np.maximum(u * wgt * g, 0).astype(dtype)
        else:
            u_next = np.where(win, np.maximum(u * g, 0), 0).astype(dtype)
        if k >= psf_hold:
            Uk = _rfft2(u_next, dtype) if fault == "psf_from_next" else U
            Uc = Uk if fault == "no_conj" else np.conj(Uk)
            num = _irfft2(R * Uc, (M, N), dtype)[:prows, :pcols].astype(dtype)
            if free_boundary and fault != "no_den":
                den = _irfft2(Wspec * Uc, (M, N), dtype)[:prows, :pcols].astype(dtype)
                pos = den > 0
                q = np.where(pos, np.maximum(p * num / np.where(pos, den, 1), 0), 0).astype(dtype)
            else:
                q = np.maximum(p * num, 0).astype(dtype)
            s = float(np.sum(q, dtype=np.float64))
            if s > 0 and np.isfinite(s):
                p = q.copy() if fault == "no_renorm" else (q.astype(np.float64) / s).astype(dtype)
                H = _rfft2(_pad(p, M, N, dtype), dtype)
                if free_boundary and fault != "alpha_fixed":
                    seen, wgt = coverage(H)
        u = u_next
    return (u if free_boundary else u[:rows, :cols]), p


def blind_model(d, p0, M, N, iterations, free_boundary=False, weights=None, psf_hold=0, sigma=SIGMA, out_shape=None, norm_area=NORM_NONE,
                dtype=np.float64, fault=None, info=None):
    """(image, psf) as fdr_richardson_lucy_blind_f32 returns them: the top-left out_shape (default d.shape) of u_n, normalised by
    norm_area, and p_n"""
    u, p = blind_state(d, p0, M, N, iterations, free_boundary, weights, psf_hold, sigma, dtype, fault=fault, info=info)
    orows, ocols = np.asarray(d).shape if out_shape is None or not free_boundary else out_shape
    return normalize(u[:orows, :ocols], norm_area, M, N), p


def psf_gaussian(size, sigma=0.0):
    """fdr_psf_gaussian: exp(-((i - c)^2 + (j - c)^2) / (2 sigma^2)), c = size // 2, in double over its double sum, rounded once"""
    sigma = size / 4.0 if sigma == 0 else float(sigma)
    i = np.arange(size, dtype=np.float64) - size // 2
    g = np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def shake_psf(size):
    """a curved camera-shake PSF, size x size (9 and 7 are used): a half-sine-bent path from the top rows to the bottom ones (it
    stays 0.14 (size - 1) clear of both), drawn as a stroke of Gaussian width 0.38 px with an exposure that grows threefold along
    the path, sum 1"""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    p = np.zeros((size, size))
    c = (size - 1) / 2.0
    for t in np.linspace(0.0, 1.0, 200):
        y = (0.14 + 0.72 * t) * (size - 1)
        x = c + 0.2 * (size - 1) * np.sin(np.pi * t)
        p += (0.25 + 1.5 * t) * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * 0.38 * 0.38))
    return (p / p.sum()).astype(np.float32)


def scene(S, seed):
    """float64 S x S scene: background 0.1, 12 discs of radius 3 .. 11 and height 0.2 .. 1, 30 point sources of 2 .. 6"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    img = np.full((S, S), 0.1)
    for _ in range(12):
        cy, cx, rad, h = rng.uniform(0, S), rng.uniform(0, S), rng.uniform(3, 11), rng.uniform(0.2, 1.0)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] += h
    for _ in range(30):
        img[rng.integers(0, S), rng.integers(0, S)] += rng.uniform(2, 6)
    return img


def blur_periodic(img, psf):
    """circular blur of the whole square `img` with psf top-left in it: what the plan's operator does on a full-plane window"""
    S = img.shape[0]
    return np.fft.irfft2(np.fft.rfft2(img) * np.fft.rfft2(_pad(np.asarray(psf, dtype=np.float64), S, S, np.float64)), s=img.shape)


def shift_corr(p, q, reach=3):
    """the shift-tolerant correlation: the maximum over circular shifts of up to `reach` in each direction of the centred normalised
    correlation of two equally sized planes (blind deconvolution fixes the PSF only up to a shift inside its support)"""
    a = np.asarray(p, dtype=np.float64) - np.mean(p, dtype=np.float64)
    b = np.asarray(q, dtype=np.float64) - np.mean(q, dtype=np.float64)
    na, nb = np.sqrt(np.sum(a * a)), np.sqrt(np.sum(b * b))
    if na == 0 or nb == 0:
        return 0.0
    return max(float(np.sum(np.roll(a, (dy, dx), axis=(0, 1)) * b)) / (na * nb) for dy in range(-reach, reach + 1)
               for dx in range(-reach, reach + 1))


def shift_psnr(x, ref, reach=3, margin=0):
    """the best PSNR in dB (peak = max(ref) - min(ref)) of x against ref over circular shifts of up to `reach`; `margin` pixels at
    every side are left out (a crop's rim, where a shift wraps)"""
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    peak = float(ref.max() - ref.min())
    sl = (slice(margin, x.shape[0] - margin), slice(margin, x.shape[1] - margin))
    best = min(float(np.mean((np.roll(x, (dy, dx), axis=(0, 1))[sl] - ref[sl]) ** 2)) for dy in range(-reach, reach + 1)
               for dx in range(-reach, reach + 1))
    return 10.0 * np.log10(peak * peak / best)


QUALITY = dict(S=128, noise=0.005, n=80, psf=9, crop=dict(S=256, at=(70, 90), rows=100, cols=100, M=128, N=128))


def plain_case(seed):
    """(truth, blurred float32 data, true PSF): the 128^2 scene blurred periodically by the 9 x 9 shake PSF, Gaussian noise 0.005"""
    q = QUALITY
    truth = scene(q["S"], seed)
    psf = shake_psf(q["psf"])
    d = blur_periodic(truth, psf) + np.random.default_rng(seed + 1000).normal(0, q["noise"], truth.shape)
    return truth, d.astype(np.float32), psf


def crop_case(seed):
    """(truth window, data window float32, true PSF): a 100^2 crop of the 256^2 scene blurred periodically, for a 128^2 plan"""
    q = QUALITY
    c = q["crop"]
    big = scene(c["S"], seed)
    psf = shake_psf(q["psf"])
    blurred = blur_periodic(big, psf) + np.random.default_rng(seed + 1000).normal(0, q["noise"], big.shape)
    y, x = c["at"]
    return big[y:y + c["rows"], x:x + c["cols"]], blurred[y:y + c["rows"], x:x + c["cols"]].astype(np.float32), psf


# ---- the inputs and the tolerance of the device tests (test_blind_gpu.py), pinned against the fault models in test_blind_host.py ----
GPU_FLOOR = 1e-5   # 3 times the 3.3e-6 DESIGN.md section 12 records for 30 RL iterations
GPU_FACTOR = 10.0  # the device may be this many times the float32 replay's error (its transforms are FMA / table based, not numpy's)
COLUMN_M = (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192)  # every column length the new column kernel is instantiated for, N = 32
COLUMN_PSFS = ((3, 3), (5, 12))
COLUMN_N_ITER = 3
ROW_N = (32, 256, 4096, 8192)  # M = 16, a 3 x 3 PSF
PSF_WINDOWS = ((1, 1), (9, 9), (31, 31))  # the PSF window of pass C, on 32 x 32 and 32 x 8192 plans (a 31-row PSF needs 32 rows)
FREE_CASES = ((64, 128, 50, 100), (256, 256, 200, 180))  # M, N, rows, cols; a 9 x 9 PSF
FREE_N_ITER = (5, 20)


def gpu_tol(err32):
    """the bound of the device's error (max-abs over max |model|) from the float32 replay's on the same input"""
    return max(GPU_FACTOR * err32, GPU_FLOOR)


def gpu_image(rows, cols, seed):
    """float32 rows x cols positive test picture: a pedestal with mild texture, a few bright points, a dark corner with negative pixels"""
    rng = np.random.default_rng(seed)
    img = 0.2 + 0.3 * rng.random((rows, cols))
    k = max(4, rows * cols // 48)
    img[rng.integers(0, rows, k), rng.integers(0, cols, k)] += rng.uniform(1, 4, k)
    img[: max(1, rows // 16), : max(1, cols // 16)] -= 0.4
    return img.astype(np.float32)


def start_psf(prows, pcols, seed):
    """a dense random positive prows x pcols PSF with a soft peak, sum 1"""
    rng = np.random.default_rng(seed)
    i = (np.arange(prows) - prows // 2)[:, None] / max(prows, 2)
    j = (np.arange(pcols) - pcols // 2)[None, :] / max(pcols, 2)
    p = (0.3 + rng.random((prows, pcols))) * np.exp(-4.0 * (i * i + j * j))
    return (p / p.sum()).astype(np.float32)


def gpu_mask(rows, cols, seed):
    """weights with 2 % zeros"""
    return (np.random.default_rng(seed).random((rows, cols)) >= 0.02).astype(np.float32)
