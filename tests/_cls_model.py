"""float64 model of the constrained least-squares (CLS) filter of fdr_set_psf_cls*: W = conj(H) / (|H|^2 + K + gamma L^2),
L(u, v) = 4 sin^2(pi u / M) + 4 sin^2(pi v / N), the symbol of the periodic 5-point Laplacian.  Pinned in test_cls_host.py
(against the DFT of the 3 x 3 Laplacian kernel, and cls_raw(gamma = 0) against wiener_raw) before it judges the GPU
(test_cls_gpu.py).  The GPU cases are listed here so that the CPU fault pins run on exactly the same inputs."""
import numpy as np

LAPLACIAN = np.array([[0, -1, 0], [-1, 4, -1], [0, -1, 0]], dtype=np.float64)


def lap2(M, N):
    """L(u, v)^2 on the full M x N plane, float64 (the sin^2 form: no cancellation at small u, v)"""
    a = 4.0 * np.sin(np.pi * np.arange(M) / M) ** 2
    b = 4.0 * np.sin(np.pi * np.arange(N) / N) ** 2
    return (a[:, None] + b[None, :]) ** 2


def cls_raw(img, psf, K, gamma, M, N):
    """The raw M x N plane before normalisation with the CLS filter, through the Hermitian half spectrum as wiener_raw does it."""
    img = np.asarray(img, dtype=np.float64)
    psf = np.asarray(psf, dtype=np.float64)
    f = np.zeros((M, N))
    f[:img.shape[0], :img.shape[1]] = img
    h = np.zeros((M, N))
    h[:psf.shape[0], :psf.shape[1]] = psf
    G = np.fft.rfft2(f)
    H = np.fft.rfft2(h)
    den = np.abs(H) ** 2 + K + gamma * lap2(M, N)[:, :N // 2 + 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        W = np.where(den != 0, np.conj(H) / den, 0)
    return np.fft.irfft2(G * W, s=(M, N))


# ---- the GPU cases (test_cls_gpu.py) ----------------------------------------------------------------------------------------
GAMMAS = (0.005, 0.05, 1.0)
KS = (1e-4, 1e-2)

# (M, N, flags name or None): half spectrum 8^2 .. 8192^2 and two long shapes, full spectrum, N = 16 (full spectrum below 32
# columns), simple plans (the flag, M < 8, M > 8192), mixed radix
SHAPES = ([(1 << k, 1 << k, None) for k in range(3, 14)] + [(256, 2048, None), (2048, 256, None)] +
          [(256, 256, "FLAG_FULL_SPECTRUM"), (64, 1024, "FLAG_FULL_SPECTRUM"), (512, 16, None)] +
          [(512, 512, "FLAG_SIMPLE_PATH"), (4, 4096, None), (16384, 64, None)] +
          [(1080, 1920, "FLAG_MIXED_RADIX"), (4320, 4320, "FLAG_MIXED_RADIX"), (3000, 5000, "FLAG_MIXED_RADIX")])
BIG = 1 << 20    # plans above this many pixels: one gamma per (PSF, K), the three in turn (the float64 model costs seconds a case)
HUGE = 1 << 24   # above this: one case per PSF plus K = 0 with the motion PSF


def motion_psf(oracle, size, angle, M, N):
    """oracle.motion_blur_kernel cut to the plan (its central window, renormalised) when it is larger"""
    psf = oracle.motion_blur_kernel(size, angle)
    r, c = psf.shape
    if r <= M and c <= N:
        return psf
    r0, c0 = (r - min(r, M)) // 2, (c - min(c, N)) // 2
    h = psf[r0:r0 + min(r, M), c0:c0 + min(c, N)].astype(np.float64)
    return (h / h.sum()).astype(np.float32)


def psfs(oracle, M, N):
    """(name, PSF): two motion PSFs, a dense zero-mean PSF (uniform noise / sqrt(M N), shifted to mean 0) and a delta"""
    dense = np.random.default_rng(M * 31 + N).random((M, N)) / np.sqrt(M * N)
    delta = np.zeros((M // 2 + 1, N // 2 + 1), dtype=np.float32)
    delta[M // 2, N // 2] = 1.0
    return [("motion 15/30", motion_psf(oracle, 15, 30.0, M, N)), ("motion 50/123.4", motion_psf(oracle, 50, 123.4, M, N)),
            ("dense zero-mean", (dense - dense.mean()).astype(np.float32)), ("delta", delta)]


def cases(oracle, M, N):
    """(psf name, PSF, K, gamma) of one plan: every PSF x K x gamma, plus K = 0 (textbook CLS) with the motion and delta PSFs;
    above BIG pixels one gamma per (PSF, K), the three in turn; above HUGE one (K, gamma) per PSF, in turn."""
    ps = psfs(oracle, M, N)
    pairs = [(n, p, K) for n, p in ps for K in KS] + [(n, p, 0.0) for n, p in ps if n in ("motion 15/30", "delta")]
    if M * N > HUGE:
        return [(n, p, KS[i % len(KS)], GAMMAS[i % len(GAMMAS)]) for i, (n, p) in enumerate(ps)] + [
            (ps[0][0], ps[0][1], 0.0, GAMMAS[1])]
    if M * N > BIG:
        return [(n, p, K, GAMMAS[i % len(GAMMAS)]) for i, (n, p, K) in enumerate(pairs)]
    return [(n, p, K, g) for n, p, K in pairs for g in GAMMAS]
