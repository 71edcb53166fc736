"""float64 numpy model of the optimal-size operator (fft_serial::wienerDeblur_myfft padded to M x N): the yardstick of the
mixed-radix fast path at sizes where the naive-DFT oracle is too slow.  Pinned against oracle.wiener in
test_mixed_radix_host.py before it judges the GPU."""
import numpy as np


def wiener_raw(img, psf, K, M, N):
    """The raw M x N plane before normalisation: pad image and PSF top-left to M x N, W = conj(H) / (|H|^2 + K), real part
    of the inverse transform (taken as the inverse of the Hermitian half spectrum)."""
    img = np.asarray(img, dtype=np.float64)
    psf = np.asarray(psf, dtype=np.float64)
    f = np.zeros((M, N))
    f[:img.shape[0], :img.shape[1]] = img
    h = np.zeros((M, N))
    h[:psf.shape[0], :psf.shape[1]] = psf
    G = np.fft.rfft2(f)
    H = np.fft.rfft2(h)
    W = np.conj(H) / (np.abs(H) ** 2 + K)
    return np.fft.irfft2(G * W, s=(M, N))


def wiener_model(img, psf, K, M, N, norm_cropped=True):
    """wiener_raw, crop, min-max normalise over the cropped rows x cols (norm_cropped) or over the padded M x N area."""
    rows, cols = np.shape(img)
    raw = wiener_raw(img, psf, K, M, N)
    area = raw[:rows, :cols] if norm_cropped else raw
    lo, hi = area.min(), area.max()
    out = raw[:rows, :cols]
    return (out - lo) / (hi - lo) if hi > lo else np.zeros_like(out)


def smooth(n):
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


def optimal_size(n):
    m = max(n, 1)
    while not smooth(m):
        m += 1
    return m
