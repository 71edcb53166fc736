"""float64 model of the motion-blur estimate (fdr_cepstrum_f32*, fdr_estimate_motion_f32*; include/fdr.h).  numpy only.

The plan is M x N, the image window rows x cols (row stride `stride`) at its top-left corner:

    x = w . img on the window, 0 elsewhere;  w[i, j] = hann(rows)[i] hann(cols)[j]  (numpy.hanning)
    G = DFT2(x) on M x N;  eps = 1e-6 sum |x|
    c = Re IDFT2(log(|G| + eps))                               (the power cepstrum; IDFT2 includes 1 / (M N))
    S[a, l] = c bilinearly at row -l sin(theta_a), column +l cos(theta_a), periodic; theta_a = a step
    (a*, l*) = argmin S (ties: lowest flat index, angle-major); confidence = (median S - min S) / (1.4826 MAD S)

A uniform linear blur of length L puts sinc zeros into |G| in stripes across the motion direction; in c they show as a negative peak
at distance L along it.  The row axis points down, so theta is the angle convention of motionBlurKernel / fdr_psf_motion.

Also here: the synthetic scenes and the linear blur the recovery tests use, and the endpoint error they are judged by.  Pinned in
test_motion_host.py before it judges the GPU (test_motion_gpu.py)."""
import math
from collections import namedtuple

import numpy as np

DEFAULT_STEP = 0.5
DEFAULT_MIN_LENGTH = 3
DEFAULT_MAX_LENGTH_CAP = 100
EPS_REL = 1e-6
MAD_SCALE = 1.4826

Estimate = namedtuple("Estimate", "length angle score confidence n_angles n_lengths")

# Thresholds of the device results against this model, from one run of test_motion_gpu.py on an MI355X, each at most 4x the
# largest value measured there.  CEP_TOL bounds max |got - model| of the cepstrum per bin over every plan of the per-bin tests
# (measured 8.2e-7 at 4096^2, on the Nyquist row; c[0, 0] is about 5 to 12 there); TABLE_TOL max |got - model| of a score table
# (measured 2.6e-7, the cat on 1024 x 2048).
CEP_TOL = 3.2e-6
TABLE_TOL = 1.0e-6
# the recovery bounds the feature promises
ENDPOINT_TOL = 1.5
CONF_BLURRED_MIN = 12.0
CONF_SHARP_MAX = 8.0

# the synthetic grid: (length, angle) pairs, each at 512^2 and 600 x 900
SYNTH_PAIRS = [(9, 0.0), (15, 10.0), (21, 77.5), (30, 123.4), (40, 45.0), (64, 160.0), (12, 171.0), (80, 100.0)]
SYNTH_SIZES = [(512, 512), (600, 900)]
# the two golden pictures and the blur their README states
GOLDEN = [("car_blurred.png", 40, 45.0), ("cat_blurred.png", 50, 30.0)]


def defaults(rows, cols, min_length=0, max_length=0, angle_step=0.0):
    """the arguments with 0 replaced by their defaults; (min_length, max_length, step, n_angles, n_lengths)"""
    lo = int(min_length) or DEFAULT_MIN_LENGTH
    hi = int(max_length) or min(DEFAULT_MAX_LENGTH_CAP, min(int(rows), int(cols)) // 4)
    step = float(angle_step) or DEFAULT_STEP
    return lo, hi, step, int(math.ceil(180.0 / step)), hi - lo + 1


def hann(n):
    """0.5 - 0.5 cos(2 pi k / (n - 1)), k < n: numpy.hanning(n)"""
    return np.hanning(n)


def window_plane(img, M, N, dtype=np.float64):
    rows, cols = img.shape
    x = np.zeros((M, N), dtype=dtype)
    x[:rows, :cols] = np.outer(hann(rows), hann(cols)).astype(dtype) * img.astype(dtype)
    return x


def cepstrum_model(img, M, N):
    """c (M x N float64) of the window `img` in an M x N plan; all zeros for an all-zero window"""
    x = window_plane(img, M, N)
    total = float(np.abs(x).sum())
    if total == 0.0:
        return np.zeros((M, N))
    G = np.fft.fft2(x)
    return np.real(np.fft.ifft2(np.log(np.abs(G) + EPS_REL * total)))


def trig_table(n_angles, step):
    """(cos, sin) of theta_a = a step, evaluated in double (the table the device gets)"""
    th = np.deg2rad(np.arange(n_angles, dtype=np.float64) * step)
    return np.cos(th), np.sin(th)


def score_table(c, min_length, max_length, step):
    """S[a, l - min_length] (n_angles x n_lengths): c bilinearly at row -l sin(theta_a), column l cos(theta_a), periodic"""
    M, N = c.shape
    n_angles = int(math.ceil(180.0 / step))
    cs, sn = trig_table(n_angles, step)
    ls = np.arange(min_length, max_length + 1, dtype=np.float64)
    y = -ls[None, :] * sn[:, None]
    x = ls[None, :] * cs[:, None]
    i0, j0 = np.floor(y), np.floor(x)
    fy, fx = y - i0, x - j0
    i0 = i0.astype(np.int64) % M
    j0 = j0.astype(np.int64) % N
    i1, j1 = (i0 + 1) % M, (j0 + 1) % N
    return ((1 - fy) * ((1 - fx) * c[i0, j0] + fx * c[i0, j1]) + fy * ((1 - fx) * c[i1, j0] + fx * c[i1, j1]))


def pick(S, min_length, step):
    """(length, angle, score, confidence) of a score table, in double (S may be float32)"""
    S = np.asarray(S, dtype=np.float64)
    k = int(np.argmin(S))  # the first of exact ties, flat index angle-major
    a, l = divmod(k, S.shape[1])
    smin = float(S.flat[k])
    med = float(np.median(S))
    mad = float(np.median(np.abs(S - med)))
    conf = (med - smin) / (MAD_SCALE * mad) if mad > 0 else 0.0
    return min_length + l, a * step, smin, conf


def estimate(img, M, N, min_length=0, max_length=0, angle_step=0.0, table=False):
    rows, cols = img.shape
    lo, hi, step, na, nl = defaults(rows, cols, min_length, max_length, angle_step)
    c = cepstrum_model(img, M, N)
    if not np.any(c):
        est = Estimate(0, 0.0, 0.0, 0.0, na, nl)
        return (est, np.zeros((na, nl))) if table else est
    S = score_table(c, lo, hi, step)
    est = Estimate(*pick(S, lo, step), na, nl)
    return (est, S) if table else est


def endpoint_err(L, a, L_hat, a_hat):
    """min || L e(a) -+ L_hat e(a_hat) ||, e(a) = (cos a, sin a), angles in degrees: a blur and its reverse are the same blur"""
    e = np.array([math.cos(math.radians(a)), math.sin(math.radians(a))]) * L
    f = np.array([math.cos(math.radians(a_hat)), math.sin(math.radians(a_hat))]) * L_hat
    return float(min(np.linalg.norm(e - f), np.linalg.norm(e + f)))


def scene(M, N, seed):
    """a seeded M x N test scene in [0, 255]: a gradient, 60 filled ellipses and texture noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:M, 0:N].astype(np.float64)
    img = 40.0 + 120.0 * (xx / N) * rng.uniform(0.3, 1.0) + 60.0 * (yy / M) * rng.uniform(0.3, 1.0)
    for _ in range(60):
        cy, cx = rng.uniform(0, M), rng.uniform(0, N)
        ry, rx = rng.uniform(4, M / 8), rng.uniform(4, N / 8)
        t = rng.uniform(0, np.pi)
        dy, dx = yy - cy, xx - cx
        u = (dx * np.cos(t) + dy * np.sin(t)) / rx
        v = (-dx * np.sin(t) + dy * np.cos(t)) / ry
        img[u * u + v * v <= 1.0] = rng.uniform(0, 255)
    img += rng.normal(0.0, 10.0, (M, N))
    return np.clip(img, 0.0, 255.0)


def linear_blur(img, psf):
    """linear convolution of img with psf (zero-padded FFT convolution), cropped 'same' (centred)"""
    rows, cols = img.shape
    kr, kc = psf.shape
    fr, fc = rows + kr - 1, cols + kc - 1
    full = np.fft.irfft2(np.fft.rfft2(img, (fr, fc)) * np.fft.rfft2(np.asarray(psf, dtype=np.float64), (fr, fc)), (fr, fc))
    r0, c0 = (kr - 1) // 2, (kc - 1) // 2
    return full[r0:r0 + rows, c0:c0 + cols]


def blurred_scene(rows, cols, L, a, psf, seed, noise=1.0):
    """scene blurred by psf (motionBlurKernel(L, a)), noise sigma `noise`, rounded to integers in [0, 255]"""
    rng = np.random.default_rng(seed + 1)
    b = linear_blur(scene(rows, cols, seed), psf) + rng.normal(0.0, noise, (rows, cols))
    return np.clip(np.round(b), 0.0, 255.0)


def load_golden(path):
    """the channel mean of a golden picture, float64 in [0, 255]"""
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float64).mean(axis=2)


def optimal_dft_size(n):
    """smallest 2^a 3^b 5^c >= n (fdr_optimal_dft_size)"""
    m = max(int(n), 1)
    while True:
        k = m
        for f in (2, 3, 5):
            while k % f == 0:
                k //= f
        if k == 1:
            return m
        m += 1


def plan_sizes(rows, cols):
    """the power-of-two and the smallest 2^a 3^b 5^c plan of a rows x cols picture, at least 32 each"""
    p2 = lambda n: 1 << max(5, (int(n) - 1).bit_length())
    return [(p2(rows), p2(cols)), (max(32, optimal_dft_size(rows)), max(32, optimal_dft_size(cols)))]
