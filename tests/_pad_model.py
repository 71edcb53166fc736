"""float64 model of the smooth padding of the Wiener / CLS calls (FDR_OPT_PAD_MODE = FDR_PAD_SMOOTH, include/fdr.h; DESIGN.md
section 16), and the cropped-scene experiment that measures what it is for.

The window is d (rows x cols), the plan is M x N, e is the extended plane:

    ramp(n)[j] = 0.5 - 0.5 cos(pi (j + 1) / (n + 1)),  j = 0 .. n-1      (0 < ramp < 1, ramp[j] + ramp[n-1-j] = 1)
    r < rows, c >= cols :  t = ramp(N - cols)[c - cols];  e[r, c] = (1 - t) d[r, cols-1] + t d[r, 0]
    r >= rows, all c    :  t = ramp(M - rows)[r - rows];  e[r, c] = (1 - t) e[rows-1, c] + t e[0, c]
    result = window( IDFT2( W . DFT2(e) ) ),  normalised as with zero padding

Pinned in test_pad_host.py (properties, two injected faults, the quality table) before it judges the GPU (test_pad_gpu.py).

DEVICE_TOL: the project's fast-mode bound on max |device - model| of the normalised output (MEASURED_MAX: the largest value one
MI355X run of test_pad_gpu.py::test_device_against_model gave)."""
import numpy as np

from _cls_model import cls_raw
from _mixed_model import wiener_raw
from _rl_model import smooth_image

PAD_ZERO, PAD_SMOOTH = 0, 1
DEVICE_TOL = 1e-4   # the fast-mode bound of the project (include/fdr.h, FDR_MODE_FAST); not derived from the measurement below
# Largest max-abs measured on an MI355X over the 76 runs of test_device_against_model (19 shapes x Wiener / CLS x cropped / padded):
# 1.27e-6 (1023 x 1023 in 1024^2, Wiener, NORM_PADDED); the smallest distance of the zero-padded model in those runs is 6.8e-2.
MEASURED_MAX = 1.27e-6


def ramp(n):
    """the n blending weights of a padding of n elements: rises from just above 0 (next to the picture's last column / row) to
    just below 1 (next to the wrap neighbour, column / row 0)"""
    j = np.arange(n, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(np.pi * (j + 1) / (n + 1))


def extend(d, M, N, fault=None):
    """the M x N extended plane e of the window d.  fault (test_pad_host.py only): "reversed_ramp" uses the weights back to front,
    "rows_from_zero_padded" blends the pad rows from the zero-padded plane instead of the column-extended one."""
    d = np.asarray(d, dtype=np.float64)
    rows, cols = d.shape
    assert 1 <= rows <= M and 1 <= cols <= N
    e = np.zeros((M, N))
    e[:rows, :cols] = d
    if cols < N:
        t = ramp(N - cols)
        if fault == "reversed_ramp":
            t = t[::-1]
        e[:rows, cols:] = (1 - t)[None, :] * d[:, cols - 1:cols] + t[None, :] * d[:, 0:1]
    if rows < M:
        t = ramp(M - rows)
        if fault == "reversed_ramp":
            t = t[::-1]
        src = e
        if fault == "rows_from_zero_padded":
            src = np.zeros((M, N))
            src[:rows, :cols] = d
        e[rows:, :] = (1 - t)[:, None] * src[rows - 1:rows, :] + t[:, None] * src[0:1, :]
    return e


def pad_plane(d, M, N, pad):
    """the M x N plane the transform sees: zeros outside the window, or the smooth extension"""
    if pad == PAD_SMOOTH:
        return extend(d, M, N)
    e = np.zeros((M, N))
    e[:np.shape(d)[0], :np.shape(d)[1]] = d
    return e


def restore_raw(d, psf, K, M, N, pad, gamma=0.0):
    """the raw M x N plane IDFT2(W . DFT2(e)) before normalisation; psf lies top-left in the plan as for every fdr_wiener_* call
    (an M x N psf is the whole plane: a caller rolls a centred PSF there).  gamma > 0: the CLS filter."""
    e = pad_plane(d, M, N, pad)
    return cls_raw(e, psf, K, gamma, M, N) if gamma > 0 else wiener_raw(e, psf, K, M, N)


def normalized(raw, rows, cols, padded):
    """the rows x cols output: min-max over the whole plan (FDR_NORM_PADDED) or over the window (FDR_NORM_CROPPED)"""
    w = raw[:rows, :cols]
    area = raw if padded else w
    lo, hi = area.min(), area.max()
    return (w - lo) / (hi - lo)


# ---- the cropped-scene experiment -------------------------------------------------------------------------------------------------
SCENE = 1024
QUALITY_SHAPES = [(400, 440, 512, 512), (500, 500, 512, 512), (480, 640, 512, 1024), (512, 512, 1024, 1024)]  # rows, cols, M, N
QUALITY_SEEDS = (3, 4, 5)
QUALITY_K = 0.01
NOISE_SIGMA = 0.002
CROP_AT = (256, 256)  # top-left corner of every window in the scene
MIN_GAIN_DB = 10.0    # smooth over zero padding, in the model and on the device
# What the float64 model gives on these twelve cases (test_pad_host.py prints each): smooth over zero padding 13.5 .. 16.6 dB, smooth over
# the blurred input 0.69 .. 3.95 dB (the smallest three with the 12 px margin of 500 x 500 in 512^2, which is less than the PSF's box).


def scene(seed, size=SCENE):
    """float64 size x size scene in [0, 1]: smooth_image (blobs and a bar on a pedestal) plus 1/f^1.5 texture of standard deviation 0.05
    plus a bright rectangle, clamped at 0 and divided by its maximum (the pedestal stays: a photograph is not dark at its borders)"""
    rng = np.random.default_rng(seed)
    s = smooth_image(size, size, seed).astype(np.float64)
    fy, fx = np.fft.fftfreq(size)[:, None], np.fft.rfftfreq(size)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0
    spec = (rng.standard_normal(f.shape) + 1j * rng.standard_normal(f.shape)) / f ** 1.5
    spec[0, 0] = 0.0
    tex = np.fft.irfft2(spec, s=(size, size))
    s = s + 0.05 * tex / tex.std()
    s[int(0.42 * size):int(0.50 * size), int(0.30 * size):int(0.45 * size)] += 0.4
    s = np.maximum(s, 0)
    return s / s.max()


def centred_psf_plane(psf, M, N):
    """psf (odd sides) in an M x N plane, rolled to put its centre at (0, 0): restoring with it leaves the picture in place"""
    psf = np.asarray(psf, dtype=np.float64)
    h = np.zeros((M, N))
    h[:psf.shape[0], :psf.shape[1]] = psf
    return np.roll(h, (-(psf.shape[0] // 2), -(psf.shape[1] // 2)), axis=(0, 1))


def quality_case(psf, seed, rows, cols):
    """(truth, blurred): the rows x cols crop of the scene, and the same crop of the scene blurred periodically by the centred psf
    with noise of NOISE_SIGMA added; float32, what a caller would hand to the library"""
    s = scene(seed)
    H = np.fft.rfft2(centred_psf_plane(psf, SCENE, SCENE))
    b = np.fft.irfft2(np.fft.rfft2(s) * H, s=(SCENE, SCENE))
    b = b + NOISE_SIGMA * np.random.default_rng(seed + 1000).standard_normal(b.shape)
    r0, c0 = CROP_AT
    return s[r0:r0 + rows, c0:c0 + cols].astype(np.float32), b[r0:r0 + rows, c0:c0 + cols].astype(np.float32)


def psnr(x, truth):
    """PSNR in dB over the whole window against the truth (peak 1)"""
    x = np.asarray(x, dtype=np.float64)
    return float(-10.0 * np.log10(np.mean((x - np.asarray(truth, dtype=np.float64)) ** 2)))


def quality_psf(length=15, angle=30.0, box=21):
    """the experiment's PSF: a `length` px line at `angle` degrees centred in a box x box plane, normalised to sum 1 (made on the
    CPU, as test_tv_host.py makes its line PSF)"""
    k = np.zeros((box, box))
    c, h = box // 2, (length - 1) / 2.0
    for t in np.linspace(-h, h, 8 * length):
        k[int(round(c - t * np.sin(np.deg2rad(angle)))), int(round(c + t * np.cos(np.deg2rad(angle))))] = 1
    return (k / k.sum()).astype(np.float32)


def quality_failures(what, p_blurred, p_zero, p_smooth, min_gain=MIN_GAIN_DB, min_over_blurred=0.0):
    """the conditions of the quality table on one case's three PSNRs (an empty list: it passed).  `not a >= b`: NaN fails."""
    bad = []
    if not p_smooth - p_zero >= min_gain:
        bad.append("%s: smooth %.2f dB is not %.1f dB above zero padding %.2f dB" % (what, p_smooth, min_gain, p_zero))
    if not p_smooth - p_blurred > min_over_blurred:
        bad.append("%s: smooth %.2f dB does not beat the blurred input %.2f dB by more than %.1f dB" % (what, p_smooth, p_blurred, min_over_blurred))
    return bad
