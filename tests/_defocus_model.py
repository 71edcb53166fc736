"""float64 model of the defocus estimate (fdr_psf_disk*, fdr_estimate_defocus_f32*, fdr_estimate_blur_f32*; include/fdr.h).  numpy only.

A uniform disk of radius R has the transfer function J1(2 pi R rho) / (pi R rho): rings of zeros in |G|, which the power cepstrum c
of _motion_model (same window, same eps) shows as a negative ring of radius about 2 R.  With S = _motion_model.score_table(c, ...):

    T[d]  = median over the angles a of S[a, d]                (numpy.median: 0.5 (s[(n - 1) / 2] + s[n / 2]) of the sorted column)
    k*    = argmin T (exact ties: the lowest index);  d* = min_diameter + k*
    confidence = (median T - T[k*]) / (1.4826 MAD T)           (0 when the MAD is 0)
    d_sub = d* + 0.5 (T[k* - 1] - T[k* + 1]) / (T[k* - 1] - 2 T[k*] + T[k* + 1]), the offset clamped to +-0.5; d* itself at either
            end of the table or when the denominator is 0
    radius = DEFOCUS_A d_sub + DEFOCUS_B

The median over the directions, not the mean: a motion blur puts one deep peak on the circle, which moves the mean (a mean
profile answers a 9 px motion blur with a confidence above 20) and leaves the median alone.

disk(size, radius) is fdr_psf_disk: pixel (i, j) gets the share of its unit square inside the disk about c = size // 2, counted on a
16 x 16 grid of sub-samples in integers (units of 1 / 32 px), so the device and this model agree bit for bit.

Pinned in test_defocus_host.py before it judges the GPU (test_defocus_gpu.py)."""
import math
from collections import namedtuple

import numpy as np

import _motion_model as mm

SUB = 16  # sub-samples per pixel and axis
MAX_ANGLES = 4096
MOTION_CONF_MIN = 10.0  # FDR_MOTION_CONF_MIN
DEFOCUS_CONF_MIN = 6.0  # FDR_DEFOCUS_CONF_MIN
BLUR_NONE, BLUR_MOTION, BLUR_DEFOCUS = 0, 1, 2

# radius = DEFOCUS_A d_sub + DEFOCUS_B: the least-squares line of calibrate() over CAL_RADII x CAL_SCENES (FDR_DEFOCUS_A / _B of
# include/fdr.h; test_defocus_host.py refits them)
DEFOCUS_A = 0.52304
DEFOCUS_B = -0.01685
CAL_RADII = [2, 2.5, 3, 3.7, 4.5, 5.2, 6, 7, 8, 9.3, 10.5, 12, 13]
CAL_SCENES = [(512, 512, 7), (600, 900, 11), (512, 512, 21)]
# the recovery grid: radii outside the fit, on two scenes outside it
REC_RADII = [2.2, 3.3, 5, 6.5, 9, 11.5]
REC_SCENES = [(512, 512, 31), (600, 900, 32)]
# sharp scenes: seed 1000, the first scene of the motion estimate's own grid (test_motion_host.py bounds its motion confidence)
SHARP_SCENES = [(256, 256, 1000), (512, 512, 1000), (600, 900, 1000)]
# the bounds the feature promises.  The largest radius error of this model over REC_RADII x REC_SCENES is
# 0.0563 px (R = 5 and 6.5 at 512^2); the tolerance is twice that
DEFOCUS_RADIUS_TOL = 0.113
CONF_DEFOCUS_MIN = 6.0   # every disk case of the calibration and recovery grids
CONF_OTHER_MAX = 4.0     # every motion-blurred and every sharp scene
# max |T - model| of a profile.  PROFILE_F32_BOUND: the float32 restatement on the CPU (profile_f32; test_defocus_host.py) reaches
# 2.8e-8 over the recovery grid, |T| up to 0.07; the bound is twice that.  DEFOCUS_PROFILE_TOL, the device's: 4x the largest value of
# one run of test_defocus_gpu.py on an MI355X (1.16e-7, the cat on 1024 x 2048; 3e-9 to 1.1e-7 over all its cases)
PROFILE_F32_BOUND = 5.6e-8
DEFOCUS_PROFILE_TOL = 4.7e-7

Estimate = namedtuple("Estimate", "diameter ring radius score confidence n_angles n_diameters")


def disk_counts(size, radius):
    """(size x size int64) sub-samples of each pixel inside the disk: (double)(X^2 + Y^2) <= q, q = (2 SUB radius)^2 in double"""
    c = size // 2
    e = 2.0 * SUB * float(radius)
    q = e * e
    k = np.arange(SUB, dtype=np.int64)
    i = np.arange(size, dtype=np.int64)
    X = ((2 * k + 1)[None, :] + 2 * SUB * (i[:, None] - c) - SUB).ravel()
    X2 = X * X
    inside = (X2[:, None] + X2[None, :]).astype(np.float64) <= q
    return inside.reshape(size, SUB, size, SUB).sum(axis=(1, 3)).astype(np.int64)


def disk(size, radius):
    """fdr_psf_disk: count / total count, divided in double and rounded once to float32"""
    n = disk_counts(size, radius)
    return (n.astype(np.float64) / float(n.sum())).astype(np.float32)


def disk_size(radius):
    """the size the fdr_set_psf_disk* setters generate: 2 ceil(radius) + 1"""
    return 2 * int(math.ceil(radius)) + 1


def disk_radius_max(size):
    c = size // 2
    return min(c, size - 1 - c) + 0.5


def defaults(rows, cols, min_diameter=0, max_diameter=0, angle_step=0.0):
    """(min_diameter, max_diameter, step, n_angles, n_diameters): the defaults of the motion estimate"""
    return mm.defaults(rows, cols, min_diameter, max_diameter, angle_step)


def profile(S):
    """T[d] = numpy.median over the angles of the score table S (n_angles x n_diameters)"""
    return np.median(np.asarray(S, dtype=np.float64), axis=0)


def pick(T, min_diameter):
    """(diameter, ring, radius, score, confidence) of a profile, in double (T may be float32)"""
    T = np.asarray(T, dtype=np.float64)
    k = int(np.argmin(T))
    med = float(np.median(T))
    mad = float(np.median(np.abs(T - med)))
    conf = (med - T[k]) / (mm.MAD_SCALE * mad) if mad > 0 else 0.0
    off = 0.0
    if 0 < k < len(T) - 1:
        den = T[k - 1] - 2.0 * T[k] + T[k + 1]
        if den != 0.0:
            off = min(0.5, max(-0.5, 0.5 * (T[k - 1] - T[k + 1]) / den))
    ring = min_diameter + k + off
    return min_diameter + k, ring, DEFOCUS_A * ring + DEFOCUS_B, float(T[k]), conf


def estimate_from_cepstrum(c, rows, cols, min_diameter=0, max_diameter=0, angle_step=0.0, with_profile=False):
    lo, hi, step, na, nd = defaults(rows, cols, min_diameter, max_diameter, angle_step)
    if na > MAX_ANGLES:
        raise ValueError("more than %d angles" % MAX_ANGLES)
    if not np.any(c):
        est, T = Estimate(0, 0.0, 0.0, 0.0, 0.0, na, nd), np.zeros(nd)
    else:
        T = profile(mm.score_table(c, lo, hi, step))
        est = Estimate(*pick(T, lo), na, nd)
    return (est, T) if with_profile else est


def estimate(img, M, N, min_diameter=0, max_diameter=0, angle_step=0.0, with_profile=False):
    rows, cols = img.shape
    return estimate_from_cepstrum(mm.cepstrum_model(img, M, N), rows, cols, min_diameter, max_diameter, angle_step, with_profile)


def classify(motion_conf, defocus_conf):
    """the blur kind of the two confidences, each over its own threshold"""
    m, f = motion_conf / MOTION_CONF_MIN, defocus_conf / DEFOCUS_CONF_MIN
    if m < 1.0 and f < 1.0:
        return BLUR_NONE
    return BLUR_MOTION if m >= f else BLUR_DEFOCUS


def plan_size(rows, cols):
    """the plan estimateDefocusBlur / estimateBlur use: the smallest 2^a 3^b 5^c of each dimension, at least 32"""
    return mm.plan_sizes(rows, cols)[1]


def defocused_scene(rows, cols, radius, seed, noise=1.0):
    """scene(rows, cols, seed) blurred linearly with disk(2 ceil(R) + 1, R), noise sigma `noise`, rounded to integers in [0, 255]"""
    return mm.blurred_scene(rows, cols, 0, 0.0, disk(disk_size(radius), radius), seed, noise)


def calibrate(radii=CAL_RADII, scenes=CAL_SCENES, ring_of=None):
    """(A, B, rings): the least-squares line radius = A d_sub + B over the grid; rings[(rows, cols, seed, R)] = d_sub.  ring_of(rows,
    cols, seed, R) may supply the ring of a case computed elsewhere (by this model)."""
    def model_ring(rows, cols, seed, R):
        return estimate(defocused_scene(rows, cols, R, seed), *plan_size(rows, cols)).ring
    ring_of = ring_of or model_ring
    rings = {(rows, cols, seed, R): ring_of(rows, cols, seed, R) for rows, cols, seed in scenes for R in radii}
    d = np.array(list(rings.values()))
    r = np.array([k[3] for k in rings], dtype=np.float64)
    A, B = np.polyfit(d, r, 1)
    return float(A), float(B), rings


# ---- a float32 restatement of the profile: the arithmetic of the device on the CPU (the floor of DEFOCUS_PROFILE_TOL) ----
def cepstrum_f32(img, M, N):
    """the device's cepstrum arithmetic on the CPU: float32 window, complex64 transforms, float32 log and scale"""
    x = mm.window_plane(img, M, N, dtype=np.float32)
    eps = np.float32(mm.EPS_REL * float(np.abs(x.astype(np.float64)).sum()))
    G = np.fft.fft2(x.astype(np.complex64))
    L = (np.log(np.abs(G).astype(np.float32) + eps) * np.float32(1.0 / (M * N))).astype(np.complex64)
    return np.real(np.fft.ifft2(L, norm="forward")).astype(np.float32)


def profile_f32(c32, min_diameter, max_diameter, step):
    """T of a float32 cepstrum with the device's arithmetic: float weights and sums in the gather, 0.5f (a + b) for the median"""
    M, N = c32.shape
    n_angles = int(math.ceil(180.0 / step))
    cs, sn = mm.trig_table(n_angles, step)
    ds = np.arange(min_diameter, max_diameter + 1, dtype=np.float64)
    y, x = -ds[None, :] * sn[:, None], ds[None, :] * cs[:, None]
    i0, j0 = np.floor(y), np.floor(x)
    fy, fx = (y - i0).astype(np.float32), (x - j0).astype(np.float32)
    i0, j0 = i0.astype(np.int64) % M, j0.astype(np.int64) % N
    i1, j1 = (i0 + 1) % M, (j0 + 1) % N
    one = np.float32(1.0)
    r0 = (one - fx) * c32[i0, j0] + fx * c32[i0, j1]
    r1 = (one - fx) * c32[i1, j0] + fx * c32[i1, j1]
    S = np.sort((one - fy) * r0 + fy * r1, axis=0)
    return np.float32(0.5) * (S[(n_angles - 1) // 2] + S[n_angles // 2])


# ---- the wrong implementations the host tests must catch ----
def profile_mean(S):
    return np.mean(np.asarray(S, dtype=np.float64), axis=0)


def profile_upper_middle(S):
    S = np.sort(np.asarray(S, dtype=np.float64), axis=0)
    return S[S.shape[0] // 2]


def disk_hard(size, radius):
    """a disk without sub-samples: 1 where the pixel's centre lies inside"""
    c = size // 2
    i = np.arange(size) - c
    n = ((i[:, None] ** 2 + i[None, :] ** 2) <= radius * radius).astype(np.float64)
    return n


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2))
    return 10.0 * math.log10(255.0 ** 2 / mse)
