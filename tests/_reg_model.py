"""float64 model of choosing the regularisation weight from the picture (fdr_noise_sigma_f32*, fdr_reg_curve_f32*,
fdr_choose_reg_f32*; include/fdr.h).

The plan is M x N, the window rows x cols at its top-left corner, pad(d) is d there and 0 elsewhere.  H is the DFT2 of the operator
PSF (top-left in the plan), L(u, v) = 4 sin^2(pi u / M) + 4 sin^2(pi v / N), and for a pair (K, gamma)

    G = DFT2(pad(d));  P = |G|^2 / (M N)
    t = K + gamma L^2;  den = |H|^2 + t;  q = den > 0 ? t / den : 0
    rho = sum over all M N bins of P q^2;  trace = sum over all M N bins of q;  gcv = M N rho / trace^2  (+inf when trace = 0)

The model sums over the FULL spectrum with weight 1 for every bin, so it knows nothing of the half spectrum, the packed column
or the Hermitian weights of the device.  Pinned in test_reg_host.py (against the spatial residual of the CLS restoration,
Parseval, the trace's limit, Gaussian noise of known sigma, and injected faults) before it judges the GPU (test_reg_gpu.py).  The GPU
cases are listed here so that the CPU fault pins run on exactly the same inputs."""
import functools
import math
from collections import namedtuple

import numpy as np

import _cls_model
import _pad_model
import _spectral
import _tv_model

REG_DISCREPANCY, REG_GCV = 0, 1
REG_PARAM_K, REG_PARAM_GAMMA = 0, 1
REG_AT_LOW, REG_AT_HIGH = 1, 2
DEFAULT_LO, DEFAULT_HI, DEFAULT_N, DEFAULT_REFINE = 1e-8, 1e2, 32, 2

Choice = namedtuple("Choice", "value sigma residual trace gcv flags evaluations")

FAULTS = ("nyquist_twice", "real_bins_twice", "dc_nyquist_swapped", "mirror_row", "lap_not_squared", "target_plan_area", "power_unscaled",
          "extras_dropped")
# mirror_row (a[m] instead of a[M - m] for the upper half of the packed column) changes nothing: a[m] = 4 sin^2(pi m / M) is
# symmetric about M / 2, and so are |H| and P of a real plane along column N / 2.  test_reg_host.py pins that it is invisible;
# no input could make the GPU test see it.
INVISIBLE_FAULTS = ("mirror_row",)

# ---- thresholds of test_reg_gpu.py: 4x the largest value one run on an MI355X measured (beside each), none above 1e-4 -----------
# rho and trace of one candidate against this model.  trace, and rho where it is at least RHO_FLOOR of sum d^2, relative to the
# model's value; a smaller rho (q^2 has taken nearly everything: what is left is the transform's rounding noise in the other
# bins) relative to sum d^2.
# Measured over the 14 plans x 2 PSFs x (tones + random) x 20 candidates, the windows and the Parseval runs: rho 5.09e-5, trace
# 5.41e-6 (512 x 32, dense PSF).  The rho maximum is one picture: the tone (1, 16) of the 16 x 32 plan with the motion PSF, whose
# |H| = 2.7e-3 there is a near-zero of the cut line's spectrum.  With K = 1e-6 (q = 0.12) that bin's q^2 moves by 1.3e-4 per 1e-7
# of absolute error in H -- d(q^2) / q^2 = -2 d|H|^2 / (|H|^2 + t) -- and the float32 operator table is 4e-8 off there; a tone
# picture has no other bin to average it out.  Every other case is at or below 6.9e-6 (2048 x 32, dense PSF, tone (1, 1)).
RHO_FLOOR = 1e-3
MEASURED_CURVE_MAX = 5.09e-5
CURVE_TOL = 2.1e-4
NOISE_TOL = 1e-12        # double arithmetic on both sides; measured 0 on every window
# discrepancy: |log(value / model value)|; measured 9.86e-6 (pad scene, 4 % noise, gamma searched)
MEASURED_VALUE_LOG_MAX = 9.86e-6
VALUE_LOG_TOL = 4e-5
# GCV: the model's gcv at the device's value over the model's minimum, minus 1.  Measured 0 in all twelve cases (the device takes the
# model's candidate in every round), and 4 x 0 is no bound: what a swap of two candidates can cost is the error of the device's
# gcv = M N rho / trace^2 on such pictures, rho's plus twice trace's (random pictures: 4.8e-6 + 2 x 5.4e-6).
GCV_EXCESS_TOL = 1.6e-5


def pad_plane(d, M, N):
    d = np.asarray(d, dtype=np.float64)
    plane = np.zeros((M, N))
    plane[:d.shape[0], :d.shape[1]] = d
    return plane


def power(d, M, N, fault=None):
    """P on the full M x N spectrum"""
    G = np.fft.fft2(pad_plane(d, M, N))
    P = G.real ** 2 + G.imag ** 2
    return P if fault == "power_unscaled" else P / (M * N)


def lap(M, N):
    """L(u, v) on the full M x N plane (the sin^2 form)"""
    a = 4.0 * np.sin(np.pi * np.arange(M) / M) ** 2
    b = 4.0 * np.sin(np.pi * np.arange(N) / N) ** 2
    return a[:, None] + b[None, :]


def operator_terms(psf, M, N, fault=None):
    """(|H|^2, L or L^2 as the fault has it, weights) on the full M x N spectrum"""
    H = np.fft.fft2(pad_plane(psf, M, N))
    h2 = H.real ** 2 + H.imag ** 2
    L = lap(M, N)
    w = np.ones((M, N))
    if fault == "nyquist_twice":
        w[:, N // 2] = 2.0
    elif fault == "real_bins_twice":
        for u in (0, M // 2):
            for v in (0, N // 2):
                w[u, v] = 2.0
    elif fault == "extras_dropped":
        w[0, N // 2] = w[M // 2, N // 2] = 0.0
    elif fault == "dc_nyquist_swapped":
        h2, L = h2.copy(), L.copy()
        h2[:, [0, N // 2]] = h2[:, [N // 2, 0]]
        L[:, [0, N // 2]] = L[:, [N // 2, 0]]
    elif fault == "mirror_row":
        a = 4.0 * np.sin(np.pi * np.arange(M) / M) ** 2
        b = 4.0 * np.sin(np.pi * (N // 2) / N) ** 2
        L = L.copy()
        L[:, N // 2] = a[(M - np.arange(M)) % M] + b
    l2 = L if fault == "lap_not_squared" else L * L
    return h2, l2, w


def q_of(h2, l2, K, gamma):
    t = K + gamma * l2
    den = h2 + t
    return np.where(den > 0, t / np.where(den > 0, den, 1.0), 0.0)


def curve_from(P, terms, K, gamma):
    """(rho[], trace[]) of the pairs (K[i], gamma[i]) from P = power(...) and terms = operator_terms(...)"""
    h2, l2, w = terms
    K = np.atleast_1d(np.asarray(K, dtype=np.float64))
    gamma = np.atleast_1d(np.asarray(gamma, dtype=np.float64))
    rho, tr = np.empty(K.size), np.empty(K.size)
    wP = w * P
    for i in range(K.size):
        q = q_of(h2, l2, float(K[i]), float(gamma[i]))
        rho[i] = float(np.sum(wP * q * q))
        tr[i] = float(np.sum(w * q))
    return rho, tr


def curve(d, psf, M, N, K, gamma, fault=None):
    return curve_from(power(d, M, N, fault), operator_terms(psf, M, N, fault), K, gamma)


def gcv(rho, trace, M, N):
    return M * N * rho / (trace * trace) if trace > 0 else math.inf


MASK = np.array([[1, -2, 1], [-2, 4, -2], [1, -2, 1]], dtype=np.float64)


def noise_sigma(d):
    """Immerkaer's estimate on the window d (rows, cols >= 3)"""
    d = np.asarray(d, dtype=np.float64)
    rows, cols = d.shape
    c = np.zeros((rows - 2, cols - 2))
    for i in range(3):
        for j in range(3):
            c += MASK[i, j] * d[i:i + rows - 2, j:j + cols - 2]
    return math.sqrt(math.pi / 2.0) * float(np.abs(c).sum()) / (6.0 * (rows - 2) * (cols - 2))


def log_grid(lo, hi, n):
    """v_i = lo (hi / lo)^(i / (n - 1)), the ends lo and hi themselves; python floats (the C library's pow, as the host code)"""
    v = [lo * (hi / lo) ** (i / (n - 1)) for i in range(n)]
    v[0], v[-1] = lo, hi
    return v


def choose(d, psf, M, N, method=REG_GCV, param=REG_PARAM_GAMMA, fixed=0.0, sigma=0.0, tau=0.0, lo=0.0, hi=0.0, n_grid=0, refine=-1,
           fault=None, state=None):
    """the search of fdr_choose_reg_f32 in float64.  state: (P, terms) computed before, for several searches on one picture"""
    d = np.asarray(d, dtype=np.float64)
    rows, cols = d.shape
    tau = tau or 1.0
    if lo == 0.0 and hi == 0.0:
        lo, hi = DEFAULT_LO, DEFAULT_HI
    n = n_grid or DEFAULT_N
    refine = DEFAULT_REFINE if refine == -1 else refine
    if method == REG_DISCREPANCY and sigma == 0.0:
        sigma = noise_sigma(d)
    P, terms = state if state is not None else (power(d, M, N, fault), operator_terms(psf, M, N, fault))
    evaluations = 0

    def sweep(a, b):
        v = log_grid(a, b, n)
        K = v if param == REG_PARAM_K else [fixed] * n
        g = [fixed] * n if param == REG_PARAM_K else v
        rho, tr = curve_from(P, terms, K, g)
        return v, rho, tr

    def finish(value, v, rho, tr, i, flags):
        return Choice(value, sigma, rho[i], tr[i], gcv(rho[i], tr[i], M, N), flags, evaluations)

    v, rho, tr = sweep(lo, hi)
    evaluations += n
    if method == REG_DISCREPANCY:
        assert np.all(np.diff(rho) >= -1e-9 * max(float(rho[-1]), 1e-300)), "rho is not non-decreasing"
        T = tau * (M * N if fault == "target_plan_area" else rows * cols) * sigma * sigma
        if not rho[-1] > 0:
            return finish(hi, v, rho, tr, n - 1, REG_AT_HIGH)
        if rho[0] >= T:
            return finish(lo, v, rho, tr, 0, REG_AT_LOW)
        if rho[-1] < T:
            return finish(hi, v, rho, tr, n - 1, REG_AT_HIGH)
        r = 0
        while True:
            i = 1
            while i < n - 1 and rho[i] < T:
                i += 1
            if r == refine:
                break
            v, rho, tr = sweep(v[i - 1], v[i])
            evaluations += n
            r += 1
        va, vb, ra, rb = v[i - 1], v[i], rho[i - 1], rho[i]
        value = vb
        dr = math.log(rb) - math.log(ra) if ra > 0 else 0.0
        if dr > 0:  # (a bracket refined down to neighbouring doubles has dr = 0: its upper end)
            la, lb = math.log(va), math.log(vb)
            f = min(max((math.log(T) - math.log(ra)) / dr, 0.0), 1.0)
            value = min(max(math.exp(la + f * (lb - la)), va), vb)
        low = math.log(value) - math.log(va) <= math.log(vb) - math.log(value)
        return finish(value, v, rho, tr, i - 1 if low else i, 0)
    r = 0
    while True:
        g = [gcv(rho[k], tr[k], M, N) for k in range(n)]
        i = 0
        for k in range(1, n):
            if g[k] < g[i]:
                i = k
        if r == refine:
            break
        v, rho, tr = sweep(v[max(i - 1, 0)], v[min(i + 1, n - 1)])
        evaluations += n
        r += 1
    value = v[i]
    return finish(value, v, rho, tr, i, REG_AT_LOW if value == lo else (REG_AT_HIGH if value == hi else 0))


# ---- the GPU cases (test_reg_gpu.py) --------------------------------------------------------------------------------------------
# every LOGM instantiation of the power pass (the 1024-thread one included), a long row, a small square, many workgroups and
# partials in both directions
CURVE_PLANS = [(1 << k, 32) for k in range(3, 14)] + [(8, 8192), (64, 64), (1024, 1024)]
WINDOW_PLANS = [(8, 32), (64, 64), (1024, 1024)]  # windows (M - 3, N - 5) with stride N + 7, and 3 x 3
PSF_NAMES = ("dense zero-mean", "motion 15/30")

# 20 pairs (K, gamma) spanning both weights: (0, 0), K alone, gamma alone, both; 20 is not a multiple of the 16 of one sweep
CANDIDATES = ([(0.0, 0.0)] + [(K, 0.0) for K in (1e-6, 1e-4, 1e-2, 1.0, 1e2)] + [(0.0, g) for g in (1e-6, 1e-4, 1e-2, 1.0, 1e2)] +
              [(1e-5, 1e-3), (1e-3, 1e-5), (1e-2, 1e-2), (0.1, 1e-6), (1e-6, 0.1), (3.0, 7.0), (1e-4, 10.0), (10.0, 1e-4), (1e3, 1e3)])
assert len(CANDIDATES) == 20
PARSEVAL_K = 1e30


def curve_psfs(oracle, M, N):
    return [(n, p) for n, p in _cls_model.psfs(oracle, M, N) if n in PSF_NAMES]


def tone(M, N, u, v):
    """cos(2 pi (u i / M + v j / N)) as float32: all of its power in the bins (u, v) and (M - u, N - v)"""
    i = np.arange(M, dtype=np.float64)[:, None]
    j = np.arange(N, dtype=np.float64)[None, :]
    return np.cos(2.0 * np.pi * ((u * i / M + v * j / N) % 1.0)).astype(np.float32)


def tone_bins(M, N):
    """the bins of the tone pictures: every edge row frequency with column frequencies 0 and N/2 (the packed column, both halves),
    every edge column frequency with row frequencies 0 and M/2, and the edge bins paired up; (0, 0) is the constant picture"""
    eu, ev = _spectral.edge_bins(M), _spectral.edge_bins(N)
    bins = [(u, v) for u in eu for v in (0, N // 2)] + [(u, v) for v in ev for u in (0, M // 2)] + list(zip(eu, ev))
    return sorted(set(bins))


def random_picture(M, N, rows=None, cols=None, stride=None):
    """uniform [0, 1) float32 window inside a buffer of row stride `stride` filled with a sentinel the window must not pick up"""
    rows, cols = rows or M, cols or N
    stride = stride or cols
    buf = np.full((rows, stride), 1e6, dtype=np.float32)
    buf[:, :cols] = np.random.default_rng(M * 7 + N * 3 + rows).random((rows, cols), dtype=np.float32)
    return buf


def curve_pictures(M, N):
    """(name, picture) of one plan: the tones, then one random picture"""
    return [("tone %d,%d" % b, tone(M, N, *b)) for b in tone_bins(M, N)] + [("random", random_picture(M, N))]


def curve_errors(rho, tr, rho_m, tr_m, sum_d2):
    """(largest rho error, largest trace error) of one picture's candidates, as CURVE_TOL defines them"""
    rho, tr, rho_m, tr_m = (np.asarray(x, dtype=np.float64) for x in (rho, tr, rho_m, tr_m))
    er = np.abs(rho - rho_m) / np.maximum(rho_m, RHO_FLOOR * sum_d2) if sum_d2 > 0 else np.abs(rho - rho_m)
    et = np.abs(tr - tr_m) / np.where(tr_m > 0, tr_m, 1.0)
    return float(np.max(er)), float(np.max(et))


NOISE_WINDOWS = [(3, 3, 3), (3, 3, 11), (3, 40, 47), (40, 3, 3), (17, 300, 301), (300, 517, 600), (1030, 70, 70)]  # rows, cols, stride

# the choice: two 512^2 scenes blurred periodically by the centred 15 px / 30 deg line, Gaussian noise of three levels (of the peak 1)
CHOICE_SIZE = 512
CHOICE_SCENES = ("pad scene", "blocks")
CHOICE_NOISE = (0.002, 0.01, 0.04)
CHOICE_SEED = 7
WINDOW_CHOICE = ("blocks", 0.01, 400, 300)  # scene, level, rows, cols: a window smaller than the plan
QUALITY_GRID = 81  # points of the grid over 1e-8 .. 1e2 the best PSNR is taken on


@functools.lru_cache(maxsize=None)
def choice_psf():
    """the M x N float32 PSF plane, centred at (0, 0)"""
    return _pad_model.centred_psf_plane(_pad_model.quality_psf(15, 30.0), CHOICE_SIZE, CHOICE_SIZE).astype(np.float32)


@functools.lru_cache(maxsize=None)
def choice_case(scene, level):
    """(truth float64, blurred float32) of one scene and noise level"""
    n = CHOICE_SIZE
    s = _pad_model.scene(3, n) if scene == "pad scene" else _tv_model.blocks_scene(n, n)
    H = np.fft.rfft2(choice_psf().astype(np.float64))
    b = np.fft.irfft2(np.fft.rfft2(s) * H, s=(n, n))
    b = b + level * float(s.max()) * np.random.default_rng(CHOICE_SEED).standard_normal(b.shape)
    return s, b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def choice_state(scene, level):
    _, b = choice_case(scene, level)
    n = CHOICE_SIZE
    return power(b, n, n), operator_terms(choice_psf(), n, n)


def restore(blurred, K, gamma):
    """the CLS restoration of a choice case with (K, gamma), float64"""
    n = CHOICE_SIZE
    return _cls_model.cls_raw(blurred, choice_psf(), K, gamma, n, n)


def pair_of(param, value, fixed=0.0):
    return (value, fixed) if param == REG_PARAM_K else (fixed, value)


@functools.lru_cache(maxsize=None)
def best_psnr(scene, level, param):
    """(best PSNR, its weight) of the restoration over QUALITY_GRID log-spaced weights in 1e-8 .. 1e2, the other weight 0"""
    truth, b = choice_case(scene, level)
    best = (-math.inf, None)
    for v in log_grid(DEFAULT_LO, DEFAULT_HI, QUALITY_GRID):
        p = _pad_model.psnr(restore(b, *pair_of(param, v)), truth)
        if p > best[0]:
            best = (p, v)
    return best


# What the restoration with the chosen weight must reach: (method, param) -> dB below the best of the grid; GCV with K is reported
# only (it under-regularises by 1 to 6 dB here, the known weakness of GCV with a flat penalty).  This model alone, on the six cases
# (test_reg_host.py prints each): GCV-gamma 0.00 .. 0.13 dB below the best, discrepancy-gamma 0.36 .. 0.89 dB, discrepancy-K
# 0.07 .. 1.27 dB.
QUALITY_MARGIN = {(REG_GCV, REG_PARAM_GAMMA): 0.5, (REG_DISCREPANCY, REG_PARAM_GAMMA): 1.5, (REG_DISCREPANCY, REG_PARAM_K): 1.5}
# The restoration must also beat the blurred input where this model does so alone.  With gamma it does in all six cases, by either
# method (3.2 .. 10.5 dB); the GCV-gamma floor at the 0.2 % level is left out all the same, as the feature's specification has it.
# With K searched by the discrepancy principle the model beats the blurred input in three cases only: a flat penalty cannot restore
# these scenes at 1 % noise and above, where even the best K of the grid stays below the blurred input (pad scene 1 %: best 33.60 dB,
# blurred 36.28 dB; 4 %: 27.15 / 27.61; blocks 4 %: 23.96 / 24.08).  The floor is narrowed to the cases the model passes:
K_BEATS_BLURRED = {("pad scene", 0.002), ("blocks", 0.002), ("blocks", 0.01)}  # model: +0.81, +7.10, +2.24 dB


def beats_blurred_required(method, param, scene, level):
    if (method, param) not in QUALITY_MARGIN:
        return False
    if param == REG_PARAM_K:
        return (scene, level) in K_BEATS_BLURRED
    return not (method == REG_GCV and level == CHOICE_NOISE[0])
