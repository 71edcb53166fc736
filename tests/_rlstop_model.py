"""float64 model of the fit trace and the stopping rules of fdr_richardson_lucy_auto_f32* (include/fdr.h), built on the models of the
four Richardson-Lucy forms (_rl_model.py, _rlfree_model.py, _rlaccel_model.py).

With y_k the input of step k (u_k in the plain forms, the extrapolated point in the accelerated ones), c = blur(y_k) on the window,
d+ = max(d, 0) and w the pixel's weight (1 in the plain form; the weights m, or 1, in the free-boundary form):

    res_k = sum w (d+ - c)^2
    kl_k  = sum w ( c - d+ + (d+ > 0 and c > TAU ? d+ ln(d+ / c) : 0) )
    S = rows cols (plain form) or sum(W) (free-boundary form)
    RESIDUAL: stat_k = res_k, target = tau sigma^2 S          KL: stat_k = 2 gain kl_k / S, target = tau
    k* = the first k with stat_k <= target;  iterations_done = min(n, c ceil((k* + 1) / c)), c = check_every;  output u_(iterations_done)

Pinned against a direct evaluation from blur_model and against injected faults in test_rlstop_host.py before it judges the GPU
(test_rlstop_gpu.py)."""
import math

import numpy as np

from _reg_model import noise_sigma
from _rl_model import TAU, blur_model, op_spectrum
from _rlaccel_model import accelerate, rl_step_fn, rlfree_step_fn
from _rlfree_model import SIGMA, fullblur

STOP_NONE, STOP_RESIDUAL, STOP_KL = 0, 1, 2  # FDR_RL_STOP_*

# TRACE_TOL bounds |got - model| / |model| of every trace entry (res_k and kl_k) of the device against this model.  The stop decision
# of test_rlstop_gpu.py relies on 1e-3 (it keeps the model's stat_k / target 1 % away from 1), so TRACE_TOL may never exceed that.
# The device forms c in float32 (about 1e-6 of max c per pixel, BLUR_TOL of _rl_model.py) and the sums in double from there; the
# terms (d+ - c)^2 and the KL terms are differences of nearby numbers, so an entry carries c's error amplified by the inverse of the
# relative misfit.  One run of test_rlstop_gpu.py on an MI355X measured at most MEASURED_TRACE_MAX: 4.7e-7 in check (a) (n = 3, every
# shape, window and form; the largest on the 8 x 4096 plane, ragged window) and 5.15e-6 over the up to 12 steps of check (b) (plain
# accelerated form, Gaussian noise 0.005: a fit to about 1 %).  The tolerance is at most 4 times the largest.
MEASURED_TRACE_MAX = 5.15e-6
TRACE_TOL = 2e-5
assert TRACE_TOL <= 1e-3

DECISION_MARGIN = 0.01  # the model's stat_k / target stays this far from 1 for every k up to the stop, or the case proves nothing

FAULTS = ("stat_after_update", "unweighted", "stop_unfinished", "check_floor", "kl_no_guard")


def fit_stats(dp, c, w=None, tau=TAU, kl_guard=True):
    """(res, kl) of the reblurred point c against d+ on the window, float64; w None = all ones"""
    dp = np.asarray(dp, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    w = np.ones_like(dp) if w is None else np.asarray(w, dtype=np.float64)
    ok = (dp > 0) & (c > tau) if kl_guard else dp > 0  # the fault: the logarithm wherever d+ > 0, whatever c is
    cc = np.where(c > tau, c, 1.0) if kl_guard else np.maximum(np.abs(c), 1e-300)
    log_term = np.where(ok, dp * np.log(np.where(ok, dp / cc, 1.0)), 0.0)
    return float(np.sum(w * (dp - c) ** 2)), float(np.sum(w * (c - dp + log_term)))


def decide(trace, n, rule, target, S, gain=0.0, check_every=1, fault=None):
    """(iterations_done, stopped, statistic, k*) from the trace of a run to n; k* is None without a hit"""
    c = check_every or 1
    stat = [0.0] * len(trace)
    if rule == STOP_RESIDUAL:
        stat = [t[0] for t in trace]
    elif rule == STOP_KL:
        stat = [2.0 * gain * t[1] / S if S > 0 else math.inf for t in trace]
    if rule == STOP_NONE:
        return n, 0, 0.0, None
    hit = next((k for k in range(n) if stat[k] <= target), None)
    if hit is None:
        return n, 0, (stat[n - 1] if n else 0.0), None
    if fault == "stop_unfinished":
        done = hit
    elif fault == "check_floor":
        done = min(n, c * ((hit + 1) // c))
    else:
        done = min(n, c * -(-(hit + 1) // c))
    return done, 1, stat[hit], hit


def run_model(d, psf, M, N, n, free_boundary=False, accelerate_=False, weights=None, cov_sigma=SIGMA, fault=None):
    """n steps of one form on the window d: dict(trace = (n, 2) array, path = {k: raw u_k, k <= n} (window of the plain form, whole
    plan of the free-boundary form), S)"""
    assert fault is None or fault in FAULTS
    d = np.asarray(d, dtype=np.float64)
    rows, cols = d.shape
    dp = np.maximum(d, 0)
    H = op_spectrum(psf, M, N)
    w = None
    if free_boundary:
        st, step = rlfree_step_fn(d, psf, M, N, weights, cov_sigma)
        u0 = st["u"]
        w = st["W"][:rows, :cols]
        S = float(np.sum(w))
        reblur = lambda y: fullblur(y, H)[:rows, :cols]
    else:
        u0, step = rl_step_fn(d, psf, M, N)
        S = float(rows * cols)
        reblur = lambda y: blur_model(y, psf, M, N, H=H)
    if fault == "unweighted":
        w, S = None, float(rows * cols)
    trace = []

    def traced(y):
        u_next = step(y)
        trace.append(fit_stats(dp, reblur(u_next if fault == "stat_after_update" else y), w, kl_guard=fault != "kl_no_guard"))
        return u_next

    path = dict.fromkeys(range(n + 1))
    if accelerate_:
        accelerate(u0, traced, n, keep=path)
    else:
        u = u0
        path[0] = u
        for k in range(n):
            u = traced(u)
            path[k + 1] = u
    return dict(trace=np.array(trace, dtype=np.float64).reshape(n, 2), path=path, S=S, d=d)


def stop_model(run, rule=STOP_NONE, sigma=0.0, gain=0.0, tau=0.0, check_every=0, fault=None):
    """the rule applied to a run of run_model: dict(u = the raw u_(iterations_done), iterations_done, stopped, sigma, target, statistic,
    hit = k* or None, stat = stat_k of the whole run)"""
    tr, S, n = run["trace"], run["S"], len(run["trace"])
    tau_ = tau or 1.0
    sigma_ = float(sigma)
    if rule == STOP_RESIDUAL and sigma_ == 0.0:
        sigma_ = noise_sigma(run["d"].astype(np.float32))
    target = tau_ * sigma_ * sigma_ * S if rule == STOP_RESIDUAL else (tau_ if rule == STOP_KL else 0.0)
    done, stopped, statistic, hit = decide(tr, n, rule, target, S, gain, check_every, fault)
    stat = tr[:, 0] if rule == STOP_RESIDUAL else (2.0 * gain * tr[:, 1] / S if rule == STOP_KL else np.zeros(n))
    return dict(u=run["path"][done], iterations_done=done, stopped=stopped, sigma=sigma_, target=target, statistic=statistic, hit=hit, stat=stat)


def trace_error(got, want):
    """max over the entries of |got - want| / |want| (both (k, 2) arrays; NaN when either holds one)"""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def decision_margin(m):
    """min |stat_k / target - 1| over the k the decision looks at (all k up to the stop, or all n without one)"""
    last = m["hit"] if m["hit"] is not None else len(m["stat"]) - 1
    if last < 0 or m["target"] <= 0:
        return math.inf
    return float(np.min(np.abs(m["stat"][: last + 1] / m["target"] - 1.0)))


# ---- the scenes of the stop (test_rlstop_host.py on the model, test_rlstop_gpu.py on the device) ----
def scene(M, N, seed):
    """a positive M x N picture with smooth blobs and sharp rectangles, values in [0.05, 1]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:M, 0:N].astype(np.float64)
    img = np.full((M, N), 0.08)
    for _ in range(5):
        cy, cx = rng.uniform(0.1, 0.9) * M, rng.uniform(0.1, 0.9) * N
        s = rng.uniform(0.03, 0.1) * min(M, N)
        img += rng.uniform(0.3, 0.8) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    for _ in range(8):
        h, w = rng.integers(max(2, M // 16), max(3, M // 4)), rng.integers(max(2, N // 16), max(3, N // 4))
        y, x = rng.integers(0, M - h), rng.integers(0, N - w)
        img[y:y + h, x:x + w] += rng.uniform(0.1, 0.5)
    return np.clip(img / img.max(), 0.05, 1.0)


def noisy_case(truth, cpsf, noise, level, seed):
    """the truth blurred circularly with the centred PSF plane cpsf, then Gaussian noise of sigma `level` (noise 'gauss') or Poisson
    noise at `level` photons per unit (noise 'poisson'); float32"""
    M, N = truth.shape
    blurred = fullblur(truth, np.fft.rfft2(cpsf.astype(np.float64)))
    rng = np.random.default_rng(seed)
    if noise == "gauss":
        return (blurred + rng.normal(0, level, (M, N))).astype(np.float32)
    return (rng.poisson(np.maximum(blurred, 0) * level) / level).astype(np.float32)


# ---- the comparisons test_rlstop_gpu.py applies to the device (test_rlstop_host.py shows that each fault above fails one) ----
def trace_ok(got, want):
    """(error, error <= TRACE_TOL) of a device trace against the model's first len(got) entries"""
    e = trace_error(got, np.asarray(want)[: len(got)])
    return e, bool(e <= TRACE_TOL)


def stop_ok(done, stopped, m):
    """the count and the flag against the model's"""
    return int(done) == m["iterations_done"] and int(stopped) == m["stopped"]


def guard_case():
    """(M, N, d, psf): a picture whose reblurred start is 0 where the picture is not -- the PSF is a delta of weight 1/2 at (2, 3), the
    picture two blocks that do not overlap their own shift -- so the KL sum needs its guard c > TAU.  The amplitude 1e-3 keeps the
    rounding of a float32 transform (1e-6 of the largest value) two orders below TAU: c <= TAU on the device wherever it is 0 here.
    The weight 1/2 keeps kl_0 = sum(c) - sum(d+) away from 0 (a unit PSF conserves the sum, and a relative error means nothing)."""
    M, N = 16, 64
    d = np.zeros((M, N), dtype=np.float32)
    d[4:6, 10:13] = np.float32(1e-3) * (1 + np.arange(6, dtype=np.float32).reshape(2, 3) / 8)
    d[9:11, 40:43] = np.float32(2e-3)
    psf = np.zeros((3, 4), dtype=np.float32)
    psf[2, 3] = 0.5
    return M, N, d, psf


STOP_PLAN = (128, 256)
STOP_WINDOW = (112, 230)  # the free-boundary forms take this crop of the noisy plane
STOP_N = 40
STOP_SEED = 5
STOP_NOISE = {"gauss": 0.005, "poisson": 2000.0}
# (configuration, free_boundary, accelerate) -> tau: the first of 1, 1.04, 1.08, ... at which the model keeps DECISION_MARGIN (the plain
# form's residual falls slowly, so its neighbours crowd the target); `res` = RESIDUAL with sigma given, `est` = with sigma estimated
STOP_TAU = {("res", False, False): 1.0, ("res", False, True): 1.0, ("res", True, False): 1.0, ("res", True, True): 1.0,
            ("est", False, False): 1.1, ("est", False, True): 1.0, ("est", True, False): 1.0, ("est", True, True): 1.0,
            ("kl", False, False): 1.04, ("kl", False, True): 1.0, ("kl", True, False): 1.0, ("kl", True, True): 1.04}
STOP_CONFIGS = {"res": ("gauss", STOP_RESIDUAL, dict(sigma=0.005)), "est": ("gauss", STOP_RESIDUAL, dict(sigma=0.0)),
                "kl": ("poisson", STOP_KL, dict(gain=2000.0))}


def stop_scene(motion_psf, noise):
    """(centred PSF plane, noisy 128 x 256 plane) of check (b); motion_psf: the 9 px / 30 degree motion PSF"""
    from _rl_model import centred_psf
    M, N = STOP_PLAN
    cp = centred_psf(motion_psf, M, N)
    return cp, noisy_case(scene(M, N, STOP_SEED), cp, noise, STOP_NOISE[noise], STOP_SEED + 100)
