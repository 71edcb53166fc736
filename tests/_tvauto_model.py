"""float64 model of noise-constrained total-variation deconvolution (fdr_tv_deconv_auto_f32*; include/fdr.h).

The plan, the window, m = pad(weights), pad(d), H, D, L and shrink are those of _tvfree_model.py.  The caller states the noise level
sigma instead of the weight mu:

    minimise over x on the whole plan  TV(x)   subject to   sum m (blur(x) - pad(d))^2 <= c2 = tau sigma^2 S,   S = sum m

by the ADMM iteration of _tvfree_model.py (nu = 0 selects NU_RATIO rho, tau = 0 selects 1) with the weight of every data step taken
from the discrepancy of that step:

    c = blur(x);  res_e = sum m (c + q - pad(d))^2;  res_c = sum m (c - pad(d))^2;  S = sum m          (over the window, in double)
    g = 0 for res_e <= c2;  MAX_RATIO for c2 = 0 or a quotient that is not finite;  else min(sqrt(res_e / c2) - 1, MAX_RATIO)
    mu_k = float32(nu g)
    e = c + q;  s = (mu_k m pad(d) + nu e) / (mu_k m + nu);  q = e - s;  r = s - q;  ... the rest of the free iteration

For weights of 0 and 1, s is the projection of e onto the ball.  trace[k] = (res_c, res_e, mu_k).

Pinned in test_tvauto_host.py (the projection, convergence to the fixed-mu minimiser, quality, injected faults) before it judges the
GPU (test_tvauto_gpu.py)."""
import numpy as np

from _reg_model import noise_sigma
from _rl_model import NORM_NONE, op_spectrum, psnr
from _tv_model import dx, dxT, dy, dyT, shrink, solve_table
from _tvfree_model import QUALITY, finish, pad_to, quality_case, tvfree_model

MAX_RATIO = 1e6  # FDR_TV_AUTO_MAX_RATIO
NU_RATIO = 25.0  # FDR_TV_AUTO_NU_RATIO

# Thresholds from one run of test_tvauto_gpu.py on an MI355X, at most 4x the largest value measured there.
# TVA_TOL: max |got - model| / max |model| (FDR_NORM_NONE) or max-abs (normalised outputs) of the device against this model in
# float64.  Measured maxima: 8.69e-6 over n = 1, 2, 3 (2048 x 512, window 2000 x 333; 7.22e-6 at 256^2, window 200 x 151, motion 15/30,
# rho 2, nu 50, sigma 0.3, n = 1; 7.2e-7 at 8 x 32, 3.4e-6 at 16 x 32, 4.85e-6 at 64 x 128, 1.65e-6 at 8192 x 32), 3.16e-6 over n = 30 and
# 100 (64 x 64, window 60 x 50; 1.76e-6 at 512 x 256, masked) and 9.28e-6 on the quality scene (n = 100, masked; 8.45e-6 and 9.2e-6
# with sigma given and estimated).  The largest short-case values are those of sigma 0.3, where mu_k = 0 and x is the solve by
# 1 / (nu |H|^2 + rho L) of its own blur alone; with nu = 25 rho the solve amplifies rounding where |H| is small, as the periodic
# call does with a large mu.  The same model in float32 / complex64 (sums in double) gives 2.19e-6 at 64 x 128 (sigma 0.3, motion 15/30)
# and 3.89e-6 on the quality scene at n = 100 (test_tvauto_host.py): the device stays within 4x of its arithmetic class.
# TVA_TRACE_TOL: the relative error of res_c, res_e and mu_k of the trace (mu_k where the model's is not 0; where it is 0 the
# device's must be 0 too).  Measured maxima: 1.31e-5 (8 x 32, delta PSF, rho 10, nu 4, fractional weights, sigma 0.3: mu_k = 0.042 in
# the third step, one step before the clamp) and 1.89e-6 everywhere else; the float32 model gives 1.53e-6 on the quality scene.
# mu_k = nu (sqrt(res_e / c2) - 1) amplifies the relative error of res_e by sqrt(res_e / c2) / (2 (sqrt(res_e / c2) - 1)), 47 times
# at that maximum, which is why the trace has a tolerance of its own.
TVA_TOL = 3.5e-5
TVA_TRACE_TOL = 5e-5

FAULTS = ("no_sqrt", "res_c", "S_area", "mu_lag", "no_clamp", "unweighted")


def ratio(res_e, c2, fault=None):
    """g of one step"""
    if fault != "no_clamp" and res_e <= c2:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        quot = np.float64(res_e) / np.float64(c2)
    if c2 == 0.0 or not np.isfinite(quot):
        return MAX_RATIO
    return min(float(quot - 1.0 if fault == "no_sqrt" else np.sqrt(quot) - 1.0), MAX_RATIO)


def project(e, d_pad, m, c2):
    """(s, mu / nu): e moved towards d where m counts, by the model's formula with g = mu / nu"""
    g = ratio(float(np.sum(m * (e - d_pad) ** 2)), c2)
    return (g * m * d_pad + e) / (g * m + 1.0), g


def tvauto_iterates(d, psf, M, N, sigma, rho=2.0, iterations=100, weights=None, tau=0.0, nu=0.0, anisotropic=False, dtype=np.float64, fault=None):
    """yields dict(x, q, s, c, trace=(res_c, res_e, mu_k), sigma, c2, S) after the start (x and sigma alone) and after every iteration.
    sigma = 0: Immerkaer's estimate of the window (the weights are not looked at).  dtype float32 runs the planes and spectra in
    single precision and keeps the sums in double: the arithmetic class of the device.  fault (for the CPU pins only): 'no_sqrt'
    (g = res_e / c2 - 1), 'res_c' (res_c in the place of res_e), 'S_area' (S = rows cols despite weights), 'mu_lag' (the previous
    step's mu, 0 at first), 'no_clamp' (g < 0 kept), 'unweighted' (the three sums without m)."""
    assert fault is None or fault in FAULTS, fault
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    d = np.asarray(d, dtype=dtype)
    rows, cols = d.shape
    sigma = float(sigma) if sigma else noise_sigma(d)
    tau = float(tau) if tau else 1.0
    nu = float(nu) if nu else NU_RATIO * float(rho)
    H = op_spectrum(psf, M, N)
    T = solve_table(H, M, N, nu, rho).astype(dtype)
    Hf, Hb = H.astype(cdt), np.conj(H).astype(cdt)
    pad = pad_to(d, M, N, dtype)
    m = np.zeros((M, N), dtype=dtype)
    m[:rows, :cols] = 1 if weights is None else np.asarray(weights, dtype=dtype)
    inside = np.zeros((M, N), dtype=bool)
    inside[:rows, :cols] = True
    nu_, rho_ = dtype(nu), dtype(rho)
    x = pad.copy()
    wx = np.zeros((M, N), dtype=dtype)
    wy = np.zeros((M, N), dtype=dtype)
    q = np.zeros((M, N), dtype=dtype)
    t = dtype(1.0) / rho_
    m64, pad64 = m.astype(np.float64), pad.astype(np.float64)
    msum = inside.astype(np.float64) if fault == "unweighted" else m64
    last_mu = 0.0
    yield dict(x=x, sigma=sigma)
    for _ in range(iterations):
        c = np.fft.irfft2(np.fft.rfft2(x).astype(cdt) * Hf, s=(M, N)).astype(dtype)
        c64, q64 = c.astype(np.float64), q.astype(np.float64)
        res_e = float(np.sum(msum * ((c64 + q64) - pad64) ** 2))
        res_c = float(np.sum(msum * (c64 - pad64) ** 2))
        S = float(rows * cols) if fault == "S_area" else float(np.sum(msum))
        c2 = tau * sigma * sigma * S
        mu_now = float(np.float32(nu * ratio(res_c if fault == "res_c" else res_e, c2, fault)))
        mu_k = last_mu if fault == "mu_lag" else mu_now
        last_mu = mu_now
        e = c + q
        a = dtype(mu_k) * m
        s = np.where(inside, (a * pad + nu_ * e) / (a + nu_), e).astype(dtype)
        q = np.where(inside, e - s, 0).astype(dtype)
        r = np.where(inside, s - q, c).astype(dtype)
        b = np.fft.irfft2(np.fft.rfft2(r).astype(cdt) * Hb, s=(M, N)).astype(dtype)
        gx, gy = dx(x) + wx, dy(x) + wy
        zx, zy = shrink(gx, gy, t, bool(anisotropic))
        wx, wy = gx - zx, gy - zy
        vx, vy = zx - wx, zy - wy
        rhs = (nu_ * b + rho_ * (dxT(vx) + dyT(vy))).astype(dtype)
        x = np.fft.irfft2(np.fft.rfft2(rhs).astype(cdt) * T, s=(M, N)).astype(dtype)
        yield dict(x=x, q=q, s=s, c=c, e=e, trace=(res_c, res_e, mu_k), sigma=sigma, c2=c2, S=S)


def tvauto_model(d, psf, M, N, sigma, rho=2.0, iterations=100, weights=None, tau=0.0, nu=0.0, anisotropic=False, nonneg=False, norm_area=NORM_NONE,
                 out_shape=None, dtype=np.float64, fault=None):
    """(the output of fdr_tv_deconv_auto_f32 on the window d: the top-left out_shape (default d.shape) of x, the trace as an n x 3 array)"""
    st, trace = None, []
    for st in tvauto_iterates(d, psf, M, N, sigma, rho, iterations, weights, tau, nu, anisotropic, dtype, fault):
        if "trace" in st:
            trace.append(st["trace"])
    return finish(st["x"], out_shape or np.asarray(d).shape, nonneg, norm_area, M, N), np.array(trace, dtype=np.float64).reshape(-1, 3)


def trace_err(got, want):
    """the largest relative error of a trace against the model's: res_c, res_e, and mu_k where the model's is not 0 (where it is 0 the
    other must be 0: infinite error otherwise)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return float("inf")
    if not got.size:
        return 0.0
    worst = 0.0
    for k in range(3):
        g, w = got[:, k], want[:, k]
        zero = w == 0
        if np.any(g[zero] != 0):
            return float("inf")
        if np.any(~zero):
            worst = max(worst, float(np.max(np.abs(g[~zero] - w[~zero]) / np.abs(w[~zero]))))
    return worst if worst == worst else float("inf")


# the two noise levels of the short cases: 0.02 keeps mu_k active at every step, 0.3 makes a ball so wide that the clamp at 0 is hit
SHORT_SIGMAS = (0.02, 0.3)


def f32(v):
    """the value a float parameter has on the device"""
    return float(np.float32(v))


_qual = {}


def quality_numbers():
    """the model on the quality scene, once: PSNR of the blurred crop, the best of the hand-tuned free calls at 100 steps, and the auto
    call with sigma given, estimated, and with the stuck pixels masked (shared with test_tvauto_gpu.py)"""
    if not _qual:
        c, q = quality_case(), QUALITY
        args = (c["psf"], q["M"], q["N"])
        _qual["blurred"] = psnr(c["d"], c["truth"])
        _qual["tuned"] = {mu: psnr(tvfree_model(c["d"], *args, mu, q["rho"], 100), c["truth"]) for mu in (50.0, 100.0, 200.0, 500.0, 1000.0, 2000.0)}
        _qual["best"] = max(_qual["tuned"].values())
        for name, img, sigma, wt in (("given", c["d"], f32(q["noise"]), None), ("estimated", c["d"], 0.0, None),
                                     ("masked", c["stuck"], f32(q["noise"]), c["keep"])):
            st = None
            for st in tvauto_iterates(img, *args, sigma, q["rho"], 100, wt):
                pass
            _qual[name] = dict(x=st["x"][:q["rows"], :q["cols"]].copy(), psnr=psnr(st["x"][:q["rows"], :q["cols"]], c["truth"]), sigma=st["sigma"],
                               ratio=st["trace"][0] / st["c2"], mu=st["trace"][2])
    return _qual
