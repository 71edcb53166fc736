"""float64 model of free-boundary and noise-constrained total-variation deconvolution in groups (fdr_tv_deconv_free_batch_f32*,
fdr_tv_deconv_auto_batch_f32*; include/fdr.h), on the pieces of _tvfree_model.py, _tvauto_model.py and
_tvcolor_model.py.

d is [C, rows, cols]: C crops of one size with one operator PSF and one weights plane (or none).  Uncoupled, every image runs the
iteration of _tvfree_model.py (mu given) or of _tvauto_model.py (a noise level per image) on its own.  Coupled (vectorial TV,
FDR_TV_COUPLE_CHANNELS) the images are the channels of one picture and ONE step of the iteration changes:

    m = sqrt(sum over c of gx_c^2 + gy_c^2), c = 0, 1, .. in that order;  s = m > t ? 1 - t / m : 0;  z_c = s g_c      (joint_shrink)

The data step (s_update), the duals q_c, w_c, b_c, the solve and -- auto form -- the ball tau sigma_c^2 S, the three sums and mu_k
(ratio) stay per channel.

Pinned in test_tvfreebatch_host.py (C = 1 against the single models, uncoupled against the per-image models, injected faults,
quality) before it judges the GPU (test_tvfreebatch_gpu.py).

TVFB_TOL, TVFB_AUTO_TOL, TVFB_TRACE_TOL: the bounds of the coupled GPU cases against this model in float64: max |got - model| /
max |model| of an image (FDR_NORM_NONE) for the free and the auto form, and the relative error of a trace as trace_err of
_tvauto_model.py measures it.  Set as TVF_TOL and TVA_TOL were: at most 4x the largest value of one run of test_tvfreebatch_gpu.py
on an MI355X (three channels, the 15 x 15 line PSF, fractional weights, mu 50, rho 2, nu 3 (free) / 20 (auto), sigmas 0.02 / 0.05 /
0.03).  Measured maxima:
    free   2.54e-6 (64 x 128, window 37 x 101, M x N output, n = 30); over n = 1, 2, 3: 1.58e-6 (the same plan, n = 3), 1.19e-6 at
           128 x 512 with the window 100 x 333, 3.9e-7 at 8 x 32
    auto   4.34e-6 (64 x 128, window 37 x 101, n = 30); over n = 1, 2, 3: 2.32e-6 (128 x 512, window 100 x 333, n = 1), 1.53e-6 at
           64 x 128, 6.6e-7 at 8 x 32
    trace  1.39e-6 (64 x 128, n = 30); over n = 1, 2, 3: 7.5e-7 (64 x 128, n = 3), 4.2e-7 at 128 x 512, 1.4e-7 at 8 x 32
The same model in float32 / complex64 (sums in double) on the CPU gives, on the same cases, 4.9e-7 / 1.07e-6 / 2.8e-7 at 64 x 128
with n = 30, 3.0e-7 / 5.9e-7 / 1.3e-7 there with n = 3 and 4.4e-7 / 1.22e-6 / 1.4e-7 at 128 x 512 with n = 3 (free / auto / trace):
the device stays within 10x of its arithmetic class everywhere (5.2x, 4.1x and 4.9x at the three maxima; at most 5.8x, the trace
at 64 x 128 with n = 3).  The uncoupled forms have no tolerance: they are held to the bits of the single calls."""
import numpy as np

from _reg_model import noise_sigma
from _rl_model import NORM_NONE, normalize, op_spectrum
from _tv_model import dx, dxT, dy, dyT, shrink, solve_table
from _tvauto_model import NU_RATIO, ratio
from _tvcolor_model import joint_shrink
from _tvfree_model import pad_to, s_update

TVFB_TOL = 1.0e-5        # free, coupled: 4 x 2.54e-6
TVFB_AUTO_TOL = 1.7e-5   # auto, coupled: 4 x 4.34e-6
TVFB_TRACE_TOL = 5.5e-6  # the traces of the coupled auto form: 4 x 1.39e-6

FAULTS = ("channelwise", "shared_mu", "shared_q", "sigma_first", "weights_first_only", "partials_alias")
FREE_FAULTS = ("channelwise", "shared_q", "weights_first_only")  # the faults that the free form can have


def group_iterates(d, psf, M, N, mu=None, sigmas=None, rho=2.0, iterations=50, weights=None, tau=0.0, nu=0.0, anisotropic=False,
                   coupled=False, dtype=np.float64, fault=None):
    """yields dict(x [C, M, N], q, trace [C, 3] (auto form), sigma [C]) after the start (x and sigma alone) and after every iteration.
    mu given: the free form; mu None: the auto form with the noise levels sigmas (a scalar serves all; 0 = Immerkaer's estimate of
    that image).  dtype float32 runs planes and spectra in single precision and keeps the sums in double.  fault (CPU pins only), each
    a way a group kernel can be wrong while a single call is right: 'channelwise' (coupled asked for, every channel its own norm),
    'shared_mu' (image 0's mu_k for all), 'shared_q' (all images read and write image 0's q plane, in order), 'sigma_first' (image
    0's sigma for all), 'weights_first_only' (images 1 .. see weights of 1), 'partials_alias' (image z's sums include image 0's)."""
    assert fault is None or fault in FAULTS, fault
    auto = mu is None
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    d = np.asarray(d, dtype=dtype)
    C, rows, cols = d.shape
    if auto:
        sg = np.broadcast_to(np.asarray(sigmas, dtype=np.float64), (C,))
        sigma = [float(sg[c]) if sg[c] else noise_sigma(d[c]) for c in range(C)]
        if fault == "sigma_first":
            sigma = [sigma[0]] * C
        tau = float(tau) if tau else 1.0
        nu = float(nu) if nu else NU_RATIO * float(rho)
    else:
        sigma = [0.0] * C
        nu = float(nu) if nu else float(rho)
    H = op_spectrum(psf, M, N)
    T = solve_table(H, M, N, nu, rho).astype(dtype)
    Hf, Hb = H.astype(cdt), np.conj(H).astype(cdt)
    pad = np.stack([pad_to(d[c], M, N, dtype) for c in range(C)])
    m = np.zeros((C, M, N), dtype=dtype)
    for c in range(C):
        m[c, :rows, :cols] = 1 if weights is None or (fault == "weights_first_only" and c > 0) else np.asarray(weights, dtype=dtype)
    inside = np.zeros((M, N), dtype=bool)
    inside[:rows, :cols] = True
    nu_, rho_ = dtype(nu), dtype(rho)
    x = pad.copy()
    wx = np.zeros((C, M, N), dtype=dtype)
    wy = np.zeros((C, M, N), dtype=dtype)
    q = np.zeros((C, M, N), dtype=dtype)
    t = dtype(1.0) / rho_
    m64, pad64 = m.astype(np.float64), pad.astype(np.float64)
    yield dict(x=x, sigma=sigma)
    for _ in range(iterations):
        cs = np.stack([np.fft.irfft2(np.fft.rfft2(x[c]).astype(cdt) * Hf, s=(M, N)).astype(dtype) for c in range(C)])
        trace = np.zeros((C, 3))
        mus = [dtype(mu) if not auto else None] * C
        if auto:  # the sums of every image before any data step, as the norm launch makes them
            sums = []
            for c in range(C):
                qc = q[0] if fault == "shared_q" else q[c]
                c64, q64 = cs[c].astype(np.float64), qc.astype(np.float64)
                sums.append([float(np.sum(m64[c] * ((c64 + q64) - pad64[c]) ** 2)), float(np.sum(m64[c] * (c64 - pad64[c]) ** 2)),
                             float(np.sum(m64[c]))])
            if fault == "partials_alias":
                sums = [sums[0]] + [[a + b0 for a, b0 in zip(sums[c], sums[0])] for c in range(1, C)]
            for c in range(C):
                res_e, res_c, S = sums[c]
                mu_k = float(np.float32(nu * ratio(res_e, tau * sigma[c] * sigma[c] * S)))
                trace[c] = (res_c, res_e, mu_k)
            if fault == "shared_mu":
                trace[:, 2] = trace[0, 2]
            mus = [dtype(trace[c, 2]) for c in range(C)]
        r = np.empty_like(cs)
        for c in range(C):
            k = 0 if fault == "shared_q" else c
            e = cs[c] + q[k]
            s = np.where(inside, s_update(e, pad[c], m[c], mus[c], nu_), e).astype(dtype)
            q[k] = np.where(inside, e - s, 0).astype(dtype)
            r[c] = np.where(inside, s - q[k], cs[c]).astype(dtype)
        b = np.stack([np.fft.irfft2(np.fft.rfft2(r[c]).astype(cdt) * Hb, s=(M, N)).astype(dtype) for c in range(C)])
        gx = np.stack([dx(x[c]) for c in range(C)]) + wx
        gy = np.stack([dy(x[c]) for c in range(C)]) + wy
        if coupled:
            zx, zy = joint_shrink(gx, gy, t, "channelwise" if fault == "channelwise" else None)
        else:
            z = [shrink(gx[c], gy[c], t, bool(anisotropic)) for c in range(C)]
            zx, zy = np.stack([p[0] for p in z]), np.stack([p[1] for p in z])
        wx, wy = gx - zx, gy - zy
        vx, vy = zx - wx, zy - wy
        x_new = []
        for c in range(C):
            rhs = (nu_ * b[c] + rho_ * (dxT(vx[c]) + dyT(vy[c]))).astype(dtype)
            x_new.append(np.fft.irfft2(np.fft.rfft2(rhs).astype(cdt) * T, s=(M, N)).astype(dtype))
        x = np.stack(x_new)
        yield dict(x=x, q=q.copy(), trace=trace, sigma=sigma)


def group_model(d, psf, M, N, mu=None, sigmas=None, rho=2.0, iterations=50, weights=None, tau=0.0, nu=0.0, anisotropic=False, coupled=False,
                nonneg=False, norm_area=NORM_NONE, out_shape=None, dtype=np.float64, fault=None):
    """(the outputs [C, out_shape] of the batched call, float64, every image clamped and normalised on its own; the traces
    [C, n, 3], all zero for the free form)"""
    d = np.asarray(d)
    C = d.shape[0]
    st, traces = None, []
    for st in group_iterates(d, psf, M, N, mu, sigmas, rho, iterations, weights, tau, nu, anisotropic, coupled, dtype, fault):
        if "trace" in st:
            traces.append(st["trace"])
    orows, ocols = out_shape or d.shape[1:]
    out = np.asarray(st["x"][:, :orows, :ocols], dtype=np.float64)
    if nonneg:
        out = np.maximum(out, 0)
    tr = np.array(traces, dtype=np.float64).reshape(-1, C, 3).transpose(1, 0, 2)
    return np.stack([normalize(o, norm_area, M, N) for o in out]), tr


def rel_err(got, want):
    """max |got - want| / max |want|"""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)) / np.max(np.abs(want)))


# ---- the coupled cases of test_tvfreebatch_gpu.py, shared with the fault pins of test_tvfreebatch_host.py ----
# (M, N, rows, cols): one tile with a full window, a cropped window of a residue 1 mod 4, and one of several tiles
COUPLED_PLANS = [(8, 32, 8, 32), (64, 128, 37, 101), (128, 512, 100, 333)]
COUPLED_IDS = ["%dx%d-win%dx%d" % c for c in COUPLED_PLANS]
COUPLED_SIGMAS = (0.02, 0.05, 0.03)  # one noise level per channel: the balls differ
COUPLED = dict(mu=50.0, rho=2.0, nu_free=3.0, nu_auto=20.0)


def coupled_case(M, N, rows, cols, seed=7):
    """(d [3, rows, cols] float32, psf, fractional weights): three channels with common edges, texture above the threshold 1 / rho
    and negative pixels; the 15 x 15 line PSF (dense 5 x 5 where the plan is smaller), centred where the window is cropped"""
    from _rl_model import centred_psf, dense_psf
    from _rltv_model import line_psf
    from _tvcolor_model import colour_images
    from _tvfree_model import tvf_weights
    psf = line_psf()
    if psf.shape[0] > M or psf.shape[1] > N:
        psf = dense_psf(5, 5)
    if (rows, cols) != (M, N):
        psf = centred_psf(psf, M, N)
    return colour_images(M, N, rows, cols, 3, seed), psf, tvf_weights("fractional", rows, cols, seed)
