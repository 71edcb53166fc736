"""Richardson-Lucy with the TV prior in groups, with vectorial coupling (fdr_richardson_lucy_tv_batch_f32*,
fdr_rl_tv_factor_group_f32_dev; include/fdr.h): the float64 specification, built from _rltv_model.py, _rl_batch_model.py and the
buffer layouts of _batch_model.py; fault models; the colour quality scene.  test_rltv_batch_host.py turns the fault models against the
judge (the one of _rl_batch_model.py) before test_rltv_batch_gpu.py judges the GPU.

A call cuts `count` images into launch groups of `group`; a group runs to completion: the start of every image, then per iteration
ONE factor launch for the group, from the estimates that enter the step, and one launch per pass of the form, then the output of
every image.  Uncoupled, image k's factor is tv_factor of _rltv_model.py on its own estimate.  Coupled, the images are the channels
of one picture and share the norm of the prior:

    m^2 = eps^2 + sum_c (gx_c^2 + gy_c^2)      (added in the order c = 0, 1, ..)
    p_c = grad u_c / m;   g_c = 1 - lambda div p_c;   factor_c = w / g_c

m is no smaller than a channel's own, so |div p_c| <= 2 + sqrt 2 and g >= 0.57 hold as in the channel-wise form; the model asserts
g >= 0.5."""
import numpy as np

import _batch_model as bm
from _rl_batch_model import judge  # noqa: F401  (the judge of the GPU test: bits against the single calls, error against the model)
from _rl_model import NORM_NONE, TAU, blur_model, centred_psf, normalize, op_spectrum, psnr
from _rlfree_model import SIGMA, fullblur
from _rltv_model import EPS, _f32, line_psf, tv_factor, tv_grad

TILE = 64  # the factor kernels' tile (kRltvTileW, kRltvTileH): where the coupled kernel recomputes p from its halo
COUPLED_FAULTS = ("channelwise_norm", "first_channel_norm", "halo_own_norm", "sum_no_root")
CALL_FAULTS = ("factor_image0", "factor_previous_group", "factor_new_u", "ignore_out_pitch", "drop_last_group")

# Device against this model, coupled form (the uncoupled form is judged bit for bit against the single calls and by the constants
# of _rltv_model.py).  The coupled kernel rounds as the single one does -- one reciprocal square root, products, one correctly
# rounded division -- with nch - 1 more additions under the root, so the constants of _rltv_model.py (RLTV_FACTOR_TOL = 9e-7,
# RLTV_TOL = 3e-5, RLTV_FREE_TOL = 6e-5) are the bounds here too: the coupled form has no constants of its own, and the GPU test
# holds every coupled case within 10x of the float32 CPU run of this model as well.  Measured on the MI355X by one run of
# test_rltv_batch_gpu.py (in brackets the float32 CPU run of the same case):
#   coupled factor, relative to max(w): 2.46e-7 (2.27e-7), the largest over the eight shapes, 1 to 8 planes, every layout and both
#           parameter pairs (at 63 x 65; 2.33e-7 at 65 x 127, 2.26e-7 at 129 x 129)
#   coupled plain form, 3 channels: 64x128 win 37x101 1.25e-6 (5.4e-7; n = 30 at eps = 0.05), 256 win 200x151 2.08e-6 (4.2e-7; the same n)
#   coupled free form, masked, M x N output: 64x128 1.03e-5 (2.6e-6; n = 1 at eps = 1e-3), 256 win 200x151 1.61e-5 (1.15e-5; n = 3)
#   case by case the device is within a factor of 5.0 of the float32 CPU run (256 win 200x151, plain form, n = 30)
#   uncoupled, against the model through the single calls' bits: 1.43e-6 over the length sweeps, 9.5e-6 over the forms test
#   the colour quality scene at 1000 photons, n = 100: coupled 28.329 dB (model 28.329), channel-wise 28.160 dB (model 28.161)


# ---- the coupled factor ---------------------------------------------------------------------------------------------------
def tv_g_coupled(us, lam, eps=EPS, dtype=np.float64, fault=None):
    """[g_c]: g_c = 1 - lambda div(grad u_c / m), m the joint norm of the channels `us` ([C, R, Cc]), every operation in `dtype`.
    fault (CPU pins): one of COUPLED_FAULTS
      channelwise_norm    every channel under its own norm (the uncoupled kernel)
      first_channel_norm  channel 0's norm for all
      halo_own_norm       the p that a tile takes from its halo (left of and above each TILE x TILE tile) under the channel's own norm
      sum_no_root         m^2 in the place of m"""
    assert fault is None or fault in COUPLED_FAULTS
    us = [np.asarray(u, dtype=dtype) for u in us]
    lam, eps = dtype(_f32(lam)), dtype(_f32(EPS if eps == 0 else eps))
    e2 = max(eps * eps, dtype(np.finfo(np.float32).tiny))
    grads = [tv_grad(u) for u in us]
    own = [np.sqrt((gx * gx + gy * gy) + e2) for gx, gy in grads]
    m2 = np.full(us[0].shape, e2, dtype=dtype)
    for gx, gy in grads:  # c = 0, 1, ..
        m2 = m2 + (gx * gx + gy * gy)
    joint = m2 if fault == "sum_no_root" else np.sqrt(m2)
    out = []
    for c, (gx, gy) in enumerate(grads):
        m = own[c] if fault == "channelwise_norm" else own[0] if fault == "first_channel_norm" else joint
        px, py = (gx / m).astype(dtype), (gy / m).astype(dtype)
        nx, ny = np.zeros_like(px), np.zeros_like(py)
        nx[:, 1:] = px[:, :-1]
        ny[1:, :] = py[:-1, :]
        if fault == "halo_own_norm":
            ox, oy = gx / own[c], gy / own[c]
            nx[:, TILE::TILE] = ox[:, TILE - 1:-1:TILE]
            ny[TILE::TILE, :] = oy[TILE - 1:-1:TILE, :]
        g = 1 - lam * ((px - nx) + (py - ny))
        assert g.dtype == dtype
        if fault is None:
            assert float(g.min()) >= 0.5, "g = %g < 0.5" % float(g.min())
        out.append(g)
    return out


def tv_factor_coupled(us, lam, eps=EPS, w=None, dtype=np.float64, fault=None):
    """[factor_c] = w / g_c (w = 1 for None; one w for all channels)"""
    wv = dtype(1) if w is None else np.asarray(w, dtype=dtype)
    return [(wv / g).astype(dtype) for g in tv_g_coupled(us, lam, eps, dtype, fault)]


# ---- a launch group of either form, coupled or not ------------------------------------------------------------------------
def _free_setup(rows, cols, M, N, H, weights, sigma, dtype):
    m = np.ones((rows, cols), dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)
    W = np.zeros((M, N), dtype=dtype)
    W[:rows, :cols] = m
    alpha = fullblur(W, H, adjoint=True, dtype=dtype)  # once per call
    seen = alpha > sigma
    wgt = np.where(seen, 1 / np.where(seen, alpha, 1), 0).astype(dtype)
    win = np.zeros((M, N), dtype=bool)
    win[:rows, :cols] = True
    return dict(m=m, W=W, seen=seen, wgt=wgt, win=win, sw=float(np.sum(W, dtype=np.float64)))


def group_run(form, ds, psf, M, N, iterations, lam, eps=EPS, weights=None, sigma=SIGMA, coupled=False, dtype=np.float64, tau=TAU, H=None,
              free=None, fault=None, held=None, at=None):
    """The estimates [u_k] of one launch group after `iterations` steps: the windows `ds` in the plain form (u on the window), the
    whole plan in the free-boundary form (u is M x N).  fault: a COUPLED_FAULT (coupled) or factor_image0, factor_previous_group,
    factor_new_u; held: {k: the factor slot k held when the previous group ended}, updated in place; at: {n: callback(us)} called
    after step n."""
    ds = [np.asarray(d, dtype=dtype) for d in ds]
    rows, cols = ds[0].shape
    if H is None:
        H = op_spectrum(psf, M, N)
    dp = [np.maximum(d, 0) for d in ds]
    if form == "plain":
        u = [x.copy() for x in dp]
        w = None
    else:
        if free is None:
            free = _free_setup(rows, cols, M, N, H, weights, sigma, dtype)
        dw = []
        for x in dp:
            p = np.zeros((M, N), dtype=dtype)
            p[:rows, :cols] = free["m"] * x
            dw.append(p)
        u = [np.where(free["seen"], (float(np.sum(x, dtype=np.float64)) / free["sw"] if free["sw"] > 0 else 0.0), 0).astype(dtype) for x in dw]
        w = free["wgt"]
    n = len(ds)
    f = None
    for it in range(iterations):
        # the factor launch of the group, from the estimates that enter the step
        if coupled:
            f = tv_factor_coupled(u, lam, eps, w, dtype, fault if fault in COUPLED_FAULTS else None)
        else:
            f = [tv_factor(x, lam, eps, w=w, dtype=dtype) for x in u]
        if fault == "factor_image0":
            f = [f[0]] * n
        if fault == "factor_previous_group" and held:
            f = [held.get(k, f[k]) for k in range(n)]
        for k in range(n):
            if form == "plain":
                c = blur_model(u[k], psf, M, N, H=H, dtype=dtype)
                r = np.where(c > tau, dp[k] / np.where(c > tau, c, 1), 0).astype(dtype)
                g = blur_model(r, psf, M, N, adjoint=True, H=H, dtype=dtype)
            else:
                c = fullblur(u[k], H, dtype=dtype)
                ok = free["win"] & (c > tau)
                r = np.where(ok, dw[k] / np.where(ok, c, 1), 0).astype(dtype)
                g = fullblur(r, H, adjoint=True, dtype=dtype)
            if fault == "factor_new_u":
                un = np.maximum((u[k] if w is None else u[k] * w) * g, 0).astype(dtype)
                u[k] = np.maximum(un * tv_factor(un, lam, eps, dtype=dtype), 0).astype(dtype)
            else:
                u[k] = np.maximum(u[k] * f[k] * g, 0).astype(dtype)
        if at and it + 1 in at:
            at[it + 1](u)
    if held is not None and f is not None:
        for k in range(n):
            held[k] = f[k]
    return u


def rltv_coupled_model(ds, psf, M, N, iterations, lam, eps=EPS, norm_area=NORM_NONE, dtype=np.float64, fault=None):
    """the coupled plain form on the channels `ds` ([C, rows, cols]): [C, rows, cols], every channel normalised on its own"""
    us = group_run("plain", ds, psf, M, N, iterations, lam, eps, coupled=True, dtype=dtype, fault=fault)
    return np.stack([normalize(u, norm_area, M, N) for u in us])


def rltv_free_coupled_model(ds, psf, M, N, iterations, lam, eps=EPS, weights=None, sigma=SIGMA, out_shape=None, norm_area=NORM_NONE,
                            dtype=np.float64, fault=None):
    """the coupled free-boundary form: the top-left out_shape (default the window) of every channel's u, normalised on its own"""
    us = group_run("free", ds, psf, M, N, iterations, lam, eps, weights, sigma, coupled=True, dtype=dtype, fault=fault)
    orows, ocols = np.asarray(ds[0]).shape if out_shape is None else out_shape
    return np.stack([normalize(u[:orows, :ocols], norm_area, M, N) for u in us])


def references(form, imgs, psf, M, N, iterations, lam, eps, area, weights=None, sigma=SIGMA, out_shape=None, coupled=False, dtype=np.float64):
    """the model's results for the images of a call: image by image (uncoupled: any grouping gives these) or as one coupled group"""
    from _rltv_model import rltv_free_model, rltv_model
    if coupled:
        if form == "plain":
            return rltv_coupled_model(imgs, psf, M, N, iterations, lam, eps, area, dtype)
        return rltv_free_coupled_model(imgs, psf, M, N, iterations, lam, eps, weights, sigma, out_shape, area, dtype)
    if form == "plain":
        return np.stack([rltv_model(d, psf, M, N, iterations, lam, eps, area, dtype) for d in imgs])
    return np.stack([rltv_free_model(d, psf, M, N, iterations, lam, eps, weights, sigma, out_shape, area, dtype) for d in imgs])


# ---- the batched call over the buffer layouts -----------------------------------------------------------------------------
def batched_call(form, flat_in, lay, olay, psf, M, N, iterations, lam, eps, area, group, weights=None, sigma=SIGMA, coupled=False, fault=None):
    """The batched call in float64: image i read through img_pitch and stride, the groups of bm.launches, group_run per group, the
    store through out_pitch and out_stride into a SENTINEL-filled buffer (olay: the output side).  fault: one of CALL_FAULTS or,
    coupled, of COUPLED_FAULTS
      factor_image0          every image of a group is updated with the factor of the group's first image (one plane for the group)
      factor_previous_group  from the second group on, the update takes the factor the slot held when the previous group ended
      factor_new_u           the factor is taken from the updated estimate (the fault of _rltv_model.py)
      ignore_out_pitch       image i is stored at i * out_rows * out_stride
      drop_last_group        a last group smaller than `group` is not run"""
    assert form in ("plain", "free") and (fault is None or fault in CALL_FAULTS + COUPLED_FAULTS)
    rows, cols = lay.rows, lay.cols
    H = op_spectrum(psf, M, N)
    out = bm.new_output(olay, np.float64)
    free = _free_setup(rows, cols, M, N, H, weights, sigma, np.float64) if form == "free" else None
    held = {}
    i0 = 0
    for n in bm.launches(lay.count, group):
        if fault == "drop_last_group" and n < group and i0 > 0:
            break
        ds = [np.asarray(bm._window(flat_in, (i0 + k) * lay.img_pitch, rows, cols, lay.stride), dtype=np.float64) for k in range(n)]
        us = group_run(form, ds, psf, M, N, iterations, lam, eps, weights, sigma, coupled and n > 1, H=H, free=free, fault=fault, held=held)
        for k in range(n):
            res = normalize(us[k][:olay.rows, :olay.cols], area, M, N)
            base = olay.lead + (i0 + k) * olay.rows * olay.out_stride if fault == "ignore_out_pitch" else bm.out_base(olay, i0 + k)
            bm._window(out, base, olay.rows, olay.cols, olay.out_stride)[...] = res
        i0 += n
    return out


# ---- the colour quality scene ---------------------------------------------------------------------------------------------
# Three channels of S x S = 128 x 128: the 12 rectangles of _rltv_model.rect_scene (sides S/16 .. S/3, default_rng(3)) with ONE
# geometry and a level of its own per channel (uniform in 0.2 .. 1) on a 0.1 pedestal, scaled to max 1; every channel blurred
# circularly with the 15 px / 30 degree line_psf() centred at (0, 0) and given Poisson noise (default_rng(4), channel after channel)
# at `photons` per unit; restored by the plain form on the 128^2 plan, eps = 1e-3.  PSNR over the three channels against the truth.
# Measured with this model in float64, each form at its best lambda of QUALITY_GRID[photons] (dB; in brackets the lambda):
#   1000 photons, n = 100: channel-wise 28.161 (0.01),  coupled 28.329 (0.015):  gain 0.17 dB
#   1000 photons, n = 200: channel-wise 29.926 (0.01),  coupled 30.336 (0.0125): gain 0.41 dB
#    200 photons, n = 100: channel-wise 24.793 (0.02),  coupled 24.897 (0.025):  gain 0.10 dB
#    200 photons, n = 200: channel-wise 25.198 (0.02),  coupled 25.413 (0.025):  gain 0.22 dB
# The coupled optimum lies at a 1.25x to 1.5x larger lambda, and above its optimum the coupled form loses less: at 1000 photons,
# n = 200, lambda = 0.025 it gives 28.32 dB against 26.25 dB channel-wise; at 200 photons, n = 200, lambda = 0.03, 25.33 against 24.25.
# Below the optima the channel-wise form is ahead (lambda = 0.0075, 1000 photons, n = 200: 29.80 against 29.02): the joint norm
# weakens the prior at a given lambda.
QUALITY_S = 128
QUALITY_EPS = 1e-3
QUALITY_GRID = {1000.0: (0.0075, 0.01, 0.0125, 0.015, 0.02), 200.0: (0.015, 0.02, 0.025, 0.03)}
# (photons, iterations): (channel-wise best, coupled best) as measured; test_rltv_batch_host.py asserts coupled >= channel-wise and a gain
# of at least half the measured one
QUALITY_MEASURED = {(1000.0, 100): (28.161, 28.329), (1000.0, 200): (29.926, 30.336), (200.0, 100): (24.793, 24.897), (200.0, 200): (25.198, 25.413)}


def colour_scene(S=QUALITY_S, channels=3, seed=3):
    rng = np.random.default_rng(seed)
    img = np.full((channels, S, S), 0.1)
    for _ in range(12):
        h, w = rng.integers(S // 16, S // 3, 2)
        y, x = rng.integers(0, S - h), rng.integers(0, S - w)
        img[:, y:y + h, x:x + w] = rng.uniform(0.2, 1.0, channels)[:, None, None]
    return img / img.max()


def colour_quality_case(photons, S=QUALITY_S):
    """dict(truth [3, S, S], d (float32 [3, S, S]), psf (the centred PSF plane of the plan), M, N)"""
    scene = colour_scene(S)
    plane = centred_psf(line_psf(), S, S)
    Hc = np.fft.rfft2(plane.astype(np.float64))
    rng = np.random.default_rng(4)
    d = []
    for ch in scene:
        blurred = np.fft.irfft2(np.fft.rfft2(ch) * Hc, s=ch.shape)
        d.append(rng.poisson(np.maximum(blurred, 0) * photons) / photons)
    return dict(truth=scene, d=np.stack(d).astype(np.float32), psf=plane, M=S, N=S)


def colour_quality_run(case, iterations, lam, coupled, eps=QUALITY_EPS, dtype=np.float64):
    """{n: PSNR over the channels} of the plain form on a colour quality case for every n in `iterations` (one run to the largest)"""
    got = {}
    at = {n: (lambda us, n=n: got.__setitem__(n, psnr(np.stack(us), case["truth"]))) for n in iterations}
    H = op_spectrum(case["psf"], case["M"], case["N"])
    if coupled:
        group_run("plain", case["d"], case["psf"], case["M"], case["N"], max(iterations), lam, eps, coupled=True, dtype=dtype, H=H, at=at)
    else:  # channel after channel, each a group of one
        per = {n: [] for n in iterations}
        for ch in case["d"]:
            group_run("plain", [ch], case["psf"], case["M"], case["N"], max(iterations), lam, eps, dtype=dtype, H=H,
                      at={n: (lambda us, n=n: per[n].append(us[0])) for n in iterations})
        got = {n: psnr(np.stack(per[n]), case["truth"]) for n in iterations}
    return got
