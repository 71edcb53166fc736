"""Poisson-likelihood TV deconvolution (fdr_tv_deconv_poisson_f32*, its batches and the data step alone) on the MI355X.  The step
alone, bit for bit against the float32 model of tests/_tvpoisson_model.py (single launch and groups of 2, 3 and 8 with an odd pitch;
weights none / mask / fractional; b = 0 and b > 0; data with zeros and negatives; sentinels outside the window); the whole call for
n = 1, 2, 3 and n = 30, 100 against the float64 model; then bits (determinism, batch against single, coupled with one channel,
n = 0, what mu, b and the weights change), isolation from the other calls of a plan in both directions, the refusals, the pass
names, the workspace, restoration quality, the wrappers and the CLI.  Each case prints a `TVP` line with its measured values
(pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, dense_psf, psnr, rel_err
from _spectral import tone_image
from _tvpoisson_model import (QUALITY, SHORT, SHORT_IDS, TVP_TOL, WEIGHT_KINDS, finish, quality_case, short_combos, step_f32, tvf_weights,
                              tvp_image, tvpoisson_iterates, tvpoisson_model)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AREAS = (NORM_NONE, NORM_CROPPED, NORM_PADDED)
STEP_CASES, STEP_IDS = SHORT[:5], SHORT_IDS[:5]


def _strided(a, stride):
    """device copy of the window a with row stride `stride`, NaN between the rows: a read outside the window poisons the result"""
    import torch
    src = np.full((a.shape[0], stride), np.nan, dtype=np.float32)
    src[:, :a.shape[1]] = a
    return torch.from_numpy(src).cuda()


def _flat_windows(imgs, stride, pitch):
    """device copy of `count` windows, image i at i * pitch floats with row stride `stride`, NaN everywhere else"""
    import torch
    count, rows, cols = imgs.shape
    src = np.full(((count - 1) * pitch + rows * stride,), np.nan, dtype=np.float32)
    for i in range(count):
        for r in range(rows):
            src[i * pitch + r * stride: i * pitch + r * stride + cols] = imgs[i, r]
    return torch.from_numpy(src).cuda()


def _read_windows(d_out, count, shape, stride, pitch):
    """[count, shape] from the device, after checking that everything outside the windows is still NaN"""
    flat = d_out.cpu().numpy()
    seen = np.zeros(flat.shape, dtype=bool)
    outs = np.empty((count,) + tuple(shape), dtype=np.float32)
    for i in range(count):
        for r in range(shape[0]):
            at = i * pitch + r * stride
            outs[i, r] = flat[at:at + shape[1]]
            seen[at:at + shape[1]] = True
    assert np.all(np.isnan(flat[~seen])), "a store landed outside the output windows"
    return outs


# ---- 1. the step alone, bit for bit ---------------------------------------------------------------------------------------------------
def _step_planes(M, N, count, seed):
    """c = blur(x)-like and q planes with values everywhere: what lies outside the window is the sentinel that must come back"""
    rng = np.random.default_rng(seed)
    return (rng.normal(0.3, 0.4, (count, M, N)).astype(np.float32), rng.normal(0.0, 0.15, (count, M, N)).astype(np.float32))


@pytest.mark.parametrize("count", [1, 2, 3, 8])
@pytest.mark.parametrize("case", STEP_CASES, ids=STEP_IDS)
def test_step_bit_for_bit(fdr, case, count):
    """fdr_tv_poisson_step_f32_dev (count = 1) and fdr_tv_poisson_step_group_f32_dev (2, 3 and 8 images, an odd pitch of the data so
    that the images differ in 16-byte alignment, planes 4 floats apart with NaN between them) give the bits of step_f32, inside the
    window, and leave every float outside it as it was"""
    import torch
    M, N, rows, cols, stride, wstride = case[:6]
    P = M * N
    pitch = rows * stride + (1 if (rows * stride) % 2 == 0 else 2)  # odd
    cp = P + 4
    imgs = np.stack([tvp_image(M, N, rows, cols, 31 + 5 * i) * np.float32(1.0 + 0.2 * i) for i in range(count)])
    assert (imgs < 0).any() and (imgs == 0).any()
    c0, q0 = _step_planes(M, N, count, M + N + count)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:  # (the step needs no PSF)
        for kind in WEIGHT_KINDS:
            w = tvf_weights(kind, rows, cols, M + 3 * N)
            for mu, nu, b in ((50.0, 3.0, 0.0), (8.0, 2.0, 0.05)):
                d_in = _flat_windows(imgs, stride, pitch)
                d_w = _strided(w, wstride) if w is not None else None
                planes = []
                for src in (c0, q0):
                    flat = np.full(((count - 1) * cp + P,), np.nan, dtype=np.float32)
                    for i in range(count):
                        flat[i * cp:i * cp + P] = src[i].ravel()
                    planes.append(torch.from_numpy(flat).cuda())
                d_c, d_q = planes
                if count == 1:
                    p.tv_poisson_step_dev(d_c.data_ptr(), d_q.data_ptr(), d_in.data_ptr(), rows, cols, stride, mu, nu, b,
                                          d_w.data_ptr() if d_w is not None else None, wstride)
                else:
                    p.tv_poisson_step_group_dev(d_c.data_ptr(), cp, d_q.data_ptr(), cp, d_in.data_ptr(), pitch, count, rows, cols, stride, mu, nu, b,
                                                d_w.data_ptr() if d_w is not None else None, wstride)
                torch.cuda.synchronize()
                gc, gq = d_c.cpu().numpy(), d_q.cpu().numpy()
                for i in range(count):
                    wc, wq = step_f32(c0[i], q0[i], imgs[i], w, mu, nu, b)
                    what = (kind, mu, nu, b, i)
                    assert np.array_equal(gq[i * cp:i * cp + P].reshape(M, N), wq), ("q", what)
                    assert np.array_equal(gc[i * cp:i * cp + P].reshape(M, N), wc), ("c", what)
                    if i + 1 < count:
                        assert np.all(np.isnan(gc[i * cp + P:(i + 1) * cp])) and np.all(np.isnan(gq[i * cp + P:(i + 1) * cp])), "a store between the planes"
                    assert not np.array_equal(wc[:rows, :cols], c0[i][:rows, :cols])


def test_step_keeps_nan_data_nan_and_zero_weights_out(fdr):
    """a NaN in the data gives a NaN in s at that pixel alone; weight 0 makes the step s = e (q = 0, r = e) whatever the data hold"""
    import torch
    M, N, rows, cols = 8, 32, 7, 29
    img = tvp_image(M, N, rows, cols, 3)
    img[2, 5] = np.nan
    img[4, 7] = np.nan
    w = np.ones((rows, cols), dtype=np.float32)
    w[4, 7] = 0
    c0, q0 = _step_planes(M, N, 1, 1)
    d_c, d_q, d_in, d_w = (torch.from_numpy(a).cuda() for a in (c0[0], q0[0], img, w))
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.tv_poisson_step_dev(d_c.data_ptr(), d_q.data_ptr(), d_in.data_ptr(), rows, cols, cols, 20.0, 2.0, 0.01, d_w.data_ptr(), cols)
        torch.cuda.synchronize()
    gc, gq = d_c.cpu().numpy(), d_q.cpu().numpy()
    wc, wq = step_f32(c0[0], q0[0], img, w, 20.0, 2.0, 0.01)
    assert np.array_equal(gc, wc, equal_nan=True) and np.array_equal(gq, wq, equal_nan=True)
    assert np.isnan(gc[2, 5]) and np.isnan(gq[2, 5]) and np.isnan(gc).sum() == 1
    assert gq[4, 7] == 0 and gc[4, 7] == c0[0][4, 7] + q0[0][4, 7]


# ---- 2. the whole call against the float64 model --------------------------------------------------------------------------------------
def _dev_call(p, img, stride, weights, wstride, out_shape, out_stride, mu, rho, n, nu=0.0, b=0.0, aniso=False, nonneg=False, area=NORM_NONE):
    """Plan.tv_deconv_poisson_dev on device copies of img and weights (each with its own row stride); returns the output window after
    checking that nothing was stored outside it (NaN fence)"""
    import torch
    rows, cols = img.shape
    d_in = _strided(img, stride)
    d_w = _strided(weights, wstride) if weights is not None else None
    d_out = torch.full((out_shape[0], out_stride), float("nan"), dtype=torch.float32, device="cuda")
    p.tv_deconv_poisson_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), out_stride, mu, rho, n, d_w.data_ptr() if d_w is not None else None,
                            wstride, nu, b, aniso, nonneg, area, out_shape[0], out_shape[1])
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(np.isnan(out[:, out_shape[1]:])), "a store landed outside the output window"
    return out[:, :out_shape[1]]


def _planes(img, psf, M, N, mu, rho, nu, b, aniso, weights, ns):
    """{n: the M x N plane x of the float64 model after n iterations} from one run of the iteration"""
    out = {}
    for k, st in enumerate(tvpoisson_iterates(img, psf, M, N, mu, rho, max(ns), weights, nu, b, aniso)):
        if k in ns:
            out[k] = np.array(st["x"], dtype=np.float64)
    return out


def _error(got, want, area):
    return rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(got.astype(np.float64) - want)))


BACKGROUNDS = (0.0, 0.05, 0.3)  # of the motion, dense and delta combos of short_combos, in their order


def _run(fdr, case, ns, combos_of, kinds, areas=AREAS):
    M, N, rows, cols, stride, wstride, out_stride, outs = case
    img = tvp_image(M, N, rows, cols, M + 3 * N)
    bad, worst = [], 0.0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for (name, psf, mu, rho, nu, aniso, nonneg), b in zip(combos_of(fdr.motionBlurKernel(15, 30.0), M, N, rows, cols), BACKGROUNDS):
            p.set_operator_psf(psf)
            for kind in kinds:
                w = tvf_weights(kind, rows, cols, M + 3 * N)
                planes = _planes(img, psf, M, N, mu, rho, nu, b, aniso, w, ns)
                for n in ns:
                    for out_shape in outs:
                        for area in areas:
                            got = _dev_call(p, img, stride, w, wstride, out_shape, out_stride, mu, rho, n, nu, b, aniso, nonneg, area)
                            e = _error(got, finish(planes[n], out_shape, nonneg, area, M, N), area)
                            what = "%dx%d win %dx%d out %dx%d %s b=%g w=%s n=%d norm=%d" % (M, N, rows, cols, out_shape[0], out_shape[1], name, b, kind, n, area)
                            print("TVP\ttvpoisson\t%s\terr=%.3g" % (what, e))
                            worst = max(worst, e) if e == e else float("nan")
                            if not e <= TVP_TOL:
                                bad.append("%s: error %.3g > %.3g" % (what, e, TVP_TOL))
    print("TVP\tworst\t%dx%d win %dx%d n<=%d\t%.3g" % (M, N, rows, cols, max(ns), worst))
    return bad


@pytest.mark.parametrize("case", SHORT, ids=SHORT_IDS)
def test_short_against_model(fdr, case):
    bad = _run(fdr, case, (1, 2, 3), short_combos, WEIGHT_KINDS)
    assert not bad, "\n".join(bad)


LONG = [((64, 64, 60, 50, 53, 51, 67, ((60, 50), (64, 64))), ("none", "fractional")),
        ((512, 256, 500, 250, 251, 253, 256, ((500, 250),)), ("mask",))]


def _long_combos(motion, M, N, rows, cols):
    return short_combos(motion, M, N, rows, cols)[:2 if M * N <= 4096 else 1]


@pytest.mark.parametrize("case,kinds", LONG, ids=["64x64-win60x50", "512x256-win500x250-masked"])
def test_long_against_model(fdr, case, kinds):
    bad = _run(fdr, case, (30, 100), _long_combos, kinds, (NORM_NONE, NORM_PADDED))
    assert not bad, "\n".join(bad)


# ---- 3. bits --------------------------------------------------------------------------------------------------------------------------
def test_zero_iterations_return_the_padded_window(fdr):
    M, N, rows, cols = 16, 32, 9, 30
    img = tvp_image(M, N, rows, cols, 7)
    want = np.zeros((M, N), dtype=np.float32)
    want[:rows, :cols] = img
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(dense_psf(5, 5))
        assert np.array_equal(_dev_call(p, img, 31, None, 0, (M, N), 35, 10.0, 2.0, 0, b=0.1), want)
        assert np.array_equal(_dev_call(p, img, 31, None, 0, (rows, cols), 35, 10.0, 2.0, 0, nonneg=True), np.maximum(img, 0))
        assert np.array_equal(p.tv_deconv_poisson(img, 10.0, iterations=0, full_plane=True), want)


def test_bits(fdr):
    """two calls give the same bytes; all-ones weights give the bytes of no weights; the host form equals the _dev form; nu = 0 is
    nu = rho; mu, b and the weights each change the result by more than 1e-3"""
    M, N, rows, cols = 256, 512, 200, 301
    img = tvp_image(M, N, rows, cols, 5)
    w = tvf_weights("fractional", rows, cols, 5)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(centred_psf(fdr.motionBlurKernel(15, 30.0), M, N))
        for wt in (None, w):
            a = p.tv_deconv_poisson(img, 20.0, 2.0, 7, wt, 3.0, 0.05, False, True, NORM_PADDED, True)
            assert np.array_equal(a, p.tv_deconv_poisson(img, 20.0, 2.0, 7, wt, 3.0, 0.05, False, True, NORM_PADDED, True)), "two runs differ"
            dev = _dev_call(p, img, 303, wt, 305, (M, N), N + 1, 20.0, 2.0, 7, 3.0, 0.05, False, True, NORM_PADDED)
            assert np.array_equal(a, dev), "host and _dev forms differ"
        none = p.tv_deconv_poisson(img, 20.0, 2.0, 7, background=0.05)
        ones = np.ones((rows, cols), dtype=np.float32)
        assert np.array_equal(p.tv_deconv_poisson(img, 20.0, 2.0, 7, ones, background=0.05), none), "all-ones weights are not the bytes of no weights"
        assert np.array_equal(p.tv_deconv_poisson(img, 20.0, 2.0, 7, nu=2.0, background=0.05), none), "nu = 0 is not nu = rho"
        for what, other in (("mu", p.tv_deconv_poisson(img, 40.0, 2.0, 7, background=0.05)), ("b", p.tv_deconv_poisson(img, 20.0, 2.0, 7)),
                            ("weights", p.tv_deconv_poisson(img, 20.0, 2.0, 7, w, background=0.05)),
                            ("the step", p.tv_deconv_free(img, 20.0, 2.0, 7))):
            e = rel_err(other, none)
            print("TVP\tbits\tanother %s moves the result by %.3g" % (what, e))
            assert e > 1e-3, what


def _single(p, d_in, i, pitch, rows, cols, stride, d_w, wstride, out_shape, out_stride, mu, rho, n, nu, b, aniso, nonneg, area):
    import torch
    d_out = torch.full((out_shape[0] * out_stride,), float("nan"), dtype=torch.float32, device="cuda")
    p.tv_deconv_poisson_dev(d_in.data_ptr() + 4 * i * pitch, rows, cols, stride, d_out.data_ptr(), out_stride, mu, rho, n,
                            d_w.data_ptr() if d_w is not None else None, wstride, nu, b, aniso, nonneg, area, out_shape[0], out_shape[1])
    torch.cuda.synchronize()
    return _read_windows(d_out, 1, out_shape, out_stride, 0)[0]


@pytest.mark.parametrize("group", [1, 3, 4, 8])
def test_batch_uncoupled_has_the_bits_of_the_single_call(fdr, group):
    """5 images in groups of 1, 3 (3 + 2), 4 (4 + 1) and 8: every image has the bits of the single _dev call on the same plan, with an odd
    loose pitch (the images differ in 16-byte alignment), odd strides, the three weights, both shrinkages, the three norm_area values
    and the M x N output window; and the coupled form on one channel is the single call too"""
    import torch
    M, N, rows, cols, stride, wstride, out_stride = 64, 128, 37, 101, 103, 101, 131
    count, n = 5, 2
    pitch = rows * stride + 2  # odd
    imgs = np.stack([tvp_image(M, N, rows, cols, 11 + 7 * i) * np.float32(1.0 - 0.1 * i) for i in range(count)])
    d_in = _flat_windows(imgs, stride, pitch)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(centred_psf(fdr.motionBlurKernel(15, 30.0), M, N))
        for kind, aniso, area, out_shape, b in (("none", False, NORM_NONE, (rows, cols), 0.0), ("mask", True, NORM_CROPPED, (M, N), 0.05),
                                                ("fractional", False, NORM_PADDED, (rows, cols), 0.3)):
            w = tvf_weights(kind, rows, cols, 3)
            d_w = _strided(w, wstride) if w is not None else None
            opitch = out_shape[0] * out_stride + 3
            p.set_batching(1, group)
            d_out = torch.full(((count - 1) * opitch + out_shape[0] * out_stride,), float("nan"), dtype=torch.float32, device="cuda")
            p.tv_deconv_poisson_batch_dev(d_in.data_ptr(), pitch, count, rows, cols, stride, d_out.data_ptr(), opitch, out_stride, 30.0, 2.0, n,
                                          d_w.data_ptr() if d_w is not None else None, wstride, 3.0, b, aniso, True, area, out_shape[0], out_shape[1])
            torch.cuda.synchronize()
            got = _read_windows(d_out, count, out_shape, out_stride, opitch)
            p.set_batching(1, 1)
            for i in range(count):
                want = _single(p, d_in, i, pitch, rows, cols, stride, d_w, wstride, out_shape, out_stride, 30.0, 2.0, n, 3.0, b, aniso, True, area)
                assert np.array_equal(got[i], want), (kind, i, float(np.abs(got[i] - want).max()))
            assert not np.array_equal(got[0], got[1])
            if not aniso:
                p.set_batching(1, group)
                d_one = torch.full((out_shape[0] * out_stride,), float("nan"), dtype=torch.float32, device="cuda")
                p.tv_deconv_poisson_batch_dev(d_in.data_ptr() + 4 * pitch, pitch, 1, rows, cols, stride, d_one.data_ptr(), opitch, out_stride, 30.0, 2.0,
                                              n, d_w.data_ptr() if d_w is not None else None, wstride, 3.0, b, False, True, area, out_shape[0],
                                              out_shape[1], True)
                torch.cuda.synchronize()
                assert np.array_equal(_read_windows(d_one, 1, out_shape, out_stride, 0)[0], got[1]), "coupled, one channel"
                p.set_batching(1, 1)


# ---- 4. isolation -----------------------------------------------------------------------------------------------------------------------
def test_isolation_both_ways(fdr):
    """Wiener, blur, RL, periodic TV, free TV and auto TV give the same bytes on one plan before and after Poisson calls, also after a
    grouped Poisson call has grown the workspaces; the Poisson calls give the same bytes before and after them"""
    M, N = 256, 512
    img = tone_image(M, N, 21)
    pos = np.clip(img, 0, None) + np.float32(0.05)
    win = np.ascontiguousarray(pos[:150, :350])
    w = tvf_weights("mask", 150, 350, 1)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(25, 123.4)

        def others():
            p.set_psf_motion(15, 30.0, 0.01)
            return [p.wiener(img), p.blur(img), p.blur(img, adjoint=True), p.richardson_lucy(pos, 4), p.tv_deconv(img, 2.0, 2.0, 3),
                    p.tv_deconv_free(win, 100.0, 2.0, 3, w, 0.0, False, True, NORM_PADDED, True), p.tv_deconv_free(win, 100.0, 2.0, 2, None, 7.0, True),
                    p.tv_deconv_auto(win, 0.02, 2.0, 3, w)[0]]

        def poisson_calls():
            return [p.tv_deconv_poisson(win, 20.0, 2.0, 4, w, 0.0, 0.05, False, True, NORM_PADDED, True),
                    p.tv_deconv_poisson(win, 20.0, 2.0, 3, None, 7.0, 0.0, True), p.tv_deconv_poisson(pos, 8.0, 10.0, 2)]

        before = others()
        pois0 = poisson_calls()
        after = others()
        pois1 = poisson_calls()
        p.set_batching(1, 3)  # the workspaces grow to three images
        grouped = p.tv_deconv_poisson_batch(np.stack([win, win[::-1], win[:, ::-1]]), 20.0, 2.0, 3, None, 7.0, 0.0, True)
        p.set_batching(1, 1)
        grown = others()
        pois2 = poisson_calls()
        for k, (x, y, z) in enumerate(zip(before, after, grown)):
            assert np.array_equal(x, y), "call %d changed after the Poisson calls" % k
            assert np.array_equal(x, z), "call %d changed after the workspaces grew" % k
        for k, (x, y, z) in enumerate(zip(pois0, pois1, pois2)):
            assert np.array_equal(x, y) and np.array_equal(x, z), "Poisson call %d changed after the other calls" % k
        assert np.array_equal(grouped[0], pois0[1])
    with fdr.Plan(M, N, fdr.MODE_FAST) as q:  # and each is what a fresh plan gives
        q.set_operator_psf_motion(25, 123.4)
        assert np.array_equal(q.tv_deconv_poisson(pos, 8.0, 10.0, 2), pois0[2])
        assert np.array_equal(q.tv_deconv_free(win, 100.0, 2.0, 2, None, 7.0, True), before[6])


# ---- 5. refusals, passes, allocations -------------------------------------------------------------------------------------------------
def _census(p):
    return {name: c for name, _, c in p.pass_times() if c}


def test_refusals(fdr):
    """every refusal returns its code with an empty launch census and the output untouched; a valid call then gives the bytes it gave
    before"""
    import torch
    L = fdr.lib
    M = N = 64
    rows, cols, count = 40, 48, 3
    px = rows * cols
    psf = dense_psf(5, 5)
    imgs = np.stack([tvp_image(M, N, rows, cols, 3 + i) for i in range(count)])
    wts = tvf_weights("fractional", rows, cols, 3)
    d = torch.from_numpy(imgs).cuda()
    dw = torch.from_numpy(wts).cuda()
    do = torch.full((count, rows, cols), 7.0, dtype=torch.float32, device="cuda")
    dc = torch.full((count, M, N), 7.0, dtype=torch.float32, device="cuda")
    dq = torch.full((count, M, N), 7.0, dtype=torch.float32, device="cuda")
    nan, inf = float("nan"), float("inf")

    def single(p, i=d.data_ptr(), w=dw.data_ptr(), o=do.data_ptr(), rows=rows, cols=cols, stride=cols, wstride=cols, out_stride=cols, mu=10.0, rho=2.0,
               nu=0.0, b=0.05, n=1, aniso=0, area=0, out_rows=rows, out_cols=cols, prm=True, plan=True, **_):
        q = fdr.TvPoissonParams(mu, rho, nu, b, n, aniso, 0, area, out_rows, out_cols)
        return L.fdr_tv_deconv_poisson_f32_dev(p._h if plan else None, i, rows, cols, stride, w, wstride, o, out_stride, ctypes.byref(q) if prm else None, None)

    def batch(p, i=d.data_ptr(), w=dw.data_ptr(), o=do.data_ptr(), count=count, rows=rows, cols=cols, stride=cols, wstride=cols, out_stride=cols, pitch=px,
              opitch=px, mu=10.0, rho=2.0, nu=0.0, b=0.05, n=1, aniso=0, area=0, out_rows=rows, out_cols=cols, coupling=0, prm=True, plan=True):
        q = fdr.TvPoissonBatchParams(mu, rho, nu, b, n, aniso, 0, area, out_rows, out_cols, coupling)
        return L.fdr_tv_deconv_poisson_batch_f32_dev(p._h if plan else None, i, pitch, count, rows, cols, stride, w, wstride, o, opitch, out_stride,
                                                     ctypes.byref(q) if prm else None, None)

    def step(p, c=dc.data_ptr(), q=dq.data_ptr(), i=d.data_ptr(), w=dw.data_ptr(), rows=rows, cols=cols, stride=cols, wstride=cols, mu=10.0, nu=2.0, b=0.05,
             count=None, cp=M * N, qp=M * N, pitch=px, plan=True):
        h = p._h if plan else None
        if count is None:
            return L.fdr_tv_poisson_step_f32_dev(h, c, q, i, rows, cols, stride, w, wstride, mu, nu, b, None)
        return L.fdr_tv_poisson_step_group_f32_dev(h, c, cp, q, qp, i, pitch, count, rows, cols, stride, w, wstride, mu, nu, b, None)

    common = (dict(plan=False), dict(prm=False), dict(i=None), dict(o=None), dict(mu=0.0), dict(mu=-1.0), dict(mu=nan), dict(mu=inf), dict(rho=0.0),
              dict(rho=nan), dict(nu=-1.0), dict(nu=inf), dict(b=-0.01), dict(b=nan), dict(b=inf), dict(n=-1), dict(area=3), dict(rows=65), dict(rows=0),
              dict(stride=cols - 1), dict(wstride=cols - 1), dict(out_stride=cols - 1), dict(out_rows=rows - 1), dict(out_cols=cols - 1), dict(out_rows=M + 1),
              dict(o=d.data_ptr()), dict(o=dw.data_ptr()))
    batch_only = (dict(count=-1), dict(coupling=2), dict(coupling=-1), dict(coupling=1, aniso=1), dict(coupling=1, count=3),  # (the group is 2)
                  dict(o=d.data_ptr() + 4 * (2 * px + 5)), dict(i=do.data_ptr() + 4 * px), dict(w=do.data_ptr() + 4 * (2 * px + 8)))
    steps = (dict(plan=False), dict(c=None), dict(q=None), dict(i=None), dict(rows=65), dict(cols=0), dict(stride=cols - 1), dict(wstride=cols - 1),
             dict(mu=0.0), dict(mu=nan), dict(nu=0.0), dict(nu=nan), dict(nu=-2.0), dict(b=-1.0), dict(b=inf), dict(c=dc.data_ptr() + 4), dict(q=dq.data_ptr() + 8),
             dict(q=dc.data_ptr()), dict(i=dc.data_ptr()), dict(w=dq.data_ptr()))
    group_steps = (dict(count=0), dict(count=9), dict(count=3, cp=M * N - 4), dict(count=3, qp=M * N + 2), dict(count=2, q=dc.data_ptr() + 4 * M * N))

    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 2)
        assert single(p) == -4 and b"operator PSF" in L.fdr_last_error()
        p.set_operator_psf(psf)
        good = p.tv_deconv_poisson(imgs[0], 10.0, 2.0, 3, wts, 0.0, 0.05, full_plane=True)
        good_b = p.tv_deconv_poisson_batch(imgs, 10.0, 2.0, 2, wts, 0.0, 0.05)
        p.profile(True)
        p.pass_times()  # (read: the counts start again)
        for fn, cases in ((single, common), (batch, common + batch_only)):
            for kw in cases:
                assert fn(p, **kw) == -1, (fn.__name__, kw)
                assert fdr.lib.fdr_last_error()
        for kw in steps:
            assert step(p, **kw) == -1, ("step", kw)
        for kw in steps + group_steps:
            assert step(p, **dict(dict(count=2), **kw)) == -1, ("step group", kw)
        torch.cuda.synchronize()
        assert _census(p) == {}, "a refused call launched something"
        p.profile(False)
        for t in (do, dc, dq):
            assert bool((t == 7.0).all()), "a refused call wrote"
        assert batch(p, count=0) == 0 and bool((do == 7.0).all())
        assert single(p, w=None, wstride=0) == 0 and batch(p, coupling=1, count=2) == 0  # no weights: their stride does not matter
        assert step(p) == 0 and step(p, count=3) == 0 and step(p, w=None, wstride=0, b=0.0) == 0
        torch.cuda.synchronize()
        assert np.array_equal(p.tv_deconv_poisson(imgs[0], 10.0, 2.0, 3, wts, 0.0, 0.05, full_plane=True), good)
        assert np.array_equal(p.tv_deconv_poisson_batch(imgs, 10.0, 2.0, 2, wts, 0.0, 0.05), good_b)
        with pytest.raises(fdr.FdrError):
            p.tv_deconv_poisson(imgs[0], 10.0, background=-1.0)
        with pytest.raises(ValueError):
            p.tv_deconv_poisson(imgs[0], 10.0, weights=wts[:-1])
        want = tvpoisson_model(imgs[0], psf, M, N, 10.0, 2.0, 3, wts, 0.0, 0.05, out_shape=(M, N))
        assert rel_err(good, want) <= TVP_TOL
    for PM, PN, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (75, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX, "mixed radix")):
        with fdr.Plan(PM, PN, mode, flags=flags) as p:
            assert single(p, rows=8, cols=8, stride=8, wstride=8, out_stride=8, out_rows=8, out_cols=8) == -1, what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert single(p) == -4


def test_pass_names(fdr):
    """a fresh profiled plan holds every pass of a Poisson call: the free call's, with the data step under its own name"""
    with fdr.Plan(256, 512, fdr.MODE_FAST) as p:
        p.profile(True)
        p.set_operator_psf_motion(15, 30.0)
        img = np.clip(tone_image(256, 512, 1, 200, 300), 0, None)
        p.tv_deconv_poisson(img, 50.0, 2.0, 3, None, 0.0, 0.05, False, True, NORM_PADDED)
        p.tv_deconv_poisson(img, 50.0, 2.0, 2, tvf_weights("mask", 200, 300, 1))
        names = _census(p)
        p.set_batching(1, 3)
        p.tv_deconv_poisson_batch(np.stack([img, img, img]), 50.0, 2.0, 2, coupled=True)
        coupled = _census(p)
    print("TVP\tpasses\t%s" % names)
    data = "TVP data: Poisson s, q, r = 2s-e (window)"
    assert len(names) <= fdr.MAX_PASSES and len(set(names) | set(coupled)) <= fdr.MAX_PASSES
    want = {"O rows: PSF pad+FFT (operator)": 1, "O cols: FFT -> H/MN, conj(H)/MN": 1, "TV table: 1/(nu|H|^2+rho L)/MN (free)": 1,
            "TVF init: x = pad(d), w = q = 0": 2, data: 5, "TV spatial: shrink+dual+div (free)": 5,
            "A op rows: pad+FFT (blur / RL)": 15, "B' op cols: FFT*H*IFFT": 5, "B' op cols: FFT*conj(H)*IFFT": 5, "C op rows: IFFT+crop (blur)": 10,
            "B' op cols: FFT*T*IFFT (TVF solve)": 5, "C op rows: IFFT (TVF x)": 5, "TVF out: crop+clamp": 2, "E TVF minmax+normalize": 1}
    for n, c in want.items():
        assert names.get(n) == c, (n, names.get(n), c)
    assert set(names) == set(want), set(names) ^ set(want)
    assert not any(n.startswith("TVF data") for n in list(names) + list(coupled))
    assert coupled.get(data) == 2 and coupled.get("TV spatial: joint shrink+dual+div (free)") == 2, coupled


def test_second_call_allocates_nothing(fdr):
    import torch
    M, N, rows, cols = 1024, 1024, 1000, 900
    img = np.clip(tvp_image(M, N, rows, cols, 2), 0, None)
    d_in = torch.from_numpy(img).cuda()
    d_w = torch.from_numpy(tvf_weights("mask", rows, cols, 2)).cuda()
    d_out = torch.empty((M, N), dtype=torch.float32, device="cuda")
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0)
        f0 = torch.cuda.mem_get_info()[0]
        p.tv_deconv_poisson_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 50.0, 2.0, 2)
        torch.cuda.synchronize()
        f1 = torch.cuda.mem_get_info()[0]
        p.tv_deconv_poisson_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 70.0, 3.0, 2, d_w.data_ptr(), cols, 5.0, 0.1, True, True, NORM_PADDED, M, N)
        p.tv_deconv_free_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 50.0, 2.0, 1)  # (the free call's workspaces are these)
        p.tv_deconv_poisson_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 50.0, 2.0, 2)
        torch.cuda.synchronize()
        f2 = torch.cuda.mem_get_info()[0]
    print("TVP\tallocations\tfirst call %d bytes, later calls %d bytes" % (f0 - f1, f1 - f2))
    assert f0 - f1 >= 8 * 4 * M * N, "the first call did not allocate the free call's workspaces"
    assert f1 == f2, "a later call allocated device memory"


# ---- 6. quality ---------------------------------------------------------------------------------------------------------------------------
def test_restoration_quality(fdr):
    """the scenes of test_tvpoisson_host.py at their best mu of the grid: the device is within TVP_TOL of the model, so the margins
    pinned on the CPU hold for it; the coupled form on a three-channel version runs and stays finite"""
    q = QUALITY
    with fdr.Plan(q["M"], q["N"], fdr.MODE_FAST) as p:
        for photons, mu in ((100, 8.0), (1000, 16.0)):
            c = quality_case(photons)
            p.set_operator_psf(c["psf"])
            model = tvpoisson_model(c["d"], c["psf"], q["M"], q["N"], mu, q["rho"], q["n"], None, q["nu"], 0.0, False, True)
            got = p.tv_deconv_poisson(c["d"], mu, q["rho"], q["n"], None, q["nu"], 0.0, False, True)
            free = p.tv_deconv_free(c["d"], 4 * mu if photons == 100 else 8 * mu, q["rho"], q["n"], None, q["nu"], False, True)
            pm, pg, pf = psnr(model, c["truth"]), psnr(got, c["truth"]), psnr(free, c["truth"])
            print("TVP\tquality\t%d photons mu %g n=%d\tmodel %.3f dB, GPU %.3f dB, rel=%.3g (blurred noisy crop %.2f dB, free TV on the GPU at its best mu %.2f dB)"
                  % (photons, mu, q["n"], pm, pg, rel_err(got, model), psnr(c["d"], c["truth"]), pf))
            assert rel_err(got, model) <= TVP_TOL and abs(pg - pm) <= 0.02
            assert pg >= pf + (0.95 if photons == 100 else 0.61)
        c = quality_case(100)
        chans = np.stack([c["d"], c["d"] * np.float32(0.8), c["d"][::-1] * np.float32(0.6)])
        p.set_batching(1, 3)
        out = p.tv_deconv_poisson_batch(chans, 8.0, q["rho"], 30, None, q["nu"], 0.0, False, True, coupled=True)
        alone = p.tv_deconv_poisson_batch(chans, 8.0, q["rho"], 30, None, q["nu"], 0.0, False, True)
        assert np.all(np.isfinite(out)) and out.min() >= 0 and rel_err(out, alone) > 1e-3


# ---- 7. wrappers and the CLI ----------------------------------------------------------------------------------------------------------
def test_python_wrappers(fdr):
    """tvDeblurPoisson_myfft equals the Plan call on the _rlfree_plan_size plan; tvDeblurPoisson_RGB equals the per-channel loop"""
    img = np.clip(tvp_image(512, 1024, 300, 700, 2), 0, None)
    psf = fdr.motionBlurKernel(15, 30.0)
    w = tvf_weights("mask", 300, 700, 2)
    assert fdr._rlfree_plan_size(300, 700, 15, 15) == (512, 1024)
    chans = [np.ascontiguousarray(img[::-1]), img, np.ascontiguousarray(img[:, ::-1])]
    with fdr.Plan(512, 1024, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        want = p.tv_deconv_poisson(img, 20.0, 2.0, 3, w, 0.0, 0.05, False, True)
        full = p.tv_deconv_poisson(img, 20.0, 2.0, 3, None, 4.0, 0.0, True, False, NORM_CROPPED, True)
        rgb_want = [p.tv_deconv_poisson(c, 20.0, 2.0, 3, w, 0.0, 0.05, False, True, NORM_PADDED) for c in chans]
        p.set_batching(1, 3)
        coupled_want = p.tv_deconv_poisson_batch(np.stack(chans), 20.0, 2.0, 3, w, 0.0, 0.05, False, True, NORM_PADDED, False, True)
    assert np.array_equal(fdr.tvDeblurPoisson_myfft(img, psf, 20.0, iterations=3, weights=w, background=0.05, nonneg=True), want)
    assert np.array_equal(fdr.tvDeblurPoisson_myfft(img, psf, 20.0, 2.0, 3, None, 4.0, 0.0, True, False, 0, NORM_CROPPED, True), full)
    e = rel_err(want, tvpoisson_model(img, psf, 512, 1024, 20.0, 2.0, 3, w, 0.0, 0.05, nonneg=True))
    print("TVP\ttvDeblurPoisson_myfft\t300x700 in 512x1024\terr=%.3g" % e)
    assert e <= TVP_TOL
    rgb = list(chans)
    fdr.tvDeblurPoisson_RGB(rgb, psf, 20.0, iterations=3, nonneg=True, norm_area=NORM_PADDED, weights=w, background=0.05)
    for k in range(3):
        assert np.array_equal(rgb[k], rgb_want[k]), k
    rgb = list(chans)
    fdr.tvDeblurPoisson_RGB(rgb, psf, 20.0, iterations=3, nonneg=True, norm_area=NORM_PADDED, weights=w, background=0.05, coupled=True)
    assert np.array_equal(np.stack(rgb), coupled_want) and not np.array_equal(rgb[0], rgb_want[0])


def test_cpp_wrapper(fdr, tmp_path):
    """fft_gpu::tvDeblurPoisson_RGB (tools/cli/poisson_shim_test) equals the batched call it is defined by, uncoupled and coupled"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "poisson_shim_test"])
    exe = os.path.join(ROOT, "tools", "cli", "poisson_shim_test")
    rows, cols = 100, 180
    chans = np.stack([np.clip(tvp_image(128, 256, rows, cols, 40 + i), 0, None) for i in range(3)])
    src = str(tmp_path / "in.f32")
    chans.tofile(src)
    M, N = fdr._rlfree_plan_size(rows, cols, 9, 9)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(fdr.motionBlurKernel(9, 20.0))
        p.set_batching(1, 3)
        for coupled in (0, 1):
            out = str(tmp_path / ("out%d.f32" % coupled))
            r = subprocess.run([exe, src, str(rows), str(cols), "9", "20", "12.5", "4", "3", "0.05", str(coupled), out], capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            want = p.tv_deconv_poisson_batch(chans, 12.5, 3.0, 4, None, 0.0, 0.05, False, True, NORM_PADDED, False, bool(coupled))
            assert np.array_equal(np.fromfile(out, dtype=np.float32).reshape(3, rows, cols), want), coupled


def test_cli_tv_poisson(fdr, tmp_path):
    """tools/cli/gpu --tv mu --poisson [--background b] [--mask m.png] [--tv-color]: the planes (--raw-out) equal the Python path --
    three tv_deconv_poisson(..., nonneg, NORM_PADDED) calls with the mask's weights on the plan tvDeblurPoisson_myfft uses, or with
    --tv-color the coupled batch"""
    from PIL import Image
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")
    png = os.path.join(ROOT, "tests", "golden", "car_blurred.png")
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    keep = np.random.default_rng(8).random((h, w)) >= 0.02
    mask_png = str(tmp_path / "mask.png")
    Image.fromarray(np.repeat((keep * np.uint8(255))[:, :, None], 3, axis=2).astype(np.uint8), "RGB").save(mask_png)
    outs = {}
    for tag, extra in (("masked", ["--mask", mask_png, "--background", "0.02"]), ("plain", []), ("colour", ["--tv-color", "--background", "0.02"])):
        out_raw = str(tmp_path / (tag + ".f32"))
        r = subprocess.run([gpu, png, "40", "45", "--tv", "30", "--tv-iters", "8", "--poisson"] + extra + ["--raw-out", out_raw,
                            "--out", str(tmp_path / (tag + ".png"))], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Deblurring 3 channels took(gpu[total-variation poisson mu 30 background " in r.stdout, r.stdout
        outs[tag] = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
    M, N = fdr._rlfree_plan_size(h, w, 40, 40)
    bgr = [np.ascontiguousarray(rgb[:, :, c]) for c in (2, 1, 0)]
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(fdr.motionBlurKernel(40, 45.0))
        for tag, wt, b in (("masked", keep.astype(np.float32), 0.02), ("plain", None, 0.0)):
            for k in range(3):
                want = p.tv_deconv_poisson(bgr[k], 30.0, 2.0, 8, wt, 0.0, b, False, True, fdr.NORM_PADDED)
                assert np.array_equal(outs[tag][k], want), (tag, k, float(np.abs(outs[tag][k] - want).max()))
        p.set_batching(1, 3)
        want = p.tv_deconv_poisson_batch(np.stack(bgr), 30.0, 2.0, 8, None, 0.0, 0.02, False, True, fdr.NORM_PADDED, False, True)
        assert np.array_equal(outs["colour"], want)
    assert not np.array_equal(outs["masked"], outs["plain"]) and not np.array_equal(outs["colour"], outs["plain"])
