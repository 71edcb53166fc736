"""Free-boundary, weighted TV deconvolution (fdr_tv_deconv_free_f32*) on the MI355X against the float64 model of
tests/_tvfree_model.py: 1 .. 3 iterations on the short cases (windows of every column residue mod 4, odd strides of the image, the
weights and the output, the window equal to the plan and one row and three columns short of it, the window and the whole plan as
output), with no weights, a 0 / 1 mask and fractional weights, both shrinkages, nonneg, every norm_area and motion / dense / delta
PSFs; 30 and 100 iterations; then bits (determinism, all-ones weights, host against _dev form, isolation from the other calls of a
plan in both directions, the shared solve table), restoration quality, the refusals, the pass names, the workspace, the wrappers and
the CLI.  Each case prints a `TVF` line with its measured values (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, dense_psf, psnr, rel_err
from _spectral import tone_image
from _tvfree_model import (QUALITY, SHORT, SHORT_IDS, TVF_TOL, WEIGHT_KINDS, finish, quality_case, short_combos, tvf_image, tvf_weights,
                           tvfree_iterates, tvfree_model)

pytestmark = pytest.mark.gpu

AREAS = (NORM_NONE, NORM_CROPPED, NORM_PADDED)


def _strided(a, stride):
    """device copy of the window a with row stride `stride`, NaN between the rows: a read outside the window poisons the result"""
    import torch
    src = np.full((a.shape[0], stride), np.nan, dtype=np.float32)
    src[:, :a.shape[1]] = a
    return torch.from_numpy(src).cuda()


def _dev_call(p, img, stride, weights, wstride, out_shape, out_stride, mu, rho, n, nu=0.0, aniso=False, nonneg=False, area=NORM_NONE):
    """Plan.tv_deconv_free_dev on device copies of img and weights (each with its own row stride); returns the output window after
    checking that nothing was stored outside it (NaN fence)"""
    import torch
    rows, cols = img.shape
    d_in = _strided(img, stride)
    d_w = _strided(weights, wstride) if weights is not None else None
    d_out = torch.full((out_shape[0], out_stride), float("nan"), dtype=torch.float32, device="cuda")
    p.tv_deconv_free_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), out_stride, mu, rho, n, d_w.data_ptr() if d_w is not None else None,
                         wstride, nu, aniso, nonneg, area, out_shape[0], out_shape[1])
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(np.isnan(out[:, out_shape[1]:])), "a store landed outside the output window"
    return out[:, :out_shape[1]]


def _planes(img, psf, M, N, mu, rho, nu, aniso, weights, ns):
    """{n: the M x N plane x of the float64 model after n iterations} from one run of the iteration"""
    out = {}
    for k, st in enumerate(tvfree_iterates(img, psf, M, N, mu, rho, max(ns), weights, nu, aniso)):
        if k in ns:
            out[k] = np.array(st["x"], dtype=np.float64)
    return out


def _error(got, want, area):
    return rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(got.astype(np.float64) - want)))


def _run(fdr, case, ns, combos_of, kinds, areas=AREAS):
    M, N, rows, cols, stride, wstride, out_stride, outs = case
    img = tvf_image(M, N, rows, cols, M + 3 * N)
    bad, worst = [], 0.0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for name, psf, mu, rho, nu, aniso, nonneg in combos_of(fdr.motionBlurKernel(15, 30.0), M, N, rows, cols):
            p.set_operator_psf(psf)
            for kind in kinds:
                w = tvf_weights(kind, rows, cols, M + 3 * N)
                planes = _planes(img, psf, M, N, mu, rho, nu, aniso, w, ns)
                for n in ns:
                    for out_shape in outs:
                        for area in areas:
                            got = _dev_call(p, img, stride, w, wstride, out_shape, out_stride, mu, rho, n, nu, aniso, nonneg, area)
                            e = _error(got, finish(planes[n], out_shape, nonneg, area, M, N), area)
                            what = "%dx%d win %dx%d out %dx%d %s w=%s n=%d norm=%d" % (M, N, rows, cols, out_shape[0], out_shape[1], name, kind, n, area)
                            print("TVF\ttvfree\t%s\terr=%.3g" % (what, e))
                            worst = max(worst, e) if e == e else float("nan")
                            if not e <= TVF_TOL:
                                bad.append("%s: error %.3g > %.3g" % (what, e, TVF_TOL))
    print("TVF\tworst\t%dx%d win %dx%d n<=%d\t%.3g" % (M, N, rows, cols, max(ns), worst))
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
    bad = _run(fdr, case, (0, 30, 100), _long_combos, kinds, (NORM_NONE, NORM_PADDED))
    assert not bad, "\n".join(bad)


def test_zero_iterations_return_the_padded_window(fdr):
    """iterations = 0: pad(d) on the output window, zeros beyond the input window, clamped with nonneg; no operator pass runs"""
    M, N, rows, cols = 16, 32, 9, 30
    img = tvf_image(M, N, rows, cols, 7) - np.float32(0.3)
    assert (img < 0).any() and (img > 0).any()
    want = np.zeros((M, N), dtype=np.float32)
    want[:rows, :cols] = img
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(dense_psf(5, 5))
        assert np.array_equal(_dev_call(p, img, 31, None, 0, (M, N), 35, 10.0, 2.0, 0), want)
        assert np.array_equal(_dev_call(p, img, 31, None, 0, (rows, cols), 35, 10.0, 2.0, 0, nonneg=True), np.maximum(img, 0))
        assert np.array_equal(p.tv_deconv_free(img, 10.0, iterations=0, full_plane=True), want)


def test_bits(fdr):
    """two calls give the same bytes; all-ones weights give the bytes of no weights; the host form equals the _dev form"""
    M, N, rows, cols = 256, 512, 200, 301
    img = tvf_image(M, N, rows, cols, 5)
    w = tvf_weights("fractional", rows, cols, 5)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(centred_psf(fdr.motionBlurKernel(15, 30.0), M, N))
        for wt in (None, w):
            a = p.tv_deconv_free(img, 100.0, 2.0, 7, wt, 3.0, False, True, NORM_PADDED, True)
            assert np.array_equal(a, p.tv_deconv_free(img, 100.0, 2.0, 7, wt, 3.0, False, True, NORM_PADDED, True)), "two runs differ"
            dev = _dev_call(p, img, 303, wt, 305, (M, N), N + 1, 100.0, 2.0, 7, 3.0, False, True, NORM_PADDED)
            assert np.array_equal(a, dev), "host and _dev forms differ"
        none = p.tv_deconv_free(img, 100.0, 2.0, 7)
        ones = np.ones((rows, cols), dtype=np.float32)
        assert np.array_equal(p.tv_deconv_free(img, 100.0, 2.0, 7, ones), none), "all-ones weights are not the bytes of no weights"
        assert np.array_equal(_dev_call(p, img, 303, ones, 304, (rows, cols), 301, 100.0, 2.0, 7), none)
        assert np.array_equal(p.tv_deconv_free(img, 100.0, 2.0, 7, nu=2.0), none), "nu = 0 is not nu = rho"
        assert rel_err(p.tv_deconv_free(img, 100.0, 2.0, 7, w), none) > 1e-3 and rel_err(p.tv_deconv_free(img, 100.0, 2.0, 7, nu=5.0), none) > 1e-3


def test_isolation_both_ways(fdr):
    """Wiener, CLS, blur, plain RL, free RL, periodic TV and the motion estimate give the same bytes before and after free TV calls on
    one plan, and free TV gives the same bytes before and after them -- periodic TV with the free call's nu as its mu, and with another
    mu and rho, among them: the solve table is shared"""
    M, N = 512, 1024
    img = tone_image(M, N, 21)
    pos = np.clip(img, 0, None) + np.float32(0.05)
    win = np.ascontiguousarray(img[:300, :700])
    w = tvf_weights("mask", 300, 700, 1)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(50, 123.4)

        def others():
            p.set_psf_motion(15, 30.0, 0.01)
            wi = p.wiener(img)
            p.set_psf_motion(15, 30.0, 0.01, gamma=0.05)
            c = p.wiener(img)
            est = p.estimate_motion(img, scores=True)
            return [wi, c, p.blur(img), p.blur(img, adjoint=True), p.richardson_lucy(pos, 5), p.richardson_lucy_free(np.ascontiguousarray(pos[:300, :700]), 4, w),
                    p.tv_deconv(img, 2.0, 2.0, 3), p.tv_deconv(win, 20.0, 10.0, 3, True), np.asarray(est[-1])], est[:-1]

        def free_calls():
            return [p.tv_deconv_free(win, 100.0, 2.0, 4, w, 0.0, False, True, NORM_PADDED, True), p.tv_deconv_free(win, 100.0, 2.0, 3, None, 7.0, True),
                    p.tv_deconv_free(img, 20.0, 10.0, 2)]

        before, est0 = others()
        free0 = free_calls()
        after, est1 = others()
        free1 = free_calls()
        for k, (x, y) in enumerate(zip(before, after)):
            assert np.array_equal(x, y), "call %d changed after the free-boundary TV calls" % k
        assert repr(est0) == repr(est1)
        for k, (x, y) in enumerate(zip(free0, free1)):
            assert np.array_equal(x, y), "free-boundary TV call %d changed after the other calls" % k
    with fdr.Plan(M, N, fdr.MODE_FAST) as q:  # and each is what a fresh plan gives
        q.set_operator_psf_motion(50, 123.4)
        assert np.array_equal(q.tv_deconv_free(img, 20.0, 10.0, 2), free0[2])
        assert np.array_equal(q.tv_deconv(img, 2.0, 2.0, 3), before[6])


def test_restoration_quality(fdr):
    """the cropped scene of test_tvfree_host.py: the device equals the model to 0.02 dB at mu 500, n = 30 and on the masked case at
    n = 100, so the margins pinned on the CPU hold for the device"""
    c, q = quality_case(), QUALITY
    with fdr.Plan(q["M"], q["N"], fdr.MODE_FAST) as p:
        p.set_operator_psf(c["psf"])
        periodic = psnr(p.tv_deconv(c["d"], q["mu"], q["rho"], 100), c["truth"])
        unmasked = psnr(p.tv_deconv_free(c["stuck"], q["mu"], q["rho"], q["n_masked"]), c["truth"])
        for what, img, wt, n in (("free boundary", c["d"], None, q["n"]), ("stuck, masked", c["stuck"], c["keep"], q["n_masked"])):
            model = tvfree_model(img, c["psf"], q["M"], q["N"], q["mu"], q["rho"], n, wt)
            got = p.tv_deconv_free(img, q["mu"], q["rho"], n, wt)
            pm, pg = psnr(model, c["truth"]), psnr(got, c["truth"])
            print("TVF\tquality\t%s n=%d\tmodel %.3f dB, GPU %.3f dB, rel=%.3g (blurred %.2f dB, periodic TV on the GPU %.2f dB, unmasked %.2f dB)"
                  % (what, n, pm, pg, rel_err(got, model), psnr(c["d"], c["truth"]), periodic, unmasked))
            assert abs(pg - pm) <= 0.02, (what, pm, pg)
            assert rel_err(got, model) <= TVF_TOL
            if wt is None:
                assert pg >= psnr(c["d"], c["truth"]) + 15.0 and pg >= periodic + 15.0
            else:
                assert pg >= unmasked + 20.0


def test_refusals(fdr):
    """every refusal leaves a plan that then completes a valid call with the bytes it gave before"""
    import torch
    L = fdr.lib
    M = N = 64
    rows, cols = 40, 48
    psf = dense_psf(5, 5)
    img = tvf_image(M, N, rows, cols, 3)
    wts = tvf_weights("fractional", rows, cols, 3)
    out = np.empty((M, N), dtype=np.float32)

    def call(p, i=img, w=wts, o=out, rows=rows, cols=cols, stride=cols, wstride=cols, out_stride=N, mu=10.0, rho=2.0, nu=0.0, n=1, area=2,
             out_rows=M, out_cols=N, prm=True):
        q = fdr.TvFreeParams(mu, rho, nu, n, 0, 0, area, out_rows, out_cols)
        return L.fdr_tv_deconv_free_f32(p._h, i.ctypes.data if i is not None else None, rows, cols, stride, w.ctypes.data if w is not None else None,
                                        wstride, o.ctypes.data if o is not None else None, out_stride, ctypes.byref(q) if prm else None)

    for PM, PN, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (64, 64, fdr.MODE_FAST, fdr.FLAG_SIMPLE_PATH, "simple"),
                                      (64, 64, fdr.MODE_FAST, fdr.FLAG_FULL_SPECTRUM, "full spectrum"), (64, 16, fdr.MODE_FAST, 0, "N < 32"),
                                      (75, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX, "mixed radix")):
        im = tone_image(PM, PN, 2, min(PM, 64), min(PN, 64))
        with fdr.Plan(PM, PN, mode, flags=flags) as p:
            p.set_psf(fdr.motionBlurKernel(15, 30.0), 0.01)
            before = p.wiener(im)
            assert call(p, rows=8, cols=8, stride=8, wstride=8, out_stride=8, out_rows=8, out_cols=8) == -1, what
            assert np.array_equal(p.wiener(im), before), what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert call(p) == -4
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        assert call(p) == -4 and b"operator PSF" in L.fdr_last_error()
        p.set_operator_psf(psf)
        good = p.tv_deconv_free(img, 10.0, 2.0, 3, wts, full_plane=True)
        inside = out[:rows]  # a view of the output: overlaps it
        for kw in (dict(mu=0.0), dict(mu=-1.0), dict(mu=float("nan")), dict(mu=float("inf")), dict(rho=0.0), dict(rho=-2.0), dict(rho=float("nan")),
                   dict(rho=float("inf")), dict(nu=-1.0), dict(nu=float("nan")), dict(nu=float("inf")), dict(n=-1), dict(area=3), dict(area=-1),
                   dict(prm=False), dict(i=None), dict(o=None), dict(rows=65), dict(cols=65, stride=65, wstride=65, out_stride=65), dict(rows=0),
                   dict(stride=cols - 1), dict(wstride=cols - 1), dict(out_stride=N - 1), dict(out_rows=rows - 1), dict(out_cols=cols - 1),
                   dict(out_rows=M + 1), dict(out_cols=N + 1, out_stride=N + 1), dict(i=inside, stride=N), dict(w=inside, wstride=N)):
            assert call(p, **kw) == -1, kw
            assert np.array_equal(p.tv_deconv_free(img, 10.0, 2.0, 3, wts, full_plane=True), good), kw
        assert call(p, w=None, wstride=0) == 0  # no weights: their stride does not matter
        q = fdr.TvFreeParams(10.0, 2.0, 0.0, 1, 0, 0, 2, M, N)
        assert L.fdr_tv_deconv_free_f32(None, img.ctypes.data, rows, cols, cols, None, 0, out.ctypes.data, N, ctypes.byref(q)) == -1
        d = torch.from_numpy(img).cuda()  # the _dev form: the output may not be the input
        q = fdr.TvFreeParams(10.0, 2.0, 0.0, 1, 0, 0, 2, rows, cols)
        assert L.fdr_tv_deconv_free_f32_dev(p._h, d.data_ptr(), rows, cols, cols, None, 0, d.data_ptr(), cols, ctypes.byref(q), None) == -1
        assert b"overlaps the input" in L.fdr_last_error()
        with pytest.raises(fdr.FdrError):
            p.tv_deconv_free(img, -1.0)
        with pytest.raises(ValueError):
            p.tv_deconv_free(img, 10.0, weights=wts[:-1])
        want = tvfree_model(img, psf, M, N, 10.0, 2.0, 3, wts, out_shape=(M, N))
        assert rel_err(good, want) <= TVF_TOL and np.array_equal(p.tv_deconv_free(img, 10.0, 2.0, 3, wts, full_plane=True), good)


def test_pass_names(fdr):
    """a fresh profiled plan holds every pass of a free call, the data step under a name of its own"""
    with fdr.Plan(256, 512, fdr.MODE_FAST) as p:
        p.profile(True)
        p.set_operator_psf_motion(15, 30.0)
        img = tone_image(256, 512, 1, 200, 300)
        p.tv_deconv_free(img, 50.0, 2.0, 3, None, 0.0, False, True, NORM_PADDED)
        p.tv_deconv_free(img, 50.0, 2.0, 2, tvf_weights("mask", 200, 300, 1))
        names = {n: c for n, _, c in p.pass_times()}
        p.tv_deconv_free(img, 60.0, 2.0, 1)          # another mu: the table does not depend on it
        p.tv_deconv_free(img, 60.0, 2.0, 1, nu=3.0)  # another nu: the table again, never the PSF's transforms
        p.tv_deconv_free(img, 60.0, 3.0, 1, nu=3.0)  # another rho: again
        later = {n: c for n, _, c in p.pass_times()}  # (the counts since the first read)
    print("TVF\tpasses\t%s" % names)
    assert len(names) <= fdr.MAX_PASSES
    assert later["TV table: 1/(nu|H|^2+rho L)/MN (free)"] == 2 and later["O rows: PSF pad+FFT (operator)"] == 0
    want = {"O rows: PSF pad+FFT (operator)": 1, "O cols: FFT -> H/MN, conj(H)/MN": 1, "TV table: 1/(nu|H|^2+rho L)/MN (free)": 1,
            "TVF init: x = pad(d), w = q = 0": 2, "TVF data: s, q, r = 2s-e (window)": 5, "TV spatial: shrink+dual+div (free)": 5,
            "A op rows: pad+FFT (blur / RL)": 15, "B' op cols: FFT*H*IFFT": 5, "B' op cols: FFT*conj(H)*IFFT": 5, "C op rows: IFFT+crop (blur)": 10,
            "B' op cols: FFT*T*IFFT (TVF solve)": 5, "C op rows: IFFT (TVF x)": 5, "TVF out: crop+clamp": 2, "E TVF minmax+normalize": 1}
    for n, c in want.items():
        assert names.get(n) == c, (n, names.get(n), c)
    assert set(names) == set(want), set(names) ^ set(want)


def test_second_call_allocates_nothing(fdr):
    import torch
    M, N, rows, cols = 1024, 1024, 1000, 900
    ws = 8 * M * N  # the two planes the free form adds
    img = tvf_image(M, N, rows, cols, 2)
    d_in = torch.from_numpy(img).cuda()
    d_w = torch.from_numpy(tvf_weights("mask", rows, cols, 2)).cuda()
    d_out = torch.empty((M, N), dtype=torch.float32, device="cuda")
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0)
        p.tv_deconv_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 50.0, 2.0, 1)  # the periodic call's workspace
        torch.cuda.synchronize()
        f0 = torch.cuda.mem_get_info()[0]
        p.tv_deconv_free_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 50.0, 2.0, 2)
        torch.cuda.synchronize()
        f1 = torch.cuda.mem_get_info()[0]
        p.tv_deconv_free_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 70.0, 3.0, 2, d_w.data_ptr(), cols, 5.0, True, True, NORM_PADDED, M, N)
        p.tv_deconv_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 50.0, 2.0, 1)
        p.tv_deconv_free_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 50.0, 2.0, 2)
        torch.cuda.synchronize()
        f2 = torch.cuda.mem_get_info()[0]
    print("TVF\tallocations\tfirst call %d bytes (two planes %d), later calls %d bytes" % (f0 - f1, ws, f1 - f2))
    assert f0 - f1 >= ws, "the first call did not allocate its two planes"
    assert f1 == f2, "a later call allocated device memory"


def test_python_wrappers(fdr):
    """tvDeblurFree_myfft equals the Plan call on the _rlfree_plan_size plan; tvDeblurFree_RGB equals three such calls"""
    img = tvf_image(512, 1024, 300, 700, 2)
    psf = fdr.motionBlurKernel(15, 30.0)
    w = tvf_weights("mask", 300, 700, 2)
    assert fdr._rlfree_plan_size(300, 700, 15, 15) == (512, 1024)
    with fdr.Plan(512, 1024, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        want = p.tv_deconv_free(img, 50.0, 2.0, 3, w, 0.0, False, True)
        full = p.tv_deconv_free(img, 50.0, 2.0, 3, None, 4.0, True, False, NORM_CROPPED, True)
        chans = [np.ascontiguousarray(img[::-1]), img, np.ascontiguousarray(img[:, ::-1])]
        rgb_want = [p.tv_deconv_free(c, 50.0, 2.0, 3, w, 0.0, False, True, NORM_PADDED) for c in chans]
    assert np.array_equal(fdr.tvDeblurFree_myfft(img, psf, 50.0, iterations=3, weights=w, nonneg=True), want)
    assert np.array_equal(fdr.tvDeblurFree_myfft(img, psf, 50.0, 2.0, 3, None, 4.0, True, False, 0, NORM_CROPPED, True), full)
    model = tvfree_model(img, psf, 512, 1024, 50.0, 2.0, 3, w, nonneg=True)
    e = rel_err(want, model)
    print("TVF\ttvDeblurFree_myfft\t300x700 in 512x1024\terr=%.3g" % e)
    assert e <= TVF_TOL
    fdr.tvDeblurFree_RGB(chans, psf, 50.0, iterations=3, nonneg=True, norm_area=NORM_PADDED, weights=w)
    for k in range(3):
        assert np.array_equal(chans[k], rgb_want[k]), k


def test_cli_tv_free_boundary(fdr, tmp_path):
    """tools/cli/gpu --tv mu --free-boundary [--mask m.png]: the planes (--raw-out) equal three tv_deconv_free(..., nonneg as the --tv
    leg, NORM_PADDED) calls with the mask's weights on the plan tvDeblurFree_myfft uses; --tv-color beside it prints the usage text"""
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(root, "tools", "cli", "gpu")
    png = os.path.join(root, "tests", "golden", "car_blurred.png")
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    keep = np.random.default_rng(8).random((h, w)) >= 0.02
    mask_png = str(tmp_path / "mask.png")
    Image.fromarray(np.repeat((keep * np.uint8(255))[:, :, None], 3, axis=2).astype(np.uint8), "RGB").save(mask_png)
    outs = {}
    for tag, extra in (("masked", ["--mask", mask_png]), ("plain", [])):
        out_raw = str(tmp_path / (tag + ".f32"))
        r = subprocess.run([gpu, png, "40", "45", "--tv", "200", "--tv-iters", "10", "--free-boundary"] + extra + ["--raw-out", out_raw,
                            "--out", str(tmp_path / (tag + ".png"))], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Deblurring 3 channels took(gpu[total-variation free-boundary mu 200 rho 2 n 10]): " in r.stdout, r.stdout
        outs[tag] = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
    M, N = fdr._rlfree_plan_size(h, w, 40, 40)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(fdr.motionBlurKernel(40, 45.0))
        for tag, wt in (("masked", keep.astype(np.float32)), ("plain", None)):
            for k, c in enumerate((2, 1, 0)):  # B, G, R
                want = p.tv_deconv_free(np.ascontiguousarray(rgb[:, :, c]), 200.0, 2.0, 10, wt, 0.0, False, True, fdr.NORM_PADDED)
                assert np.array_equal(outs[tag][k], want), (tag, k, float(np.abs(outs[tag][k] - want).max()))
    assert not np.array_equal(outs["masked"], outs["plain"])
    r = subprocess.run([gpu, png, "40", "45", "--tv", "200", "--free-boundary", "--tv-color"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "Usage" in r.stdout and "--free-boundary" in r.stdout, (r.returncode, r.stdout[-300:])
