"""Noise-constrained TV deconvolution (fdr_tv_deconv_auto_f32*) on the MI355X against the float64 model of tests/_tvauto_model.py:
1 .. 3 iterations on the short cases of the free call (windows of every column residue mod 4, odd strides of the image, the
weights and the output, the window equal to the plan, 2048 x 512) and on a tall narrow plan whose window makes 512 partials, so
that the fold's strided loop runs twice, with no weights, a 0 / 1 mask and fractional weights and both noise levels (mu_k active
in every step; the clamp at 0), outputs and traces; 30 and 100 iterations; the quality scene; then bits (determinism, all-ones
weights, host against _dev form, n = 0, all-zero weights), isolation from the other calls of a plan in both directions, the
refusals, the allocation, the pass names, the wrappers and the CLI.  Each case prints a `TVA` line with its measured values
(pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, dense_psf, psnr, rel_err
from _spectral import tone_image
from _tvauto_model import SHORT_SIGMAS, TVA_TOL, TVA_TRACE_TOL, f32, quality_numbers, trace_err, tvauto_iterates, tvauto_model
from _tvfree_model import QUALITY, SHORT, SHORT_IDS, WEIGHT_KINDS, finish, quality_case, short_combos, tvf_image, tvf_weights

pytestmark = pytest.mark.gpu

AREAS = (NORM_NONE, NORM_CROPPED, NORM_PADDED)


def _strided(a, stride):
    """device copy of the window a with row stride `stride`, NaN between the rows: a read outside the window poisons the result"""
    import torch
    src = np.full((a.shape[0], stride), np.nan, dtype=np.float32)
    src[:, :a.shape[1]] = a
    return torch.from_numpy(src).cuda()


def _dev_call(p, img, stride, weights, wstride, out_shape, out_stride, sigma, rho, n, nu=0.0, aniso=False, nonneg=False, area=NORM_NONE, tau=0.0,
              trace=True):
    """Plan.tv_deconv_auto_dev on device copies of img and weights (each with its own row stride); returns (the output window, the
    trace) after checking that nothing was stored outside either (NaN fences)"""
    import torch
    rows, cols = img.shape
    d_in = _strided(img, stride)
    d_w = _strided(weights, wstride) if weights is not None else None
    d_out = torch.full((out_shape[0], out_stride), float("nan"), dtype=torch.float32, device="cuda")
    d_tr = torch.full((3 * n + 3,), float("nan"), dtype=torch.float64, device="cuda") if trace else None
    p.tv_deconv_auto_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), out_stride, sigma, rho, n, d_w.data_ptr() if d_w is not None else None,
                         wstride, tau, nu, aniso, nonneg, area, out_shape[0], out_shape[1], d_tr.data_ptr() if trace else None)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(np.isnan(out[:, out_shape[1]:])), "a store landed outside the output window"
    tr = None
    if trace:
        tr = d_tr.cpu().numpy()
        assert np.all(np.isnan(tr[3 * n:])), "a store landed behind the trace"
        tr = tr[:3 * n].reshape(n, 3)
    return out[:, :out_shape[1]], tr


def _model(img, psf, M, N, sigma, rho, nu, aniso, weights, ns):
    """({n: the M x N plane x of the float64 model after n iterations}, the trace of max(ns) iterations) from one run"""
    out, trace = {}, []
    for k, st in enumerate(tvauto_iterates(img, psf, M, N, sigma, rho, max(ns), weights, nu=nu, anisotropic=aniso)):
        if k in ns:
            out[k] = np.array(st["x"], dtype=np.float64)
        if "trace" in st:
            trace.append(st["trace"])
    return out, np.array(trace, dtype=np.float64).reshape(-1, 3)


def _error(got, want, area):
    return rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(got.astype(np.float64) - want)))


def _run(fdr, case, ns, combos_of, kinds, sigmas, areas=AREAS):
    M, N, rows, cols, stride, wstride, out_stride, outs = case
    img = tvf_image(M, N, rows, cols, M + 3 * N)
    bad, worst, worst_tr = [], 0.0, 0.0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for name, psf, _, rho, nu, aniso, nonneg in combos_of(fdr.motionBlurKernel(15, 30.0), M, N, rows, cols):
            p.set_operator_psf(psf)
            for kind in kinds:
                w = tvf_weights(kind, rows, cols, M + 3 * N)
                for sigma in sigmas:
                    planes, mtrace = _model(img, psf, M, N, f32(sigma), rho, nu, aniso, w, ns)
                    for n in ns:
                        for out_shape in outs:
                            for area in areas:
                                got, tr = _dev_call(p, img, stride, w, wstride, out_shape, out_stride, sigma, rho, n, nu, aniso, nonneg, area)
                                e = _error(got, finish(planes[n], out_shape, nonneg, area, M, N), area)
                                et = trace_err(tr, mtrace[:n])
                                what = "%dx%d win %dx%d out %dx%d %s w=%s sigma=%g n=%d norm=%d" % (M, N, rows, cols, out_shape[0], out_shape[1], name, kind,
                                                                                                  sigma, n, area)
                                print("TVA\ttvauto\t%s\terr=%.3g trace=%.3g mu_k=%s" % (what, e, et, " ".join("%.4g" % v for v in mtrace[:min(n, 3), 2])))
                                worst = max(worst, e) if e == e else float("nan")
                                worst_tr = max(worst_tr, et)
                                if not e <= TVA_TOL:
                                    bad.append("%s: error %.3g > %.3g" % (what, e, TVA_TOL))
                                if not et <= TVA_TRACE_TOL:
                                    bad.append("%s: trace error %.3g > %.3g" % (what, et, TVA_TRACE_TOL))
    print("TVA\tworst\t%dx%d win %dx%d n<=%d\t%.3g\ttrace %.3g" % (M, N, rows, cols, max(ns), worst, worst_tr))
    return bad


def _short_combos(motion, M, N, rows, cols):
    """short_combos of the free call (its mu is not used); the megapixel plan keeps the first (float64 model time)"""
    c = short_combos(motion, M, N, rows, cols)
    return c[:1] if M * N >= 1 << 20 else c


@pytest.mark.parametrize("case", SHORT, ids=SHORT_IDS)
def test_short_against_model(fdr, case):
    bad = _run(fdr, case, (1, 2, 3), _short_combos, WEIGHT_KINDS, SHORT_SIGMAS)
    assert not bad, "\n".join(bad)


def test_fold_adds_two_partials_per_thread(fdr):
    """8192 x 32, window 8190 x 29: 512 workgroups of the norm kernel, so every thread of the fold adds two partials of each sum
    (the 2048 x 512 case above makes 250, fewer than the fold has threads)"""
    case = (8192, 32, 8190, 29, 31, 30, 33, ((8190, 29),))
    bad = _run(fdr, case, (1, 3), lambda *a: [c for c in short_combos(*a) if c[0].startswith("dense")], ("fractional",), SHORT_SIGMAS[:1], (NORM_NONE,))
    assert not bad, "\n".join(bad)


def test_fold_takes_a_second_round(fdr):
    """4096^2, window 4082 x 4079, 2 % masked: 4084 workgroups of the norm kernel, more than the 2048 partials of each sum that the
    fold's 256 threads take per round.  No float64 model at this size: in the first step q = 0, so res_e is res_c bit for bit, S is
    the number of kept pixels exactly, and res_c is sum m (c - d)^2 of the device's own blur (Plan.blur, held to its model by the operator's tests)
    summed in float64 here, to 1e-5"""
    M = N = 4096
    rows, cols = 4082, 4079
    rng = np.random.default_rng(12)
    img = rng.random((rows, cols), dtype=np.float32)
    keep = (rng.random((rows, cols)) > 0.02).astype(np.float32)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0)
        _, res, trace = p.tv_deconv_auto(img, 0.02, 2.0, 1, keep)
        c = p.blur(img).astype(np.float64)
    want = float(np.sum(keep * (c - img) ** 2))
    print("TVA\tsecond round\tS %.0f (kept %d), res_c %.9g (float64 sum of the device's blur %.9g, rel %.3g)"
          % (res.S, int(keep.sum()), trace[0, 0], want, abs(trace[0, 0] - want) / want))
    assert res.S == float(keep.sum()) and trace[0, 0] == trace[0, 1] == res.discrepancy
    assert abs(trace[0, 0] - want) <= 1e-5 * want


LONG = [((64, 64, 60, 50, 53, 51, 67, ((60, 50), (64, 64))), ("none",)),
        ((512, 256, 500, 250, 251, 253, 256, ((500, 250),)), ("mask",))]


@pytest.mark.parametrize("case,kinds", LONG, ids=["64x64-win60x50", "512x256-win500x250-masked"])
def test_long_against_model(fdr, case, kinds):
    bad = _run(fdr, case, (30, 100), lambda *a: short_combos(*a)[:1], kinds, SHORT_SIGMAS[:1], (NORM_NONE, NORM_PADDED))
    assert not bad, "\n".join(bad)


def test_restoration_quality(fdr):
    """the cropped scene of test_tvauto_host.py, 100 steps with the defaults: the device equals the model to 0.02 dB with sigma given,
    estimated, and given with the stuck pixels masked, so the margins pinned on the CPU hold for the device"""
    c, q, num = quality_case(), QUALITY, quality_numbers()
    with fdr.Plan(q["M"], q["N"], fdr.MODE_FAST) as p:
        p.set_operator_psf(c["psf"])
        for name, img, sigma, wt in (("given", c["d"], q["noise"], None), ("estimated", c["d"], 0.0, None), ("masked", c["stuck"], q["noise"], c["keep"])):
            got, res, trace = p.tv_deconv_auto(img, sigma, q["rho"], 100, wt)
            pm, pg = num[name]["psnr"], psnr(got, c["truth"])
            print("TVA\tquality\t%s\tmodel %.3f dB, GPU %.3f dB, rel=%.3g, sigma %.6g (model %.6g), mu %.5g (model %.5g), discrepancy / target %.4f "
                  "(blurred %.2f dB, best tuned %.2f dB)" % (name, pm, pg, rel_err(got, num[name]["x"]), res.sigma, num[name]["sigma"], res.mu,
                                                             num[name]["mu"], res.discrepancy / res.target, num["blurred"], num["best"]))
            assert abs(pg - pm) <= 0.02, (name, pm, pg)
            assert pg >= num["blurred"] + 15.0 and pg >= num["best"] - 0.5
            assert res.sigma == pytest.approx(num[name]["sigma"], rel=1e-5) and res.S == (q["rows"] * q["cols"] if wt is None else float(wt.sum()))
            assert res.target == pytest.approx(res.sigma ** 2 * res.S, rel=1e-12)
            assert (res.discrepancy, res.mu) == (trace[-1, 0], trace[-1, 2]) and trace.shape == (100, 3)


def test_bits(fdr):
    """two calls give the same bytes and the same trace; all-ones weights give the bytes of no weights; the host form equals the
    _dev form; n = 0 gives the bytes of the free call with n = 0; all-zero weights give a finite result with mu_k = 0"""
    M, N, rows, cols = 256, 512, 200, 301
    img = tvf_image(M, N, rows, cols, 5)
    w = tvf_weights("fractional", rows, cols, 5)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(centred_psf(fdr.motionBlurKernel(15, 30.0), M, N))
        for wt in (None, w):
            a, ra, ta = p.tv_deconv_auto(img, 0.02, 2.0, 7, wt, 1.5, 30.0, False, True, NORM_PADDED, True)
            b, rb, tb = p.tv_deconv_auto(img, 0.02, 2.0, 7, wt, 1.5, 30.0, False, True, NORM_PADDED, True)
            assert np.array_equal(a, b) and np.array_equal(ta, tb) and ra == rb, "two runs differ"
            dev, td = _dev_call(p, img, 303, wt, 305, (M, N), N + 1, 0.02, 2.0, 7, 30.0, False, True, NORM_PADDED, 1.5)
            assert np.array_equal(a, dev) and np.array_equal(ta, td), "host and _dev forms differ"
            assert np.array_equal(_dev_call(p, img, 303, wt, 305, (M, N), N + 1, 0.02, 2.0, 7, 30.0, False, True, NORM_PADDED, 1.5, trace=False)[0], a)
            assert np.all(ta[:, 2] > 0) and np.all(np.isfinite(ta))
        none, _, tn = p.tv_deconv_auto(img, 0.02, 2.0, 7)
        ones = np.ones((rows, cols), dtype=np.float32)
        o, _, to = p.tv_deconv_auto(img, 0.02, 2.0, 7, ones)
        assert np.array_equal(o, none) and np.array_equal(to, tn), "all-ones weights are not the bytes of no weights"
        o, to = _dev_call(p, img, 303, ones, 304, (rows, cols), 301, 0.02, 2.0, 7)
        assert np.array_equal(o, none) and np.array_equal(to, tn)
        assert np.array_equal(p.tv_deconv_auto(img, 0.02, 2.0, 7, nu=50.0, tau=1.0)[0], none), "nu = 0 is not 25 rho, or tau = 0 is not 1"
        est = p.tv_deconv_auto(img, 0.0, 2.0, 7)
        assert est[1].sigma == p.noise_sigma(img) and np.array_equal(p.tv_deconv_auto(img, 0.0, 2.0, 7)[0], est[0])  # sigma as fdr_noise_sigma_f32
        assert rel_err(p.tv_deconv_auto(img, 0.02, 2.0, 7, w)[0], none) > 1e-3 and rel_err(p.tv_deconv_auto(img, 0.05, 2.0, 7)[0], none) > 1e-3
        # n = 0: pad(d), as the free call
        z, rz, tz = p.tv_deconv_auto(img, 0.02, 2.0, 0, w, nonneg=True, norm_area=NORM_CROPPED, full_plane=True)
        assert np.array_equal(z, p.tv_deconv_free(img, 10.0, 2.0, 0, w, nonneg=True, norm_area=NORM_CROPPED, full_plane=True))
        assert tz.shape == (0, 3) and (rz.mu, rz.discrepancy, rz.S) == (0.0, 0.0, 0.0)
        # no pixel counts: the ball is a point that every e lies in
        zero, rzero, tzero = p.tv_deconv_auto(img, 0.02, 2.0, 5, np.zeros((rows, cols), dtype=np.float32), full_plane=True)
        assert np.all(np.isfinite(zero)) and np.array_equal(tzero, np.zeros((5, 3))) and rzero.S == 0.0 and rzero.target == 0.0


def test_isolation_both_ways(fdr):
    """Wiener, blur, plain RL, periodic TV and free TV give the same bytes before and after auto calls on one plan, and the auto calls
    give the same bytes before and after them -- periodic and free TV with the auto call's nu as their mu / nu among them: the solve
    table is shared"""
    M, N = 512, 1024
    img = tone_image(M, N, 21)
    pos = np.clip(img, 0, None) + np.float32(0.05)
    win = np.ascontiguousarray(img[:300, :700])
    w = tvf_weights("mask", 300, 700, 1)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(50, 123.4)

        def others():
            p.set_psf_motion(15, 30.0, 0.01)
            return [p.wiener(img), p.blur(img), p.blur(img, adjoint=True), p.richardson_lucy(pos, 5), p.tv_deconv(img, 2.0, 2.0, 3),
                    p.tv_deconv(win, 50.0, 2.0, 3, True), p.tv_deconv_free(win, 100.0, 2.0, 4, w, 0.0, False, True, NORM_PADDED, True),
                    p.tv_deconv_free(win, 100.0, 2.0, 3, None, 50.0, True)]

        def auto_calls():
            r = [p.tv_deconv_auto(win, 0.02, 2.0, 4, w, 0.0, 0.0, False, True, NORM_PADDED, True), p.tv_deconv_auto(win, 0.0, 2.0, 3, None, 1.2, 7.0, True),
                 p.tv_deconv_auto(img, 0.05, 10.0, 2)]
            return [x[0] for x in r] + [x[2] for x in r]

        before = others()
        auto0 = auto_calls()
        after = others()
        auto1 = auto_calls()
        for k, (x, y) in enumerate(zip(before, after)):
            assert np.array_equal(x, y), "call %d changed after the auto calls" % k
        for k, (x, y) in enumerate(zip(auto0, auto1)):
            assert np.array_equal(x, y), "auto call %d changed after the other calls" % k
    with fdr.Plan(M, N, fdr.MODE_FAST) as q:  # and each is what a fresh plan gives
        q.set_operator_psf_motion(50, 123.4)
        assert np.array_equal(q.tv_deconv_auto(img, 0.05, 10.0, 2)[0], auto0[2])
        assert np.array_equal(q.tv_deconv_free(win, 100.0, 2.0, 3, None, 50.0, True), before[7])


def test_refusals(fdr):
    """every refusal leaves a plan that then completes a valid call with the bytes it gave before"""
    import torch
    L = fdr.lib
    M = N = 64
    rows, cols = 40, 48
    psf = dense_psf(5, 5)
    img = tvf_image(M, N, rows, cols, 3)
    wts = tvf_weights("mask", rows, cols, 3)
    out = np.empty((M, N), dtype=np.float32)

    def call(p, i=img, w=wts, o=out, rows=rows, cols=cols, stride=cols, wstride=cols, out_stride=N, sigma=0.02, tau=0.0, rho=2.0, nu=0.0, n=1, area=2,
             out_rows=M, out_cols=N, prm=True):
        q = fdr.TvAutoParams(sigma, tau, rho, nu, n, 0, 0, area, out_rows, out_cols)
        return L.fdr_tv_deconv_auto_f32(p._h, i.ctypes.data if i is not None else None, rows, cols, stride, w.ctypes.data if w is not None else None,
                                        wstride, o.ctypes.data if o is not None else None, out_stride, ctypes.byref(q) if prm else None, None, None)

    for PM, PN, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (64, 64, fdr.MODE_FAST, fdr.FLAG_SIMPLE_PATH, "simple"),
                                      (64, 64, fdr.MODE_FAST, fdr.FLAG_FULL_SPECTRUM, "full spectrum"), (75, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX, "mixed radix")):
        im = tone_image(PM, PN, 2, min(PM, 64), min(PN, 64))
        with fdr.Plan(PM, PN, mode, flags=flags) as p:
            p.set_psf(fdr.motionBlurKernel(15, 30.0), 0.01)
            before = p.wiener(im)
            assert call(p, rows=8, cols=8, stride=8, wstride=8, out_stride=8, out_rows=8, out_cols=8) == -1, what
            assert np.array_equal(p.wiener(im), before), what
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        assert call(p) == -4 and b"operator PSF" in L.fdr_last_error()
        p.set_operator_psf(psf)
        good = p.tv_deconv_auto(img, 0.02, 2.0, 3, wts, full_plane=True)[0]
        inside = out[:rows]  # a view of the output: overlaps it
        for kw in (dict(sigma=-0.01), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")),
                   dict(rho=0.0), dict(rho=-2.0), dict(rho=float("nan")), dict(rho=float("inf")), dict(nu=-1.0), dict(nu=float("nan")), dict(nu=float("inf")),
                   dict(n=-1), dict(area=3), dict(prm=False), dict(i=None), dict(o=None), dict(rows=65), dict(rows=0), dict(stride=cols - 1),
                   dict(wstride=cols - 1), dict(out_stride=N - 1), dict(out_rows=rows - 1), dict(out_cols=cols - 1), dict(out_rows=M + 1),
                   dict(i=inside, stride=N), dict(w=inside, wstride=N),
                   dict(sigma=0.0, rows=2, stride=cols), dict(sigma=0.0, cols=2, stride=2, wstride=2)):
            assert call(p, **kw) == -1, kw
            assert np.array_equal(p.tv_deconv_auto(img, 0.02, 2.0, 3, wts, full_plane=True)[0], good), kw
        assert call(p, rows=2) == 0 and call(p, sigma=0.0, rows=3) == 0  # a window below 3 x 3 is refused only when sigma is to be estimated
        assert call(p, w=None, wstride=0) == 0
        # the _dev form: the output may not be the input, and the trace may overlap no window
        d = torch.from_numpy(img).cuda()
        dw = torch.from_numpy(wts).cuda()
        do = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
        tr = torch.zeros(64, dtype=torch.float64, device="cuda")
        q = fdr.TvAutoParams(0.02, 0.0, 2.0, 0.0, 2, 0, 0, 2, rows, cols)

        def dev(i, w, o, t):
            return L.fdr_tv_deconv_auto_f32_dev(p._h, i, rows, cols, cols, w, cols, o, cols, ctypes.byref(q), t, None)

        assert dev(d.data_ptr(), dw.data_ptr(), d.data_ptr(), None) == -1 and b"overlaps the input" in L.fdr_last_error()
        for t, what in ((d.data_ptr() + 16, b"trace overlaps the input"), (dw.data_ptr() + 8, b"trace overlaps the weights"),
                        (do.data_ptr() + 4 * rows * cols - 8, b"trace overlaps the output")):
            assert dev(d.data_ptr(), dw.data_ptr(), do.data_ptr(), t) == -1 and what in L.fdr_last_error(), what
        assert dev(d.data_ptr(), dw.data_ptr(), do.data_ptr(), tr.data_ptr()) == 0
        torch.cuda.synchronize()
        with pytest.raises(fdr.FdrError):
            p.tv_deconv_auto(img, -1.0)
        with pytest.raises(ValueError):
            p.tv_deconv_auto(img, 0.02, weights=wts[:-1])
        want, _ = tvauto_model(img, psf, M, N, f32(0.02), 2.0, 3, wts, out_shape=(M, N))
        assert rel_err(good, want) <= TVA_TOL and np.array_equal(p.tv_deconv_auto(img, 0.02, 2.0, 3, wts, full_plane=True)[0], good)


def test_pass_names(fdr):
    """a fresh profiled plan holds every pass of an auto call in the table of FDR_MAX_PASSES names: the norm and mu launches under
    one name, the data step under its own; the noise estimate is the sixteenth"""
    img = tone_image(256, 512, 1, 200, 300)
    with fdr.Plan(256, 512, fdr.MODE_FAST) as p:
        p.profile(True)
        p.set_operator_psf_motion(15, 30.0)
        p.tv_deconv_auto(img, 0.02, 2.0, 3, None, 0.0, 0.0, False, True, NORM_PADDED)
        p.tv_deconv_auto(img, 0.02, 2.0, 2, tvf_weights("mask", 200, 300, 1))
        names = {n: c for n, _, c in p.pass_times()}
        p.tv_deconv_auto(img, 0.05, 2.0, 1)          # another sigma: the table does not depend on it
        p.tv_deconv_auto(img, 0.05, 2.0, 1, nu=3.0)  # another nu: the table again, never the PSF's transforms
        p.tv_deconv_auto(img, 0.0, 2.0, 1, nu=3.0)   # sigma estimated: one more pass
        later = {n: c for n, _, c in p.pass_times()}  # (the counts since the first read)
    print("TVA\tpasses\t%s" % names)
    want = {"O rows: PSF pad+FFT (operator)": 1, "O cols: FFT -> H/MN, conj(H)/MN": 1, "TV table: 1/(nu|H|^2+rho L)/MN (free)": 1,
            "TVF init: x = pad(d), w = q = 0": 2, "TVA norm+mu: res_e, res_c, S -> mu_k": 5, "TVA data: s, q, r = 2s-e (mu_k)": 5,
            "TV spatial: shrink+dual+div (free)": 5, "A op rows: pad+FFT (blur / RL)": 15, "B' op cols: FFT*H*IFFT": 5, "B' op cols: FFT*conj(H)*IFFT": 5,
            "C op rows: IFFT+crop (blur)": 10, "B' op cols: FFT*T*IFFT (TVF solve)": 5, "C op rows: IFFT (TVF x)": 5, "TVF out: crop+clamp": 2,
            "E TVF minmax+normalize": 1}
    for n, c in want.items():
        assert names.get(n) == c, (n, names.get(n), c)
    assert set(names) == set(want) and len(names) == 15 <= fdr.MAX_PASSES
    assert later["TV table: 1/(nu|H|^2+rho L)/MN (free)"] == 1 and later["O rows: PSF pad+FFT (operator)"] == 0
    assert later["TVA noise: sum |d * n|"] == 1 and len(later) == 16 <= fdr.MAX_PASSES


def test_second_call_allocates_nothing(fdr):
    import torch
    M, N, rows, cols = 1024, 1024, 1000, 900
    img = tvf_image(M, N, rows, cols, 2)
    d_in = torch.from_numpy(img).cuda()
    d_w = torch.from_numpy(tvf_weights("mask", rows, cols, 2)).cuda()
    d_out = torch.empty((M, N), dtype=torch.float32, device="cuda")
    d_tr = torch.empty(6, dtype=torch.float64, device="cuda")
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0)
        p.tv_deconv_free_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 50.0, 2.0, 1)  # the free call's workspaces
        torch.cuda.synchronize()
        f0 = torch.cuda.mem_get_info()[0]
        p.tv_deconv_auto_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 0.02, 2.0, 2)
        torch.cuda.synchronize()
        f1 = torch.cuda.mem_get_info()[0]
        p.tv_deconv_auto_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 0.0, 3.0, 2, d_w.data_ptr(), cols, 1.5, 5.0, True, True, NORM_PADDED, M, N,
                             d_tr.data_ptr())
        p.tv_deconv_free_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 50.0, 2.0, 1)
        p.tv_deconv_auto_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), N, 0.02, 2.0, 2)
        torch.cuda.synchronize()
        f2 = torch.cuda.mem_get_info()[0]
    print("TVA\tallocations\tfirst call %d bytes, later calls %d bytes" % (f0 - f1, f1 - f2))
    assert f0 - f1 <= 4 << 20, "the first call allocated more than its small block"
    assert f1 == f2, "a later call allocated device memory"


def test_python_wrappers(fdr):
    """tvDeblurAuto_myfft equals the Plan call on the _rlfree_plan_size plan; tvDeblurAuto_RGB equals three such calls, sigma given
    and estimated per channel"""
    img = tvf_image(512, 1024, 300, 700, 2)
    psf = fdr.motionBlurKernel(15, 30.0)
    w = tvf_weights("mask", 300, 700, 2)
    chans = [np.ascontiguousarray(img[::-1] * np.float32(0.75)), img, np.ascontiguousarray(img[:, ::-1] * np.float32(0.5))]
    with fdr.Plan(512, 1024, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        want = p.tv_deconv_auto(img, 0.02, 2.0, 3, w, 0.0, 0.0, False, True)
        rgb_want = {s: [p.tv_deconv_auto(c, s, 2.0, 3, w, 0.0, 0.0, False, True, NORM_PADDED) for c in chans] for s in (0.02, 0.0)}
    got = fdr.tvDeblurAuto_myfft(img, psf, 0.02, iterations=3, weights=w, nonneg=True)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2])
    model, mtrace = tvauto_model(img, psf, 512, 1024, f32(0.02), 2.0, 3, w, nonneg=True)
    e, et = rel_err(got[0], model), trace_err(got[2], mtrace)
    print("TVA\ttvDeblurAuto_myfft\t300x700 in 512x1024\terr=%.3g trace=%.3g" % (e, et))
    assert e <= TVA_TOL and et <= TVA_TRACE_TOL
    for s in (0.02, 0.0):
        c = list(chans)
        res = fdr.tvDeblurAuto_RGB(c, psf, s, iterations=3, nonneg=True, norm_area=NORM_PADDED, weights=w)
        for k in range(3):
            assert np.array_equal(c[k], rgb_want[s][k][0]) and res[k] == rgb_want[s][k][1], (s, k)
    assert len({r[1].sigma for r in rgb_want[0.0]}) == 3  # estimated per channel


def test_cli_tv_auto(fdr, tmp_path):
    """tools/cli/gpu --tv auto --sigma 0.02 [--mask m.png]: the planes (--raw-out) equal three tv_deconv_auto(..., nonneg as the --tv
    leg, NORM_PADDED) calls with the mask's weights on the plan tvDeblurAuto_myfft uses, and the printed lines carry their results;
    --tv-color beside it prints the usage text"""
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
    outs, lines = {}, {}
    for tag, extra in (("masked", ["--mask", mask_png]), ("plain", [])):
        out_raw = str(tmp_path / (tag + ".f32"))
        r = subprocess.run([gpu, png, "40", "45", "--tv", "auto", "--sigma", "0.02", "--tv-iters", "10"] + extra + ["--raw-out", out_raw,
                            "--out", str(tmp_path / (tag + ".png"))], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Deblurring 3 channels took(gpu[total-variation auto rho 2 n 10]): " in r.stdout, r.stdout
        outs[tag] = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
        lines[tag] = [l for l in r.stdout.splitlines() if l.startswith("total-variation: ")]
        assert len(lines[tag]) == 3, r.stdout
    M, N = fdr._rlfree_plan_size(h, w, 40, 40)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(fdr.motionBlurKernel(40, 45.0))
        for tag, wt in (("masked", keep.astype(np.float32)), ("plain", None)):
            for k, c in enumerate((2, 1, 0)):  # B, G, R
                want, res, _ = p.tv_deconv_auto(np.ascontiguousarray(rgb[:, :, c]), 0.02, 2.0, 10, wt, 0.0, 0.0, False, True, fdr.NORM_PADDED)
                assert np.array_equal(outs[tag][k], want), (tag, k, float(np.abs(outs[tag][k] - want).max()))
                assert lines[tag][k] == "total-variation: sigma %.9g target %.9g mu %.9g discrepancy %.9g" % (res.sigma, res.target, res.mu, res.discrepancy)
    assert not np.array_equal(outs["masked"], outs["plain"])
    r = subprocess.run([gpu, png, "40", "45", "--tv", "auto", "--tv-color"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "Usage" in r.stdout and "--tv auto" in r.stdout, (r.returncode, r.stdout[-300:])
    r = subprocess.run([gpu, png, "40", "45", "--tv", "auto", "--rl", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "Usage" in r.stdout, (r.returncode, r.stdout[-300:])
