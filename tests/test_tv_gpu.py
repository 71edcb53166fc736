"""Total-variation deconvolution (fdr_tv_deconv_f32*) on the MI355X against the float64 model of tests/_tv_model.py: 1 .. 3 iterations
on every plan shape up to 8192^2, 30 and 100 iterations up to 2048 x 512, full planes and cropped strided windows, both shrinkages,
nonneg, every norm_area, motion / dense / delta PSFs, mu over two decades and rho in {1, 2, 10}; then restoration quality,
determinism, isolation from the other calls of a plan, the refusals, the pass names and the CLI.  Each case prints a `TV` line with
its measured values (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, dense_psf, normalize, psnr, rel_err
from _spectral import delta_psf, tone_image
from _tv_model import TV_TOL, blocks_scene, tv_iterates, tv_model
from test_tv_host import QUALITY, quality_case

pytestmark = pytest.mark.gpu


def _dev_call(fn, img, rows, cols, stride, out_stride, *args):
    """runs fn(d_img, rows, cols, stride, d_out, out_stride, *args) on device copies of img (row stride `stride`); returns the
    rows x cols output window after checking that nothing was stored outside it (NaN fence)"""
    import torch
    src = np.zeros((rows, stride), dtype=np.float32)
    src[:, :cols] = img
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((rows, out_stride), float("nan"), dtype=torch.float32, device="cuda")
    fn(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), out_stride, *args)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(np.isnan(out[:, cols:])), "a store landed outside the output window"
    return out[:, :cols]


def tv_image(M, N, seed, rows, cols):
    """float32 window with edges, texture above the thresholds used here (1 / rho >= 0.1) and negative pixels"""
    rng = np.random.default_rng(seed)
    return (blocks_scene(M, N, seed)[:rows, :cols] + 0.2 * rng.random((rows, cols)) - 0.15).astype(np.float32)


def _combos(fdr, M, N, full):
    """(name, psf, mu, rho, anisotropic, nonneg): PSFs motion / dense / delta, mu 5 .. 500, rho 1, 2, 10, both shrinkages"""
    motion = fdr.motionBlurKernel(15, 30.0)
    out = [("motion15/30 mu500 rho2 iso", motion if full else centred_psf(motion, M, N), 500.0, 2.0, False, False),
           ("dense5 mu50 rho1 aniso nonneg", dense_psf(5, 5), 50.0, 1.0, True, True),
           ("delta(2,3) mu5 rho10 iso nonneg", delta_psf(2, 3), 5.0, 10.0, False, True),
           ("motion15/30 mu50 rho10 aniso", motion, 50.0, 10.0, True, False)]
    out = [c for c in out if c[1].shape[0] <= M and c[1].shape[1] <= N]
    if M * N >= 4096 * 4096:  # float64 model time
        out = out[:1] if M * N >= 8192 * 8192 else [out[0], out[3]]
    return out


def _models(img, psf, M, N, mu, rho, aniso, ns):
    """{n: the raw window of the float64 model after n iterations} from one run of the iteration"""
    rows, cols = img.shape
    out = {}
    for k, (x, _, _, _) in enumerate(tv_iterates(img, psf, M, N, mu, rho, max(ns), aniso)):
        if k in ns:
            out[k] = np.array(x[:rows, :cols], dtype=np.float64)
    return out


def _run(fdr, M, N, rows, cols, stride, ns, tol, areas=(NORM_NONE, NORM_CROPPED, NORM_PADDED)):
    full = rows is None
    rows, cols = (M, N) if full else (rows, cols)
    img = tv_image(M, N, M + 3 * N, rows, cols)
    bad, worst = [], 0.0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for name, psf, mu, rho, aniso, nonneg in _combos(fdr, M, N, full):
            p.set_operator_psf(psf)
            raw = _models(img, psf, M, N, mu, rho, aniso, ns)
            for n in ns:
                want_raw = np.maximum(raw[n], 0) if nonneg else raw[n]
                for area in areas:
                    if full:
                        got = p.tv_deconv(img, mu, rho, n, aniso, nonneg, area)
                    else:
                        got = _dev_call(p.tv_deconv_dev, img, rows, cols, stride, stride + 2, mu, rho, n, aniso, nonneg, area)
                    want = normalize(want_raw, area, M, N)
                    e = rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(got.astype(np.float64) - want)))
                    what = "%dx%d win %dx%d %s n=%d norm=%d" % (M, N, rows, cols, name, n, area)
                    print("TV\ttv\t%s\terr=%.3g" % (what, e))
                    worst = max(worst, e) if e == e else float("nan")
                    if not e <= tol:
                        bad.append("%s: error %.3g > %.3g" % (what, e, tol))
    print("TV\tworst\t%dx%d win %dx%d n<=%d\t%.3g" % (M, N, rows, cols, max(ns), worst))
    return bad


SHORT = [(8, 32, None, None, None), (256, 256, None, None, None), (256, 2048, None, None, None), (2048, 256, None, None, None),
         (1024, 1024, None, None, None), (4096, 4096, None, None, None), (8192, 8192, None, None, None),
         (256, 256, 200, 151, 163), (1024, 512, 1000, 333, 347), (64, 128, 37, 101, 103), (16, 32, 9, 30, 31)]


@pytest.mark.parametrize("M,N,rows,cols,stride", SHORT)
def test_tv_short_against_model(fdr, M, N, rows, cols, stride):
    areas = (NORM_NONE, NORM_CROPPED, NORM_PADDED) if M * N < 4096 * 4096 else (NORM_NONE,)
    bad = _run(fdr, M, N, rows, cols, stride, (1, 2, 3), TV_TOL, areas)
    assert not bad, "\n".join(bad)


LONG = [(256, 256, None, None, None), (64, 64, 60, 50, 53), (512, 256, 500, 250, 251), (2048, 512, 2000, 500, 512)]


@pytest.mark.parametrize("M,N,rows,cols,stride", LONG)
def test_tv_long_against_model(fdr, M, N, rows, cols, stride):
    bad = _run(fdr, M, N, rows, cols, stride, (0, 30, 100), TV_TOL)
    assert not bad, "\n".join(bad)


def test_restoration_quality(fdr):
    """the piecewise-constant scene of test_tv_host.py: the device equals the model to 0.02 dB and beats the best Wiener filter
    and 30 Richardson-Lucy iterations (both from the float64 models) by the model's own margin"""
    q = QUALITY
    truth, cp, blurred, wiener, rl = quality_case(fdr.motionBlurKernel(*q["psf"]))
    model = tv_model(blurred, cp, q["M"], q["N"], q["mu"], q["rho"], q["n"])
    with fdr.Plan(q["M"], q["N"], fdr.MODE_FAST) as p:
        p.set_operator_psf(cp)
        got = p.tv_deconv(blurred, q["mu"], q["rho"], q["n"])
    pm, pg = psnr(model, truth), psnr(got, truth)
    print("TV\tquality\tPSNR blurred %.2f dB, best Wiener %.2f dB, RL 30 %.2f dB, TV model %.2f dB, TV GPU %.2f dB, rel=%.3g"
          % (psnr(blurred, truth), wiener, rl, pm, pg, rel_err(got, model)))
    assert abs(pg - pm) <= 0.02, (pm, pg)
    assert pm >= max(wiener, rl) + 1.0 and pg > max(wiener, rl), (pg, pm, wiener, rl)


def test_determinism_aliasing_and_parameter_changes(fdr):
    import torch
    M, N = 512, 1024
    img = tv_image(M, N, 5, M, N)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0)
        a = p.tv_deconv(img, 100.0, 2.0, 7)
        assert np.array_equal(a, p.tv_deconv(img, 100.0, 2.0, 7)), "two TV runs differ"
        dev = _dev_call(p.tv_deconv_dev, img, M, N, N, N, 100.0, 2.0, 7, False, False, NORM_NONE)
        assert np.array_equal(a, dev), "host and _dev forms differ"
        d = torch.from_numpy(img).cuda()  # the output may be the input
        p.tv_deconv_dev(d.data_ptr(), M, N, N, d.data_ptr(), N, 100.0, 2.0, 7)
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), a), "in place differs"
        b = p.tv_deconv(img, 10.0, 2.0, 7)     # mu, then rho, then the PSF change: each what a fresh plan gives
        c = p.tv_deconv(img, 10.0, 5.0, 7, True)
        p.set_operator_psf(dense_psf(3, 7))
        e = p.tv_deconv(img, 10.0, 5.0, 7, True)
        assert np.array_equal(p.tv_deconv(img, 100.0, 2.0, 0), img)  # n = 0: the window of pad(d)
    with fdr.Plan(M, N, fdr.MODE_FAST) as q:
        q.set_operator_psf(dense_psf(3, 7))
        assert np.array_equal(q.tv_deconv(img, 10.0, 5.0, 7, True), e), "a PSF change was not seen"
        q.set_operator_psf_motion(15, 30.0)
        assert np.array_equal(q.tv_deconv(img, 10.0, 5.0, 7, True), c), "a rho change was not seen"
        assert np.array_equal(q.tv_deconv(img, 10.0, 2.0, 7), b), "a mu change was not seen"
        assert np.array_equal(q.tv_deconv(img, 100.0, 2.0, 7), a)
    assert rel_err(b, a) > 1e-3 and rel_err(c, b) > 1e-3 and rel_err(e, c) > 1e-3


def test_isolation(fdr):
    """Wiener, CLS, blur, RL and the motion estimate give the same bytes before and after TV calls on the same plan"""
    M, N = 512, 1024
    img = tone_image(M, N, 21)
    pos = np.clip(img, 0, None) + np.float32(0.05)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(50, 123.4)

        def others():
            p.set_psf_motion(15, 30.0, 0.01)
            w = p.wiener(img)
            p.set_psf_motion(15, 30.0, 0.01, gamma=0.05)
            c = p.wiener(img)
            est = p.estimate_motion(img, scores=True)
            return [w, c, p.blur(img), p.blur(img, adjoint=True), p.richardson_lucy(pos, 5), np.asarray(est[-1])], est[:-1]

        before, est0 = others()
        for aniso in (False, True):
            p.tv_deconv(img, 100.0, 2.0, 5, aniso, True, NORM_PADDED)
        p.tv_deconv(img[:300, :700], 20.0, 10.0, 3)
        after, est1 = others()
        for k, (x, y) in enumerate(zip(before, after)):
            assert np.array_equal(x, y), "call %d changed after the TV calls" % k
        assert repr(est0) == repr(est1)


def test_refusals(fdr):
    L = fdr.lib
    psf = fdr.motionBlurKernel(15, 30.0)
    img = tone_image(64, 64, 3)
    out = np.empty_like(img)

    def call(p, rows=64, cols=64, stride=64, out_stride=64, mu=10.0, rho=2.0, n=1, area=2, prm=True):
        q = fdr.TvParams(mu, rho, n, 0, 0, area)
        return L.fdr_tv_deconv_f32(p._h, img.ctypes.data, rows, cols, stride, out.ctypes.data, out_stride, ctypes.byref(q) if prm else None)

    for M, N, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (64, 64, fdr.MODE_FAST, fdr.FLAG_SIMPLE_PATH, "simple"),
                                    (64, 64, fdr.MODE_FAST, fdr.FLAG_FULL_SPECTRUM, "full spectrum"), (64, 16, fdr.MODE_FAST, 0, "N < 32"),
                                    (16384, 64, fdr.MODE_FAST, 0, "M > 8192"), (64, 16384, fdr.MODE_FAST, 0, "N > 8192"),
                                    (75, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX, "mixed radix")):
        im = tone_image(M, N, 2, min(M, 64), min(N, 64))
        with fdr.Plan(M, N, mode, flags=flags) as p:
            p.set_psf(psf, 0.01)
            before = p.wiener(im)
            assert call(p, 8, 8) == -1, what
            assert np.array_equal(p.wiener(im), before), what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert call(p) == -4
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        assert call(p) == -4  # no operator PSF
        assert b"operator PSF" in L.fdr_last_error()
        p.set_operator_psf(psf)
        for kw in (dict(mu=0.0), dict(mu=-1.0), dict(mu=float("nan")), dict(mu=float("inf")), dict(rho=0.0), dict(rho=-2.0),
                   dict(rho=float("nan")), dict(rho=float("inf")), dict(n=-1), dict(area=3), dict(area=-1), dict(prm=False),
                   dict(rows=65), dict(cols=65, stride=65, out_stride=65), dict(rows=0), dict(stride=63), dict(out_stride=63)):
            assert call(p, **kw) == -1, kw
        assert L.fdr_tv_deconv_f32(p._h, None, 64, 64, 64, out.ctypes.data, 64, ctypes.byref(fdr.TvParams(1, 1, 1, 0, 0, 2))) == -1
        with pytest.raises(fdr.FdrError):
            p.tv_deconv(img, -1.0)
        want = tv_model(img, psf, 64, 64, 10.0, 2.0, 3)
        assert rel_err(p.tv_deconv(img, 10.0, 2.0, 3), want) <= TV_TOL  # the plan still works


def test_pass_names(fdr):
    with fdr.Plan(256, 512, fdr.MODE_FAST) as p:
        p.profile(True)
        p.set_operator_psf_motion(15, 30.0)
        img = tone_image(256, 512, 1, 200, 300)
        p.tv_deconv(img, 50.0, 2.0, 3, False, True, NORM_PADDED)
        p.tv_deconv(img, 50.0, 2.0, 2)
        names = {n: c for n, _, c in p.pass_times()}
        p.tv_deconv(img, 60.0, 2.0, 1)   # another mu, another rho: the table again, never the PSF's transforms
        p.tv_deconv(img, 60.0, 3.0, 1)
        p.tv_deconv(img, 60.0, 3.0, 1)
        later = {n: c for n, _, c in p.pass_times()}  # (the counts since the first read)
    print("TV\tpasses\t%s" % names)
    assert later["TV table: 1/(mu|H|^2+rho L)/MN"] == 2 and later["O rows: PSF pad+FFT (operator)"] == 0 and later["O cols: FFT -> H/MN, conj(H)/MN"] == 0
    want = {"O rows: PSF pad+FFT (operator)": 1, "O cols: FFT -> H/MN, conj(H)/MN": 1, "TV table: 1/(mu|H|^2+rho L)/MN": 1, "TV init: x = pad(d), w = 0": 2, "TV spatial: shrink+dual+div": 5,
            "A op rows: pad+FFT (blur / RL)": 7, "B' op cols: FFT*conj(H)*IFFT": 2, "C op rows: IFFT+crop (blur)": 2,
            "B' op cols: FFT*T*IFFT (TV solve)": 5, "C op rows: IFFT (TV x)": 5, "TV out: crop+clamp": 2, "E TV minmax+normalize": 1}
    for n, c in want.items():
        assert names.get(n) == c, (n, names.get(n), c)


def test_python_one_call(fdr):
    img = tv_image(300, 700, 2, 300, 700)
    psf = fdr.motionBlurKernel(15, 30.0)
    got = fdr.tvDeblur_myfft(img, psf, 50.0, iterations=3, nonneg=True)
    assert fdr._rl_plan_size(300, 700) == (512, 1024)
    want = tv_model(img, psf, 512, 1024, 50.0, 2.0, 3, nonneg=True)
    e = rel_err(got, want)
    print("TV\ttvDeblur_myfft\t300x700 in 512x1024\terr=%.3g" % e)
    assert e <= TV_TOL


def test_cli_tv(fdr, tmp_path):
    """tools/cli/gpu --tv mu: a timed total-variation leg whose planes (--raw-out) equal three tv_deconv(..., nonneg, NORM_PADDED)
    calls on the same padded plan, and whose written PNG is the colour epilogue of those planes; --tv with --cls, --verify, --rl or
    --mode parity, and --tv-iters without --tv, are refused"""
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(root, "tools", "cli", "gpu")
    png = os.path.join(root, "tests", "golden", "car_blurred.png")
    out_png, out_raw = str(tmp_path / "tv.png"), str(tmp_path / "tv.f32")
    r = subprocess.run([gpu, png, "40", "45", "--tv", "200", "--tv-iters", "10", "--tv-rho", "5", "--out", out_png, "--raw-out", out_raw],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Deblurring 3 channels took(gpu[total-variation mu 200 rho 5 n 10]): " in r.stdout, r.stdout
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    planes = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
    M, N = fdr._rl_plan_size(h, w)
    want = []
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(fdr.motionBlurKernel(40, 45.0))
        for k, c in enumerate((2, 1, 0)):  # B, G, R
            want.append(p.tv_deconv(np.ascontiguousarray(rgb[:, :, c]), 200.0, 5.0, 10, False, True, fdr.NORM_PADDED))
            assert np.array_equal(planes[k], want[k]), (k, float(np.abs(planes[k] - want[k]).max()))
    bgr8 = fdr.applyWhiteBalance_u8([np.ascontiguousarray(rgb[:, :, c]) for c in (2, 1, 0)], want)
    written = np.asarray(Image.open(out_png).convert("RGB"))
    assert np.array_equal(written[:, :, ::-1], np.asarray(bgr8).reshape(h, w, 3)), "the written PNG is not the Python path's picture"
    for extra in (["--tv", "200", "--cls", "0.05"], ["--tv", "200", "--verify"], ["--tv", "200", "--mode", "parity"], ["--tv", "200", "--rl", "3"],
                  ["--tv-iters", "5"], ["--tv", "0"], ["--tv", "200", "--tv-rho", "0"]):
        r = subprocess.run([gpu, png, "40", "45"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "Usage" in r.stdout, (extra, r.returncode, r.stdout[-300:])
