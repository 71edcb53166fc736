"""The blur operator and Richardson-Lucy deconvolution (fdr_blur_f32*, fdr_richardson_lucy_f32*) on the MI355X, against the float64
model of tests/_rl_model.py: blur in both directions (max-abs and per bin), adjointness on the device, RL for 0 .. 30 iterations
with every norm_area, invariants (delta PSF, flux, constant image, near-zero input), restoration quality, isolation from the
Wiener filter, determinism, the refusals, the pass names and the CLI.  Each case prints an `RL` line with its measured values
(pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _rl_model import (ADJ_TOL, BLUR_BIN_TOL, BLUR_TOL, DELTA_TOL, FLUX_TOL, NORM_CROPPED, NORM_NONE, NORM_PADDED, RL_TOL, blur_model,
                       centred_psf, dense_psf, normalize, op_spectrum, psnr, rel_err, rl_model, smooth_image)
from _spectral import bin_error, delta_psf, tone_image

pytestmark = pytest.mark.gpu

BLUR_SHAPES = [  # (M, N, rows, cols, stride); rows = cols = None: the full plane
    (8, 32, None, None, None), (256, 256, None, None, None), (1024, 1024, None, None, None), (4096, 4096, None, None, None),
    (8192, 8192, None, None, None), (256, 2048, None, None, None), (2048, 256, None, None, None),
    (256, 256, 200, 151, 163), (1024, 512, 1000, 333, 347), (64, 128, 37, 101, 103), (2048, 2048, 1500, 1999, 2001)]


def _psfs(fdr, M, N):
    """name, PSF: motion 15/30, motion 50/123.4, a delta and a dense random PSF, those that fit the plan"""
    out = [("motion15/30", fdr.motionBlurKernel(15, 30.0)), ("motion50/123.4", fdr.motionBlurKernel(50, 123.4)),
           ("delta(2,3)", delta_psf(2, 3)), ("dense9", dense_psf(11))]
    out = [(n, p) for n, p in out if p.shape[0] <= M and p.shape[1] <= N]
    if M * N >= 8192 * 8192:  # float64 model time: the two PSFs with the most structure
        out = [o for o in out if o[0] in ("motion50/123.4", "dense9")]
    return out


def _dev_call(fn, img, rows, cols, stride, out_stride, *args):
    """runs fn(d_img, rows, cols, stride, d_out, out_stride, *args) on device copies of img (row stride `stride`); returns the
    rows x cols output window"""
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


@pytest.mark.parametrize("M,N,rows,cols,stride", BLUR_SHAPES)
def test_blur_against_model(fdr, M, N, rows, cols, stride):
    full = rows is None
    rows, cols = (M, N) if full else (rows, cols)
    img = tone_image(M, N, M * 31 + N, rows, cols)
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for name, psf in _psfs(fdr, M, N):
            p.set_operator_psf(psf)
            H = op_spectrum(psf, M, N)
            for adj in (False, True):
                want = blur_model(img, psf, M, N, adjoint=adj, H=H)
                if full:
                    got = p.blur(img, adjoint=adj)
                else:
                    got = _dev_call(p.blur_dev, img, rows, cols, stride, stride + 2, adj)
                sp = rel_err(got, want)
                e, at = bin_error(got, want) if full else (float("nan"), None)
                what = "%dx%d win %dx%d %s %s" % (M, N, rows, cols, name, "adjoint" if adj else "forward")
                print("RL\tblur\t%s\trel=%.3g\tbin=%.3g\tat=%s" % (what, sp, e, at))
                if not sp <= BLUR_TOL:
                    bad.append("%s: max-abs %.3g > %.3g" % (what, sp, BLUR_TOL))
                if full and not e <= BLUR_BIN_TOL:
                    bad.append("%s: per-bin error %.3g > %.3g at %s" % (what, e, BLUR_BIN_TOL, at))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("M,N,rows,cols", [(8, 32, 8, 32), (256, 256, 256, 256), (1024, 512, 999, 345), (4096, 4096, 4096, 4096)])
def test_blur_adjoint_on_device(fdr, M, N, rows, cols):
    rng = np.random.default_rng(M + N)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    y = rng.standard_normal((rows, cols)).astype(np.float32)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for name, psf in _psfs(fdr, M, N):
            p.set_operator_psf(psf)
            bx = p.blur(x).astype(np.float64)
            bty = p.blur(y, adjoint=True).astype(np.float64)
            lhs, rhs = float(np.sum(bx * y)), float(np.sum(x * bty))
            scale = float(np.linalg.norm(bx) * np.linalg.norm(y))
            d = abs(lhs - rhs) / scale
            print("RL\tadjoint\t%dx%d win %dx%d %s\tdefect=%.3g" % (M, N, rows, cols, name, d))
            assert d <= ADJ_TOL, (name, d)


RL_SMALL = [(256, 256, None, None), (1024, 1024, None, None), (512, 256, 500, 250), (64, 64, 60, 50), (8, 32, None, None),
            (2048, 512, 2000, 512)]


def _rl_cases(fdr, M, N, rows, cols, iterations):
    """(what, got, want, norm_area) of one plan: every iteration count and norm_area.  Full planes: motion 15/30 placed top-left
    (and a dense 5 x 5 PSF up to 256^2).  Cropped windows: the same motion PSF centred (centred_psf) and the dense PSF.  A
    top-left motion PSF has no weight at (0, 0), so on a cropped window c = blur(u) is exactly 0 along the first rows / columns
    (their taps reach only the zeros outside the window); single-precision transforms leave c at the 1e-7 max|c| level there,
    around FDR_RL_TAU, and r = d+ / c is then arbitrary: the float64 model cannot judge those pixels."""
    img = np.clip(tone_image(M, N, M + 17 * N, rows, cols), 0, None) + np.float32(0.05)
    img[: max(1, rows // 16), : max(1, cols // 16)] -= np.float32(0.5)  # negative pixels: RL starts from d+
    motion = fdr.motionBlurKernel(15, 30.0)
    full = (rows, cols) == (M, N)
    psfs = [("motion15/30", motion)] if full else [("motion15/30 centred", centred_psf(motion, M, N))]
    if M * N <= 256 * 256 or not full:
        psfs.append(("dense5", dense_psf(5, 5)))
    psfs = [(n, q) for n, q in psfs if q.shape[0] <= M and q.shape[1] <= N]
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for name, psf in psfs:
            p.set_operator_psf(psf)
            for n in iterations:
                raw = rl_model(img, psf, M, N, n)
                for area in (NORM_NONE, NORM_CROPPED, NORM_PADDED):
                    got = p.richardson_lucy(img, n, area)
                    yield "%dx%d win %dx%d %s n=%d norm=%d" % (M, N, rows, cols, name, n, area), got, normalize(raw, area, M, N), area


def _judge(cases):
    bad = []
    for what, got, want, area in cases:
        e = rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(got.astype(np.float64) - want)))
        print("RL\trl\t%s\terr=%.3g" % (what, e))
        if not e <= RL_TOL:
            bad.append("%s: error %.3g > %.3g" % (what, e, RL_TOL))
    return bad


@pytest.mark.parametrize("M,N,rows,cols", RL_SMALL)
def test_rl_against_model_small(fdr, M, N, rows, cols):
    rows, cols = (M, N) if rows is None else (rows, cols)
    bad = _judge(_rl_cases(fdr, M, N, rows, cols, (0, 1, 5, 30)))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("M,N,iters", [(4096, 4096, (1, 3)), (8192, 8192, (1,))])
def test_rl_against_model_large(fdr, M, N, iters):
    bad = _judge(_rl_cases(fdr, M, N, M, N, iters))
    assert not bad, "\n".join(bad)


def test_delta_psf_keeps_d_plus(fdr):
    M, N = 256, 512
    img = tone_image(M, N, 9) - np.float32(0.6)
    img[np.abs(img) <= 1e-6] = 0.01  # no pixel in (0, tau]: those go to 0 by the guard
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(delta_psf(0, 0))
        for n in (1, 5):
            got = p.richardson_lucy(img, n)
            e = rel_err(got, np.maximum(img, 0))
            print("RL\tdelta\tn=%d\terr=%.3g" % (n, e))
            assert e <= DELTA_TOL, (n, e)


def test_flux_and_constant_fixed_point(fdr):
    M = N = 512
    psf = fdr.motionBlurKernel(15, 30.0).astype(np.float64)
    psf = (psf / psf.sum()).astype(np.float32)
    img = smooth_image(M, N, 4)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        u = p.richardson_lucy(img, 30)
        flux = abs(float(np.sum(u, dtype=np.float64)) / float(np.sum(img, dtype=np.float64)) - 1.0)
        print("RL\tflux\t30 iterations\trel=%.3g\tpsf sum - 1 = %.3g" % (flux, float(np.sum(psf, dtype=np.float64)) - 1))
        assert flux <= FLUX_TOL, flux
        c = np.full((M, N), 0.37, dtype=np.float32)
        u = p.richardson_lucy(c, 30)
        e = float(np.max(np.abs(u.astype(np.float64) - 0.37))) / 0.37
        print("RL\tconstant\t30 iterations\trel=%.3g" % e)
        assert e <= FLUX_TOL, e


def test_near_zero_input_stays_finite(fdr):
    M, N = 256, 256
    img = np.zeros((M, N), dtype=np.float32)
    img[100:140, 60:200] = 0.8
    img[10:20, 10:20] = 1e-9   # below tau
    img[200:, :] = -0.2       # negative: d+ = 0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0)
        for area in (NORM_NONE, NORM_CROPPED, NORM_PADDED):
            got = p.richardson_lucy(img, 30, area)
            assert np.all(np.isfinite(got)), area
            assert float(got.min()) >= 0.0, area
            assert np.all(got[200:, :] <= 1e-3 * float(got.max())) or area != NORM_NONE
        got = p.richardson_lucy(np.zeros((M, N), dtype=np.float32), 5, NORM_PADDED)  # all zero: flat, normalised to 0
        assert np.array_equal(got, np.zeros((M, N), dtype=np.float32))


def test_restoration_quality(fdr):
    M = N = 512
    truth = smooth_image(M, N, 7).astype(np.float64)
    psf = fdr.motionBlurKernel(15, 30.0).astype(np.float64)
    psf = (psf / psf.sum()).astype(np.float32)
    blurred = blur_model(truth, psf, M, N) + np.random.default_rng(1).normal(0, 2e-3, (M, N))
    blurred = blurred.astype(np.float32)
    model = rl_model(blurred, psf, M, N, 30)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        got = p.richardson_lucy(blurred, 30)
    p0, pm, pg = psnr(blurred, truth), psnr(model, truth), psnr(got, truth)
    print("RL\tquality\tPSNR blurred %.2f dB, model %.2f dB, GPU %.2f dB" % (p0, pm, pg))
    assert pm - p0 >= 1.0, "the model's own run gains only %.2f dB" % (pm - p0)
    assert pg - p0 >= (pm - p0) - 0.1, (p0, pm, pg)
    assert abs(pg - pm) <= 0.1, (pm, pg)


def test_isolation_and_determinism(fdr):
    import torch
    M, N = 512, 1024
    img = tone_image(M, N, 21)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_psf_motion(15, 30.0, 0.01)
        before = p.wiener(img)
        n = p.filter_bytes()
        blk = torch.empty(n, dtype=torch.uint8, device="cuda")
        p.export_filter_dev(blk.data_ptr(), n)
        torch.cuda.synchronize()
        w0 = blk.cpu().numpy().copy()
        p.set_operator_psf_motion(50, 123.4)
        p.blur(img)
        a = p.richardson_lucy(img, 5, NORM_NONE)
        b = p.richardson_lucy(img, 5, NORM_NONE)
        assert np.array_equal(a, b), "two RL runs differ"
        dev = _dev_call(lambda *args: p.richardson_lucy_dev(*args), img, M, N, N, N, 5, NORM_NONE)
        assert np.array_equal(a, dev), "host and _dev forms differ"
        p.export_filter_dev(blk.data_ptr(), n)
        torch.cuda.synchronize()
        assert np.array_equal(blk.cpu().numpy(), w0), "the operator calls changed the Wiener filter"
        assert np.array_equal(p.wiener(img), before), "Wiener output changed after the operator calls"
        p.set_psf_motion(15, 30.0, 0.05)  # and setting the Wiener filter leaves the operator alone
        assert np.array_equal(p.richardson_lucy(img, 5, NORM_NONE), a)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_MIXED_RADIX) as q:  # no effect on powers of two
        q.set_operator_psf_motion(50, 123.4)
        assert np.array_equal(q.richardson_lucy(img, 5, NORM_NONE), a)


def test_refusals(fdr):
    import torch
    L = fdr.lib
    psf = fdr.motionBlurKernel(15, 30.0)
    img = tone_image(64, 64, 3)
    out = np.empty_like(img)

    def op_calls(p, expect):
        assert L.fdr_set_operator_psf(p._h, psf.ctypes.data, 15, 15, 15) == expect
        assert L.fdr_set_operator_psf_motion(p._h, 15, 30.0, None) == expect
        assert L.fdr_blur_f32(p._h, img.ctypes.data, 8, 8, 64, out.ctypes.data, 64, 0) == expect
        assert L.fdr_richardson_lucy_f32(p._h, img.ctypes.data, 8, 8, 64, out.ctypes.data, 64, 1, 2) == expect

    for M, N, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (64, 64, fdr.MODE_FAST, fdr.FLAG_SIMPLE_PATH, "simple"),
                                    (64, 64, fdr.MODE_FAST, fdr.FLAG_FULL_SPECTRUM, "full spectrum"), (64, 16, fdr.MODE_FAST, 0, "N < 32"),
                                    (16384, 64, fdr.MODE_FAST, 0, "M > 8192"), (64, 16384, fdr.MODE_FAST, 0, "N > 8192"),
                                    (75, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX, "mixed radix")):
        im = tone_image(M, N, 2, min(M, 64), min(N, 64))
        with fdr.Plan(M, N, mode, flags=flags) as p:
            p.set_psf(psf, 0.01)
            before = p.wiener(im)
            op_calls(p, -1)
            assert np.array_equal(p.wiener(im), before), what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        op_calls(p, -4)
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        assert L.fdr_blur_f32(p._h, img.ctypes.data, 64, 64, 64, out.ctypes.data, 64, 0) == -4  # no operator PSF
        assert L.fdr_richardson_lucy_f32(p._h, img.ctypes.data, 64, 64, 64, out.ctypes.data, 64, 1, 2) == -4
        assert L.fdr_set_operator_psf(p._h, psf.ctypes.data, 0, 15, 15) == -1
        big = np.ones((65, 10), dtype=np.float32)
        assert L.fdr_set_operator_psf(p._h, big.ctypes.data, 65, 10, 10) == -1
        p.set_operator_psf(psf)
        assert L.fdr_richardson_lucy_f32(p._h, img.ctypes.data, 64, 64, 64, out.ctypes.data, 64, -1, 2) == -1
        for area in (3, -1):
            assert L.fdr_richardson_lucy_f32(p._h, img.ctypes.data, 64, 64, 64, out.ctypes.data, 64, 1, area) == -1
        wide = np.zeros((65, 65), dtype=np.float32)
        assert L.fdr_blur_f32(p._h, wide.ctypes.data, 65, 64, 65, wide.ctypes.data, 65, 0) == -1
        assert L.fdr_richardson_lucy_f32(p._h, wide.ctypes.data, 64, 65, 65, wide.ctypes.data, 65, 1, 2) == -1
        d = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        base = d.data_ptr()
        for off in (0, 4 * 63 * 64):  # the same window, and an output starting inside the input's last row
            assert L.fdr_richardson_lucy_f32_dev(p._h, ctypes.c_void_p(base), 64, 64, 64, ctypes.c_void_p(base + off), 64, 1, 2, None) == -1
        assert b"overlaps" in L.fdr_last_error()
        torch.cuda.synchronize()
        want = rl_model(img, psf, 64, 64, 3)
        assert rel_err(p.richardson_lucy(img, 3), want) <= RL_TOL  # the plan still works


def test_pass_names(fdr):
    with fdr.Plan(256, 512, fdr.MODE_FAST) as p:
        p.profile(True)
        p.set_operator_psf_motion(15, 30.0)
        img = tone_image(256, 512, 1, 200, 300)
        p.blur(img)
        p.richardson_lucy(img, 2, NORM_PADDED)
        names = {n: c for n, _, c in p.pass_times()}
    print("RL\tpasses\t%s" % names)
    want = {"O rows: PSF pad+FFT (operator)": 1, "O cols: FFT -> H/MN, conj(H)/MN": 1, "A op rows: pad+FFT (blur / RL)": 5,
            "B' op cols: FFT*H*IFFT": 3, "B' op cols: FFT*conj(H)*IFFT": 2, "C op rows: IFFT+crop (blur)": 1,
            "RL init: u = max(d, 0)": 1, "C op rows: IFFT+RL ratio": 2, "C op rows: IFFT+RL update": 2, "E RL minmax+normalize": 1}
    for n, c in want.items():
        assert names.get(n) == c, (n, names.get(n), c)


def test_cli_rl(fdr, tmp_path):
    """tools/cli/gpu --rl n: a timed Richardson-Lucy leg whose planes (--raw-out) equal three richardson_lucy(..., NORM_PADDED) calls
    on the same padded plan and are the written image; --rl with --cls, --verify or --mode parity is refused"""
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(root, "tools", "cli", "gpu")
    png = os.path.join(root, "tests", "golden", "car_blurred.png")
    out_png, out_raw = str(tmp_path / "rl.png"), str(tmp_path / "rl.f32")
    r = subprocess.run([gpu, png, "40", "45", "--rl", "10", "--out", out_png, "--raw-out", out_raw], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Deblurring 3 channels took(gpu[richardson-lucy 10]): " in r.stdout, r.stdout
    assert os.path.getsize(out_png) > 0
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    planes = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
    M, N = fdr._rl_plan_size(h, w)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(fdr.motionBlurKernel(40, 45.0))
        for k, c in enumerate((2, 1, 0)):  # B, G, R
            want = p.richardson_lucy(np.ascontiguousarray(rgb[:, :, c]), 10, fdr.NORM_PADDED)
            assert np.array_equal(planes[k], want), (k, float(np.abs(planes[k] - want).max()))
    for extra in (["--cls", "0.05"], ["--verify"], ["--mode", "parity"]):
        r = subprocess.run([gpu, png, "40", "45", "--rl", "10"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "Usage" in r.stdout, (extra, r.returncode, r.stdout[-300:])
