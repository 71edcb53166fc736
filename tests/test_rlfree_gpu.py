"""Free-boundary, weighted Richardson-Lucy (fdr_richardson_lucy_free_f32*) on the MI355X against the float64 model of
tests/_rlfree_model.py: 0 .. 30 iterations with every norm_area, both output windows and two coverage thresholds, the flux
invariant, determinism, stores outside the output window, isolation from every other call of the plan, the refusals, the pass
names, restoration quality and the CLI.  Each case prints an `RLF` line with its measured values (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _rl_model import FLUX_TOL, NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, dense_psf, normalize, psnr, rel_err
from _rlfree_model import (QUALITY, RLFREE_TOL, SIGMA, SIGMA_MARGIN, flux_defect, quality_case, rlfree_model, rlfree_state,
                           sigma_margin)
from _spectral import tone_image

pytestmark = pytest.mark.gpu

SIGMAS = (1e-2, 1e-3)


def _mask(rows, cols, seed, zero=0.02):
    return (np.random.default_rng(seed).random((rows, cols)) >= zero).astype(np.float32)


def _case(fdr, name):
    """M, N, rows, cols, stride, psf, weights of the named case"""
    motion = fdr.motionBlurKernel(15, 30.0)
    if name == "512 win 480 centred motion":
        return 512, 512, 480, 480, 480, centred_psf(motion, 512, 512), None
    if name == "256 win 200x151 dense9 top-left":
        return 256, 256, 200, 151, 163, dense_psf(11), None
    if name == "1024x512 win 1000x333 motion top-left masked":
        return 1024, 512, 1000, 333, 347, motion, _mask(1000, 333, 5)
    if name == "64x128 win 37x101 dense5 masked":
        return 64, 128, 37, 101, 103, dense_psf(5, 5), _mask(37, 101, 6, 0.1)
    if name == "2048x512 win 2000x500":
        return 2048, 512, 2000, 500, 500, centred_psf(motion, 2048, 512), None
    if name == "256 full plane":
        return 256, 256, 256, 256, 256, motion, None
    if name == "4096 win 4000x3900":
        return 4096, 4096, 4000, 3900, 3900, centred_psf(motion, 4096, 4096), None
    if name == "8192 win 8000x8100":
        return 8192, 8192, 8000, 8100, 8100, centred_psf(motion, 8192, 8192), None
    raise KeyError(name)


SMALL = ["512 win 480 centred motion", "256 win 200x151 dense9 top-left", "1024x512 win 1000x333 motion top-left masked",
         "64x128 win 37x101 dense5 masked", "2048x512 win 2000x500", "256 full plane"]
LARGE = [("4096 win 4000x3900", (1, 3)), ("8192 win 8000x8100", (1,))]


def _image(M, N, rows, cols):
    img = np.clip(tone_image(M, N, M + 17 * N, rows, cols), 0, None) + np.float32(0.05)
    img[: max(1, rows // 16), : max(1, cols // 16)] -= np.float32(0.5)  # negative pixels: dw uses d+
    return img


def _dev_call(p, img, weights, rows, cols, stride, out_rows, out_cols, iterations, sigma, area):
    """Plan.richardson_lucy_free_dev on device copies (row stride `stride`, weights stride + 1); the output has NaN-filled guard
    columns, which must stay NaN; returns the out_rows x out_cols window"""
    import torch
    src = np.zeros((rows, stride), dtype=np.float32)
    src[:, :cols] = img
    d_in = torch.from_numpy(src).cuda()
    d_w, ws = None, 0
    if weights is not None:
        ws = stride + 1
        w = np.full((rows, ws), 7.0, dtype=np.float32)  # the padding must not be read
        w[:, :cols] = weights
        d_w = torch.from_numpy(w).cuda()
    out_stride = out_cols + 3
    d_out = torch.full((out_rows + 1, out_stride), float("nan"), dtype=torch.float32, device="cuda")
    p.richardson_lucy_free_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), out_stride, iterations,
                               d_weights=d_w.data_ptr() if d_w is not None else None, wstride=ws, sigma=sigma, norm_area=area,
                               out_rows=out_rows, out_cols=out_cols)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(np.isnan(out[:out_rows, out_cols:])) and np.all(np.isnan(out[out_rows:, :])), "a store landed outside the output window"
    return out[:out_rows, :out_cols]


def _err(got, want, area):
    return rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(got.astype(np.float64) - want)))


def _run_case(fdr, name, iterations):
    """compares every (sigma, n, output window, norm_area) of one case; returns the failures"""
    M, N, rows, cols, stride, psf, w = _case(fdr, name)
    img = _image(M, N, rows, cols)
    bad, worst = [], 0.0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        for sigma in SIGMAS:
            for n in iterations:
                st = rlfree_state(img, psf, M, N, n, weights=w, sigma=float(np.float32(sigma)))
                margin = sigma_margin(st["alpha"], float(np.float32(sigma)))
                assert margin >= SIGMA_MARGIN, "%s: a model alpha lies %.3g from sigma %g" % (name, margin, sigma)
                u32 = rlfree_state(img, psf, M, N, n, weights=w, sigma=float(np.float32(sigma)), dtype=np.float32)["u"]
                for orows, ocols in ((rows, cols), (M, N)):
                    raw = st["u"][:orows, :ocols]
                    cpu32 = rel_err(u32[:orows, :ocols], raw)
                    for area in (NORM_NONE, NORM_CROPPED, NORM_PADDED):
                        if (orows, ocols) == (rows, cols) and stride == cols and area != NORM_NONE:
                            got = p.richardson_lucy_free(img, n, weights=w, sigma=sigma, norm_area=area)  # the host form
                        elif (orows, ocols) == (M, N) and area == NORM_CROPPED:
                            got = p.richardson_lucy_free(img, n, weights=w, sigma=sigma, norm_area=area, full_plane=True)
                        else:
                            got = _dev_call(p, img, w, rows, cols, stride, orows, ocols, n, sigma, area)
                        e = _err(got, normalize(raw, area, M, N), area)
                        worst = max(worst, e)
                        what = "%s sigma=%g n=%d out=%dx%d norm=%d" % (name, sigma, n, orows, ocols, area)
                        print("RLF\trlfree\t%s\terr=%.3g\tcpu32=%.3g\tmargin=%.3g" % (what, e, cpu32, margin))
                        if not e <= RLFREE_TOL:
                            bad.append("%s: error %.3g > %s" % (what, e, RLFREE_TOL))
                        # (one float32 rounding, 2^-23, stands in where the CPU run happens to hit the model exactly: n = 0)
                        if area == NORM_NONE and not e <= 10 * max(cpu32, float(np.finfo(np.float32).eps)):
                            bad.append("%s: error %.3g above 10x the float32 CPU run's %.3g" % (what, e, cpu32))
    print("RLF\tworst\t%s\t%.3g" % (name, worst))
    return bad


@pytest.mark.parametrize("name", SMALL)
def test_against_model_small(fdr, name):
    bad = _run_case(fdr, name, (0, 1, 3, 30))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name,iters", LARGE)
def test_against_model_large(fdr, name, iters):
    bad = _run_case(fdr, name, iters)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["512 win 480 centred motion", "1024x512 win 1000x333 motion top-left masked"])
def test_flux_invariant_on_device(fdr, name):
    """sum(alpha u) = sum(dw) after every iteration, alpha and dw from the float64 model, u from the device"""
    M, N, rows, cols, stride, psf, w = _case(fdr, name)
    img = np.clip(_image(M, N, rows, cols), 0.01, None)  # every c > tau
    st = rlfree_state(img, psf, M, N, 0, weights=w)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        for n in (1, 3, 30):
            st["u"] = p.richardson_lucy_free(img, n, weights=w, full_plane=True)
            f = flux_defect(st)
            print("RLF\tflux\t%s n=%d\tdefect=%.3g" % (name, n, f))
            assert f <= FLUX_TOL, (n, f)


def test_determinism_and_forms(fdr):
    M, N, rows, cols, stride, psf, w = _case(fdr, "1024x512 win 1000x333 motion top-left masked")
    img = _image(M, N, rows, cols)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        a = p.richardson_lucy_free(img, 5, weights=w)
        b = p.richardson_lucy_free(img, 5, weights=w)
        assert np.array_equal(a, b), "two runs differ"
        dev = _dev_call(p, img, w, rows, cols, stride, rows, cols, 5, SIGMA, NORM_NONE)
        assert np.array_equal(a, dev), "host and _dev forms differ"
        full = p.richardson_lucy_free(img, 5, weights=w, full_plane=True)
        assert np.array_equal(full[:rows, :cols], a), "the window of the full-plane output differs"
        ones = p.richardson_lucy_free(img, 5, weights=np.ones_like(img))
        assert np.array_equal(ones, p.richardson_lucy_free(img, 5)), "all-ones weights differ from no weights"
    got = fdr.richardsonLucyFree_myfft(img, psf, 5, weights=w)  # its own plan: 1024 x 512 holds 1000 + 14 and 333 + 14
    assert fdr._rlfree_plan_size(rows, cols, *psf.shape) == (M, N) and np.array_equal(got, a)


def test_isolation(fdr):
    """Wiener, CLS, blur, plain RL, TV and the motion estimate give the same bytes before and after free-boundary calls"""
    import torch
    M, N, rows, cols = 512, 1024, 480, 1000
    img = tone_image(M, N, 21, rows, cols)
    w = _mask(rows, cols, 3)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0)

        def others():
            p.set_psf_motion(15, 30.0, 0.01)
            out = [p.wiener(img)]
            n = p.filter_bytes()
            blk = torch.empty(n, dtype=torch.uint8, device="cuda")
            p.export_filter_dev(blk.data_ptr(), n)
            torch.cuda.synchronize()
            out.append(blk.cpu().numpy().copy())
            p.set_psf_motion(15, 30.0, 0.01, gamma=0.05)
            out.append(p.wiener(img))
            out += [p.blur(img), p.blur(img, adjoint=True), p.richardson_lucy(img, 3), p.tv_deconv(img, 200.0, iterations=3)]
            est, table = p.estimate_motion(img, scores=True)
            out += [np.array([est.length, est.angle, est.score, est.confidence]), table]
            return out

        before = others()  # allocates the TV and motion workspaces
        p.richardson_lucy_free(img, 3, weights=w)
        p.richardson_lucy_free(img, 2, norm_area=NORM_PADDED, full_plane=True)
        after = others()
        for k, (a, b) in enumerate(zip(before, after)):
            assert np.array_equal(a, b), "result %d changed after the free-boundary calls" % k
        # and the other calls leave the free-boundary result alone
        assert np.array_equal(p.richardson_lucy_free(img, 3, weights=w), p.richardson_lucy_free(img, 3, weights=w))


def test_refusals(fdr):
    import torch
    L = fdr.lib
    psf = fdr.motionBlurKernel(15, 30.0)
    img = tone_image(64, 64, 3)
    out = np.empty((64, 64), dtype=np.float32)
    w = np.ones((64, 64), dtype=np.float32)

    def prm(n=1, sigma=1e-2, area=2, orows=8, ocols=8):
        return ctypes.byref(fdr.RlFreeParams(n, sigma, area, orows, ocols))

    def call(p, rows=8, cols=8, stride=64, wp=None, ws=64, op=None, ostride=64, pr=None):
        return L.fdr_richardson_lucy_free_f32(p._h, img.ctypes.data, rows, cols, stride, wp, ws, out.ctypes.data if op is None else op, ostride,
                                              prm() if pr is None else pr)

    for M, N, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (64, 64, fdr.MODE_FAST, fdr.FLAG_SIMPLE_PATH, "simple"),
                                    (64, 64, fdr.MODE_FAST, fdr.FLAG_FULL_SPECTRUM, "full spectrum"), (64, 16, fdr.MODE_FAST, 0, "N < 32"),
                                    (75, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX, "mixed radix")):
        with fdr.Plan(M, N, mode, flags=flags) as p:
            assert call(p) == -1, what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert call(p) == -4
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        p.profile(True)
        assert call(p) == -4 and b"operator PSF" in L.fdr_last_error()  # no operator PSF
        p.set_operator_psf(psf)
        p.pass_times()  # reads and clears the records of the PSF passes
        assert L.fdr_richardson_lucy_free_f32(p._h, img.ctypes.data, 8, 8, 64, None, 0, out.ctypes.data, 64, None) == -1  # null params
        assert L.fdr_richardson_lucy_free_f32(p._h, None, 8, 8, 64, None, 0, out.ctypes.data, 64, prm()) == -1
        assert call(p, pr=prm(n=-1)) == -1
        for sigma in (0.0, 1.0, -0.5, 2.0, float("nan")):
            assert call(p, pr=prm(sigma=sigma)) == -1, sigma
        assert b"sigma" in L.fdr_last_error()
        for area in (3, -1):
            assert call(p, pr=prm(area=area)) == -1
        for orows, ocols in ((7, 8), (8, 7), (65, 8), (8, 65), (0, 0)):
            assert call(p, pr=prm(orows=orows, ocols=ocols)) == -1, (orows, ocols)
        assert call(p, ostride=32, pr=prm(orows=8, ocols=40)) == -1  # out_stride < out_cols
        assert call(p, rows=65) == -1 and call(p, cols=65, stride=65) == -1 and call(p, rows=0) == -1 and call(p, stride=4) == -1
        assert call(p, wp=w.ctypes.data, ws=4) == -1  # weights stride < cols
        assert call(p, op=img.ctypes.data) == -1 and b"overlaps the input" in L.fdr_last_error()
        assert call(p, wp=w.ctypes.data, op=w.ctypes.data + 4 * 64 * 3) == -1 and b"overlaps the weights" in L.fdr_last_error()
        d = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        base = d.data_ptr()
        assert L.fdr_richardson_lucy_free_f32_dev(p._h, ctypes.c_void_p(base), 64, 64, 64, None, 0, ctypes.c_void_p(base + 4 * 63 * 64), 64,
                                                  prm(orows=64, ocols=64), None) == -1
        torch.cuda.synchronize()
        assert sum(c for _, _, c in p.pass_times()) == 0, "a refused call launched a pass"
        want = rlfree_model(img, psf, 64, 64, 3)
        got = p.richardson_lucy_free(img, 3)
        assert rel_err(got, want) <= RLFREE_TOL  # the plan still works


def test_pass_names(fdr):
    with fdr.Plan(256, 512, fdr.MODE_FAST) as p:
        p.profile(True)
        p.set_operator_psf_motion(15, 30.0)
        img = tone_image(256, 512, 1, 200, 300)
        p.richardson_lucy_free(img, 2, norm_area=NORM_PADDED)
        p.richardson_lucy_free(img, 1)
        names = {n: c for n, _, c in p.pass_times()}
    print("RLF\tpasses\t%s" % names)
    want = {"RLF setup: dw, W, sums": 2, "RLF start: wgt = 1/alpha, u": 2, "A op rows: pad+FFT (blur / RL)": 2 + 2 * 3,
            "B' op cols: FFT*H*IFFT": 3, "B' op cols: FFT*conj(H)*IFFT": 2 + 3, "C op rows: IFFT+crop (blur)": 2,
            "C op rows: IFFT+RL ratio (free)": 3, "C op rows: IFFT+RL update (weighted)": 3, "RLF out: crop": 1, "E RLF minmax+normalize": 1}
    for n, c in want.items():
        assert names.get(n) == c, (n, names.get(n), c)


def test_quality_matches_the_model(fdr):
    """the cropped scene of test_rlfree_host.py: the device reproduces the model's PSNR to 0.01 dB, plain, masked and against plain RL"""
    q = QUALITY
    motion = fdr.motionBlurKernel(*q["psf"]).astype(np.float64)
    motion = (motion / motion.sum()).astype(np.float32)
    truth, d, d_stuck, w = quality_case(lambda M, N: centred_psf(motion, M, N))
    cp = centred_psf(motion, q["M"], q["N"])
    with fdr.Plan(q["M"], q["N"], fdr.MODE_FAST) as p:
        p.set_operator_psf(cp)
        plain = psnr(p.richardson_lucy(d, q["n"]), truth)
        for what, img, wt in (("free boundary", d, None), ("stuck, unmasked", d_stuck, None), ("stuck, masked", d_stuck, w)):
            pm = psnr(rlfree_model(img, cp, q["M"], q["N"], q["n"], weights=wt), truth)
            pg = psnr(p.richardson_lucy_free(img, q["n"], weights=wt), truth)
            print("RLF\tquality\t%s\tmodel %.3f dB, GPU %.3f dB (blurred %.2f dB, plain RL on the GPU %.2f dB)" % (what, pm, pg, psnr(d, truth), plain))
            assert abs(pg - pm) <= 0.01, (what, pm, pg)
            if what == "free boundary":
                assert pg >= plain + 10.0, (plain, pg)
                free = pg
            if what == "stuck, unmasked":
                unmasked = pg
            if what == "stuck, masked":
                assert pg >= unmasked + 10.0 and pg >= free - 1.0, (unmasked, pg, free)


def test_cli_free_boundary_mask(fdr, tmp_path):
    """tools/cli/gpu --rl n --free-boundary --mask m.png: the planes (--raw-out) equal three richardson_lucy_free(..., NORM_PADDED)
    calls with the mask's weights on the plan richardsonLucyFree_myfft uses, and are the written image; --free-boundary without
    --rl and --mask without --free-boundary are refused"""
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
        out_png, out_raw = str(tmp_path / (tag + ".png")), str(tmp_path / (tag + ".f32"))
        r = subprocess.run([gpu, png, "40", "45", "--rl", "10", "--free-boundary"] + extra + ["--out", out_png, "--raw-out", out_raw],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Deblurring 3 channels took(gpu[richardson-lucy free-boundary 10]): " in r.stdout, r.stdout
        outs[tag] = (np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w), np.asarray(Image.open(out_png).convert("RGB")))
    psf = fdr.motionBlurKernel(40, 45.0)
    M, N = fdr._rlfree_plan_size(h, w, 40, 40)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        for tag, wt in (("masked", keep.astype(np.float32)), ("plain", None)):
            planes = []
            for k, c in enumerate((2, 1, 0)):  # B, G, R
                want = p.richardson_lucy_free(np.ascontiguousarray(rgb[:, :, c]), 10, weights=wt, norm_area=fdr.NORM_PADDED)
                assert np.array_equal(outs[tag][0][k], want), (tag, k, float(np.abs(outs[tag][0][k] - want).max()))
                planes.append(want)
            # the written PNG is the Python path's result through the same white-balance epilogue
            bgr = fdr.applyWhiteBalance_u8([np.ascontiguousarray(rgb[:, :, c]) for c in (2, 1, 0)], planes)
            assert np.array_equal(outs[tag][1], bgr[:, :, ::-1]), tag
    assert not np.array_equal(outs["masked"][0], outs["plain"][0])
    for args in (["--free-boundary"], ["--rl", "10", "--mask", mask_png], ["--free-boundary", "--mask", mask_png]):
        r = subprocess.run([gpu, png, "40", "45"] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "Usage" in r.stdout, (args, r.returncode, r.stdout[-300:])
