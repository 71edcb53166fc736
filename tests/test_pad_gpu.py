"""Smooth padding of the Wiener / CLS calls (FDR_OPT_PAD_MODE = FDR_PAD_SMOOTH) on the MI355X: the normalised output of every pass A
kernel against the float64 model of tests/_pad_model.py, FDR_PAD_ZERO against itself byte for byte (never set, set, switched there and
back; a full window in either mode), batches and batch-graph replays against one-by-one calls, the quality table of test_pad_host.py
on the device output, the refusals, the Python wrappers and the CLI flag.

Each model case prints a `PAD` line with its measured value (pytest -s)."""
import ctypes
import os

import numpy as np
import pytest

from _pad_model import (DEVICE_TOL, MIN_GAIN_DB, PAD_SMOOTH, PAD_ZERO, QUALITY_K, QUALITY_SEEDS, QUALITY_SHAPES, centred_psf_plane, normalized,
                        psnr, quality_case, quality_failures, quality_psf, restore_raw)
from _rl_model import smooth_image

pytestmark = pytest.mark.gpu


def _f32(x):
    return float(np.float32(x))


def _picture(rows, cols, seed):
    """a smooth positive picture with some noise: its left / right and top / bottom borders differ, as a crop's do"""
    rng = np.random.default_rng(seed)
    return (smooth_image(max(rows, 8), max(cols, 8), seed)[:rows, :cols] + 0.05 * rng.random((rows, cols))).astype(np.float32)


# rows, cols, M, N, flag -- which pass A kernel runs, and what is padded
MODEL_CASES = [
    # one image in a 1024^2 plan: the split kernel (1024-point rows)
    (1024, 900, 1024, 1024, 0),     # columns only
    (700, 1024, 1024, 1024, 0),     # rows only
    (700, 900, 1024, 1024, 0),      # both
    (1023, 1023, 1024, 1024, 0),    # a margin of 1
    (3, 1000, 1024, 1024, 0),       # a window of 3 rows
    (701, 901, 1024, 1024, 0),      # width (and height) not a multiple of 4
    # 4096-point rows: the packed kernel
    (128, 4000, 128, 4096, 0),
    (100, 4096, 128, 4096, 0),
    (100, 4000, 128, 4096, 0),
    (127, 4095, 128, 4096, 0),
    (3, 4001, 128, 4096, 0),
    (50, 1001, 64, 1024, "FLAG_FULL_SPECTRUM"),  # the packed kernel on the full spectrum
    (30, 50, 32, 64, 0),            # 8 values per thread, several groups per workgroup
    # 8192-point rows: the persistent kernel
    (64, 8000, 64, 8192, 0),
    (50, 8192, 64, 8192, 0),
    (50, 8000, 64, 8192, 0),
    (63, 8191, 64, 8192, 0),
    (3, 8001, 64, 8192, 0),
    (50, 8001, 64, 8192, "FLAG_FULL_SPECTRUM"),
]


@pytest.mark.parametrize("rows,cols,M,N,flag", MODEL_CASES)
def test_device_against_model(fdr, rows, cols, M, N, flag):
    """max |device - model| of the normalised output <= DEVICE_TOL (1e-4, the fast-mode bound), NORM_CROPPED and NORM_PADDED, Wiener
    and CLS.  Largest value measured on an MI355X: _pad_model.MEASURED_MAX."""
    flags = getattr(fdr, flag) if flag else 0
    img = _picture(rows, cols, rows * 7919 + cols)
    psf = fdr.motionBlurKernel(15, 30.0)
    K = _f32(0.01)
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
        for gamma in (0.0, _f32(0.05)):
            p.set_psf(psf, K, gamma=gamma)
            raw = restore_raw(img, psf, K, M, N, PAD_SMOOTH, gamma=gamma)
            raw_zero = restore_raw(img, psf, K, M, N, PAD_ZERO, gamma=gamma)
            for norm, padded in ((fdr.NORM_CROPPED, False), (fdr.NORM_PADDED, True)):
                got = p.wiener(img, norm)
                want = normalized(raw, rows, cols, padded)
                e = float(np.max(np.abs(got.astype(np.float64) - want)))
                away = float(np.max(np.abs(normalized(raw_zero, rows, cols, padded) - want)))  # what zero padding would give
                what = "%dx%d in %dx%d %s gamma=%g %s" % (rows, cols, M, N, flag or "", gamma, "padded" if padded else "cropped")
                print("PAD\tmodel\t%s\terr=%.3g\tzero_padding_differs_by=%.3g" % (what, e, away))
                if not e <= DEVICE_TOL:  # 1e-4; largest measured 1.27e-6 (_pad_model.MEASURED_MAX)
                    bad.append("%s: max-abs %.3g > %.3g" % (what, e, DEVICE_TOL))
                if not away > 100 * DEVICE_TOL:
                    bad.append("%s: the zero-padded model is only %.3g away: the case cannot tell the modes apart" % (what, away))
    assert not bad, "\n".join(bad)


def _single_and_batch(fdr, p, img, d_in, count, rows, cols, norm):
    """(the host-pointer single call, the device batch) of one plan state"""
    import torch
    one = p.wiener(img, norm)
    d_out = torch.full_like(d_in, -1.0)
    p.wiener_batch_dev(d_in.data_ptr(), rows * cols, count, rows, cols, cols, d_out.data_ptr(), rows * cols, cols, norm)
    torch.cuda.synchronize()
    return one, d_out.cpu().numpy()


@pytest.mark.parametrize("rows,cols,M,N", [(200, 300, 256, 512), (100, 4000, 128, 4096), (50, 8000, 64, 8192)])
def test_pad_zero_is_the_unset_plan(fdr, rows, cols, M, N):
    """a plan whose option was never set, one where it was set to FDR_PAD_ZERO, and one switched to smooth and back give identical
    bytes for the same call, single and batched; smooth differs"""
    import torch
    count = 5
    imgs = np.stack([_picture(rows, cols, 40 + i) for i in range(count)])
    d_in = torch.from_numpy(imgs).cuda()
    psf = fdr.motionBlurKernel(15, 30.0)
    res = {}
    for state in ("unset", "zero", "smooth_and_back", "smooth"):
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            p.set_psf(psf, _f32(0.01))
            p.set_batching(2, 2)
            if state == "zero":
                p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_ZERO)
            elif state == "smooth_and_back":
                p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
                p.wiener(imgs[0], fdr.NORM_CROPPED)
                p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_ZERO)
            elif state == "smooth":
                p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
            res[state] = [_single_and_batch(fdr, p, imgs[0], d_in, count, rows, cols, norm) for norm in (fdr.NORM_CROPPED, fdr.NORM_PADDED)]
    for state in ("zero", "smooth_and_back"):
        for k in range(2):
            assert np.array_equal(res[state][k][0], res["unset"][k][0]), (state, k)
            assert np.array_equal(res[state][k][1], res["unset"][k][1]), (state, k)
    for k in range(2):
        assert not np.array_equal(res["smooth"][k][0], res["unset"][k][0])
        assert np.array_equal(res["unset"][k][1][0], res["unset"][k][0])  # (batch image 0 is the single call's picture)


@pytest.mark.parametrize("M,N,flag", [(256, 512, 0), (1024, 1024, 0), (64, 4096, 0), (64, 8192, 0), (64, 1024, "FLAG_FULL_SPECTRUM")])
def test_full_window_is_unchanged(fdr, M, N, flag):
    """with rows = M and cols = N there is nothing to fill: smooth and zero give identical bytes"""
    flags = getattr(fdr, flag) if flag else 0
    img = _picture(M, N, 9)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        p.set_psf(fdr.motionBlurKernel(15, 30.0), _f32(0.01))
        zero = [p.wiener(img, n) for n in (fdr.NORM_CROPPED, fdr.NORM_PADDED)]
        p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
        smooth = [p.wiener(img, n) for n in (fdr.NORM_CROPPED, fdr.NORM_PADDED)]
    assert np.array_equal(zero[0], smooth[0]) and np.array_equal(zero[1], smooth[1])


@pytest.mark.parametrize("rows,cols,M,N", [(200, 300, 256, 512), (700, 900, 1024, 1024), (60, 4000, 64, 4096), (50, 8000, 64, 8192)])
def test_smooth_batches_equal_one_by_one(fdr, rows, cols, M, N):
    """in smooth mode every image of a batch equals its one-by-one result: group 4, two streams, and a batch graph across a change of
    the mode between two otherwise identical calls"""
    import torch
    count = 9
    imgs = np.stack([_picture(rows, cols, 300 + i) for i in range(count)])
    d_in = torch.from_numpy(imgs).cuda()
    psf = fdr.motionBlurKernel(15, 30.0)

    def one_by_one(p):
        d_out = torch.full_like(d_in, -1.0)
        for i in range(count):
            p.wiener_dev(d_in[i].data_ptr(), rows, cols, cols, d_out[i].data_ptr(), cols, fdr.NORM_CROPPED)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()

    def batch(p, d_out):
        p.wiener_batch_dev(d_in.data_ptr(), rows * cols, count, rows, cols, cols, d_out.data_ptr(), rows * cols, cols, fdr.NORM_CROPPED)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()

    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_psf(psf, _f32(0.01), gamma=_f32(0.05))
        want_zero = one_by_one(p)
        p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
        want = one_by_one(p)
        assert not np.array_equal(want, want_zero)
        assert np.array_equal(want[0], p.wiener(imgs[0], fdr.NORM_CROPPED))
        for ns, grp in ((1, 1), (1, 4), (2, 1), (2, 4), (4, 2)):
            p.set_batching(ns, grp)
            assert np.array_equal(batch(p, torch.full_like(d_in, -1.0)), want), (ns, grp)
        # a captured batch graph is keyed on the mode: the same call, the same buffers, the mode changed in between
        p.set_batching(2, 4)
        p.set_option(fdr.OPT_BATCH_GRAPH, 1)
        d_out = torch.full_like(d_in, -1.0)
        assert np.array_equal(batch(p, d_out), want)
        assert np.array_equal(batch(p, d_out), want)      # the replay
        p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_ZERO)
        assert np.array_equal(batch(p, d_out), want_zero)
        p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
        assert np.array_equal(batch(p, d_out), want)
        p.set_option(fdr.OPT_BATCH_GRAPH, 0)


def test_host_batches_take_the_mode(fdr):
    """fdr_wiener_batch_f32 / fdr_wiener_batch_ptrs_f32 (the host-pointer pipeline) restore with the plan's mode"""
    rows, cols, M, N = 200, 300, 256, 512
    imgs = np.stack([_picture(rows, cols, 70 + i) for i in range(4)])
    outs = np.empty_like(imgs)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_psf(fdr.motionBlurKernel(15, 30.0), _f32(0.01))
        p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
        want = np.stack([p.wiener(im, fdr.NORM_PADDED) for im in imgs])
        rc = fdr.lib.fdr_wiener_batch_f32(p._h, imgs.ctypes.data_as(ctypes.c_void_p), rows * cols, 4, rows, cols, cols,
                                          outs.ctypes.data_as(ctypes.c_void_p), rows * cols, cols, fdr.NORM_PADDED)
        assert rc == 0, fdr.lib.fdr_last_error()
        assert np.array_equal(outs, want)
        pin = (ctypes.c_void_p * 4)(*[imgs[i].ctypes.data for i in range(4)])
        outs2 = np.empty_like(imgs)
        pout = (ctypes.c_void_p * 4)(*[outs2[i].ctypes.data for i in range(4)])
        rc = fdr.lib.fdr_wiener_batch_ptrs_f32(p._h, pin, pout, 4, rows, cols, cols, cols, fdr.NORM_PADDED)
        assert rc == 0, fdr.lib.fdr_last_error()
        assert np.array_equal(outs2, want)


@pytest.mark.parametrize("rows,cols,M,N", QUALITY_SHAPES)
def test_quality_on_the_device(fdr, rows, cols, M, N):
    """the conditions of test_pad_host.py::test_quality_table on the device output, and the device PSNR within 0.05 dB of the model's.
    The device returns the window min-max normalised (NORM_CROPPED); it is taken back to the raw scale with the extremes of the model's
    window, so both PSNRs are against the same truth on the same scale."""
    psf = quality_psf()
    h = centred_psf_plane(psf, M, N).astype(np.float32)  # the whole plane: centre at (0, 0), the picture stays in place
    K = _f32(QUALITY_K)
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_psf(h, K)
        for seed in QUALITY_SEEDS:
            truth, blurred = quality_case(psf, seed, rows, cols)
            pb = psnr(blurred, truth)
            res = {}
            for name, mode, pad in (("zero", fdr.PAD_ZERO, PAD_ZERO), ("smooth", fdr.PAD_SMOOTH, PAD_SMOOTH)):
                p.set_option(fdr.OPT_PAD_MODE, mode)
                got = p.wiener(blurred, fdr.NORM_CROPPED).astype(np.float64)
                w = restore_raw(blurred, h, K, M, N, pad)[:rows, :cols]
                lo, hi = w.min(), w.max()
                res[name] = (psnr(got * (hi - lo) + lo, truth), psnr(w, truth))
            what = "%dx%d in %dx%d seed %d" % (rows, cols, M, N, seed)
            print("PAD\tdevice quality\t%s\tblurred=%.2f\tzero=%.2f (model %.2f)\tsmooth=%.2f (model %.2f)\tgain=%.2f" %
                  (what, pb, res["zero"][0], res["zero"][1], res["smooth"][0], res["smooth"][1], res["smooth"][0] - res["zero"][0]))
            bad += quality_failures(what, pb, res["zero"][0], res["smooth"][0], MIN_GAIN_DB)
            for name in ("zero", "smooth"):
                if not abs(res[name][0] - res[name][1]) <= 0.05:
                    bad.append("%s %s: device PSNR %.3f dB, model %.3f dB" % (what, name, res[name][0], res[name][1]))
    assert not bad, "\n".join(bad)


def test_refusals(fdr):
    """each unsupported plan kind and a bad value return FDR_ERR_ARG with a message that names the option; the plan stays usable"""
    L = fdr.lib
    kinds = [
        ("parity", 64, 64, fdr.MODE_PARITY, 0),
        ("simple path", 64, 64, fdr.MODE_FAST, fdr.FLAG_SIMPLE_PATH),
        ("any size", 45, 75, fdr.MODE_FAST, fdr.FLAG_ANY_SIZE),
        ("any size, parity", 45, 75, fdr.MODE_PARITY, fdr.FLAG_ANY_SIZE),
        ("mixed radix", 45, 75, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX),
        ("tables only", 64, 64, fdr.MODE_FAST, fdr.FLAG_TABLES_ONLY),
        ("longer than 8192", 8, 16384, fdr.MODE_FAST, 0),
        ("shorter than 8", 4, 64, fdr.MODE_FAST, 0),
    ]
    for what, M, N, mode, flags in kinds:
        with fdr.Plan(M, N, mode, flags=flags) as p:
            for value in (fdr.PAD_SMOOTH, fdr.PAD_ZERO):
                assert L.fdr_plan_set_option(p._h, fdr.OPT_PAD_MODE, value) == -1, what
                assert b"FDR_OPT_PAD_MODE" in L.fdr_last_error(), what
    img = _picture(50, 60, 1)
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        p.set_psf(fdr.motionBlurKernel(15, 30.0), _f32(0.01))
        p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
        before = p.wiener(img, fdr.NORM_CROPPED)
        for value in (2, -1, 1 << 40):
            assert L.fdr_plan_set_option(p._h, fdr.OPT_PAD_MODE, value) == -1
            assert b"FDR_OPT_PAD_MODE" in L.fdr_last_error()
        with pytest.raises(fdr.FdrError):
            p.set_option(fdr.OPT_PAD_MODE, 3)
        assert np.array_equal(p.wiener(img, fdr.NORM_CROPPED), before)  # the mode is still smooth
    # accepted: the full spectrum, and FDR_FLAG_MIXED_RADIX on power-of-two sizes (where the flag has no effect)
    for flags in (fdr.FLAG_FULL_SPECTRUM, fdr.FLAG_MIXED_RADIX):
        with fdr.Plan(64, 128, fdr.MODE_FAST, flags=flags) as p:
            p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)


def test_other_operators_ignore_the_option(fdr):
    """the blur operator and Richardson-Lucy keep padding with zeros"""
    rows, cols, M, N = 50, 100, 64, 128
    img = _picture(rows, cols, 5)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(fdr.motionBlurKernel(9, 30.0))
        zero = p.richardson_lucy(img, 3, fdr.NORM_NONE)
        p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
        assert np.array_equal(p.richardson_lucy(img, 3, fdr.NORM_NONE), zero)


def test_python_wrappers(fdr):
    """wienerDeblur_myfft / _RGB_optimized / _RGB_naive with pad=PAD_SMOOTH are the plan-level call on the plan of _pad_plan_size"""
    rows, cols = 200, 300
    psf = fdr.motionBlurKernel(15, 30.0)
    chans = [_picture(rows, cols, 20 + i) for i in range(3)]
    M, N = fdr._pad_plan_size(rows, cols, 15, 15)
    assert (M, N) == (256, 512)
    for gamma in (0.0, 0.05):
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
            p.set_psf(psf, 0.01, gamma=gamma)
            want = [p.wiener(c, fdr.NORM_PADDED) for c in chans]
        got = fdr.wienerDeblur_myfft(chans[0], psf, 0.01, mode=fdr.MODE_FAST, cls_gamma=gamma, pad=fdr.PAD_SMOOTH)
        assert np.array_equal(got, want[0])
        a, b = list(chans), list(chans)
        fdr.wienerDeblur_RGB_optimized(a, psf, 0.01, mode=fdr.MODE_FAST, cls_gamma=gamma, pad=fdr.PAD_SMOOTH)
        fdr.wienerDeblur_RGB_naive(b, psf, 0.01, mode=fdr.MODE_FAST, cls_gamma=gamma, pad=fdr.PAD_SMOOTH)
        for k in range(3):
            assert np.array_equal(a[k], want[k]) and np.array_equal(b[k], want[k]), (gamma, k)
    # the default keeps the zero-padded plan of the next powers of two
    with fdr.Plan(256, 512, fdr.MODE_FAST) as p:
        p.set_psf(psf, 0.01)
        assert np.array_equal(fdr.wienerDeblur_myfft(chans[0], psf, 0.01, mode=fdr.MODE_FAST), p.wiener(chans[0], fdr.NORM_PADDED))
    with pytest.raises(ValueError):
        fdr.wienerDeblur_myfft(chans[0], psf, 0.01, mode=fdr.MODE_PARITY, pad=fdr.PAD_SMOOTH)


def test_cli_pad_planes_equal_python(fdr, tmp_path):
    """tools/cli/gpu --pad smooth --raw-out: the restored planes equal wienerDeblur_RGB_optimized(..., pad=PAD_SMOOTH), alone, with --cls
    and after `auto auto`; --pad zero is the plain run; with --mode parity it exits non-zero with the library's message."""
    import subprocess
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    png = os.path.join(root, "tests", "golden", "cat_blurred.png")
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    gpu = os.path.join(root, "tools", "cli", "gpu")

    def run(args, name):
        out_raw = str(tmp_path / name)
        r = subprocess.run([gpu, png] + args + ["--raw-out", out_raw], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w), r.stdout

    def python(length, angle, **kw):
        chans = [np.ascontiguousarray(rgb[:, :, c]) for c in (2, 1, 0)]  # B, G, R
        fdr.wienerDeblur_RGB_optimized(chans, fdr.motionBlurKernel(length, angle), 0.01, mode=fdr.MODE_FAST, **kw)
        return chans

    planes, _ = run(["50", "30", "--pad", "smooth"], "smooth.f32")
    want = python(50, 30.0, pad=fdr.PAD_SMOOTH)
    plain = python(50, 30.0)
    for k in range(3):
        assert np.array_equal(planes[k], want[k]), (k, float(np.abs(planes[k] - want[k]).max()))
    assert not np.array_equal(planes[0], plain[0])
    planes, _ = run(["50", "30", "--pad", "zero"], "zero.f32")
    for k in range(3):
        assert np.array_equal(planes[k], plain[k]), k
    planes, _ = run(["50", "30", "--pad", "smooth", "--cls", "0.05"], "smooth_cls.f32")
    want = python(50, 30.0, pad=fdr.PAD_SMOOTH, cls_gamma=0.05)
    for k in range(3):
        assert np.array_equal(planes[k], want[k]), k
    planes, text = run(["auto", "auto", "--pad", "smooth"], "smooth_auto.f32")
    est = [ln for ln in text.splitlines() if ln.startswith("estimate:")]
    assert est, text[-500:]
    tok = est[0].split()
    length, angle = int(tok[tok.index("length") + 1]), float(tok[tok.index("angle") + 1])
    want = python(length, angle, pad=fdr.PAD_SMOOTH)
    for k in range(3):
        assert np.array_equal(planes[k], want[k]), k
    r = subprocess.run([gpu, png, "50", "30", "--pad", "smooth", "--mode", "parity"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "FDR_OPT_PAD_MODE" in r.stdout + r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    r = subprocess.run([gpu, png, "50", "30", "--pad", "wavy"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
