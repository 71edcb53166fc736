"""The motion-blur estimate (fdr_cepstrum_f32*, fdr_estimate_motion_f32*) on the MI355X, against the float64 model of
tests/_motion_model.py: the cepstrum bin by bin on power-of-two, non-square, mixed-radix and strided plans, the score table and
its pick, recovery of the golden pictures and of a synthetic grid, low confidence on sharp scenes, edge inputs, determinism,
isolation from the Wiener / RL state, the refusals and the CLI.  Each case prints a `MOTION` line with its measured values
(pytest -s)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _motion_model as mm
from _spectral import tone_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def _golden(name):
    return mm.load_golden(os.path.join(GOLDEN_DIR, name)).astype(np.float32)


def _dev_cepstrum(p, img, stride):
    """fdr_cepstrum_f32_dev on a device copy of img with row stride `stride` (the padding columns NaN: never read)"""
    import torch
    rows, cols = img.shape
    src = np.full((rows, stride), np.nan, dtype=np.float32)
    src[:, :cols] = img
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.empty((p.M, p.N), dtype=torch.float32, device="cuda")
    p.cepstrum_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_in


# (M, N, flags, image) -- image: ("tone", rows, cols) or a golden picture's channel mean
CEP_CASES = [(64, 64, 0, ("tone", 64, 64)), (512, 512, 0, ("tone", 500, 383)), (4096, 4096, 0, ("tone", 4096, 4096)),
             (8192, 8192, 0, ("tone", 8000, 8192)), (2048, 256, 0, ("tone", 2048, 256)), (256, 2048, 0, ("tone", 256, 2048)),
             (360, 640, 2048, "car_blurred.png"), (800, 1920, 2048, "cat_blurred.png")]


def _image(spec, M, N):
    if isinstance(spec, str):
        return _golden(spec)
    _, rows, cols = spec
    return tone_image(M, N, M + 3 * N, rows, cols) * np.float32(255)


@pytest.mark.parametrize("M,N,flags,spec", CEP_CASES)
def test_cepstrum_per_bin(fdr, M, N, flags, spec):
    img = _image(spec, M, N)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        got = p.cepstrum(img)
    want = mm.cepstrum_model(img.astype(np.float64), M, N)
    err = np.abs(got - want)
    k = int(np.argmax(err))
    print("MOTION\tcepstrum\t%dx%d win %dx%d\tmax=%.3g at %s\tc00=%.4g" % (M, N, img.shape[0], img.shape[1], err.flat[k],
                                                                          np.unravel_index(k, err.shape), want[0, 0]))
    assert np.all(np.isfinite(got))
    assert err.flat[k] <= mm.CEP_TOL


def test_cepstrum_strided_window(fdr):
    img = _golden("cat_blurred.png")  # 782 x 1920
    M, N, stride = 1024, 2048, 1931
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        got, _ = _dev_cepstrum(p, img, stride)
        host = p.cepstrum(img)
    want = mm.cepstrum_model(img.astype(np.float64), M, N)
    err = float(np.abs(got - want).max())
    print("MOTION\tcepstrum\t%dx%d win 782x1920 stride %d\tmax=%.3g" % (M, N, stride, err))
    assert err <= mm.CEP_TOL
    assert np.array_equal(got, host), "the strided _dev form and the host form differ"


TABLE_CASES = [(512, 1024, 0, "car_blurred.png"), (360, 640, 2048, "car_blurred.png"), (1024, 2048, 0, "cat_blurred.png"),
               (800, 1920, 2048, "cat_blurred.png")]


def _check_table(est, S, want_S, lo, step, what):
    err = float(np.abs(S.astype(np.float64) - want_S).max())
    l_m, a_m, s_m, c_m = mm.pick(want_S, lo, step)
    at_gpu = want_S[int(round(est.angle / step)), est.length - lo]
    print("MOTION\ttable\t%s\tmax=%.3g\tgpu L=%d a=%.17g conf=%.2f\tmodel L=%d a=%.1f conf=%.2f" % (what, err, est.length, est.angle,
                                                                                                    est.confidence, l_m, a_m, c_m))
    assert err <= mm.TABLE_TOL, what
    assert (est.length, est.angle) == (l_m, a_m) or at_gpu - s_m <= 2 * mm.TABLE_TOL, what
    # the pick and the confidence from the returned table, in double, as the model computes them
    l_g, a_g, s_g, c_g = mm.pick(S, lo, step)
    assert (est.length, est.angle, est.score) == (l_g, a_g, np.float32(s_g)), what
    assert abs(est.confidence - c_g) <= 1e-5 * max(1.0, abs(c_g)), what


@pytest.mark.parametrize("M,N,flags,name", TABLE_CASES)
def test_score_table_against_model(fdr, M, N, flags, name):
    img = _golden(name)
    lo, hi, step, na, nl = mm.defaults(*img.shape)
    want_S = mm.score_table(mm.cepstrum_model(img.astype(np.float64), M, N), lo, hi, step)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        est, S = p.estimate_motion(img, scores=True)
    assert (est.n_angles, est.n_lengths) == (na, nl) and S.shape == (na, nl)
    _check_table(est, S, want_S, lo, step, "%s %dx%d" % (name, M, N))


def test_score_table_arguments(fdr):
    """non-default lengths and steps, a step that does not divide 180"""
    img = _golden("car_blurred.png")
    M, N = 512, 1024
    c = mm.cepstrum_model(img.astype(np.float64), M, N)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for lo, hi, step in ((2, 60, 1.0), (30, 50, 0.7), (5, 254, 7.0), (3, 3, 90.0)):
            est, S = p.estimate_motion(img, lo, hi, step, scores=True)
            assert S.shape == (int(math.ceil(180.0 / step)), hi - lo + 1)
            _check_table(est, S, mm.score_table(c, lo, hi, step), lo, step, "car %dx%d %d..%d step %g" % (M, N, lo, hi, step))


@pytest.mark.parametrize("name,L,a", mm.GOLDEN)
def test_recovers_golden(fdr, name, L, a):
    img = _golden(name)
    for M, N in mm.plan_sizes(*img.shape):
        with fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_MIXED_RADIX) as p:
            e = p.estimate_motion(img)
        err = mm.endpoint_err(L, a, e.length, e.angle)
        print("MOTION\tgolden\t%s %dx%d\tL=%d a=%.1f conf=%.1f err=%.2f" % (name, M, N, e.length, e.angle, e.confidence, err))
        assert err <= mm.ENDPOINT_TOL and e.confidence >= mm.CONF_BLURRED_MIN, (name, M, N, e)
    # the module-level call (mixed-radix plan of fdr_optimal_dft_size) on the colour picture
    from PIL import Image
    rgb = np.asarray(Image.open(os.path.join(GOLDEN_DIR, name)).convert("RGB"), dtype=np.float32)
    e = fdr.estimateMotionBlur(rgb)
    assert mm.endpoint_err(L, a, e.length, e.angle) <= mm.ENDPOINT_TOL and e.confidence >= mm.CONF_BLURRED_MIN, e


@pytest.mark.parametrize("rows,cols", mm.SYNTH_SIZES)
def test_recovers_synthetic_grid_and_sharp_scenes(fdr, rows, cols):
    bad = []
    for k, (L, a) in enumerate(mm.SYNTH_PAIRS):
        img = mm.blurred_scene(rows, cols, L, a, fdr.motionBlurKernel(L, a), seed=1000 + k).astype(np.float32)
        e = fdr.estimateMotionBlur(img)
        err = mm.endpoint_err(L, a, e.length, e.angle)
        sharp = fdr.estimateMotionBlur(mm.scene(rows, cols, 1000 + k).astype(np.float32))
        print("MOTION\tsynth\t%dx%d L=%d a=%.1f\tgot L=%d a=%.1f conf=%.1f err=%.2f\tsharp conf=%.2f" %
              (rows, cols, L, a, e.length, e.angle, e.confidence, err, sharp.confidence))
        if not (err <= mm.ENDPOINT_TOL and e.confidence >= mm.CONF_BLURRED_MIN):
            bad.append((L, a, e))
        if not sharp.confidence <= mm.CONF_SHARP_MAX:
            bad.append(("sharp", L, a, sharp))
    assert not bad, bad


def test_edge_inputs(fdr):
    with fdr.Plan(64, 128, fdr.MODE_FAST) as p:
        z = np.zeros((50, 100), dtype=np.float32)
        e, S = p.estimate_motion(z, scores=True)
        assert e == fdr.MotionEstimate(0, 0.0, 0.0, 0.0, 360, 10), e
        assert S.shape == (360, 10) and not np.any(S)
        c = p.cepstrum(z)
        assert not np.any(c)
        k = p.estimate_motion(np.full((50, 100), 7.0, dtype=np.float32))
        assert all(math.isfinite(v) for v in k[:4]), k
        assert np.all(np.isfinite(p.cepstrum(np.full((50, 100), 7.0, dtype=np.float32))))
        # the zero result does not stick: a picture afterwards is estimated as usual
        img = tone_image(64, 128, 5, 50, 100)
        lo, hi, step, _, _ = mm.defaults(50, 100)
        est, S = p.estimate_motion(img, scores=True)
        _check_table(est, S, mm.score_table(mm.cepstrum_model(img.astype(np.float64), 64, 128), lo, hi, step), lo, step, "tone 64x128")


def test_determinism_and_dev_forms(fdr):
    import torch
    img = _golden("cat_blurred.png")
    for M, N, flags in ((1024, 2048, 0), (800, 1920, fdr.FLAG_MIXED_RADIX)):
        with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
            c1, c2 = p.cepstrum(img), p.cepstrum(img)
            assert np.array_equal(c1, c2), "two cepstra differ"
            e1, S1 = p.estimate_motion(img, scores=True)
            e2, S2 = p.estimate_motion(img, scores=True)
            assert e1 == e2 and np.array_equal(S1, S2), "two estimates differ"
            d_img = torch.from_numpy(img).cuda()
            d_S = torch.full(S1.shape, float("nan"), dtype=torch.float32, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            e3 = p.estimate_motion_dev(d_img.data_ptr(), img.shape[0], img.shape[1], img.shape[1], d_scores=d_S.data_ptr(), stream=stream)
            assert e3 == e1 and np.array_equal(d_S.cpu().numpy(), S1), "the _dev estimate differs from the host form"
            e4 = p.estimate_motion_dev(d_img.data_ptr(), img.shape[0], img.shape[1], img.shape[1])
            assert e4 == e1


def test_isolation(fdr):
    import torch
    from _rl_model import NORM_NONE
    M, N = 512, 1024
    img = tone_image(M, N, 21, 400, 900)
    car = _golden("car_blurred.png")
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_psf_motion(15, 30.0, 0.01)
        w_before = p.wiener(img)
        n = p.filter_bytes()
        blk = torch.empty(n, dtype=torch.uint8, device="cuda")
        p.export_filter_dev(blk.data_ptr(), n)
        torch.cuda.synchronize()
        f_before = blk.cpu().numpy().copy()
        p.set_operator_psf_motion(50, 123.4)
        rl_before = p.richardson_lucy(img, 5, NORM_NONE)
        blur_before = p.blur(img)
        p.cepstrum(car)
        p.estimate_motion(car, scores=True)
        p.export_filter_dev(blk.data_ptr(), n)
        torch.cuda.synchronize()
        assert np.array_equal(blk.cpu().numpy(), f_before), "the estimate changed the Wiener filter"
        assert np.array_equal(p.wiener(img), w_before), "Wiener output changed after an estimate"
        assert np.array_equal(p.richardson_lucy(img, 5, NORM_NONE), rl_before), "RL output changed after an estimate"
        assert np.array_equal(p.blur(img), blur_before), "blur output changed after an estimate"
    with fdr.Plan(360, 640, fdr.MODE_FAST, flags=fdr.FLAG_MIXED_RADIX) as q:  # the mixed transform's scratch is the plan's work
        q.set_psf_motion(40, 45.0, 0.01)
        before = q.wiener(car)
        q.estimate_motion(car)
        assert np.array_equal(q.wiener(car), before), "mixed-radix Wiener output changed after an estimate"


def test_refusals(fdr):
    import torch
    L = fdr.lib
    img = tone_image(64, 64, 3)
    out = np.empty((64, 64), dtype=np.float32)
    est = fdr.MotionEstimateC()

    def calls(p, rows, cols, stride, lo=0, hi=0, step=0.0, null_est=False):
        """(host rc, _dev rc); valid buffers of rows x stride (no table), so that a refusal that did not happen could do no harm"""
        e = None if null_est else ctypes.byref(est)
        n = max(rows, 1) * max(stride, 1) + 64
        hbuf = np.zeros(n, dtype=np.float32)
        dbuf = torch.zeros(n, dtype=torch.float32, device="cuda")
        rc = (L.fdr_estimate_motion_f32(p._h, hbuf.ctypes.data, rows, cols, stride, lo, hi, step, e, None),
              L.fdr_estimate_motion_f32_dev(p._h, ctypes.c_void_p(dbuf.data_ptr()), rows, cols, stride, lo, hi, step, e, None, None))
        torch.cuda.synchronize()
        return rc

    # plans the estimate does not run on: refused, the plan still restores
    psf = fdr.motionBlurKernel(15, 30.0)
    for M, N, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (360, 640, fdr.MODE_PARITY, fdr.FLAG_ANY_SIZE, "any size"),
                                    (360, 640, fdr.MODE_FAST, fdr.FLAG_ANY_SIZE, "any size fast"), (16, 64, fdr.MODE_FAST, 0, "M < 32"),
                                    (64, 16, fdr.MODE_FAST, 0, "N < 32"), (64, 16384, fdr.MODE_FAST, 0, "N > 8192")):
        with fdr.Plan(M, N, mode, flags=flags) as p:
            p.set_psf(psf, 0.01)
            im = tone_image(M, N, 2, min(M, 64), min(N, 64))
            before = p.wiener(im)
            r, c = min(M, 64), min(N, 64)
            assert calls(p, r, c, c) == (-1, -1), what
            assert L.fdr_cepstrum_f32(p._h, im.ctypes.data, r, c, c, out.ctypes.data) == -1, what
            assert np.array_equal(p.wiener(im), before), what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert calls(p, 64, 64, 64) == (-4, -4)
        assert L.fdr_cepstrum_f32(p._h, img.ctypes.data, 64, 64, 64, out.ctypes.data) == -4
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        good = p.estimate_motion(img, scores=True)
        bad_args = [dict(rows=15, cols=64, stride=64), dict(rows=64, cols=15, stride=64), dict(rows=65, cols=64, stride=64),
                    dict(rows=64, cols=65, stride=65), dict(rows=64, cols=64, stride=63), dict(rows=-1, cols=64, stride=64),
                    dict(rows=64, cols=64, stride=64, lo=-1), dict(rows=64, cols=64, stride=64, hi=-1),
                    dict(rows=64, cols=64, stride=64, lo=1), dict(rows=64, cols=64, stride=64, lo=10, hi=9),
                    dict(rows=64, cols=64, stride=64, lo=17),  # above the default max_length 16
                    dict(rows=64, cols=64, stride=64, hi=31), dict(rows=64, cols=64, stride=64, step=-0.5),
                    dict(rows=64, cols=64, stride=64, step=90.0001), dict(rows=64, cols=64, stride=64, step=float("nan")),
                    dict(rows=64, cols=64, stride=64, step=float("inf")), dict(rows=64, cols=64, stride=64, null_est=True),
                    dict(rows=64, cols=64, stride=64, lo=2, hi=30, step=5e-5)]  # a table above 2^26 entries
        for kw in bad_args:
            assert calls(p, **kw) == (-1, -1), kw
        for r, c, s in ((15, 64, 64), (64, 15, 64), (65, 64, 64), (64, 64, 63)):
            buf = np.zeros((max(r, 1), s), dtype=np.float32)
            assert L.fdr_cepstrum_f32(p._h, buf.ctypes.data, r, c, s, out.ctypes.data) == -1, (r, c, s)
        assert L.fdr_cepstrum_f32(p._h, None, 64, 64, 64, out.ctypes.data) == -1
        assert L.fdr_cepstrum_f32_dev(p._h, None, 64, 64, 64, None, None) == -1
        # the limits themselves are accepted, and the plan still gives the same answer
        assert p.estimate_motion(img, 2, 30, 90.0).n_angles == 2
        again = p.estimate_motion(img, scores=True)
        assert again[0] == good[0] and np.array_equal(again[1], good[1])


def test_cli_auto(fdr, tmp_path):
    """tools/cli/gpu <img> auto auto: one `estimate:` line, then exactly the run of <img> L A -- the same PNG bytes"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")
    png = os.path.join(GOLDEN_DIR, "car_blurred.png")
    a_png, b_png = str(tmp_path / "auto.png"), str(tmp_path / "given.png")
    r = subprocess.run([gpu, png, "auto", "auto", "--out", a_png], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^estimate: length (\d+) angle (\S+) confidence (\S+)$", r.stdout, re.M)
    assert m, r.stdout
    L, A, C = int(m.group(1)), m.group(2), float(m.group(3))
    print("MOTION\tcli\tL=%d A=%s conf=%.2f" % (L, A, C))
    assert mm.endpoint_err(40, 45.0, L, float(A)) <= mm.ENDPOINT_TOL and C >= mm.CONF_BLURRED_MIN
    assert "low confidence" not in r.stderr
    r2 = subprocess.run([gpu, png, str(L), A, "--out", b_png], capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert open(a_png, "rb").read() == open(b_png, "rb").read(), "auto auto wrote another picture than the printed L A"
    r3 = subprocess.run([gpu, png, "auto", "45"], capture_output=True, text=True, timeout=600)
    assert r3.returncode != 0 and "Usage" in r3.stdout
