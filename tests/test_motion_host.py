"""CPU checks of the motion-blur estimate's float64 model (tests/_motion_model.py) before it judges the GPU (test_motion_gpu.py): it
recovers the blur of both golden pictures and of a synthetic grid, its confidence separates blurred from sharp scenes, a
single-precision implementation stays inside the GPU thresholds, injected faults land far outside them or far from the truth, and
the new C ABI / Python surface is declared, exported and listed."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _motion_model as mm

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
    return mm.load_golden(os.path.join(GOLDEN_DIR, name))


@pytest.mark.parametrize("name,L,a", mm.GOLDEN)
def test_model_recovers_golden(name, L, a):
    img = _golden(name)
    for M, N in mm.plan_sizes(*img.shape):
        e = mm.estimate(img, M, N)
        err = mm.endpoint_err(L, a, e.length, e.angle)
        print("MOTION\tmodel\t%s %dx%d\tL=%d a=%.1f conf=%.1f err=%.2f" % (name, M, N, e.length, e.angle, e.confidence, err))
        assert err <= mm.ENDPOINT_TOL, (name, M, N, e)
        assert e.confidence >= mm.CONF_BLURRED_MIN, (name, M, N, e)


@pytest.mark.parametrize("rows,cols", mm.SYNTH_SIZES)
def test_model_recovers_synthetic_grid(oracle, rows, cols):
    M, N = mm.plan_sizes(rows, cols)[1]
    bad = []
    for k, (L, a) in enumerate(mm.SYNTH_PAIRS):
        img = mm.blurred_scene(rows, cols, L, a, oracle.motion_blur_kernel(L, a), seed=1000 + k)
        e = mm.estimate(img, M, N)
        err = mm.endpoint_err(L, a, e.length, e.angle)
        sharp = mm.estimate(mm.scene(rows, cols, 1000 + k), M, N)
        print("MOTION\tmodel\t%dx%d L=%d a=%.1f\tgot L=%d a=%.1f conf=%.1f err=%.2f sharp conf=%.1f" %
              (rows, cols, L, a, e.length, e.angle, e.confidence, err, sharp.confidence))
        if not err <= mm.ENDPOINT_TOL or not e.confidence >= mm.CONF_BLURRED_MIN:
            bad.append((L, a, e))
        if not sharp.confidence <= mm.CONF_SHARP_MAX:
            bad.append(("sharp", L, a, sharp))
    assert not bad, bad


def test_defaults_and_edges():
    assert mm.defaults(330, 640) == (3, 82, 0.5, 360, 80)
    assert mm.defaults(782, 1920) == (3, 100, 0.5, 360, 98)
    assert mm.defaults(64, 64, 5, 9, 7.0) == (5, 9, 7.0, 26, 5)
    e, S = mm.estimate(np.zeros((40, 50)), 64, 64, table=True)
    assert e == mm.Estimate(0, 0.0, 0.0, 0.0, 360, 8) and not np.any(S)
    e = mm.estimate(np.full((40, 50), 3.0), 64, 64)
    assert all(math.isfinite(v) for v in e[:4])
    # the sampling points: theta = 90 deg is straight up (row -l), theta = 0 along the row
    c = np.zeros((64, 64))
    c[-7, 0], c[0, 7] = -1.0, -0.5
    S = mm.score_table(c, 3, 10, 0.5)
    assert abs(S[180, 7 - 3] + 1.0) < 1e-12 and S[0, 7 - 3] == -0.5
    assert mm.pick(S, 3, 0.5)[:2] == (7, 90.0)


def _cepstrum_f32(img, M, N):
    """the device's arithmetic on the CPU: float32 window, complex64 transforms, float32 log and scale"""
    x = mm.window_plane(img, M, N, dtype=np.float32)
    eps = np.float32(1e-6 * float(np.abs(x.astype(np.float64)).sum()))
    G = np.fft.fft2(x.astype(np.complex64))
    L = (np.log(np.abs(G).astype(np.float32) + eps) * np.float32(1.0 / (M * N))).astype(np.complex64)
    return np.real(np.fft.ifft2(L, norm="forward")).astype(np.float32)


def _table_f32(c, lo, hi, step):
    M, N = c.shape
    na = int(math.ceil(180.0 / step))
    cs, sn = mm.trig_table(na, step)
    ls = np.arange(lo, hi + 1, dtype=np.float64)
    y, x = -ls[None, :] * sn[:, None], ls[None, :] * cs[:, None]
    i0, j0 = np.floor(y), np.floor(x)
    fy, fx = (y - i0).astype(np.float32), (x - j0).astype(np.float32)
    i0, j0 = i0.astype(np.int64) % M, j0.astype(np.int64) % N
    i1, j1 = (i0 + 1) % M, (j0 + 1) % N
    one = np.float32(1)
    r0 = (one - fx) * c[i0, j0] + fx * c[i0, j1]
    r1 = (one - fx) * c[i1, j0] + fx * c[i1, j1]
    return ((one - fy) * r0 + fy * r1).astype(np.float32)


@pytest.mark.parametrize("name,L,a", mm.GOLDEN)
def test_single_precision_passes(name, L, a):
    img = _golden(name)
    for M, N in mm.plan_sizes(*img.shape):
        lo, hi, step, _, _ = mm.defaults(*img.shape)
        c64 = mm.cepstrum_model(img, M, N)
        c32 = _cepstrum_f32(img, M, N)
        S64 = mm.score_table(c64, lo, hi, step)
        S32 = _table_f32(c32, lo, hi, step)
        ce, te = float(np.abs(c32 - c64).max()), float(np.abs(S32 - S64).max())
        print("MOTION\tf32\t%s %dx%d\tcep=%.3g table=%.3g" % (name, M, N, ce, te))
        assert ce <= mm.CEP_TOL and te <= mm.TABLE_TOL
        assert mm.pick(S32, lo, step)[:2] == mm.pick(S64, lo, step)[:2]


def test_faults_fail():
    car, cat = _golden("car_blurred.png"), _golden("cat_blurred.png")
    M, N = mm.plan_sizes(*car.shape)[1]
    lo, hi, step, _, _ = mm.defaults(*car.shape)
    c = mm.cepstrum_model(car, M, N)
    # a y-up sign (sample row +l sin): 45 deg comes out as 135 deg, far from the truth
    c_flip = c[(-np.arange(M)) % M, :]  # sampling c at +y is sampling the row-flipped c at -y
    l_f, a_f = mm.pick(mm.score_table(c_flip, lo, hi, step), lo, step)[:2]
    assert abs(a_f - 135.0) <= 1.0 and mm.endpoint_err(40, 45.0, l_f, a_f) > 40
    # log |G|^2 in place of log |G|, and a missing 1 / (M N): the cepstrum far outside the per-bin threshold
    x = mm.window_plane(car, M, N)
    G = np.fft.fft2(x)
    eps = 1e-6 * np.abs(x).sum()
    c_sq = np.real(np.fft.ifft2(np.log(np.abs(G) ** 2 + eps)))
    c_mn = np.real(np.fft.ifft2(np.log(np.abs(G) + eps), norm="forward"))
    for bad in (c_sq, c_mn):
        assert float(np.abs(bad - c).max()) > 1e4 * mm.CEP_TOL
    # swapped row and column sampling on the cat: 30 deg comes out as 60 deg
    M2, N2 = mm.plan_sizes(*cat.shape)[1]
    lo2, hi2, step2, _, _ = mm.defaults(*cat.shape)
    c2 = mm.cepstrum_model(cat, M2, N2)
    n_angles = int(math.ceil(180.0 / step2))
    cs, sn = mm.trig_table(n_angles, step2)
    ls = np.arange(lo2, hi2 + 1, dtype=np.float64)
    y, xx = ls[None, :] * cs[:, None], -ls[None, :] * sn[:, None]  # row from cos, column from -sin
    S_sw = c2[np.round(y).astype(np.int64) % M2, np.round(xx).astype(np.int64) % N2]
    l_s, a_s = mm.pick(S_sw, lo2, step2)[:2]
    good = mm.estimate(cat, M2, N2)
    assert mm.endpoint_err(50, 30.0, good.length, good.angle) <= mm.ENDPOINT_TOL
    assert mm.endpoint_err(50, 30.0, l_s, a_s) > 20, (l_s, a_s)


NAMES = ("fdr_cepstrum_f32", "fdr_cepstrum_f32_dev", "fdr_estimate_motion_f32", "fdr_estimate_motion_f32_dev")


def test_symbols_and_surface(fdr):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fdr.h")).read()
    assert re.search(r"typedef struct fdr_motion_estimate \{[^}]*int length;[^}]*double angle_deg;[^}]*float score;[^}]*float confidence;"
                     r"[^}]*int n_angles;[^}]*int n_lengths;[^}]*\} fdr_motion_estimate;", hdr)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in NAMES:
        assert re.search(r"\bint %s\(fdr_plan\* plan," % name, hdr), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    assert [f[0] for f in fdr.MotionEstimateC._fields_] == ["length", "angle_deg", "score", "confidence", "n_angles", "n_lengths"]
    assert fdr.MotionEstimate._fields == ("length", "angle", "score", "confidence", "n_angles", "n_lengths")
    sig = inspect.signature(fdr.Plan.estimate_motion)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [
        ("img", inspect.Parameter.empty), ("min_length", 0), ("max_length", 0), ("angle_step", 0.0), ("scores", False)]
    for meth in ("cepstrum", "cepstrum_dev", "estimate_motion_dev"):
        assert callable(getattr(fdr.Plan, meth)), meth
    sig = inspect.signature(fdr.estimateMotionBlur)
    assert sig.parameters["device"].default == 0 and list(sig.parameters)[0] == "img"
    # the table shape Python allocates for scores=True follows the library's defaults
    for args in ((330, 640, 0, 0, 0.0), (782, 1920, 0, 0, 0.0), (64, 64, 5, 9, 7.0), (100, 100, 2, 20, 0.25)):
        assert fdr._motion_table_shape(*args) == mm.defaults(*args)[3:], args
    assert fdr._motion_plan_size(330, 640) == (360, 640) and fdr._motion_plan_size(20, 20) == (32, 32)
