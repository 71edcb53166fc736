"""CPU pins of tests/_pad_model.py, the float64 model of the smooth padding of the Wiener / CLS calls (FDR_OPT_PAD_MODE), before it
judges the device (test_pad_gpu.py): the ramp, the extension's defining properties, an element-by-element evaluation from four
source values, two injected faults, the quality table of the feature on cropped scenes, and the public surface.  No GPU needed.
Cases print a `PAD` line with their measured values (pytest -s)."""
import os
import re

import numpy as np
import pytest

from _pad_model import (MIN_GAIN_DB, PAD_SMOOTH, PAD_ZERO, QUALITY_K, QUALITY_SEEDS, QUALITY_SHAPES, centred_psf_plane, extend, psnr,
                        quality_case, quality_failures, quality_psf, ramp, restore_raw)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7, 8, 32), (8, 20, 8, 32), (5, 32, 8, 32), (3, 30, 16, 32), (15, 31, 16, 32), (37, 101, 64, 128)]  # rows, cols, M, N


def _window(rows, cols, seed):
    return np.random.default_rng(seed).uniform(0.1, 1.0, (rows, cols))


def property_failures(ext, d, M, N):
    """the defining properties of the extension, on ext(d, M, N) (an empty list: all hold)"""
    rows, cols = d.shape
    e = ext(d, M, N)
    bad = []
    if e.shape != (M, N) or not np.array_equal(e[:rows, :cols], d):
        bad.append("e differs from d on the window")
    lo, hi = d.min(), d.max()
    if e.min() < lo - 1e-12 or e.max() > hi + 1e-12:
        bad.append("e leaves the range of d (every element is a convex combination)")
    tol = 1e-12
    if cols < N:  # the first pad column leaves the last picture column, and the last one meets column 0, by one ramp step at most
        step = ramp(N - cols)[0]
        jump = np.abs(d[:, cols - 1] - d[:, 0])
        if np.any(np.abs(e[:rows, cols] - d[:, cols - 1]) > step * jump + tol):
            bad.append("first pad column: more than one ramp step away from the last picture column")
        if np.any(np.abs(e[:rows, N - 1] - e[:rows, 0]) > step * jump + tol):
            bad.append("last pad column: more than one ramp step away from its wrap neighbour, column 0")
    if rows < M:  # the same for the pad rows, over ALL columns (the corner included)
        step = ramp(M - rows)[0]
        jump = np.abs(e[rows - 1, :] - e[0, :])
        if np.any(np.abs(e[rows, :] - e[rows - 1, :]) > step * jump + tol):
            bad.append("first pad row: more than one ramp step away from the last picture row")
        if np.any(np.abs(e[M - 1, :] - e[0, :]) > step * jump + tol):
            bad.append("last pad row: more than one ramp step away from its wrap neighbour, row 0")
        if cols < N and np.any(e[rows:, cols:] < lo - 1e-12):
            bad.append("corner: below the range of d")
    return bad


def test_ramp():
    for n in (1, 2, 3, 12, 112, 513):
        t = ramp(n)
        assert t.shape == (n,)
        assert np.all(t > 0) and np.all(t < 1)
        assert np.all(np.diff(t) > 0)                        # monotone
        assert np.max(np.abs(t + t[::-1] - 1)) <= 1e-15      # ramp[j] + ramp[n-1-j] = 1
    assert abs(ramp(1)[0] - 0.5) <= 1e-16
    assert ramp(100)[0] < 1e-3 and ramp(100)[-1] > 1 - 1e-3  # starts at the picture's value, ends at the wrap neighbour's


@pytest.mark.parametrize("rows,cols,M,N", SHAPES)
def test_extension_properties(rows, cols, M, N):
    d = _window(rows, cols, rows * 131 + cols)
    assert property_failures(extend, d, M, N) == []


@pytest.mark.parametrize("rows,cols,M,N", SHAPES)
def test_extension_from_four_source_values(rows, cols, M, N):
    """every element straight from the formula of include/fdr.h: at most four values of d and two weights"""
    d = _window(rows, cols, 7)
    e = extend(d, M, N)
    tc = ramp(N - cols) if cols < N else None
    tr = ramp(M - rows) if rows < M else None
    worst = 0.0
    for r in range(M):
        for c in range(N):
            rc, cc = min(r, rows - 1), min(c, cols - 1)
            t = tc[c - cols] if c >= cols else 0.0
            v = (1 - t) * d[rc, cc] + t * d[rc, 0]
            if r >= rows:
                s = tr[r - rows]
                v = (1 - s) * v + s * ((1 - t) * d[0, cc] + t * d[0, 0])
            worst = max(worst, abs(v - e[r, c]))
    print("PAD\tfour values\t%dx%d in %dx%d\terr=%.3g" % (rows, cols, M, N, worst))
    assert worst <= 1e-15


def test_full_window_is_the_identity():
    d = _window(16, 32, 2)
    assert np.array_equal(extend(d, 16, 32), d)
    psf = quality_psf(5, 30.0, 7)
    assert np.array_equal(restore_raw(d, psf, 0.01, 16, 32, PAD_SMOOTH), restore_raw(d, psf, 0.01, 16, 32, PAD_ZERO))


def test_extension_is_linear():
    a, b = _window(5, 20, 3), _window(5, 20, 4)
    lhs = extend(2.5 * a - 0.75 * b, 16, 32)
    rhs = 2.5 * extend(a, 16, 32) - 0.75 * extend(b, 16, 32)
    assert np.max(np.abs(lhs - rhs)) <= 1e-14


@pytest.mark.parametrize("fault", ["reversed_ramp", "rows_from_zero_padded"])
def test_model_tests_catch_injected_faults(fault):
    """the property check passes on the model and fails on each faulty variant, on every shape that has the padding the fault lives in"""
    caught = 0
    for rows, cols, M, N in SHAPES:
        d = _window(rows, cols, 11)
        assert property_failures(extend, d, M, N) == []
        has = (rows < M and cols < N) if fault == "rows_from_zero_padded" else (rows < M or cols < N)
        if not has or (fault == "reversed_ramp" and max(M - rows, 1) <= 1 and max(N - cols, 1) <= 1):
            continue
        bad = property_failures(lambda x, m, n: extend(x, m, n, fault=fault), d, M, N)
        print("PAD\tfault %s\t%dx%d in %dx%d\t%s" % (fault, rows, cols, M, N, "; ".join(bad)))
        assert bad, (fault, rows, cols, M, N)
        caught += 1
    assert caught >= 3


@pytest.mark.parametrize("rows,cols,M,N", QUALITY_SHAPES)
def test_quality_table(rows, cols, M, N):
    """a crop of a periodically blurred scene restored by W = conj(H) / (|H|^2 + K): the smooth extension beats zero padding by at
    least MIN_GAIN_DB and beats the blurred input; PSNR over the whole window against the true crop, float64 model"""
    psf = quality_psf()
    h = centred_psf_plane(psf, M, N)
    bad = []
    for seed in QUALITY_SEEDS:
        truth, blurred = quality_case(psf, seed, rows, cols)
        pz = psnr(restore_raw(blurred, h, QUALITY_K, M, N, PAD_ZERO)[:rows, :cols], truth)
        ps = psnr(restore_raw(blurred, h, QUALITY_K, M, N, PAD_SMOOTH)[:rows, :cols], truth)
        pb = psnr(blurred, truth)
        what = "%dx%d in %dx%d seed %d" % (rows, cols, M, N, seed)
        print("PAD\tquality\t%s\tblurred=%.2f\tzero=%.2f\tsmooth=%.2f\tgain=%.2f\tover_blurred=%.2f" % (what, pb, pz, ps, ps - pz, ps - pb))
        bad += quality_failures(what, pb, pz, ps, MIN_GAIN_DB)
    assert not bad, "\n".join(bad)


def test_public_surface(fdr):
    """the constants exist and match include/fdr.h; the null-plan error; the documented plan sizes"""
    hdr = open(os.path.join(ROOT, "include", "fdr.h")).read()
    for name, want in (("FDR_OPT_PAD_MODE", 5), ("FDR_PAD_ZERO", 0), ("FDR_PAD_SMOOTH", 1)):
        m = re.search(r"^#define\s+%s\s+(\d+)" % name, hdr, re.M)
        assert m and int(m.group(1)) == want, name
    assert fdr.OPT_PAD_MODE == 5 and fdr.PAD_ZERO == 0 and fdr.PAD_SMOOTH == 1
    assert fdr.lib.fdr_plan_set_option(None, fdr.OPT_PAD_MODE, 1) == -1
    assert b"null plan" in fdr.lib.fdr_last_error()
    assert fdr._pad_plan_size(400, 440, 21, 21) == (512, 512)
    assert fdr._pad_plan_size(500, 500, 21, 21) == (1024, 1024)   # 520 > 512
    assert fdr._pad_plan_size(512, 512, 15, 15) == (1024, 1024)   # a power-of-two picture: 4x the plan
    assert fdr._pad_plan_size(480, 640, 1, 1) == (512, 1024)
    assert fdr._pad_plan_size(2, 3, 1, 1) == (8, 32)
    assert fdr._pad_plan_size(200, 300, 15, 15) == fdr._rlfree_plan_size(200, 300, 15, 15)


def test_python_keyword_refuses_parity_before_device_work(fdr):
    img = np.zeros((16, 40), dtype=np.float32)
    psf = np.ones((3, 3), dtype=np.float32) / 9
    with pytest.raises(ValueError, match="MODE_FAST"):
        fdr.wienerDeblur_myfft(img, psf, 0.01, mode=fdr.MODE_PARITY, pad=fdr.PAD_SMOOTH)
    with pytest.raises(ValueError, match="MODE_FAST"):
        fdr.wienerDeblur_RGB_optimized([img], psf, 0.01, pad=fdr.PAD_SMOOTH)
    with pytest.raises(ValueError):
        fdr.wienerDeblur_myfft(img, psf, 0.01, mode=fdr.MODE_FAST, pad=7)
