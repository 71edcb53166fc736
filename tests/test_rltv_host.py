"""CPU pins of tests/_rltv_model.py, the float64 model of Richardson-Lucy with a total-variation prior, before it judges the device
(test_rltv_gpu.py): the operator identities, lambda = 0 as the unregularised forms, injected faults, the two arithmetic regimes of
the explicit step, the quality claims on two scenes, the public surface and the refusals that need no device.  No GPU needed.
Cases print an `RLTV` line with their measured values (pytest -s)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from _rl_model import centred_psf, dense_psf, psnr, rel_err, rl_model, smooth_image
from _rlfree_model import rlfree_model
from _rltv_model import (EPS, FAULTS, MAX_LAMBDA, QUALITY_EPS, QUALITY_LAMBDA, QUALITY_N, best_plain_iterate, quality_case, quality_run,
                         rltv_free_model, rltv_model, tv_div, tv_factor, tv_g, tv_grad)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(R, C, seed):
    rng = np.random.default_rng(seed)
    return {"random": rng.random((R, C)), "smooth": smooth_image(R, C, seed).astype(np.float64), "flat": np.full((R, C), 0.7),
            "tiny": 0.5 + 1e-3 * rng.random((R, C)), "steps": np.round(3 * rng.random((R, C))) / 3}


def test_div_is_minus_the_adjoint_of_grad():
    """<grad u, p> = -<u, div p> for every u and every p = (px, py) that is 0 where the replicate edge makes the gradient 0 (px in the
    last column, py in the last row: p = grad u / m always is): div = -D^T"""
    rng = np.random.default_rng(1)
    for R, C in ((1, 1), (1, 9), (9, 1), (7, 12), (33, 20)):
        u, px, py = rng.standard_normal((3, R, C))
        px[:, -1] = 0
        py[-1, :] = 0
        gx, gy = tv_grad(u)
        lhs = float(np.sum(gx * px + gy * py))
        rhs = -float(np.sum(u * tv_div(px, py)))
        scale = max(1.0, float(np.sum(np.abs(gx * px)) + np.sum(np.abs(gy * py))))
        print("RLTV\tadjoint\t%dx%d\tdefect=%.3g" % (R, C, abs(lhs - rhs) / scale))
        assert abs(lhs - rhs) <= 1e-12 * scale, (R, C)
        assert np.all(gx[:, -1] == 0) and np.all(gy[-1, :] == 0)


def test_g_stays_above_one_half_at_the_largest_lambda():
    worst = 9.0
    for seed, (R, C) in enumerate(((64, 64), (37, 101), (1, 50), (50, 1))):
        for name, u in _inputs(R, C, seed).items():
            for eps in (1e-3, 1e-6, 0.05):
                for dtype in (np.float64, np.float32):
                    g = tv_g(u, MAX_LAMBDA, eps, dtype)  # asserts g >= 0.5 itself
                    worst = min(worst, float(g.min()))
                    assert float(g.max()) <= 1 + MAX_LAMBDA * (2 + np.sqrt(2)) + 1e-6
    print("RLTV\tg min\t%.4f" % worst)
    assert worst >= 1 - MAX_LAMBDA * (2 + np.sqrt(2)) - 1e-6  # 0.573


def test_flat_image_gives_factor_one_exactly():
    for dtype in (np.float64, np.float32):
        for shape in ((1, 1), (5, 7), (64, 65)):
            f = tv_factor(np.full(shape, 0.37), MAX_LAMBDA, 1e-6, dtype=dtype)
            assert f.dtype == dtype and np.all(f == 1)
            w = np.random.default_rng(2).random(shape)
            w[0, 0] = 0
            fw = tv_factor(np.full(shape, 0.37), MAX_LAMBDA, 1e-6, w=w, dtype=dtype)
            assert np.array_equal(fw, w.astype(dtype)) and fw[0, 0] == 0


def _small_case():
    M, N, rows, cols = 64, 128, 37, 101
    return M, N, smooth_image(M, N, 8)[:rows, :cols] - np.float32(0.05), centred_psf(dense_psf(5, 5), M, N)


def test_lambda_zero_is_the_unregularised_form():
    M, N, d, psf = _small_case()
    w = (np.random.default_rng(3).random(d.shape) > 0.1).astype(np.float32)
    for dtype in (np.float64, np.float32):
        for n in (0, 1, 5):
            assert np.array_equal(rltv_model(d, psf, M, N, n, 0.0, dtype=dtype), rl_model(d, psf, M, N, n, dtype=dtype))
            for shape in (None, (M, N)):
                assert np.array_equal(rltv_free_model(d, psf, M, N, n, 0.0, weights=w, out_shape=shape, dtype=dtype),
                                      rlfree_model(d, psf, M, N, n, weights=w, out_shape=shape, dtype=dtype))
    # and a prior changes the result
    assert rel_err(rltv_model(d, psf, M, N, 5, 0.01), rl_model(d, psf, M, N, 5)) > 1e-4


@pytest.mark.parametrize("fault", FAULTS)
def test_faults_are_visible(fault):
    """every fault variant moves the factor (where it acts on the factor) and both forms' results far beyond the device tolerances"""
    M, N, d, psf = _small_case()
    d = d + np.float32(0.02) * np.random.default_rng(5).standard_normal(d.shape).astype(np.float32)
    lam, eps = 0.05, 1e-3
    if fault != "factor_new_u":
        u = np.maximum(d.astype(np.float64), 0)
        e = float(np.max(np.abs(tv_factor(u, lam, eps, fault=fault) - tv_factor(u, lam, eps))))
        print("RLTV\tfault\t%s\tfactor diff=%.3g" % (fault, e))
        assert e > 1e-3, (fault, e)
    ep = rel_err(rltv_model(d, psf, M, N, 5, lam, eps, fault=fault), rltv_model(d, psf, M, N, 5, lam, eps))
    ef = rel_err(rltv_free_model(d, psf, M, N, 5, lam, eps, fault=fault), rltv_free_model(d, psf, M, N, 5, lam, eps))
    print("RLTV\tfault\t%s\tplain rel=%.3g free rel=%.3g" % (fault, ep, ef))
    assert ep > 1e-3 and ef > 1e-3, (fault, ep, ef)


@pytest.fixture(scope="module")
def full_case():
    return quality_case("full")


@pytest.fixture(scope="module")
def crop_case():
    return quality_case("crop")


def test_large_eps_repeats_across_arithmetics(full_case):
    """lambda = 0.01, eps = 0.05: the float32 run of the model stays within 5e-6 of the float64 run through 100 steps at 256^2
    (measured 7.7e-7)"""
    worst = 0.0
    for n in (3, 10, 30, 100):
        a = quality_run(full_case, n, 0.01, 0.05)
        b = quality_run(full_case, n, 0.01, 0.05, dtype=np.float32)
        e = float(np.max(np.abs(a - b)))
        worst = max(worst, e)
        print("RLTV\tregime\teps=0.05 n=%d\tmax=%.3g" % (n, e))
    assert worst <= 5e-6, worst


def test_small_eps_drifts_but_keeps_its_quality(full_case):
    """lambda = 0.01, eps = 1e-3 (well below 4 lambda max(u) = 0.04): the two arithmetics agree at n = 3, drift apart in max-norm by
    n = 30, and still give the same PSNR to 0.01 dB (measured: 9.2e-6 at n = 3, 2.8e-2 at n = 30, rms 6.4e-4, 0.0001 dB; 0.004 dB at
    n = 100)"""
    out = {}
    for n in (3, 30, 100):
        a = quality_run(full_case, n, 0.01, 1e-3)
        b = quality_run(full_case, n, 0.01, 1e-3, dtype=np.float32)
        out[n] = (float(np.max(np.abs(a - b))), float(np.sqrt(np.mean((a - b) ** 2))), abs(psnr(a, full_case["truth"]) - psnr(b, full_case["truth"])))
        print("RLTV\tregime\teps=1e-3 n=%d\tmax=%.3g rms=%.3g dPSNR=%.4f dB" % ((n,) + out[n]))
    assert out[3][0] <= 1e-4
    assert out[30][0] >= 1e-3, "no drift: the regime the documentation warns of is gone"
    assert out[30][2] <= 0.01 and out[100][2] <= 0.01


@pytest.mark.parametrize("which", ["full", "crop"])
def test_the_prior_beats_the_best_unregularised_iterate(which, full_case, crop_case):
    """the quality claim on both scenes: n = 100 with the prior lies at least 3 dB above the best iterate k <= 100 without it, and
    above the blurred input (measured: full 30.87 against 23.41 at k = 21, blurred 20.13; crop 32.35 against 24.68 at k = 14,
    blurred 21.70)"""
    case = full_case if which == "full" else crop_case
    blurred = psnr(case["d"], case["truth"])
    k, best = best_plain_iterate(case, 100)
    tv = psnr(quality_run(case, QUALITY_N, QUALITY_LAMBDA, QUALITY_EPS), case["truth"])
    late = psnr(quality_run(case, QUALITY_N, 0.0), case["truth"])
    print("RLTV\tquality (model)\t%s\tblurred %.2f dB, unregularised best %.2f dB at k=%d and %.2f dB at n=100, with the prior %.2f dB"
          % (which, blurred, best, k, late, tv))
    assert tv >= best + 3.0, (tv, best)
    assert tv > blurred and late < best
    if which == "crop":  # the prior does not replace the free boundary
        plain = psnr(rltv_model(case["d"], case["psf"], case["M"], case["N"], QUALITY_N, QUALITY_LAMBDA, QUALITY_EPS), case["truth"])
        print("RLTV\tquality (model)\tcrop, plain form with the prior %.2f dB" % plain)
        assert plain < 15.0


def test_flux_loss_is_small(full_case):
    """the prior gives up exact flux conservation: below 0.1 % at lambda = 0.01 (measured 0.04 %)"""
    u = quality_run(full_case, 100, 0.01, 1e-3)
    loss = abs(float(u.sum()) / float(np.maximum(full_case["d"], 0).sum(dtype=np.float64)) - 1)
    print("RLTV\tflux\tloss=%.3g" % loss)
    assert loss < 1e-3


RLTV_FUNCS = ("fdr_richardson_lucy_tv_f32", "fdr_richardson_lucy_tv_f32_dev", "fdr_rl_tv_factor_f32_dev")
FIELDS = (("int", "iterations"), ("int", "free_boundary"), ("float", "lambda"), ("float", "eps"), ("int", "norm_area"), ("float", "cov_sigma"),
          ("int", "out_rows"), ("int", "out_cols"))


def test_symbols_and_surface(fdr):
    header = open(os.path.join(ROOT, "include", "fdr.h")).read()
    m = re.search(r"typedef\s+struct\s+fdr_rl_tv_params\s*\{(.*?)\}\s*fdr_rl_tv_params\s*;", header, re.S)
    assert m, "fdr_rl_tv_params is not in the header"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = tuple((t, n.strip()) for t, names in re.findall(r"\b(int|float)\s+([^;]+);", body) for n in names.split(","))
    assert fields == FIELDS, fields
    assert [f[0] for f in fdr.RlTvParams._fields_] == [n for _, n in FIELDS]
    assert [f[1] for f in fdr.RlTvParams._fields_] == [ctypes.c_int if t == "int" else ctypes.c_float for t, _ in FIELDS]
    assert ctypes.sizeof(fdr.RlTvParams) == 32
    assert re.search(r"#define\s+FDR_RLTV_MAX_LAMBDA\s+0\.125f", header) and re.search(r"#define\s+FDR_RLTV_EPS\s+1e-3f", header)
    assert re.search(r"#define\s+FDR_VERSION\s+300\b", header)
    assert fdr.RLTV_MAX_LAMBDA == MAX_LAMBDA == 0.125 and abs(fdr.RLTV_EPS - EPS) < 1e-9
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in RLTV_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    sig = inspect.signature(fdr.Plan.richardson_lucy_tv).parameters
    assert list(sig)[:7] == ["self", "img", "iterations", "lam", "eps", "free_boundary", "weights"]
    assert (sig["eps"].default, sig["free_boundary"].default, sig["weights"].default, sig["norm_area"].default) == (0.0, False, None, fdr.NORM_NONE)
    sig = inspect.signature(fdr.Plan.richardson_lucy_tv_dev).parameters
    assert list(sig)[:9] == ["self", "d_img", "rows", "cols", "stride", "d_out", "out_stride", "iterations", "lam"]
    assert callable(fdr.Plan.rl_tv_factor_dev) and callable(fdr.rl_tv_factor_dev)
    sig = inspect.signature(fdr.richardsonLucyTV_myfft).parameters
    assert list(sig)[:7] == ["img", "psf", "iterations", "lam", "eps", "free_boundary", "weights"]
    assert (sig["eps"].default, sig["free_boundary"].default, sig["weights"].default) == (0, False, None)


def test_refusals_without_a_device(fdr):
    """what the entry points refuse before they touch a device: null pointers, and for the factor every bad argument"""
    L = fdr.lib
    img = np.ones((8, 32), dtype=np.float32)
    out = np.empty_like(img)
    prm = fdr.RlTvParams(1, 0, 0.01, 0.0, 2, 1e-2, 0, 0)
    for args in ((None, img.ctypes.data, out.ctypes.data), (1, None, out.ctypes.data), (1, img.ctypes.data, None)):
        h, i, o = args
        assert L.fdr_richardson_lucy_tv_f32(h, i, 8, 32, 32, None, 0, o, 32, ctypes.byref(prm)) == -1
        assert L.fdr_richardson_lucy_tv_f32_dev(h, i, 8, 32, 32, None, 0, o, 32, ctypes.byref(prm), None) == -1
        assert b"null argument" in L.fdr_last_error()
    # the factor entry: the pointers are only compared, never followed, before the refusal
    u, o = img.ctypes.data, out.ctypes.data

    def factor(d_u=u, rows=8, cols=32, stride=32, d_w=None, lam=0.01, eps=1e-3, d_out=o, ostride=32):
        return L.fdr_rl_tv_factor_f32_dev(0, d_u, rows, cols, stride, d_w, lam, eps, d_out, ostride, None)

    assert factor(d_u=None) == -1 and factor(d_out=None) == -1
    assert factor(rows=0) == -1 and factor(cols=0) == -1 and factor(rows=-3) == -1
    assert factor(stride=31) == -1 and factor(ostride=31) == -1 and b"stride" in L.fdr_last_error()
    for lam in (-0.01, 0.126, float("nan"), float("inf")):
        assert factor(lam=lam) == -1 and b"lambda" in L.fdr_last_error(), lam
    for eps in (-1e-3, float("nan"), float("inf")):
        assert factor(eps=eps) == -1 and b"eps" in L.fdr_last_error(), eps
    assert factor(d_out=u) == -1 and factor(d_out=u + 4 * (7 * 32 + 31)) == -1 and b"overlaps" in L.fdr_last_error()
    assert factor(d_w=o) == -1 and b"overlaps" in L.fdr_last_error()
