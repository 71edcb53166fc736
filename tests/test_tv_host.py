"""CPU checks of the total-variation model (tests/_tv_model.py) before it judges the GPU (test_tv_gpu.py): the Laplacian symbol and
the adjoint differences, the x-update against its normal equations, the shrinkage against a brute-force proximal map, convergence
of the objective and the primal residual, the delta-PSF invariants, the error class of single precision, injected faults far
outside the device tolerance, the restoration margin over the Wiener filter and Richardson-Lucy, and the C ABI / Python surface."""
import re
import subprocess

import numpy as np
import pytest

from _mixed_model import wiener_raw
from _rl_model import NORM_CROPPED, blur_model, centred_psf, dense_psf, op_spectrum, psnr, rel_err, rl_model, smooth_image
from _tv_model import (TV_TOL, blocks_scene, blur_plane, dx, dxT, dy, dyT, lap_symbol, objective, shrink, tv_iterates,
                       tv_model)


def line_psf(size, angle):
    """a motion-like line PSF made on the CPU (the GPU tests use the library's motionBlurKernel), sum 1"""
    k = np.zeros((size, size))
    c = size // 2
    for t in np.linspace(-c, c, 4 * size):
        k[int(round(c - t * np.sin(np.deg2rad(angle)))), int(round(c + t * np.cos(np.deg2rad(angle))))] = 1
    return (k / k.sum()).astype(np.float32)


@pytest.mark.parametrize("M,N", [(8, 32), (16, 64), (64, 32)])
def test_symbol_and_adjoints(M, N):
    ex = np.zeros((M, N)); ex[0, 0] = -1; ex[0, N - 1] = 1   # Dx as a circular convolution kernel: (k * x)[j] = x[j + 1] - x[j]
    ey = np.zeros((M, N)); ey[0, 0] = -1; ey[M - 1, 0] = 1
    sym = np.abs(np.fft.rfft2(ex)) ** 2 + np.abs(np.fft.rfft2(ey)) ** 2
    assert np.allclose(sym, lap_symbol(M, N), atol=1e-13, rtol=0)
    rng = np.random.default_rng(M + N)
    x, v = rng.standard_normal((M, N)), rng.standard_normal((M, N))
    assert np.allclose(np.fft.irfft2(np.fft.rfft2(x) * np.fft.rfft2(ex), s=(M, N)), dx(x), atol=1e-12)
    for D, DT in ((dx, dxT), (dy, dyT)):
        assert abs(np.sum(D(x) * v) - np.sum(x * DT(v))) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(v)
    assert dx(x)[3, N - 1] == x[3, 0] - x[3, N - 1] and dy(x)[M - 1, 5] == x[0, 5] - x[M - 1, 5]  # forward and periodic


@pytest.mark.parametrize("aniso", [False, True])
def test_x_update_solves_its_normal_equations(aniso):
    M, N, mu, rho = 32, 64, 40.0, 2.0
    d = smooth_image(M, N, 1)[:27, :50].astype(np.float64)
    psf = dense_psf(2, 5)
    H = op_spectrum(psf, M, N)
    its = list(tv_iterates(d, psf, M, N, mu, rho, 3, aniso))
    for x, _, _, rhs in its[1:]:
        lhs = mu * blur_plane(blur_plane(x, H), H, adjoint=True) + rho * (dxT(dx(x)) + dyT(dy(x)))
        assert np.max(np.abs(lhs - rhs)) <= 1e-11 * np.max(np.abs(rhs))
    assert np.array_equal(its[0][0][:27, :50], d) and not its[0][0][27:].any() and not its[0][0][:, 50:].any()  # x0 = pad(d)


def test_shrinkage_is_the_proximal_map():
    """argmin_z t |z| + |z - g|^2 / 2 by brute force on a fine grid around the closed form"""
    t = 0.5
    grid = np.linspace(-2.0, 2.0, 801)
    zx, zy = np.meshgrid(grid, grid, indexing="ij")
    for gx, gy in ((1.3, -0.4), (0.2, 0.3), (-0.9, 1.1), (0.5, 0.0), (-1.7, -1.6)):
        for aniso in (False, True):
            pen = np.abs(zx) + np.abs(zy) if aniso else np.sqrt(zx * zx + zy * zy)
            cost = t * pen + 0.5 * ((zx - gx) ** 2 + (zy - gy) ** 2)
            k = np.unravel_index(np.argmin(cost), cost.shape)
            sx, sy = shrink(np.array([gx]), np.array([gy]), t, aniso)
            assert abs(zx[k] - sx[0]) <= 0.0051 and abs(zy[k] - sy[0]) <= 0.0051, (gx, gy, aniso)


@pytest.mark.parametrize("aniso", [False, True])
def test_objective_falls_and_primal_residual_vanishes(aniso):
    M, N, mu, rho = 64, 64, 300.0, 2.0
    truth = blocks_scene(M, N, 1)
    psf = centred_psf(line_psf(7, 30.0), M, N)
    d = blur_model(truth, psf, M, N) + np.random.default_rng(0).normal(0, 0.01, (M, N))
    H = op_spectrum(psf, M, N)
    obj, res = [], []
    for x, zx, zy, _ in tv_iterates(d, psf, M, N, mu, rho, 300, aniso):
        obj.append(objective(x, d, H, mu, aniso))
        if zx is not None:
            res.append(float(np.sqrt(np.sum((dx(x) - zx) ** 2 + (dy(x) - zy) ** 2))))
    assert obj[300] < 0.5 * obj[0]
    assert abs(obj[300] - obj[250]) <= 1e-3 * obj[300]  # a plateau
    assert min(obj[200:]) >= obj[300] * (1 - 1e-3)
    assert res[-1] <= 1e-2 * max(res) and res[-1] <= 0.05


def test_delta_psf_invariants():
    M, N = 32, 64
    delta = np.ones((1, 1))
    c = np.full((M, N), 0.37)
    for aniso in (False, True):
        assert np.allclose(tv_model(c, delta, M, N, 10.0, 2.0, 20, aniso), c, atol=1e-13)
    d = smooth_image(M, N, 3).astype(np.float64) + 0.05 * np.random.default_rng(1).standard_normal((M, N))
    errs = [rel_err(tv_model(d, delta, M, N, mu, 2.0, 200), d) for mu in (10.0, 100.0, 1000.0, 10000.0)]
    assert errs[0] > errs[1] > errs[2] > errs[3] and errs[3] < 1e-2, errs
    assert np.array_equal(tv_model(d[:20, :33], delta, M, N, 10.0, 2.0, 0), d[:20, :33])  # n = 0: the window of pad(d)
    neg = d - 0.5
    out = tv_model(neg, delta, M, N, 50.0, 2.0, 5, nonneg=True)
    assert out.min() == 0 and np.array_equal(out, np.maximum(tv_model(neg, delta, M, N, 50.0, 2.0, 5), 0))
    n = tv_model(neg, delta, M, N, 50.0, 2.0, 5, norm_area=NORM_CROPPED)
    assert n.min() == 0 and n.max() == 1


RHO = 10.0  # threshold 0.1


def _cases():
    rng = np.random.default_rng(11)
    for M, N, rows, cols in ((256, 256, 256, 256), (128, 512, 100, 333)):
        img = (blocks_scene(M, N, 5)[:rows, :cols] + 0.2 * rng.random((rows, cols))).astype(np.float32)  # edges and texture above 1 / rho
        yield M, N, img, dense_psf(6, 9)


def test_single_precision_class():
    """the same model in float32 / complex64 is the device's arithmetic class: its error against the float64 model is the
    yardstick of the device thresholds (a device error more than 10x above it is a finding), and it must
    itself pass them"""
    worst = {}
    for M, N, img, psf in _cases():
        for aniso in (False, True):
            for n in (3, 30, 100):
                e = rel_err(tv_model(img, psf, M, N, 200.0, RHO, n, aniso, dtype=np.float32), tv_model(img, psf, M, N, 200.0, RHO, n, aniso))
                worst[n] = max(worst.get(n, 0.0), e)
    print("TV\tfloat32 model against float64\t%s" % {n: "%.3g" % e for n, e in worst.items()})
    assert max(worst.values()) <= TV_TOL, worst


def test_faults_are_visible():
    """each injected fault moves the result by more than 100x the device tolerance"""
    for M, N, img, psf in _cases():
        for aniso in (False, True):
            want = tv_model(img, psf, M, N, 200.0, RHO, 3, aniso)
            for fault in ("no_conj", "dxT_sign", "thr_rho", "swap_shrink"):
                e = rel_err(tv_model(img, psf, M, N, 200.0, RHO, 3, aniso, fault=fault), want)
                assert e > 100 * TV_TOL, (fault, aniso, e)
            assert rel_err(tv_model(img, psf, M, N, 200.0, RHO, 2, aniso), want) > 100 * TV_TOL  # one iteration fewer
            assert rel_err(tv_model(img, psf, M, N, 200.0, 1.25 * RHO, 3, aniso), want) > 100 * TV_TOL  # another rho


QUALITY = dict(M=512, N=512, seed=3, sigma=0.01, mu=500.0, rho=2.0, n=100, psf=(15, 30.0))


def quality_case(psf):
    """truth, blurred + noise (float32), best Wiener PSNR over a K grid, PSNR of 30 RL iterations; psf = the 15 / 30 motion PSF"""
    q = QUALITY
    truth = blocks_scene(q["M"], q["N"], q["seed"])
    cp = centred_psf(psf, q["M"], q["N"])
    blurred = (blur_model(truth, cp, q["M"], q["N"]) + np.random.default_rng(1).normal(0, q["sigma"], truth.shape)).astype(np.float32)
    wiener = max(psnr(wiener_raw(blurred, cp, K, q["M"], q["N"]), truth) for K in np.logspace(-4, 0, 25))
    rl = psnr(rl_model(blurred, cp, q["M"], q["N"], 30), truth)
    return truth, cp, blurred, wiener, rl


def test_tv_beats_wiener_and_rl_on_a_piecewise_constant_scene():
    q = QUALITY
    truth, cp, blurred, wiener, rl = quality_case(line_psf(*q["psf"]))
    tv = psnr(tv_model(blurred, cp, q["M"], q["N"], q["mu"], q["rho"], q["n"]), truth)
    print("TV\tquality (model)\tblurred %.2f dB, best Wiener %.2f dB, RL 30 %.2f dB, TV %.2f dB" % (psnr(blurred, truth), wiener, rl, tv))
    assert tv >= max(wiener, rl) + 1.0, (tv, wiener, rl)


TV_FUNCS = ("fdr_tv_deconv_f32", "fdr_tv_deconv_f32_dev")


def test_symbols_and_surface(fdr):
    import inspect
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fdr.h")).read()
    assert re.search(r"typedef\s+struct\s+fdr_tv_params\s*\{[^}]*float\s+mu;[^}]*float\s+rho;[^}]*int\s+iterations;[^}]*int\s+anisotropic;"
                     r"[^}]*int\s+nonneg;[^}]*int\s+norm_area;[^}]*\}\s*fdr_tv_params\s*;", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in TV_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    for meth in ("tv_deconv", "tv_deconv_dev"):
        assert callable(getattr(fdr.Plan, meth)), meth
    sig = inspect.signature(fdr.Plan.tv_deconv).parameters
    assert list(sig)[:3] == ["self", "img", "mu"]
    assert (sig["rho"].default, sig["iterations"].default, sig["anisotropic"].default, sig["nonneg"].default, sig["norm_area"].default) == \
        (2.0, 50, False, False, fdr.NORM_NONE)
    sig = inspect.signature(fdr.tvDeblur_myfft).parameters
    assert list(sig)[:3] == ["img", "psf", "mu"] and sig["norm_area"].default == fdr.NORM_NONE and sig["rho"].default == 2.0
    import ctypes
    assert ctypes.sizeof(fdr.TvParams) == 24 and [f[0] for f in fdr.TvParams._fields_] == ["mu", "rho", "iterations", "anisotropic", "nonneg", "norm_area"]
