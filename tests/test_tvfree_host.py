"""CPU pins of tests/_tvfree_model.py, the float64 model of free-boundary, weighted TV deconvolution, before it judges the device
(test_tvfree_gpu.py): the s-update against a brute-force minimiser, the x-update against its normal equations, both primal
residuals, the periodic limit, the quality claims of the feature on a cropped scene, injected faults far outside the device
tolerance, and the public surface.  No GPU needed; the refusals that need a plan are in test_tvfree_gpu.py.  Cases print a `TVF`
line with their measured values (pytest -s)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from _rl_model import centred_psf, dense_psf, op_spectrum, psnr, rel_err
from _tv_model import blur_plane, dx, dxT, dy, dyT, objective, tv_iterates, tv_model
from _tvfree_model import (FAULTS, QUALITY, SHORT, SHORT_IDS, TVF_TOL, free_objective, line_psf, quality_case, rect_scene, s_update,
                           short_combos, tvf_image, tvf_weights, tvfree_iterates, tvfree_model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_s_update_is_the_pointwise_minimiser():
    """argmin_s mu / 2 m (s - d)^2 + nu / 2 (s - e)^2 by brute force on a fine grid"""
    grid = np.linspace(-3.0, 3.0, 600001)
    for mu, nu, m, d, e in ((500.0, 2.0, 1.0, 0.7, -0.4), (5.0, 4.0, 0.3, -0.2, 1.9), (50.0, 3.0, 0.0, 0.9, 0.35), (200.0, 10.0, 0.02, 1.5, -2.5)):
        cost = 0.5 * mu * m * (grid - d) ** 2 + 0.5 * nu * (grid - e) ** 2
        assert abs(grid[np.argmin(cost)] - s_update(e, d, m, mu, nu)) <= 1e-5, (mu, nu, m, d, e)
    assert s_update(0.35, 0.9, 0.0, 50.0, 3.0) == pytest.approx(0.35, abs=1e-15)  # weight 0: the datum does not count


@pytest.mark.parametrize("aniso,nu", [(False, 0.0), (True, 5.0)])
def test_x_update_solves_its_normal_equations(aniso, nu):
    """(nu H^T H + rho D^T D) x = nu H^T r + rho D^T v"""
    M, N, mu, rho = 32, 64, 40.0, 2.0
    d = tvf_image(M, N, 27, 50, 1).astype(np.float64)
    w = tvf_weights("fractional", 27, 50, 1)
    psf = dense_psf(2, 5)
    H = op_spectrum(psf, M, N)
    nu_ = nu or rho
    its = list(tvfree_iterates(d, psf, M, N, mu, rho, 3, w, nu, aniso))
    for st in its[1:]:
        x, r, (vx, vy) = st["x"], st["r"], st["v"]
        lhs = nu_ * blur_plane(blur_plane(x, H), H, adjoint=True) + rho * (dxT(dx(x)) + dyT(dy(x)))
        rhs = nu_ * blur_plane(r, H, adjoint=True) + rho * (dxT(vx) + dyT(vy))
        assert np.max(np.abs(lhs - rhs)) <= 1e-9 * np.max(np.abs(rhs))
        assert not st["q"][27:].any() and not st["q"][:, 50:].any()                       # q stays 0 outside the window ...
        assert np.array_equal(st["r"][27:], st["c"][27:]) and np.array_equal(st["r"][:, 50:], st["c"][:, 50:])  # ... and r = c
    x0 = its[0]["x"]
    assert np.array_equal(x0[:27, :50], d) and not x0[27:].any() and not x0[:, 50:].any()  # x0 = pad(d)


def test_primal_residuals_fall():
    """||D x - z|| and ||blur(x) - s|| on the quality scene: at n = 300 below 0.2 of their value at n = 1 (measured 0.036 and 0.10)"""
    c, q = quality_case(), QUALITY
    H = op_spectrum(c["psf"], q["M"], q["N"])
    res = {}
    for k, st in enumerate(tvfree_iterates(c["d"], c["psf"], q["M"], q["N"], q["mu"], q["rho"], 300)):
        if k in (1, 300):
            x, (zx, zy) = st["x"], st["z"]
            res[k] = (float(np.sqrt(np.sum((dx(x) - zx) ** 2 + (dy(x) - zy) ** 2))), float(np.linalg.norm(blur_plane(x, H) - st["s"])))
    rz, rs = res[300][0] / res[1][0], res[300][1] / res[1][1]
    print("TVF\tresiduals (model)\t||Dx - z|| %.3g -> %.3g (%.3g), ||blur(x) - s|| %.3g -> %.3g (%.3g)" % (res[1][0], res[300][0], rz, res[1][1], res[300][1], rs))
    assert rz < 0.2 and rs < 0.2, (rz, rs)


def test_periodic_limit():
    """the window equal to the plan and no weights: the free iteration minimises the periodic objective.  64^2, mu 200, n = 1000:
    the two objectives agree to 1e-5 relative (measured 2e-6)"""
    S, mu, rho = 64, 200.0, 2.0
    psf = centred_psf(line_psf(), S, S)  # the quality scene at 64^2: both iterations have converged this far by n = 1000
    H = op_spectrum(psf, S, S)
    d = blur_plane(rect_scene(S), H) + 0.01 * np.random.default_rng(4).standard_normal((S, S))
    xp = xf = None
    for xp, _, _, _ in tv_iterates(d, psf, S, S, mu, rho, 1000):
        pass
    for st in tvfree_iterates(d, psf, S, S, mu, rho, 1000):
        xf = st["x"]
    op, of = objective(xp, d, H, mu, False), objective(xf, d, H, mu, False)
    assert of == pytest.approx(free_objective(xf, d, np.ones((S, S)), H, mu), rel=1e-12)
    print("TVF\tperiodic limit (model)\tobjectives %.8g (periodic) %.8g (free), rel %.3g, iterates differ by %.3g"
          % (op, of, abs(op - of) / op, float(np.max(np.abs(xp - xf)))))
    assert abs(op - of) <= 1e-5 * op


def test_quality_on_a_crop():
    """mu 500, n = 30: the free model is at least 15 dB above the blurred crop and above tv_model on that crop (measured 18.9, 27.0)"""
    c, q = quality_case(), QUALITY
    blurred = psnr(c["d"], c["truth"])
    periodic = psnr(tv_model(c["d"], c["psf"], q["M"], q["N"], q["mu"], q["rho"], 100), c["truth"])
    free = psnr(tvfree_model(c["d"], c["psf"], q["M"], q["N"], q["mu"], q["rho"], q["n"]), c["truth"])
    print("TVF\tquality (model)\tblurred crop %.2f dB, periodic TV %.2f dB, free boundary %.2f dB" % (blurred, periodic, free))
    assert free >= blurred + 15.0 and free >= periodic + 15.0, (blurred, periodic, free)


def test_zero_weights_remove_stuck_pixels():
    """2 % of the crop stuck at 1: the masked run is at least 20 dB above the unmasked one (measured 36.5)"""
    c, q = quality_case(), QUALITY
    unmasked = psnr(tvfree_model(c["stuck"], c["psf"], q["M"], q["N"], q["mu"], q["rho"], q["n_masked"]), c["truth"])
    masked = psnr(tvfree_model(c["stuck"], c["psf"], q["M"], q["N"], q["mu"], q["rho"], q["n_masked"], weights=c["keep"]), c["truth"])
    print("TVF\tstuck pixels (model)\tunmasked %.2f dB, masked %.2f dB" % (unmasked, masked))
    assert masked >= unmasked + 20.0, (unmasked, masked)


def test_all_ones_weights_are_no_weights():
    d = tvf_image(16, 32, 9, 30, 3)
    psf = dense_psf(5, 5)
    for dtype in (np.float64, np.float32):
        a = tvfree_model(d, psf, 16, 32, 50.0, 1.0, 4, None, 3.0, out_shape=(16, 32), dtype=dtype)
        b = tvfree_model(d, psf, 16, 32, 50.0, 1.0, 4, np.ones((9, 30), dtype=np.float32), 3.0, out_shape=(16, 32), dtype=dtype)
        assert np.array_equal(a, b)


def test_single_precision_class():
    """the same formulas in float32 / complex64: the arithmetic class the device is held to (TVF_TOL stays within 10x of it)"""
    c, q = quality_case(), QUALITY
    worst = 0.0
    for n in (30, 100):
        e = rel_err(tvfree_model(c["d"], c["psf"], q["M"], q["N"], q["mu"], q["rho"], n, dtype=np.float32),
                    tvfree_model(c["d"], c["psf"], q["M"], q["N"], q["mu"], q["rho"], n))
        print("TVF\tfloat32 model\tquality scene n=%d\terr=%.3g" % (n, e))
        worst = max(worst, e)
    d = tvf_image(8, 32, 8, 32, 40)
    e8 = rel_err(tvfree_model(d, dense_psf(5, 5), 8, 32, 50.0, 1.0, 3, dtype=np.float32), tvfree_model(d, dense_psf(5, 5), 8, 32, 50.0, 1.0, 3))
    print("TVF\tfloat32 model\t8x32 n=3\terr=%.3g" % e8)
    assert 1e-8 < e8 < 1e-5 and 1e-8 < worst < 1e-5


@pytest.mark.parametrize("case", SHORT, ids=SHORT_IDS)
def test_faults_are_far_outside_the_tolerance(case):
    """every fault model differs from the model by more than 100 x TVF_TOL at n = 3 on each short case of the GPU test (its dense
    PSF -- the spectrum of the centred line PSF is real, so 'no_conj' changes nothing there --, fractional weights, the largest
    output window), so the GPU judge can see it.  A fault that a case cannot show is not asked of it: 'no_mask' where the window
    is the plan."""
    M, N, rows, cols = case[:4]
    out_shape = case[7][-1]
    d = tvf_image(M, N, rows, cols, M + 3 * N)
    w = tvf_weights("fractional", rows, cols, M + 3 * N)
    name, psf, mu, rho, nu, aniso, _ = [c for c in short_combos(line_psf(), M, N, rows, cols) if c[0].startswith("dense")][0]
    want = tvfree_model(d, psf, M, N, mu, rho, 3, w, nu, aniso, out_shape=out_shape)
    for fault in FAULTS:
        if fault == "no_mask" and (rows, cols) == (M, N):
            continue
        e = rel_err(tvfree_model(d, psf, M, N, mu, rho, 3, w, nu, aniso, out_shape=out_shape, fault=fault), want)
        print("TVF\tfault\t%dx%d win %dx%d %s %s\terr=%.3g" % (M, N, rows, cols, name, fault, e))
        assert e > 100 * TVF_TOL, (fault, e)


TVFREE_FUNCS = ("fdr_tv_deconv_free_f32", "fdr_tv_deconv_free_f32_dev")


def test_symbols_and_surface(fdr):
    header = open(os.path.join(ROOT, "include", "fdr.h")).read()
    m = re.search(r"typedef\s+struct\s+fdr_tv_free_params\s*\{([^}]*)\}\s*fdr_tv_free_params\s*;", header)
    assert m, "fdr_tv_free_params is not declared"
    fields = re.findall(r"\b(float|int)\s+(\w+)\s*;", m.group(1))
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int}
    assert [(n, ctype[t]) for t, n in fields] == list(fdr.TvFreeParams._fields_)
    assert [n for _, n in fields] == ["mu", "rho", "nu", "iterations", "anisotropic", "nonneg", "norm_area", "out_rows", "out_cols"]
    assert ctypes.sizeof(fdr.TvFreeParams) == 36
    assert re.search(r"#define\s+FDR_VERSION\s+300\b", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in TVFREE_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    sig = inspect.signature(fdr.Plan.tv_deconv_free).parameters
    assert list(sig) == ["self", "img", "mu", "rho", "iterations", "weights", "nu", "anisotropic", "nonneg", "norm_area", "full_plane"]
    assert [sig[k].default for k in list(sig)[3:]] == [2.0, 50, None, 0.0, False, False, fdr.NORM_NONE, False]
    sig = inspect.signature(fdr.Plan.tv_deconv_free_dev).parameters
    assert list(sig)[:9] == ["self", "d_img", "rows", "cols", "stride", "d_out", "out_stride", "mu", "rho"]
    assert (sig["d_weights"].default, sig["wstride"].default, sig["out_rows"].default, sig["out_cols"].default, sig["nu"].default) == (None, 0, None, None, 0.0)
    sig = inspect.signature(fdr.tvDeblurFree_myfft).parameters
    assert list(sig)[:3] == ["img", "psf", "mu"] and sig["weights"].default is None and sig["iterations"].default == 50
    sig = inspect.signature(fdr.tvDeblurFree_RGB).parameters
    assert list(sig)[:3] == ["channels", "psf", "mu"] and sig["weights"].default is None
    cxx = open(os.path.join(ROOT, "include", "fft", "fft.hpp")).read()
    assert re.search(r"inline\s+void\s+tvDeblurFree_RGB\s*\(", cxx)


def test_null_arguments_are_refused_before_any_device_work(fdr):
    """a null plan, image, output or params: FDR_ERR_ARG from both entry points, on a machine without a device too"""
    L = fdr.lib
    img = np.zeros((8, 32), dtype=np.float32)
    out = np.zeros((8, 32), dtype=np.float32)
    prm = fdr.TvFreeParams(10.0, 2.0, 0.0, 1, 0, 0, 2, 8, 32)
    for h, i, o, p in ((None, img.ctypes.data, out.ctypes.data, ctypes.byref(prm)), (1, None, out.ctypes.data, ctypes.byref(prm)),
                       (1, img.ctypes.data, None, ctypes.byref(prm)), (1, img.ctypes.data, out.ctypes.data, None)):
        assert L.fdr_tv_deconv_free_f32(h, i, 8, 32, 32, None, 0, o, 32, p) == -1
        assert b"fdr_tv_deconv_free_f32: null argument" in L.fdr_last_error()
        assert L.fdr_tv_deconv_free_f32_dev(h, i, 8, 32, 32, None, 0, o, 32, p, None) == -1
        assert b"fdr_tv_deconv_free_f32_dev: null argument" in L.fdr_last_error()


def test_cli_usage_names_the_free_boundary_tv_leg():
    """--tv beside --free-boundary is a leg of its own; with --tv-color it is refused with a usage text that names it.  The refusal
    comes before the picture is read and before any device work."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")
    r = subprocess.run([gpu, "no-such-picture.png", "40", "45", "--tv", "200", "--free-boundary", "--tv-color"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Usage" in r.stdout and "--tv <mu> --free-boundary" in r.stdout and "--mask" in r.stdout, r.stdout
    for extra in (["--free-boundary"], ["--tv", "200", "--mask", "m.png"], ["--accel", "--tv", "200"], ["--tv", "0", "--free-boundary"]):
        r = subprocess.run([gpu, "no-such-picture.png", "40", "45"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Usage" in r.stdout, (extra, r.stdout)
    r = subprocess.run([gpu, "no-such-picture.png", "40", "45", "--tv", "200", "--free-boundary"], capture_output=True, text=True, timeout=120)
    assert "Usage" not in r.stdout and "Cannot read image" in r.stdout, r.stdout  # accepted: the run gets as far as the picture
