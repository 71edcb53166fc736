"""Poisson-likelihood TV deconvolution (fdr_tv_deconv_poisson_f32*) without a device: the float64 model of tests/_tvpoisson_model.py is
pinned (the s-update against its optimality condition, the two branches of the root, the objective at the iterate, convergence, the
injected faults, restoration quality against the least-squares free model), the float32 form of the step against the float64 one,
then the C surface (structs, symbols, null arguments) and the CLI's usage text."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from _rl_model import dense_psf, op_spectrum, rel_err
from _tv_model import blur_plane, dx, dy
from _tvpoisson_model import (FAULTS, QUALITY, SHORT, SHORT_IDS, TVP_TOL, line_psf, pad_to, poisson_objective, quality_case, quality_psnr, psnr,
                              s_update, short_combos, step_f32, tvf_weights, tvp_image, tvpoisson_iterates, tvpoisson_model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_step(seed, n=4000):
    rng = np.random.default_rng(seed)
    e = rng.normal(0.3, 1.0, n)
    d = np.where(rng.random(n) < 0.2, 0.0, rng.gamma(2.0, 0.5, n)) - (rng.random(n) < 0.1) * 0.3  # zeros and negatives among them
    m = np.where(rng.random(n) < 0.2, 0.0, rng.random(n))
    return e, d, m


@pytest.mark.parametrize("mu,nu,b", [(8.0, 2.0, 0.0), (100.0, 2.0, 0.05), (0.5, 7.0, 1.5), (2000.0, 0.5, 0.0)])
def test_s_update_satisfies_its_optimality_condition(mu, nu, b):
    """nu (s - e) + mu m (1 - d+ / (s + b)) = 0 to 1e-10 relative wherever d+ > 0; s + b >= 0 everywhere; m = 0 gives s = e exactly"""
    e, d, m = _random_step(int(mu) + 1)
    s = s_update(e, d, m, mu, nu, b)
    dp = np.maximum(d, 0)
    assert np.all((s + b)[m > 0] >= 0)  # (where m = 0 the step is s = e, whatever its sign)
    assert np.array_equal(s[m == 0], e[m == 0])
    on = (dp > 0) & (m > 0)
    assert on.sum() > 1000 and np.all((s + b)[on] > 0)
    u = np.where(on, s + b, 1.0)
    g = nu * (s - e) + mu * m * (1.0 - dp / u)
    scale = nu * (np.abs(s) + np.abs(e)) + mu * m * (1.0 + dp / u)
    worst = float(np.max(np.abs(g[on]) / scale[on]))
    print("TVP\ts-update\tmu %g nu %g b %g\toptimality residual %.3g" % (mu, nu, b, worst))
    assert worst <= 1e-10
    off = (dp == 0) & (m > 0)  # d+ = 0: y = max(a, 0), the minimiser of the linear term on s + b >= 0
    a = e + b - mu * m / nu
    assert off.any() and np.allclose((s + b)[off], np.maximum(a[off], 0), rtol=0, atol=1e-12)
    better = s_update(e, d, m, mu, nu, b, fault="minus_root")  # and the other root is the wrong one
    assert np.any((better + b)[on] < 0)


def test_both_branches_of_the_root_agree_at_a_zero():
    """at a = 0 the two forms of the root are sqrt(t) both; close to it on either side (|a| <= sqrt(t) / 100, where neither form
    cancels) they agree to 8 ulps, in float64 and float32"""
    for dt in (np.float64, np.float32):
        tol = 8 * np.finfo(dt).eps
        t = np.asarray([1e-2, 0.5, 3.0, 1e4], dtype=dt)
        for a in (dt(0), dt(1e-20), dt(-1e-20), dt(1e-3), dt(-1e-3)):
            rt = np.sqrt(a * a + dt(4) * t)
            first, second = dt(0.5) * (a + rt), (dt(2) * t) / (rt - a)
            assert first.dtype == dt and second.dtype == dt
            assert np.all(np.abs(first - second) <= tol * np.maximum(first, second)), (dt, a)
            if a == 0:
                assert np.all(np.abs(first - np.sqrt(t)) <= tol * np.sqrt(t)) and np.all(np.abs(second - np.sqrt(t)) <= tol * np.sqrt(t))
    # the model takes the first at a = +-0 and the second just below, and the step is continuous across the switch
    e = np.asarray([1.0, np.nextafter(1.0, 0.0)])
    s = s_update(e, np.asarray([0.7, 0.7]), np.asarray([1.0, 1.0]), 2.0, 2.0, 0.0)  # k = 1: a = 0 and just below it
    assert abs(s[0] - s[1]) <= 1e-15 and s[0] == pytest.approx(np.sqrt(0.7), rel=1e-15)


def test_float32_step_is_in_the_class_of_the_float64_step():
    """step_f32 (the device's operation order) against the float64 update on the same float32 inputs: a few ulps of the operands"""
    rng = np.random.default_rng(11)
    M, N, rows, cols = 16, 32, 9, 30
    c = rng.normal(0.4, 0.3, (M, N)).astype(np.float32)
    q = rng.normal(0.0, 0.1, (M, N)).astype(np.float32)
    d = tvp_image(M, N, rows, cols, 5)
    w = tvf_weights("fractional", rows, cols, 5)
    w[0, :4] = 0
    cn, qn = step_f32(c, q, d, w, 50.0, 3.0, 0.05)
    assert cn.dtype == np.float32 and np.array_equal(cn[rows:], c[rows:]) and np.array_equal(cn[:, cols:], c[:, cols:])
    assert np.array_equal(qn[rows:], q[rows:]) and np.array_equal(qn[:, cols:], q[:, cols:])
    e = c[:rows, :cols].astype(np.float64) + q[:rows, :cols]
    s = s_update(e, d.astype(np.float64), w.astype(np.float64), 50.0, 3.0, np.float64(np.float32(0.05)))
    assert float(np.max(np.abs(qn[:rows, :cols] - (e - s)))) <= 2e-6 and float(np.max(np.abs(cn[:rows, :cols] - (s - (e - s))))) <= 4e-6
    assert np.array_equal(qn[0, :4], np.zeros(4, dtype=np.float32)) and np.array_equal(cn[0, :4], (c[0, :4] + q[0, :4]))  # m = 0: s = e


def test_objective_at_the_iterate_is_not_above_its_perturbations():
    """64^2, window 50 x 56, fractional weights, b = 0.05, mu 30, n = 1500: the objective at x is not above that at x + small random
    perturbations (20 of them, sizes 1e-4 .. 1e-2), up to the 1e-6 relative that the iteration is still away from its limit"""
    S, rows, cols, mu, b = 64, 50, 56, 30.0, 0.05
    rng = np.random.default_rng(9)
    from _tvpoisson_model import centred_psf, rect_scene
    psf = centred_psf(line_psf(7, 30.0), S, S)
    H = op_spectrum(psf, S, S)
    truth = 0.02 + rect_scene(S) ** 3
    d = (rng.poisson((blur_plane(truth, H) + b).clip(0) * 200.0) / 200.0)[:rows, :cols]
    w = tvf_weights("fractional", rows, cols, 1).astype(np.float64)
    x = None
    for st in tvpoisson_iterates(d, psf, S, S, mu, 2.0, 1500, w, 0.0, b):
        x = st["x"]
    m = pad_to(w, S, S, np.float64)
    dp = pad_to(d, S, S, np.float64)
    f0 = poisson_objective(x, dp, m, H, mu, b)
    assert np.isfinite(f0)
    low = min(poisson_objective(x + size * rng.standard_normal((S, S)), dp, m, H, mu, b) for size in (1e-4, 1e-3, 1e-2) for _ in range(7))
    print("TVP\tobjective (model)\tat the iterate %.10g, lowest of 21 perturbations %.10g" % (f0, low))
    assert f0 <= low + 1e-6 * abs(f0)


def test_primal_residuals_fall_and_q_settles():
    """||D x - z||, ||blur(x) - s|| and the step of q on the 100-photon quality scene at mu 8: at n = 300 below 0.2 of their value at
    n = 1 (as test_tvfree_host.py pins the free iteration)"""
    c, q = quality_case(100), QUALITY
    H = op_spectrum(c["psf"], q["M"], q["N"])
    res, prev_q = {}, None
    for k, st in enumerate(tvpoisson_iterates(c["d"], c["psf"], q["M"], q["N"], 8.0, q["rho"], 300, None, q["nu"])):
        if k in (1, 300):
            x, (zx, zy) = st["x"], st["z"]
            res[k] = (float(np.sqrt(np.sum((dx(x) - zx) ** 2 + (dy(x) - zy) ** 2))), float(np.linalg.norm(blur_plane(x, H) - st["s"])),
                      float(np.linalg.norm(st["q"] - (prev_q if prev_q is not None else 0))))
        if k in (0, 299):
            prev_q = st.get("q")
    rz, rs, rq = (res[300][i] / res[1][i] for i in range(3))
    print("TVP\tresiduals (model)\t||Dx - z|| %.3g, ||blur(x) - s|| %.3g, ||q_k - q_k-1|| %.3g of their values at n = 1" % (rz, rs, rq))
    assert rz < 0.2 and rs < 0.2 and rq < 0.2, (rz, rs, rq)


def _fault_case(case):
    M, N, rows, cols = case[:4]
    d = tvp_image(M, N, rows, cols, M + 3 * N)
    assert (d < 0).mean() > 0.05 and (d == 0).any() and (d > 0).mean() > 0.3
    w = tvf_weights("fractional", rows, cols, M + 3 * N)
    name, psf, mu, rho, nu, aniso, _ = [c for c in short_combos(line_psf(), M, N, rows, cols) if c[0].startswith("dense")][0]
    return d, w, name, psf, mu, rho, nu, aniso


@pytest.mark.parametrize("case", SHORT, ids=SHORT_IDS)
def test_faults_are_far_outside_the_tolerance(case):
    """every fault model differs from the model by more than 100 x TVP_TOL at n = 3 on each short case of the GPU test (dense PSF,
    fractional weights, b = 0.05, the largest output window; the image holds zeros' neighbours and negatives), so the GPU judge
    can see it"""
    M, N = case[:2]
    out_shape = case[7][-1]
    d, w, name, psf, mu, rho, nu, aniso = _fault_case(case)
    want = tvpoisson_model(d, psf, M, N, mu, rho, 3, w, nu, 0.05, aniso, out_shape=out_shape)
    for fault in FAULTS:
        e = rel_err(tvpoisson_model(d, psf, M, N, mu, rho, 3, w, nu, 0.05, aniso, out_shape=out_shape, fault=fault), want)
        print("TVP\tfault\t%dx%d win %dx%d %s %s\terr=%.3g" % (M, N, case[2], case[3], name, fault, e))
        assert e > 100 * TVP_TOL, (fault, e)


def test_single_precision_class():
    """the same formulas in float32 / complex64 against float64: the arithmetic class the device is held to"""
    c, q = quality_case(1000), QUALITY
    worst = 0.0
    for n in (30, 100):
        e = rel_err(tvpoisson_model(c["d"], c["psf"], q["M"], q["N"], 16.0, q["rho"], n, dtype=np.float32),
                    tvpoisson_model(c["d"], c["psf"], q["M"], q["N"], 16.0, q["rho"], n))
        print("TVP\tfloat32 model\tquality scene n=%d\terr=%.3g" % (n, e))
        worst = max(worst, e)
    assert 1e-8 < worst < 1e-5


def test_quality_against_the_least_squares_model():
    """The table of DESIGN.md section 36, re-measured with this model (float64, rho = nu = 2, n = 100, output clamped at 0):
        photons   Poisson step, best mu    least-squares step, best mu    blurred noisy crop
        100       34.02 dB (mu 8)          32.12 dB (mu 32)               21.17 dB
        1000      38.08 dB (mu 16)         36.86 dB (mu 128)              22.84 dB
    gains 1.90 and 1.22 dB.  Asserted: at its best mu of the grid the Poisson form beats the least-squares form at its best mu by at
    least half the gain measured (0.95 and 0.61 dB): the gain belongs to the two float64 models and moves by a few tenths of a dB
    with the mu grid."""
    q = QUALITY
    for photons, half_gain in ((100, 0.95), (1000, 0.61)):
        c = quality_case(photons)
        pois = {mu: quality_psnr(photons, mu, True) for mu in q["mu_poisson"]}
        gaus = {mu: quality_psnr(photons, mu, False) for mu in q["mu_gauss"]}
        bp, bg = max(pois, key=pois.get), max(gaus, key=gaus.get)
        print("TVP\tquality (model)\t%d photons: Poisson %.2f dB (mu %g), least squares %.2f dB (mu %g), blurred noisy crop %.2f dB"
              % (photons, pois[bp], bp, gaus[bg], bg, psnr(c["d"], c["truth"])))
        assert q["mu_poisson"][0] < bp < q["mu_poisson"][-1] and q["mu_gauss"][0] < bg < q["mu_gauss"][-1]  # the grids bracket both
        assert pois[bp] >= gaus[bg] + half_gain, (photons, pois[bp], gaus[bg])


TVP_FUNCS = ("fdr_tv_deconv_poisson_f32", "fdr_tv_deconv_poisson_f32_dev", "fdr_tv_deconv_poisson_batch_f32", "fdr_tv_deconv_poisson_batch_f32_dev",
             "fdr_tv_poisson_step_f32_dev", "fdr_tv_poisson_step_group_f32_dev")


def test_symbols_and_surface(fdr):
    header = open(os.path.join(ROOT, "include", "fdr.h")).read()
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int}
    names = ["mu", "rho", "nu", "background", "iterations", "anisotropic", "nonneg", "norm_area", "out_rows", "out_cols"]
    for struct, cls, want, size in (("fdr_tv_poisson_params", fdr.TvPoissonParams, names, 40),
                                    ("fdr_tv_poisson_batch_params", fdr.TvPoissonBatchParams, names + ["coupling"], 44)):
        m = re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}\s*%s\s*;" % (struct, struct), header)
        assert m, "%s is not declared" % struct
        fields = re.findall(r"\b(float|int)\s+(\w+)\s*;", m.group(1))
        assert [(n, ctype[t]) for t, n in fields] == list(cls._fields_)
        assert [n for _, n in fields] == want and [t for t, _ in fields][:4] == ["float"] * 4
        assert ctypes.sizeof(cls) == size
    assert re.search(r"#define\s+FDR_VERSION\s+300\b", header) and fdr.lib.fdr_version() == 300
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in TVP_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    sig = inspect.signature(fdr.Plan.tv_deconv_poisson).parameters
    assert list(sig) == ["self", "img", "mu", "rho", "iterations", "weights", "nu", "background", "anisotropic", "nonneg", "norm_area", "full_plane"]
    assert [sig[k].default for k in list(sig)[3:]] == [2.0, 50, None, 0.0, 0.0, False, False, fdr.NORM_NONE, False]
    sig = inspect.signature(fdr.Plan.tv_deconv_poisson_dev).parameters
    assert list(sig)[:9] == ["self", "d_img", "rows", "cols", "stride", "d_out", "out_stride", "mu", "rho"]
    assert (sig["d_weights"].default, sig["wstride"].default, sig["out_rows"].default, sig["nu"].default, sig["background"].default) == (None, 0, None, 0.0, 0.0)
    for fn in ("tv_deconv_poisson_batch", "tv_deconv_poisson_batch_dev"):
        assert inspect.signature(getattr(fdr.Plan, fn)).parameters["coupled"].default is False
    assert list(inspect.signature(fdr.Plan.tv_poisson_step_dev).parameters)[:10] == ["self", "d_c", "d_q", "d_img", "rows", "cols", "stride", "mu", "nu",
                                                                                     "background"]
    assert list(inspect.signature(fdr.Plan.tv_poisson_step_group_dev).parameters)[:8] == ["self", "d_c", "c_pitch", "d_q", "q_pitch", "d_imgs",
                                                                                          "img_pitch", "count"]
    sig = inspect.signature(fdr.tvDeblurPoisson_myfft).parameters
    assert list(sig)[:3] == ["img", "psf", "mu"] and sig["weights"].default is None and sig["background"].default == 0.0
    sig = inspect.signature(fdr.tvDeblurPoisson_RGB).parameters
    assert list(sig)[:3] == ["channels", "psf", "mu"] and sig["coupled"].default is False
    cxx = open(os.path.join(ROOT, "include", "fft", "fft.hpp")).read()
    assert re.search(r"inline\s+void\s+tvDeblurPoisson_RGB\s*\([^)]*bool\s+coupled\s*=\s*false\s*\)", cxx)


def test_null_arguments_are_refused_before_any_device_work(fdr):
    """a null plan, image, output, plane or params: FDR_ERR_ARG from every entry point, on a machine without a device too"""
    L = fdr.lib
    img = np.zeros((8, 32), dtype=np.float32)
    out = np.zeros((8, 32), dtype=np.float32)
    prm = fdr.TvPoissonParams(10.0, 2.0, 0.0, 0.0, 1, 0, 0, 2, 8, 32)
    bprm = fdr.TvPoissonBatchParams(10.0, 2.0, 0.0, 0.0, 1, 0, 0, 2, 8, 32, 0)
    I, O = img.ctypes.data, out.ctypes.data
    for h, i, o, p in ((None, I, O, ctypes.byref(prm)), (1, None, O, ctypes.byref(prm)), (1, I, None, ctypes.byref(prm)), (1, I, O, None)):
        assert L.fdr_tv_deconv_poisson_f32(h, i, 8, 32, 32, None, 0, o, 32, p) == -1
        assert b"fdr_tv_deconv_poisson_f32: null argument" in L.fdr_last_error()
        assert L.fdr_tv_deconv_poisson_f32_dev(h, i, 8, 32, 32, None, 0, o, 32, p, None) == -1
        assert b"fdr_tv_deconv_poisson_f32_dev: null argument" in L.fdr_last_error()
    for h, i, o, p in ((None, I, O, ctypes.byref(bprm)), (1, None, O, ctypes.byref(bprm)), (1, I, None, ctypes.byref(bprm)), (1, I, O, None)):
        assert L.fdr_tv_deconv_poisson_batch_f32(h, i, 256, 1, 8, 32, 32, None, 0, o, 256, 32, p) == -1
        assert b"fdr_tv_deconv_poisson_batch_f32: null argument" in L.fdr_last_error()
        assert L.fdr_tv_deconv_poisson_batch_f32_dev(h, i, 256, 1, 8, 32, 32, None, 0, o, 256, 32, p, None) == -1
        assert b"fdr_tv_deconv_poisson_batch_f32_dev: null argument" in L.fdr_last_error()
    for h, c, q, i in ((None, I, O, I), (1, None, O, I), (1, I, None, I), (1, I, O, None)):
        assert L.fdr_tv_poisson_step_f32_dev(h, c, q, i, 8, 32, 32, None, 0, 1.0, 1.0, 0.0, None) == -1
        assert b"fdr_tv_poisson_step_f32_dev: null argument" in L.fdr_last_error()
        assert L.fdr_tv_poisson_step_group_f32_dev(h, c, 256, q, 256, i, 256, 1, 8, 32, 32, None, 0, 1.0, 1.0, 0.0, None) == -1
        assert b"fdr_tv_poisson_step_group_f32_dev: null argument" in L.fdr_last_error()


def test_cli_usage_names_the_poisson_leg():
    """--tv mu --poisson is a leg of its own; beside --tv auto, --rl, --cls, --tile or --mode parity, without --tv mu, or with a bad
    --background it is refused with a usage text that names it, before the picture is read and before any device work"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")
    for extra in (["--tv", "auto", "--poisson"], ["--tv", "8", "--poisson", "--rl", "5"], ["--tv", "8", "--poisson", "--cls", "0.1"],
                  ["--tv", "8", "--poisson", "--tile", "256"], ["--tv", "8", "--poisson", "--mode", "parity"], ["--poisson"],
                  ["--tv", "8", "--background", "0.1"], ["--tv", "8", "--poisson", "--background", "-1"],
                  ["--tv", "8", "--poisson", "--background", "nan"]):
        r = subprocess.run([gpu, "no-such-picture.png", "40", "45"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Usage" in r.stdout and "--tv <mu> --poisson [--background b]" in r.stdout and "--mask" in r.stdout, (extra, r.stdout)
    for args in (["40", "45", "--tv", "8", "--poisson"], ["40", "45", "--tv", "8", "--poisson", "--background", "0.05", "--tv-color", "--tv-iters", "5"],
                 ["40", "45", "--tv", "8", "--poisson", "--mask", "m.png"]):
        r = subprocess.run([gpu, "no-such-picture.png"] + args, capture_output=True, text=True, timeout=120)
        assert "Usage" not in r.stdout and "Cannot read image" in r.stdout, (args, r.stdout)  # accepted: the run gets as far as the picture
