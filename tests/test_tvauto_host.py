"""CPU pins of tests/_tvauto_model.py, the float64 model of noise-constrained TV deconvolution, before it judges the device
(test_tvauto_gpu.py): the data step against a brute-force projection onto the discrepancy ball, convergence to the minimiser of the
free model at the multiplier, the quality claims of the feature on the cropped scene of _tvfree_model.py, injected faults far
outside the device tolerance, and the public surface.  No GPU needed; the refusals that need a plan are in test_tvauto_gpu.py.
Cases print a `TVA` line with their measured values (pytest -s)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from _rl_model import centred_psf, psnr, rel_err
from _tvauto_model import (FAULTS, MAX_RATIO, NU_RATIO, SHORT_SIGMAS, TVA_TOL, f32, project, quality_numbers, ratio, tvauto_iterates, tvauto_model)
from _tvfree_model import QUALITY, SHORT, SHORT_IDS, line_psf, quality_case, short_combos, tvf_image, tvf_weights, tvfree_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_data_step_is_the_projection_onto_the_ball():
    """0 / 1 weights: s = d + the residual scaled onto the ball where m = 1, s = e where m = 0, to 1e-12, and
    sum m (s - d)^2 = min(res_e, c2)"""
    rng = np.random.default_rng(11)
    for k, (scale, frac) in enumerate(((1.0, 0.02), (0.05, 0.5), (3.0, 0.0), (1.0, 1.0))):
        e = rng.standard_normal((24, 40))
        d = e + scale * rng.standard_normal((24, 40))
        m = (rng.random((24, 40)) >= frac).astype(np.float64)
        res_e = float(np.sum(m * (e - d) ** 2))
        for c2 in (0.3 * res_e, 0.999 * res_e, 2.0 * res_e, 0.0):
            s, g = project(e, d, m, c2)
            if res_e <= c2:
                want = e
            elif c2 == 0.0:
                want = None  # the clamp: s is within 1e-6 |e - d| of d where m = 1
            else:
                want = np.where(m > 0, d + (e - d) * np.sqrt(c2 / res_e), e)
            if want is None:
                assert g == MAX_RATIO and np.max(np.abs(m * (s - d))) <= 1.1e-6 * np.max(np.abs(e - d))
                assert np.array_equal(s[m == 0], e[m == 0])
                continue
            assert np.max(np.abs(s - want)) <= 1e-12, (k, c2)
            assert float(np.sum(m * (s - d) ** 2)) == pytest.approx(min(res_e, c2), rel=1e-12, abs=1e-300)
    assert ratio(1.0, 4.0) == 0.0 and ratio(4.0, 1.0) == 1.0 and ratio(1.0, 0.0) == MAX_RATIO and ratio(0.0, 0.0) == 0.0
    assert ratio(float("nan"), 1.0) == MAX_RATIO and ratio(1e300, 1e-300) == MAX_RATIO and ratio(1e20, 1.0) == MAX_RATIO


def test_converges_to_the_fixed_mu_minimiser():
    """64^2, window 60 x 50, motion 15/30, noise 0.01, rho 2, nu 50: after 1000 steps |res_c / c2 - 1| <= 1e-3, and the iterate is
    within 1e-3 of tvfree_model at mu = mu_n run as long"""
    S, rows, cols, sigma, rho, nu, n = 64, 60, 50, 0.01, 2.0, 50.0, 1000
    from _tv_model import blur_plane
    from _rl_model import op_spectrum
    from _rltv_model import rect_scene
    psf = centred_psf(line_psf(), S, S)
    H = op_spectrum(psf, S, S)
    d = (blur_plane(rect_scene(S), H) + sigma * np.random.default_rng(4).standard_normal((S, S)))[:rows, :cols]
    st = None
    for st in tvauto_iterates(d, psf, S, S, sigma, rho, n, nu=nu):
        pass
    res_c, _, mu_n = st["trace"]
    fixed = tvfree_model(d, psf, S, S, mu_n, rho, n, nu=nu, out_shape=(S, S))
    diff = float(np.max(np.abs(st["x"] - fixed)))
    print("TVA\tconvergence (model)\tres_c / c2 = %.6f, mu_n = %.4g, max |x - x(mu_n)| = %.3g" % (res_c / st["c2"], mu_n, diff))
    assert abs(res_c / st["c2"] - 1.0) <= 1e-3
    assert diff <= 1e-3


@pytest.mark.parametrize("name", ["given", "estimated", "masked"])
def test_quality_without_a_mu(name):
    """sigma 0.01 given, estimated, and given with 2 % stuck pixels masked, 100 steps with the defaults: at least 15 dB above the
    blurred crop and within 0.5 dB of the best hand-tuned mu of the free model at 100 steps"""
    n = quality_numbers()
    r = n[name]
    print("TVA\tquality (model)\t%s: %.2f dB (blurred %.2f, best tuned %.2f of %s), sigma %.5f, discrepancy / target %.4f, mu_n %.4g"
          % (name, r["psnr"], n["blurred"], n["best"], {k: round(v, 2) for k, v in n["tuned"].items()}, r["sigma"], r["ratio"], r["mu"]))
    assert r["psnr"] >= n["blurred"] + 15.0
    assert r["psnr"] >= n["best"] - 0.5


def test_fractional_weights_are_an_approximation():
    """fractional weights: the step is not the projection and the discrepancy settles above the target.  Recorded, not barred:
    only that the run stays finite and restores (10 dB above the blurred crop)"""
    c, q = quality_case(), QUALITY
    w = tvf_weights("fractional", q["rows"], q["cols"], 1)
    st = None
    for st in tvauto_iterates(c["d"], c["psf"], q["M"], q["N"], f32(q["noise"]), q["rho"], 300, w):
        pass
    p = psnr(st["x"][:q["rows"], :q["cols"]], c["truth"])
    print("TVA\tfractional weights (model)\tn=300: discrepancy / target %.3f, mu_n %.4g, %.2f dB" % (st["trace"][0] / st["c2"], st["trace"][2], p))
    assert np.isfinite(st["x"]).all() and p >= psnr(c["d"], c["truth"]) + 10.0


def test_single_precision_class():
    """the same formulas in float32 / complex64 with the sums in double: the arithmetic class the device is held to, outputs and traces
    (TVA_TOL and TVA_TRACE_TOL stay within 10x of it where they were measured)"""
    from _tvauto_model import trace_err
    c, q = quality_case(), QUALITY
    a, ta = tvauto_model(c["d"], c["psf"], q["M"], q["N"], f32(q["noise"]), q["rho"], 100, dtype=np.float32)
    b, tb = tvauto_model(c["d"], c["psf"], q["M"], q["N"], f32(q["noise"]), q["rho"], 100)
    eq, tq = rel_err(a, b), trace_err(ta, tb)
    print("TVA\tfloat32 model\tquality scene n=100\terr=%.3g trace=%.3g" % (eq, tq))
    M, N, rows, cols = SHORT[2][:4]
    d = tvf_image(M, N, rows, cols, M + 3 * N)
    worst, worst_t = 0.0, 0.0
    for name, psf, _, rho, nu, aniso, _ in short_combos(line_psf(), M, N, rows, cols):
        for sigma in SHORT_SIGMAS:
            a, ta = tvauto_model(d, psf, M, N, f32(sigma), rho, 3, None, nu=nu, anisotropic=aniso, dtype=np.float32)
            b, tb = tvauto_model(d, psf, M, N, f32(sigma), rho, 3, None, nu=nu, anisotropic=aniso)
            e, t = rel_err(a, b), trace_err(ta, tb)
            print("TVA\tfloat32 model\t%dx%d win %dx%d %s sigma=%g n=3\terr=%.3g trace=%.3g" % (M, N, rows, cols, name, sigma, e, t))
            worst, worst_t = max(worst, e), max(worst_t, t)
    assert 1e-8 < worst < 1e-5 and 1e-8 < eq < 1e-5 and worst_t < 1e-4 and tq < 1e-4


def _fault_visible(fault, kind, sigma, trace):
    """where a fault can show at all"""
    clamped = bool(np.any(trace[:, 2] == 0))
    if fault in ("S_area", "unweighted"):
        return kind == "fractional" and not clamped  # the 2 % mask moves S by 2 %: judged on the fractional weights only
    if fault == "no_clamp":
        return clamped
    return not clamped  # no_sqrt, res_c, mu_lag need an active mu_k


@pytest.mark.parametrize("case", SHORT, ids=SHORT_IDS)
def test_faults_are_far_outside_the_tolerance(case):
    """every fault model differs from the model by more than 10 x TVA_TOL at n = 3 on each short case of the GPU test with its
    short_combos (mu unused) and both noise levels, wherever the fault is visible: 'no_clamp' where a step clamps at 0, the others
    where none does, 'S_area' and 'unweighted' on the fractional weights only (with the 2 % mask they move S by 2 % and the
    measured distances, 1.5e-4 .. 1.3e-3, leave too little room above a float32 tolerance to rely on)"""
    M, N, rows, cols = case[:4]
    out_shape = case[7][-1]
    d = tvf_image(M, N, rows, cols, M + 3 * N)
    seen = set()
    for name, psf, _, rho, nu, aniso, _ in short_combos(line_psf(), M, N, rows, cols):
        for kind in ("none", "fractional") if M * N < 1 << 20 else ("fractional",):
            w = tvf_weights(kind, rows, cols, M + 3 * N)
            for sigma in SHORT_SIGMAS:
                want, trace = tvauto_model(d, psf, M, N, f32(sigma), rho, 3, w, nu=nu, anisotropic=aniso, out_shape=out_shape)
                for fault in FAULTS:
                    if not _fault_visible(fault, kind, sigma, trace):
                        continue
                    got, _ = tvauto_model(d, psf, M, N, f32(sigma), rho, 3, w, nu=nu, anisotropic=aniso, out_shape=out_shape, fault=fault)
                    e = rel_err(got, want)
                    print("TVA\tfault\t%dx%d win %dx%d %s w=%s sigma=%g %s\terr=%.3g (mu_k %s)"
                          % (M, N, rows, cols, name, kind, sigma, fault, e, " ".join("%.3g" % v for v in trace[:, 2])))
                    assert e > 10 * TVA_TOL, (name, kind, sigma, fault, e)
                    seen.add(fault)
    assert seen == set(FAULTS), set(FAULTS) - seen


TVAUTO_FUNCS = ("fdr_tv_deconv_auto_f32", "fdr_tv_deconv_auto_f32_dev")


def _struct_fields(header, name):
    m = re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}\s*%s\s*;" % (name, name), header)
    assert m, name + " is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return re.findall(r"\b(float|int|double)\s+(\w+)\s*;", body)


def test_symbols_and_surface(fdr):
    header = open(os.path.join(ROOT, "include", "fdr.h")).read()
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int, "double": ctypes.c_double}
    fields = _struct_fields(header, "fdr_tv_auto_params")
    assert [(n, ctype[t]) for t, n in fields] == list(fdr.TvAutoParams._fields_)
    assert [n for _, n in fields] == ["sigma", "tau", "rho", "nu", "iterations", "anisotropic", "nonneg", "norm_area", "out_rows", "out_cols"]
    assert ctypes.sizeof(fdr.TvAutoParams) == 40
    fields = _struct_fields(header, "fdr_tv_auto_result")
    assert [(n, ctype[t]) for t, n in fields] == list(fdr.TvAutoResultC._fields_)
    assert [n for _, n in fields] == ["sigma", "target", "mu", "discrepancy", "S"] == list(fdr.TvAutoResult._fields)
    assert ctypes.sizeof(fdr.TvAutoResultC) == 40
    assert re.search(r"#define\s+FDR_VERSION\s+300\b", header)
    assert re.search(r"#define\s+FDR_TV_AUTO_MAX_RATIO\s+1e6\b", header) and fdr.TV_AUTO_MAX_RATIO == MAX_RATIO == 1e6
    assert re.search(r"#define\s+FDR_TV_AUTO_NU_RATIO\s+25\.f\b", header) and fdr.TV_AUTO_NU_RATIO == NU_RATIO == 25.0
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in TVAUTO_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    sig = inspect.signature(fdr.Plan.tv_deconv_auto).parameters
    assert list(sig) == ["self", "img", "sigma", "rho", "iterations", "weights", "tau", "nu", "anisotropic", "nonneg", "norm_area", "full_plane"]
    assert [sig[k].default for k in list(sig)[2:]] == [0.0, 2.0, 100, None, 0.0, 0.0, False, False, fdr.NORM_NONE, False]
    sig = inspect.signature(fdr.Plan.tv_deconv_auto_dev).parameters
    assert list(sig)[:10] == ["self", "d_img", "rows", "cols", "stride", "d_out", "out_stride", "sigma", "rho", "iterations"]
    assert (sig["iterations"].default, sig["d_weights"].default, sig["wstride"].default, sig["d_trace"].default, sig["nu"].default) == (100, None, 0, None, 0.0)
    sig = inspect.signature(fdr.tvDeblurAuto_myfft).parameters
    assert list(sig)[:3] == ["img", "psf", "sigma"] and sig["weights"].default is None and sig["iterations"].default == 100
    sig = inspect.signature(fdr.tvDeblurAuto_RGB).parameters
    assert list(sig)[:3] == ["channels", "psf", "sigma"] and sig["weights"].default is None and sig["iterations"].default == 100
    cxx = open(os.path.join(ROOT, "include", "fft", "fft.hpp")).read()
    assert re.search(r"inline\s+std::vector<fdr_tv_auto_result>\s+tvDeblurAuto_RGB\s*\(", cxx)


def test_null_arguments_are_refused_before_any_device_work(fdr):
    """a null plan, image, output or params: FDR_ERR_ARG from both entry points, on a machine without a device too; a null result and
    a null trace are fine (they are optional), so they are not what is refused"""
    L = fdr.lib
    img = np.zeros((8, 32), dtype=np.float32)
    out = np.zeros((8, 32), dtype=np.float32)
    prm = fdr.TvAutoParams(0.01, 0.0, 2.0, 0.0, 1, 0, 0, 2, 8, 32)
    res = fdr.TvAutoResultC()
    for h, i, o, p in ((None, img.ctypes.data, out.ctypes.data, ctypes.byref(prm)), (1, None, out.ctypes.data, ctypes.byref(prm)),
                       (1, img.ctypes.data, None, ctypes.byref(prm)), (1, img.ctypes.data, out.ctypes.data, None)):
        assert L.fdr_tv_deconv_auto_f32(h, i, 8, 32, 32, None, 0, o, 32, p, ctypes.byref(res), None) == -1
        assert b"fdr_tv_deconv_auto_f32: null argument" in L.fdr_last_error()
        assert L.fdr_tv_deconv_auto_f32_dev(h, i, 8, 32, 32, None, 0, o, 32, p, None, None) == -1
        assert b"fdr_tv_deconv_auto_f32_dev: null argument" in L.fdr_last_error()


def test_cli_refusals():
    """--tv auto is a leg of its own; beside --tv-color, --rl, --cls or --mode parity it is refused with the usage text, --sigma still
    needs an `auto` option, --tv 0 is still refused, and an accepted line gets as far as the picture.  Every refusal comes before the
    picture is read and before any device work."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")

    def run(*extra, where=("40", "45")):
        return subprocess.run([gpu, "no-such-picture.png", *where, *extra], capture_output=True, text=True, timeout=120)

    for extra in (["--tv", "auto", "--tv-color"], ["--tv", "auto", "--rl", "5"], ["--tv", "auto", "--cls", "0.1"], ["--tv", "auto", "--mode", "parity"],
                  ["--tv", "auto", "--sigma", "-1"], ["--tv", "auto", "--tv-tau", "-1"], ["--tv-tau", "1"], ["--tv", "200", "--tv-tau", "1"],
                  ["--tv", "200", "--sigma", "0.01"], ["--sigma", "0.01"], ["--tv", "0"], ["--tv", "auto", "--tv-iters", "-1"],
                  ["--tv", "200", "--free-boundary", "--tv-color"], ["--tv", "auto", "--free-boundary", "--tv-color"]):
        r = run(*extra)
        assert r.returncode != 0 and "Usage" in r.stdout, (extra, r.stdout)
    r = run("--tv", "auto", "--tv-color")
    assert "--tv auto" in r.stdout and "--sigma" in r.stdout and "--tv-tau" in r.stdout, r.stdout
    for extra, where in ((["--tv", "auto"], ("40", "45")), (["--tv", "auto", "--sigma", "0.02", "--tv-tau", "1.1", "--tv-iters", "30", "--tv-rho", "3"], ("40", "45")),
                         (["--tv", "auto", "--mask", "m.png"], ("40", "45")), (["--tv", "auto", "--free-boundary"], ("40", "45")),
                         (["--tv", "auto", "--sigma", "0.02"], ("auto", "auto")), (["--tv", "200", "--free-boundary"], ("40", "45"))):
        r = run(*extra, where=where)
        assert "Usage" not in r.stdout and "Cannot read image" in r.stdout, (extra, r.stdout)
