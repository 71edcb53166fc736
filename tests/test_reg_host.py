"""CPU checks of the float64 model of the regularisation choice (tests/_reg_model.py) before it judges the GPU (test_reg_gpu.py):
rho is the residual energy of the CLS restoration computed spatially, P obeys Parseval, the trace tends to M N, Immerkaer's
estimate recovers the sigma of Gaussian noise, the model alone meets the quality margins the GPU test asks of the device, every
injected fault lands far outside the GPU thresholds on the GPU test's own inputs, and the new C ABI / Python surface is declared,
exported and laid out as the binding has it."""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _pad_model
import _reg_model as rm
from _cls_model import cls_raw
from _rl_model import blur_model
from conftest import ROOT

REG_FUNCS = ("fdr_noise_sigma_f32", "fdr_noise_sigma_f32_dev", "fdr_reg_curve_f32", "fdr_reg_curve_f32_dev", "fdr_choose_reg_f32",
             "fdr_choose_reg_f32_dev")
REG_CONSTANTS = {"FDR_REG_DISCREPANCY": 0, "FDR_REG_GCV": 1, "FDR_REG_PARAM_K": 0, "FDR_REG_PARAM_GAMMA": 1, "FDR_REG_AT_LOW": 1,
                 "FDR_REG_AT_HIGH": 2}


def test_header_library_and_python_surface(fdr, tmp_path):
    text = open(os.path.join(ROOT, "include", "fdr.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in REG_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    for name, value in REG_CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
        assert getattr(fdr, name[4:]) == value == getattr(rm, name[4:]), name
    # the structures as the C compiler lays them out
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fdr.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(fdr_reg_params), offsetof(fdr_reg_params, lo), offsetof(fdr_reg_params, refine),\n'
                   '       sizeof(fdr_reg_choice), offsetof(fdr_reg_choice, gcv), offsetof(fdr_reg_choice, evaluations));\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(fdr.RegParams), fdr.RegParams.lo.offset, fdr.RegParams.refine.offset, ctypes.sizeof(fdr.RegChoiceC),
                   fdr.RegChoiceC.gcv.offset, fdr.RegChoiceC.evaluations.offset], got
    assert [f[0] for f in fdr.RegParams._fields_] == ["method", "param", "fixed", "sigma", "tau", "lo", "hi", "n_grid", "refine"]
    assert fdr.RegChoice._fields == tuple(f[0] for f in fdr.RegChoiceC._fields_) == rm.Choice._fields
    p = inspect.signature(fdr.Plan.choose_regularisation).parameters
    assert [(k, v.default) for k, v in p.items()][2:] == [("method", fdr.REG_GCV), ("param", fdr.REG_PARAM_GAMMA), ("fixed", 0.0), ("sigma", 0.0),
                                                          ("tau", 0.0), ("lo", 0.0), ("hi", 0.0), ("n_grid", 0), ("refine", -1)]
    for name in ("noise_sigma", "noise_sigma_dev", "reg_curve", "choose_regularisation_dev"):
        assert callable(getattr(fdr.Plan, name)), name
    assert list(inspect.signature(fdr.chooseRegularisation).parameters)[:2] == ["img", "psf"]
    shim = open(os.path.join(ROOT, "include", "fft", "fft.hpp")).read()
    assert "chooseRegularisation(const Mat& channel, const Mat& psf" in shim and "estimateNoiseSigma(const Mat&" in shim
    cli = open(os.path.join(ROOT, "tools", "cli", "gpu.cpp")).read()
    assert '"--k"' in cli and '"--reg"' in cli and '"--sigma"' in cli and "regularisation: K" in cli


@pytest.mark.parametrize("M,N,rows,cols", [(16, 32, 16, 32), (32, 64, 29, 59), (64, 32, 3, 3)])
def test_rho_is_the_spatial_residual(oracle, M, N, rows, cols):
    d = rm.random_picture(M, N, rows, cols)
    for name, psf in rm.curve_psfs(oracle, M, N):
        for K, gamma in rm.CANDIDATES[1:]:
            x = cls_raw(d, psf, K, gamma, M, N)
            r = rm.pad_plane(d, M, N) - blur_model(x, psf, M, N)
            rho, _ = rm.curve(d, psf, M, N, [K], [gamma])
            want = float(np.sum(r * r))
            # (1e-7: with K = 0 the zero-mean PSF leaves H(0, 0) ~ 1e-9, the restored plane carries a mean of 1e9 and the spatial
            # form loses nine digits to it; rho itself does not)
            assert abs(rho[0] - want) <= 1e-7 * max(want, 1e-9 * float(np.sum(d.astype(np.float64) ** 2))), (name, K, gamma)


def test_parseval_and_trace_limit(oracle):
    for M, N, rows, cols in ((8, 32, 8, 32), (64, 64, 61, 59), (16, 128, 3, 3)):
        d = rm.random_picture(M, N, rows, cols)
        s2 = float(np.sum(d.astype(np.float64) ** 2))
        assert abs(rm.power(d, M, N).sum() - s2) <= 1e-12 * s2
        for name, psf in rm.curve_psfs(oracle, M, N):
            rho, tr = rm.curve(d, psf, M, N, [rm.PARSEVAL_K, 0.0, 0.0], [0.0, 1e30, 0.0])
            assert abs(rho[0] - s2) <= 1e-12 * s2 and abs(tr[0] - M * N) <= 1e-12 * M * N
            # L(0, 0) = 0: gamma leaves the DC bin to |H|^2 alone, so its q is 0 there unless H(0, 0) = 0 too
            assert M * N - 1 - 1e-9 <= tr[1] <= M * N
            assert rho[2] == 0.0 and tr[2] == 0.0


def test_immerkaer_on_gaussian_noise():
    rng = np.random.default_rng(11)
    for sigma in (0.002, 0.05, 3.0):
        est = rm.noise_sigma((sigma * rng.standard_normal((512, 512))).astype(np.float32))
        print("REG\tmodel\tnoise sigma=%g\testimate=%.6g\t(%.2f %%)" % (sigma, est, 100 * (est / sigma - 1)))
        assert abs(est / sigma - 1) <= 0.02
    assert rm.noise_sigma(np.full((3, 3), 7.0)) == 0.0
    d = np.zeros((3, 3))
    d[1, 1] = 1.0
    assert abs(rm.noise_sigma(d) - math.sqrt(math.pi / 2) * 4 / 6) <= 1e-15


def test_grid_and_search_rules():
    v = rm.log_grid(1e-8, 1e2, 32)
    assert v[0] == 1e-8 and v[-1] == 1e2 and all(a < b for a, b in zip(v, v[1:]))
    assert abs(v[1] / v[0] - 10 ** (10 / 31)) < 1e-12
    z = np.zeros((20, 40))
    psf = np.ones((3, 3)) / 9
    d = rm.choose(z, psf, 32, 64, method=rm.REG_DISCREPANCY)
    g = rm.choose(z, psf, 32, 64, method=rm.REG_GCV)
    assert (d.value, d.flags, d.evaluations, d.residual) == (1e2, rm.REG_AT_HIGH, 32, 0.0)
    assert (g.value, g.flags, g.evaluations, g.gcv) == (1e-8, rm.REG_AT_LOW, 96, 0.0)
    x = rm.random_picture(32, 64, 20, 40)
    assert rm.choose(x, psf, 32, 64, method=rm.REG_DISCREPANCY, sigma=1e-9).flags == rm.REG_AT_LOW
    assert rm.choose(x, psf, 32, 64, method=rm.REG_DISCREPANCY, sigma=1e3).flags == rm.REG_AT_HIGH
    c = rm.choose(x, psf, 32, 64, method=rm.REG_DISCREPANCY, sigma=0.05, n_grid=8, refine=3)
    rho, _ = rm.curve(x, psf, 32, 64, [0.0], [c.value])
    T = 20 * 40 * 0.05 ** 2
    assert c.flags == 0 and c.evaluations == 32 and abs(rho[0] / T - 1) < 1e-3  # the interpolated value meets the target


@pytest.mark.parametrize("scene", rm.CHOICE_SCENES)
@pytest.mark.parametrize("level", rm.CHOICE_NOISE)
def test_model_meets_the_quality_margins(scene, level):
    """what test_reg_gpu.py asks of the device, of the model alone: the margins below the best weight of the 81-point grid, and the
    blurred input beaten where the table of _reg_model.py says so"""
    n = rm.CHOICE_SIZE
    truth, b = rm.choice_case(scene, level)
    state = rm.choice_state(scene, level)
    blurred = _pad_model.psnr(b, truth)
    est = rm.noise_sigma(b)
    print("REG\tmodel\t%s %g\tsigma estimate %.5f (true %.5f)\tblurred %.2f dB" % (scene, level, est, level * truth.max(), blurred))
    assert abs(est / (level * truth.max()) - 1) <= 0.02
    for method in (rm.REG_DISCREPANCY, rm.REG_GCV):
        for param in (rm.REG_PARAM_K, rm.REG_PARAM_GAMMA):
            c = rm.choose(b, rm.choice_psf(), n, n, method=method, param=param, state=state)
            got = _pad_model.psnr(rm.restore(b, *rm.pair_of(param, c.value)), truth)
            best, at = rm.best_psnr(scene, level, param)
            print("REG\tmodel\t%s %g method %d param %d\tvalue=%.4g\tpsnr=%.2f\tbest=%.2f at %.3g\tover blurred %+.2f" %
                  (scene, level, method, param, c.value, got, best, at, got - blurred))
            assert c.flags == 0 and c.evaluations == 96
            margin = rm.QUALITY_MARGIN.get((method, param))
            if margin is not None:
                assert got >= best - margin, (method, param)
            if rm.beats_blurred_required(method, param, scene, level):
                assert got > blurred, (method, param)


FAULT_PLANS = [(8, 32), (16, 32), (64, 64), (8, 8192)]
CURVE_FAULTS = [f for f in rm.FAULTS if f not in ("target_plan_area",) + rm.INVISIBLE_FAULTS]
KS = [c[0] for c in rm.CANDIDATES]
GS = [c[1] for c in rm.CANDIDATES]


def _fault_distance(oracle, fault):
    """the largest curve error (as the GPU test measures it) the fault causes on the GPU test's pictures, PSFs and candidates"""
    worst = 0.0
    for M, N in FAULT_PLANS:
        for _, psf in rm.curve_psfs(oracle, M, N):
            good, bad = rm.operator_terms(psf, M, N), rm.operator_terms(psf, M, N, fault)
            for _, d in rm.curve_pictures(M, N):
                rho_m, tr_m = rm.curve_from(rm.power(d, M, N), good, KS, GS)
                rho, tr = rm.curve_from(rm.power(d, M, N, fault), bad, KS, GS)
                worst = max((worst,) + rm.curve_errors(rho, tr, rho_m, tr_m, float(np.sum(d.astype(np.float64) ** 2))))
    return worst


@pytest.mark.parametrize("fault", CURVE_FAULTS)
def test_curve_faults_are_visible(oracle, fault):
    dist = _fault_distance(oracle, fault)
    print("REG\tfault\t%s\tdistance=%.3g\t(10 x CURVE_TOL = %.3g)" % (fault, dist, 10 * rm.CURVE_TOL))
    assert dist > 10 * rm.CURVE_TOL


def test_mirror_row_is_no_fault(oracle):
    """a[M - m] = a[m]: the fault the packed column's upper half invites changes nothing, in the model or anywhere"""
    assert _fault_distance(oracle, "mirror_row") <= 1e-12


def test_target_fault_is_visible():
    n = rm.CHOICE_SIZE
    _, b = rm.choice_case(*rm.WINDOW_CHOICE[:2])
    w = np.ascontiguousarray(b[:rm.WINDOW_CHOICE[2], :rm.WINDOW_CHOICE[3]])
    state = rm.power(w, n, n), rm.operator_terms(rm.choice_psf(), n, n)
    for param in (rm.REG_PARAM_K, rm.REG_PARAM_GAMMA):
        good = rm.choose(w, rm.choice_psf(), n, n, method=rm.REG_DISCREPANCY, param=param, state=state)
        bad = rm.choose(w, rm.choice_psf(), n, n, method=rm.REG_DISCREPANCY, param=param, state=state, fault="target_plan_area")
        dist = abs(math.log(bad.value / good.value))
        print("REG\tfault\ttarget_plan_area param %d\tlog distance=%.3g" % (param, dist))
        assert dist > 10 * rm.VALUE_LOG_TOL
