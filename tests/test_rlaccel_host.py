"""CPU pins of tests/_rlaccel_model.py, the float64 model of accelerated Richardson-Lucy, before it judges the GPU: injected faults,
n <= 2 against the plain models, flux, fixed points, the convergence claim on the model itself, and the symbols of the binding."""
import os
import re

import numpy as np
import pytest

from _rl_model import centred_psf, rl_model, smooth_image
from _rlaccel_model import (ACCEL_MAX, FAULTS, accelerate, free_divergence, free_scene, plain_divergence, plain_scene, rl_accel_model,
                            rl_accel_path, rl_step_fn, rlfree_accel_model, rlfree_accel_state, unit_psf)
from _rlfree_model import flux_defect, rlfree_model, rlfree_state
from _spectral import delta_psf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit_psf(oracle):
    """the project's CPU motion PSF 15 / 30 degrees, normalised to sum 1"""
    return unit_psf(oracle.motion_blur_kernel(15, 30.0))


@pytest.fixture(scope="module")
def small(oracle):
    """a 64 x 128 plan, window 50 x 100, the centred unit motion PSF, a picture with negative pixels"""
    M, N, rows, cols = 64, 128, 50, 100
    psf = centred_psf(_unit_psf(oracle), M, N)
    d = smooth_image(rows, cols, 3) + np.random.default_rng(3).normal(0, 2e-3, (rows, cols)).astype(np.float32)
    d[:4, :9] -= np.float32(0.4)
    return M, N, psf, d


@pytest.mark.parametrize("fault", FAULTS)
def test_faults_change_the_result(small, fault):
    """every fault moves u_12 by at least ten times the largest tolerance the GPU test may use (1e-4)"""
    M, N, psf, d = small
    for model, kw in ((rl_accel_model, {}), (rlfree_accel_model, {})):
        good, a_good = model(d, psf, M, N, 12, **kw)
        bad, a_bad = model(d, psf, M, N, 12, fault=fault, **kw)
        e = float(np.max(np.abs(good - bad)) / np.max(np.abs(good)))
        print("RLA\tfault\t%s\t%s\trel=%.3g\talpha diff=%.3g" % (model.__name__, fault, e, float(np.max(np.abs(a_good - a_bad)))))
        assert e >= 1e-3, (model.__name__, fault, e)


def test_no_clip_needs_a_negative_point(small):
    """the pin of 'no_clip' above is not vacuous: the unclipped extrapolation does go negative on that picture"""
    M, N, psf, d = small
    u0, step = rl_step_fn(d, psf, M, N)
    seen = []

    def spy(y):
        seen.append(float(y.min()))
        return step(y)

    accelerate(u0, spy, 12, fault="no_clip")
    assert min(seen) < 0.0


@pytest.mark.parametrize("n", [0, 1, 2])
def test_first_two_iterations_are_plain(small, n):
    M, N, psf, d = small
    got, alphas = rl_accel_model(d, psf, M, N, n)
    assert np.array_equal(got, rl_model(d, psf, M, N, n))
    assert np.array_equal(alphas, np.zeros(n))
    w = (np.random.default_rng(5).random(d.shape) > 0.1).astype(np.float32)
    got, alphas = rlfree_accel_model(d, psf, M, N, n, weights=w, out_shape=(M, N))
    assert np.array_equal(got, rlfree_model(d, psf, M, N, n, weights=w, out_shape=(M, N)))
    assert np.array_equal(alphas, np.zeros(n))


def test_path_is_the_run_stopped_early(small):
    M, N, psf, d = small
    keep, alphas = rl_accel_path(d, psf, M, N, (0, 3, 7))
    for n in (0, 3, 7):
        u, a = rl_accel_model(d, psf, M, N, n)
        assert np.array_equal(keep[n], u) and np.array_equal(a, alphas[:n])


def test_alphas_lie_in_range(small):
    M, N, psf, d = small
    for alphas in (rl_accel_model(d, psf, M, N, 30)[1], rlfree_accel_model(d, psf, M, N, 30)[1]):
        assert alphas[0] == 0 and alphas[1] == 0
        assert np.all((alphas >= 0) & (alphas <= ACCEL_MAX))
        assert alphas[2:].max() > 0.5  # the extrapolation does engage


def test_flux_is_conserved(small, oracle):
    """every u_k is the output of a step: sum(u) = sum(d+) on a full plane with a unit PSF, sum(alpha_cov u) = sum(dw) for the free form"""
    M, N, psf, d = small
    full = smooth_image(M, N, 4)
    for n in (3, 10, 30):
        u, _ = rl_accel_model(full, _unit_psf(oracle), M, N, n)
        flux = abs(float(np.sum(u)) / float(np.sum(full, dtype=np.float64)) - 1.0)
        st, _ = rlfree_accel_state(d, psf, M, N, n)
        print("RLA\tflux\tn=%d\tplain %.3g\tfree %.3g" % (n, flux, flux_defect(st)))
        assert flux <= 1e-12 and flux_defect(st) <= 1e-12


def test_fixed_points():
    """A delta PSF keeps d+ and a constant image stays constant.  With an exact step (the delta blur written out: c = y, no
    transform) g is exactly 0, the denominator is 0 and every alpha is 0; through the FFT g is rounding noise, its quotient is
    arbitrary within the clamp, and the estimate still stays put."""
    M, N = 32, 64
    const = np.full((M, N), 0.37, dtype=np.float32)
    for d in (smooth_image(M, N, 2) - np.float32(0.3), const, np.zeros((M, N), dtype=np.float32)):
        dp = np.maximum(d.astype(np.float64), 0)

        def exact_step(y):
            r = np.where(y > 1e-7, dp / np.where(y > 1e-7, y, 1), 0)
            return np.maximum(y * r, 0)

        u, alphas = accelerate(dp, exact_step, 8)
        assert np.array_equal(u, dp) and not alphas.any()
        u, alphas = rl_accel_model(d, delta_psf(0, 0), M, N, 8)
        assert float(np.max(np.abs(u - dp))) <= 1e-13
        assert np.all((alphas >= 0) & (alphas <= ACCEL_MAX)) and alphas[0] == 0 and alphas[1] == 0
    u, alphas = rl_accel_model(np.zeros((M, N), dtype=np.float32), delta_psf(0, 0), M, N, 8)
    assert not u.any() and not alphas.any()


def test_convergence_plain(oracle):
    """10 accelerated iterations reach at most the I-divergence of 15 plain ones (measured: that of 19 plain ones; 20 accelerated
    ones that of about 90)"""
    psf = _unit_psf(oracle)
    M = N = 512
    d = plain_scene(psf, M, N)
    acc = plain_divergence(d, psf, M, N, rl_accel_model(d, psf, M, N, 10)[0])
    pl = plain_divergence(d, psf, M, N, rl_model(d, psf, M, N, 15))
    print("RLA\tconvergence\tplain form\taccelerated 10: %.6g\tplain 15: %.6g" % (acc, pl))
    assert acc <= pl, (acc, pl)


def test_convergence_free(oracle):
    """the same for the free-boundary form, a 200 x 400 window of a 256 x 512 plan with the centred PSF (measured: 10 accelerated
    iterations reach the I-divergence of 18 to 19 plain ones, so the bound of 15 holds with a quarter to spare)"""
    psf = _unit_psf(oracle)
    M, N = 256, 512
    cp, d = free_scene(psf, M, N)
    acc = free_divergence(d, cp, M, N, rlfree_accel_state(d, cp, M, N, 10)[0]["u"])
    pl = free_divergence(d, cp, M, N, rlfree_state(d, cp, M, N, 15)["u"])
    print("RLA\tconvergence\tfree form\taccelerated 10: %.6g\tplain 15: %.6g" % (acc, pl))
    assert acc <= pl, (acc, pl)


RLA_FUNCS = ("fdr_richardson_lucy_accel_f32", "fdr_richardson_lucy_accel_f32_dev", "fdr_richardson_lucy_free_accel_f32",
             "fdr_richardson_lucy_free_accel_f32_dev")


def test_symbols_and_constants(fdr):
    header = open(os.path.join(ROOT, "include", "fdr.h")).read()
    for name in RLA_FUNCS:
        assert name in fdr.EXPORTED_SYMBOLS, name
        assert hasattr(fdr.lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    m = re.search(r"#define\s+FDR_RL_ACCEL_MAX\s+([0-9.]+)f", header)
    assert m and float(m.group(1)) == ACCEL_MAX == fdr.RL_ACCEL_MAX == 1 - 2.0 ** -10
    with pytest.raises(ValueError):
        fdr._alphas_array(3, False, True)
