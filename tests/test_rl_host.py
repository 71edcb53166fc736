"""CPU checks of the Richardson-Lucy / blur model (tests/_rl_model.py) before it judges the GPU (test_rl_gpu.py): the FFT blur against
direct circular summation, adjointness, the delta PSF, flux conservation, a single-precision implementation inside the GPU
thresholds, injected faults far outside them, and the new C ABI / Python surface."""
import re
import subprocess

import numpy as np
import pytest

from _rl_model import BLUR_TOL, NORM_CROPPED, NORM_NONE, NORM_PADDED, RL_TOL, TAU, blur_model, dense_psf, normalize, rel_err, rl_model, smooth_image


def direct_blur(x, psf, M, N, adjoint=False):
    """blur by explicit shifted sums on the M x N circle: out[r, c] = sum_{i, j} p[i, j] x[(r - i) mod M, (c - j) mod N]
    (the adjoint: x[(r + i) mod M, (c + j) mod N]), then the window"""
    rows, cols = x.shape
    plane = np.zeros((M, N))
    plane[:rows, :cols] = x
    out = np.zeros((M, N))
    s = -1 if adjoint else 1
    for i in range(psf.shape[0]):
        for j in range(psf.shape[1]):
            out += float(psf[i, j]) * np.roll(plane, (s * i, s * j), axis=(0, 1))
    return out[:rows, :cols]


CASES = [(8, 32, 8, 32), (16, 64, 11, 50), (32, 32, 32, 32), (64, 128, 40, 97)]


@pytest.mark.parametrize("M,N,rows,cols", CASES)
def test_fft_blur_is_circular_convolution(M, N, rows, cols):
    rng = np.random.default_rng(M * N)
    x = rng.standard_normal((rows, cols))
    for psf in (dense_psf(3, 5), rng.standard_normal((7, 3)), np.ones((1, 1))):
        if psf.shape[0] > M or psf.shape[1] > N:
            continue
        for adj in (False, True):
            assert np.allclose(blur_model(x, psf, M, N, adjoint=adj), direct_blur(x, psf, M, N, adjoint=adj), atol=1e-12, rtol=0)


@pytest.mark.parametrize("M,N,rows,cols", CASES + [(256, 512, 200, 301)])
def test_adjointness(M, N, rows, cols):
    rng = np.random.default_rng(7)
    x, y = rng.standard_normal((rows, cols)), rng.standard_normal((rows, cols))
    psf = dense_psf(1, min(9, M))
    lhs = np.sum(blur_model(x, psf, M, N) * y)
    rhs = np.sum(x * blur_model(y, psf, M, N, adjoint=True))
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y)


def test_delta_psf_leaves_d_plus():
    M, N = 64, 128
    rng = np.random.default_rng(3)
    d = rng.standard_normal((M, N))
    d[np.abs(d) < 1e-3] = 0.5
    d[0, 0], d[0, 1] = 0.5 * TAU, 2 * TAU  # (0, tau] becomes 0 by the guard; above tau is kept
    delta = np.ones((1, 1))
    for n in (1, 5, 30):
        u = rl_model(d, delta, M, N, n)
        want = np.maximum(d, 0)
        want[0, 0] = 0.0
        assert np.allclose(u, want, rtol=1e-12, atol=1e-15), n
    assert np.array_equal(rl_model(d, delta, M, N, 0), np.maximum(d, 0))  # n = 0: d+


def test_flux_is_conserved():
    M, N = 64, 128
    d = smooth_image(M, N, 2).astype(np.float64) + 0.01
    psf = dense_psf(4, 7)
    f0 = d.sum()
    for n in range(1, 11):
        u = rl_model(d, psf, M, N, n)
        assert abs(u.sum() / f0 - 1) <= 1e-12, n
    assert rel_err(u, d) > 1e-3  # and it did change the image


def test_normalisations():
    M, N = 32, 64
    u = np.linspace(0.2, 0.8, 20 * 40).reshape(20, 40)
    assert np.array_equal(normalize(u, NORM_NONE, M, N), u)
    c = normalize(u, NORM_CROPPED, M, N)
    assert c.min() == 0 and c.max() == 1
    p = normalize(u, NORM_PADDED, M, N)  # zeros outside the window count
    assert np.allclose(p, u / 0.8)
    full = np.linspace(0.2, 0.8, M * N).reshape(M, N)
    assert np.allclose(normalize(full, NORM_PADDED, M, N), normalize(full, NORM_CROPPED, M, N))
    assert np.array_equal(normalize(np.full((4, 4), 3.0), NORM_CROPPED, M, N), np.zeros((4, 4)))


def _fp32_cases():
    rng = np.random.default_rng(11)
    for M, N, rows, cols in ((256, 256, 256, 256), (128, 512, 100, 333)):
        img = (smooth_image(M, N, 5)[:rows, :cols] + 0.1 * rng.random((rows, cols))).astype(np.float32)
        img[:8, :8] -= 0.5
        yield M, N, img, dense_psf(6, 9)


def test_single_precision_passes():
    """numpy in single precision (complex64 spectra, float32 planes) is the device's arithmetic class: it must pass the GPU
    thresholds against the float64 model"""
    for M, N, img, psf in _fp32_cases():
        for adj in (False, True):
            assert rel_err(blur_model(img, psf, M, N, adjoint=adj, dtype=np.float32), blur_model(img, psf, M, N, adjoint=adj)) <= BLUR_TOL
        for n in (1, 5, 30):
            e = rel_err(rl_model(img, psf, M, N, n, dtype=np.float32), rl_model(img, psf, M, N, n))
            assert e <= RL_TOL, (M, N, n, e)


def test_faults_fail():
    """each fault misses the GPU thresholds by more than 5x"""
    for M, N, img, psf in _fp32_cases():
        H_ok = blur_model(img, psf, M, N, adjoint=True)
        wrong_adj = blur_model(img, psf, M, N, adjoint=False)  # an adjoint without the conjugate
        assert rel_err(wrong_adj, H_ok) > 5 * BLUR_TOL
        shifted = np.vstack([np.zeros((1, psf.shape[1])), psf])  # the PSF one row lower
        assert rel_err(blur_model(img, shifted, M, N), blur_model(img, psf, M, N)) > 5 * BLUR_TOL
        want = rl_model(img, psf, M, N, 5)
        assert rel_err(rl_model(img, psf, M, N, 4), want) > 5 * RL_TOL  # one iteration fewer
        assert rel_err(rl_model(img, psf, M, N, 5, fault="no_conj"), want) > 5 * RL_TOL
        assert rel_err(rl_model(img, shifted, M, N, 5), want) > 5 * RL_TOL
        assert img.min() < 0
        assert rel_err(rl_model(img, psf, M, N, 5, fault="raw_d"), want) > 5 * RL_TOL  # d in place of d+


RL_FUNCS = ("fdr_set_operator_psf", "fdr_set_operator_psf_dev", "fdr_set_operator_psf_motion", "fdr_blur_f32", "fdr_blur_f32_dev",
            "fdr_richardson_lucy_f32", "fdr_richardson_lucy_f32_dev")


def test_symbols_and_constants(fdr):
    import inspect
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fdr.h")).read()
    assert re.search(r"#define\s+FDR_NORM_NONE\s+2\b", header)
    assert re.search(r"#define\s+FDR_RL_TAU\s+1e-7f\b", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in RL_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    assert fdr.NORM_NONE == 2
    for meth in ("set_operator_psf", "set_operator_psf_dev", "set_operator_psf_motion", "blur", "blur_dev", "richardson_lucy",
                 "richardson_lucy_dev"):
        assert callable(getattr(fdr.Plan, meth)), meth
    assert inspect.signature(fdr.Plan.richardson_lucy).parameters["norm_area"].default == fdr.NORM_NONE
    sig = inspect.signature(fdr.richardsonLucy_myfft).parameters
    assert list(sig)[:3] == ["img", "psf", "iterations"] and sig["norm_area"].default == fdr.NORM_NONE
    assert fdr._rl_plan_size(5, 20) == (8, 32) and fdr._rl_plan_size(300, 700) == (512, 1024)
