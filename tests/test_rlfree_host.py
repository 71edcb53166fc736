"""CPU pins of tests/_rlfree_model.py, the float64 model of free-boundary, weighted Richardson-Lucy, before it judges the device
(test_rlfree_gpu.py): the coverage against direct summation, plain RL as the full-plane special case, the flux invariant, a delta
PSF, injected faults, the quality claims of the feature on a cropped scene, and the public surface.  No GPU needed.  Cases print an
`RLF` line with their measured values (pytest -s)."""
import re
import subprocess

import numpy as np
import pytest

from _rl_model import TAU, centred_psf, dense_psf, op_spectrum, psnr, rel_err, rl_model, smooth_image
from _rlfree_model import QUALITY, SIGMA, flux_defect, fullblur, quality_case, rlfree_model, rlfree_state


def line_psf(size, angle):
    """a motion-like line PSF made on the CPU as test_tv_host.py makes one (the GPU tests use motionBlurKernel), sum 1"""
    k = np.zeros((size, size))
    c = size // 2
    for t in np.linspace(-c, c, 4 * size):
        k[int(round(c - t * np.sin(np.deg2rad(angle)))), int(round(c + t * np.cos(np.deg2rad(angle))))] = 1
    return (k / k.sum()).astype(np.float32)


def _weights(rows, cols, seed, zero=0.1):
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.2, 1.0, (rows, cols))
    m[rng.random((rows, cols)) < zero] = 0
    return m.astype(np.float32)


def test_alpha_is_the_direct_sum():
    """alpha[i, j] = sum over window pixels (y, x) of m[y, x] psf[(y - i) % M, (x - j) % N]: how much data sees plan pixel (i, j)"""
    M, N, rows, cols = 8, 32, 5, 20
    psf = dense_psf(3, 3)
    m = _weights(rows, cols, 1)
    st = rlfree_state(np.ones((rows, cols)), psf, M, N, 0, weights=m)
    want = np.zeros((M, N))
    for i in range(M):
        for j in range(N):
            for a in range(3):
                for b in range(3):
                    y, x = (i + a) % M, (j + b) % N
                    if y < rows and x < cols:
                        want[i, j] += float(m[y, x]) * float(psf[a, b])
    e = float(np.max(np.abs(st["alpha"] - want)))
    print("RLF\talpha direct\terr=%.3g" % e)
    assert e <= 1e-13
    seen = want > SIGMA
    assert np.array_equal(st["wgt"] > 0, seen) and np.allclose(st["wgt"][seen], 1 / want[seen], rtol=1e-12)
    mean = float(np.sum(m.astype(np.float64))) / float(np.sum(m.astype(np.float64)))  # d = 1: sum(dw) / sum(W) = 1
    assert np.allclose(st["u"][seen], mean, rtol=1e-12) and np.all(st["u"][~seen] == 0)


def test_full_plane_window_is_plain_rl():
    """full-plane window, all-ones weights, normalised PSF: alpha = 1, and each iteration is one step of rl_model's update on the same u"""
    M, N = 32, 64
    psf = dense_psf(2, 5).astype(np.float64)
    psf /= psf.sum()  # normalised in double: the float32 PSF's sum is 1 only to 1e-8
    d = smooth_image(M, N, 3) - np.float32(0.15)  # some negative pixels
    H = op_spectrum(psf, M, N)
    st0 = rlfree_state(d, psf, M, N, 0)
    assert float(np.max(np.abs(st0["alpha"] - 1))) <= 1e-12
    dp = np.maximum(d.astype(np.float64), 0)
    u = st0["u"]
    for n in (1, 2, 5):
        got = rlfree_state(d, psf, M, N, n)["u"]
        u = st0["u"]
        for _ in range(n):  # rl_model's update from the free-boundary start
            c = fullblur(u, H)
            r = np.where(c > TAU, dp / np.where(c > TAU, c, 1), 0)
            u = np.maximum(u * fullblur(r, H, adjoint=True), 0)
        e = rel_err(got, u)
        print("RLF\tplain RL step\tn=%d\terr=%.3g" % (n, e))
        assert e <= 1e-12, (n, e)


@pytest.mark.parametrize("case", ["cropped", "masked", "topleft"])
def test_flux_invariant(case):
    M, N, rows, cols = 64, 128, 37, 101
    psf = dense_psf(5, 5) if case != "topleft" else line_psf(9, 30.0)
    if case == "cropped":
        psf = centred_psf(psf, M, N)
    m = _weights(rows, cols, 2) if case == "masked" else None
    d = smooth_image(M, N, 8)[:rows, :cols]
    for n in (1, 3, 30):
        f = flux_defect(rlfree_state(d, psf, M, N, n, weights=m))
        print("RLF\tflux\t%s n=%d\tdefect=%.3g" % (case, n, f))
        assert f <= 1e-10, (case, n, f)


def test_delta_psf_returns_d_plus():
    M, N, rows, cols = 16, 64, 11, 50
    d = smooth_image(M, N, 5)[:rows, :cols] - np.float32(0.2)
    d[np.abs(d) <= 1e-6] = 0.01
    delta = np.zeros((3, 3), dtype=np.float32)
    delta[0, 0] = 1
    for n in (1, 2, 7):
        e = rel_err(rlfree_model(d, delta, M, N, n), np.maximum(d, 0))
        assert e <= 1e-12, (n, e)
    # outside the window nothing sees the plan: alpha = 0, u = 0
    assert np.all(rlfree_state(d, delta, M, N, 3)["u"][rows:, :] == 0)


def test_faults_are_visible():
    M, N, rows, cols = 64, 128, 40, 90
    psf = centred_psf(dense_psf(7, 5), M, N)
    d = smooth_image(M, N, 6)[:rows, :cols]
    m = _weights(rows, cols, 4)
    good = rlfree_model(d, psf, M, N, 5, weights=m)
    for fault in ("no_wgt", "alpha_blur", "mask_d_only"):
        bad = rlfree_model(d, psf, M, N, 5, weights=m, fault=fault)
        e = rel_err(bad, good)
        print("RLF\tfault\t%s\trel=%.3g" % (fault, e))
        assert e > 1e-3, (fault, e)
    # a non-symmetric PSF tells blur from blur^T even without a mask
    tl = dense_psf(9, 5)
    e = rel_err(rlfree_model(d, tl, M, N, 5, fault="alpha_blur"), rlfree_model(d, tl, M, N, 5))
    assert e > 1e-3, e


def test_free_boundary_beats_plain_rl_on_a_crop():
    """the quality claim: a 480 x 480 crop of a circularly blurred 1024^2 scene, restored on a 512^2 plan, n = 30"""
    q = QUALITY
    psf = line_psf(*q["psf"])
    truth, d, _, _ = quality_case(lambda M, N: centred_psf(psf, M, N))
    cp = centred_psf(psf, q["M"], q["N"])
    plain = psnr(rl_model(d, cp, q["M"], q["N"], q["n"]), truth)
    free = psnr(rlfree_model(d, cp, q["M"], q["N"], q["n"]), truth)
    print("RLF\tquality (model)\tblurred %.2f dB, plain RL %.2f dB, free boundary %.2f dB" % (psnr(d, truth), plain, free))
    assert free >= plain + 10.0, (plain, free)
    # a top-left PSF: the result rolled back by the PSF's half-size
    tl = rlfree_state(d, psf, q["M"], q["N"], q["n"])["u"]
    tl = np.roll(tl, (psf.shape[0] // 2, psf.shape[1] // 2), axis=(0, 1))[:q["rows"], :q["cols"]]
    print("RLF\tquality (model)\ttop-left PSF, rolled back %.2f dB" % psnr(tl, truth))
    assert psnr(tl, truth) >= free - 1.0


def test_zero_weights_remove_stuck_pixels():
    q = QUALITY
    psf = line_psf(*q["psf"])
    truth, _, d_stuck, w = quality_case(lambda M, N: centred_psf(psf, M, N))
    cp = centred_psf(psf, q["M"], q["N"])
    plain = psnr(rl_model(d_stuck, cp, q["M"], q["N"], q["n"]), truth)
    unmasked = psnr(rlfree_model(d_stuck, cp, q["M"], q["N"], q["n"]), truth)
    masked = psnr(rlfree_model(d_stuck, cp, q["M"], q["N"], q["n"], weights=w), truth)
    print("RLF\tstuck pixels (model)\tplain RL %.2f dB, free boundary %.2f dB, masked %.2f dB" % (plain, unmasked, masked))
    assert masked >= unmasked + 10.0, (unmasked, masked)


RLFREE_FUNCS = ("fdr_richardson_lucy_free_f32", "fdr_richardson_lucy_free_f32_dev")


def test_symbols_and_surface(fdr):
    import ctypes
    import inspect
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fdr.h")).read()
    assert re.search(r"typedef\s+struct\s+fdr_rlfree_params\s*\{[^}]*int\s+iterations;[^}]*float\s+sigma;[^}]*int\s+norm_area;[^}]*int\s+out_rows;"
                     r"[^}]*int\s+out_cols;[^}]*\}\s*fdr_rlfree_params\s*;", header)
    assert re.search(r"#define\s+FDR_RL_SIGMA\s+1e-2f", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in RLFREE_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    sig = inspect.signature(fdr.Plan.richardson_lucy_free).parameters
    assert list(sig)[:4] == ["self", "img", "iterations", "weights"]
    assert (sig["weights"].default, sig["norm_area"].default, sig["full_plane"].default) == (None, fdr.NORM_NONE, False)
    assert abs(sig["sigma"].default - SIGMA) < 1e-9 and callable(fdr.Plan.richardson_lucy_free_dev)
    sig = inspect.signature(fdr.richardsonLucyFree_myfft).parameters
    assert list(sig)[:4] == ["img", "psf", "iterations", "weights"]
    assert fdr._rlfree_plan_size(480, 480, 15, 15) == (512, 512) and fdr._rlfree_plan_size(3, 3, 2, 2) == (8, 32)
    assert fdr._rlfree_plan_size(512, 512, 15, 15) == (1024, 1024)
    assert ctypes.sizeof(fdr.RlFreeParams) == 20
    assert [f[0] for f in fdr.RlFreeParams._fields_] == ["iterations", "sigma", "norm_area", "out_rows", "out_cols"]
