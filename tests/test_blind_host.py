"""Blind Richardson-Lucy on the CPU: the float64 model of tests/_blind_model.py pinned by its invariants, by the non-blind models it
must reduce to, by the restoration it achieves on the committed scene and by injected faults on the very inputs the device test
uses; fdr_psf_gaussian against its formula, the new symbols, the struct and the refusals that need no device."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _blind_model as bm
from _rl_model import rel_err, rl_model
from _rlfree_model import rlfree_model

SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def quality():
    """per seed: the plain 128^2 case and the 100^2 crop, 80 iterations from the Gaussian start (and the flat start), float64"""
    q = bm.QUALITY
    g = bm.psf_gaussian(q["psf"])
    flat = np.full((q["psf"], q["psf"]), 1.0 / q["psf"] ** 2, dtype=np.float32)
    out = {}
    for seed in SEEDS:
        truth, d, psf = bm.plain_case(seed)
        img, p = bm.blind_model(d, g, q["S"], q["S"], q["n"])
        _, p_flat = bm.blind_model(d, flat, q["S"], q["S"], q["n"])
        c = q["crop"]
        _, dc, _ = bm.crop_case(seed)
        _, p_free = bm.blind_model(dc, g, c["M"], c["N"], q["n"], free_boundary=True)
        _, p_plain = bm.blind_model(dc, g, c["M"], c["N"], q["n"])
        out[seed] = dict(truth=truth, d=d, psf=psf, g=g, img=img, p=p, p_flat=p_flat, p_free=p_free, p_plain=p_plain)
    return out


@pytest.mark.parametrize("free", (False, True))
def test_psf_stays_a_density_and_zeros_stay_zero(free):
    rows, cols, M, N = (50, 100, 64, 128) if free else (64, 128, 64, 128)
    img = bm.gpu_image(rows, cols, 3)
    p0 = bm.start_psf(9, 9, 4)
    p0[0, :] = p0[-1, :] = p0[:, 0] = p0[:, -1] = 0
    p0 /= p0.sum()
    for n in (1, 5, 20):
        _, p = bm.blind_model(img, p0, M, N, n, free_boundary=free)
        assert p.min() >= 0 and abs(float(p.sum()) - 1) < 1e-12
        assert not p[0, :].any() and not p[-1, :].any() and not p[:, 0].any() and not p[:, -1].any()
        # (the free form starts from a flat image, which says nothing about the PSF: its first PSF step is a rounding error long)
        assert rel_err(p, p0) > (1e-3 if n > 1 or not free else 0), "the PSF did not move"


def test_one_by_one_psf_stays_one_and_gives_rl():
    img = bm.gpu_image(32, 64, 5)
    one = np.ones((1, 1), dtype=np.float32)
    u, p = bm.blind_model(img, one, 32, 64, 7)
    assert p.shape == (1, 1) and p[0, 0] == 1.0
    assert rel_err(u, rl_model(img, one, 32, 64, 7)) < 1e-12


@pytest.mark.parametrize("hold", (6, 9))
def test_held_psf_is_the_non_blind_model(hold):
    p0 = bm.start_psf(5, 7, 2)
    img = bm.gpu_image(64, 64, 6)
    u, p = bm.blind_model(img, p0, 64, 64, 6, psf_hold=hold)
    assert np.array_equal(p, p0.astype(np.float64))
    assert rel_err(u, rl_model(img, p0, 64, 64, 6)) < 1e-12
    win = bm.gpu_image(50, 40, 7)
    w = bm.gpu_mask(50, 40, 8)
    for shape in ((50, 40), (64, 64)):
        u, p = bm.blind_model(win, p0, 64, 64, 6, free_boundary=True, weights=w, psf_hold=hold, out_shape=shape)
        assert np.array_equal(p, p0.astype(np.float64))
        assert rel_err(u, rlfree_model(win, p0, 64, 64, 6, weights=w, out_shape=shape)) < 1e-12


@pytest.mark.parametrize("seed", SEEDS)
def test_plain_form_refines_the_psf_and_restores(quality, seed):
    """128^2 full plane, noise 0.005, 80 iterations, Gaussian start: start correlation < 0.6, final >= 0.9, image >= 4 dB above the
    blurred input (shift-tolerant); the flat start stays below 0.4"""
    q = quality[seed]
    start, final = bm.shift_corr(q["g"], q["psf"]), bm.shift_corr(q["p"], q["psf"])
    gain = bm.shift_psnr(q["img"], q["truth"]) - bm.shift_psnr(q["d"], q["truth"])
    flat = bm.shift_corr(q["p_flat"], q["psf"])
    print("BLIND\tquality plain\tseed=%d\tstart=%.3f\tfinal=%.3f\tgain=%.2f dB\tflat=%.3f" % (seed, start, final, gain, flat))
    assert start < 0.6
    assert final >= 0.9
    assert gain >= 4.0
    assert flat < 0.4


@pytest.mark.parametrize("seed", SEEDS)
def test_free_form_is_the_form_for_a_crop(quality, seed):
    """the 100^2 crop of a 256^2 scene in a 128^2 plan: the free form reaches >= 0.7 and beats the plain form by >= 0.3"""
    q = quality[seed]
    free, plain = bm.shift_corr(q["p_free"], q["psf"]), bm.shift_corr(q["p_plain"], q["psf"])
    print("BLIND\tquality crop\tseed=%d\tfree=%.3f\tplain=%.3f" % (seed, free, plain))
    assert free >= 0.7
    assert free - plain >= 0.3


def _gpu_cases():
    """(name, image, start PSF, M, N, iterations, keywords) of every model comparison of test_blind_gpu.py"""
    for M in bm.COLUMN_M:
        for pr, pc in bm.COLUMN_PSFS:
            yield "col M=%d psf %dx%d" % (M, pr, pc), bm.gpu_image(M, 32, M), bm.start_psf(pr, pc, M + pr), M, 32, bm.COLUMN_N_ITER, {}
    for N in bm.ROW_N:
        yield "row N=%d" % N, bm.gpu_image(16, N, N), bm.start_psf(3, 3, N), 16, N, bm.COLUMN_N_ITER, {}
    for N in (32, 8192):
        for pr, pc in bm.PSF_WINDOWS:
            yield "win N=%d psf %dx%d" % (N, pr, pc), bm.gpu_image(32, N, N + pr), bm.start_psf(pr, pc, pr), 32, N, bm.COLUMN_N_ITER, {}
    for M, N, r, c in bm.FREE_CASES:
        for w in (None, bm.gpu_mask(r, c, 7)):
            for n in bm.FREE_N_ITER:
                yield ("free %dx%d weights=%s n=%d" % (M, N, w is not None, n), bm.gpu_image(r, c, M), bm.start_psf(9, 9, M), M, N, n,
                       dict(free_boundary=True, weights=w))


def test_faults_are_visible_on_the_device_inputs():
    """every fault model differs from the right one, in the image or in the PSF, by at least 10 times the tolerance the device test
    grants on that input.  Left out, because they cannot differ: every fault on a 1 x 1 PSF but the missing renormalisation; the
    missing renormalisation in the free form at 5 iterations (the exact EM step keeps sum(q) within 1e-5 of 1 there by itself; it
    shows at 20 iterations)."""
    weakest = {}
    for name, img, p0, M, N, n, kw in _gpu_cases():
        free = bool(kw.get("free_boundary"))
        u, p = bm.blind_model(img, p0, M, N, n, **kw)
        u32, p32 = bm.blind_model(img, p0, M, N, n, dtype=np.float32, **kw)
        tol_u, tol_p = bm.gpu_tol(rel_err(u32, u)), bm.gpu_tol(rel_err(p32, p))
        for fault in bm.FAULTS:
            if not free and fault in ("no_den", "alpha_fixed"):
                continue
            if p0.size == 1 and fault != "no_renorm":
                continue
            if free and fault == "no_renorm" and n < 20:
                continue
            uf, pf = bm.blind_model(img, p0, M, N, n, fault=fault, **kw)
            ratio = max(rel_err(uf, u) / tol_u, rel_err(pf, p) / tol_p)
            weakest[fault] = min(weakest.get(fault, np.inf), ratio)
            assert ratio >= 10, "%s: fault %s differs by only %.3g tolerances" % (name, fault, ratio)
    print("BLIND\tfaults, weakest separation in tolerances\t" + "\t".join("%s=%.3g" % kv for kv in sorted(weakest.items())))
    assert set(weakest) == set(bm.FAULTS)


def test_float32_replay_stays_close():
    """the iteration is not sensitive to precision: the complex64 replay of the quality case stays within 1e-5 of the model"""
    _, d, _ = bm.plain_case(1)
    g = bm.psf_gaussian(9)
    for n in (5, 80):
        u, p = bm.blind_model(d, g, 128, 128, n)
        u32, p32 = bm.blind_model(d, g, 128, 128, n, dtype=np.float32)
        assert rel_err(u32, u) < 1e-5 and rel_err(p32, p) < 1e-5, (n, rel_err(u32, u), rel_err(p32, p))


def test_shift_corr_tolerates_a_shift():
    p = bm.shake_psf(9)
    assert abs(bm.shift_corr(p, p) - 1) < 1e-12
    assert abs(bm.shift_corr(np.roll(p, (2, -3), axis=(0, 1)), p) - 1) < 1e-12
    assert bm.shift_corr(np.roll(p, (0, 4), axis=(0, 1)), p) < 0.9
    assert bm.shift_corr(np.full((9, 9), 1 / 81.0), p) == 0.0
    for size in (7, 9):
        q = bm.shake_psf(size)
        assert q.shape == (size, size) and q.min() >= 0 and abs(float(q.sum(dtype=np.float64)) - 1) < 1e-6


@pytest.mark.parametrize("size,sigma", ((9, 0.0), (7, 0.0), (1, 0.0), (2, 0.0), (16, 1.3), (256, 40.0)))
def test_psf_gaussian_is_the_formula(fdr, size, sigma):
    got = fdr.psf_gaussian(size, sigma)
    s = size / 4.0 if sigma == 0 else sigma
    c = size // 2
    i, j = np.mgrid[0:size, 0:size].astype(np.float64)
    want = np.exp(-((i - c) ** 2 + (j - c) ** 2) / (2 * s * s))
    want = want / want.sum()
    assert got.dtype == np.float32 and got.shape == (size, size)
    assert np.max(np.abs(got.astype(np.float64) - want)) <= np.max(want) * 2.0 ** -24  # rounded once
    assert np.array_equal(got, bm.psf_gaussian(size, sigma))
    assert np.unravel_index(np.argmax(got), got.shape) == (c, c)


BLIND_FUNCS = ("fdr_richardson_lucy_blind_f32", "fdr_richardson_lucy_blind_f32_dev", "fdr_richardson_lucy_blind_status", "fdr_psf_gaussian",
               "fdr_psf_gaussian_dev")


def test_symbols_and_surface(fdr):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fdr.h")).read()
    assert re.search(r"typedef\s+struct\s+fdr_blind_params\s*\{[^}]*int\s+iterations;[^}]*int\s+free_boundary;[^}]*int\s+psf_hold;[^}]*int\s+norm_area;"
                     r"[^}]*float\s+cov_sigma;[^}]*int\s+out_rows;[^}]*int\s+out_cols;[^}]*\}\s*fdr_blind_params\s*;", header)
    assert re.search(r"#define\s+FDR_BLIND_MAX_PSF\s+65536", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in BLIND_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    assert ctypes.sizeof(fdr.BlindParams) == 28
    assert [f[0] for f in fdr.BlindParams._fields_] == ["iterations", "free_boundary", "psf_hold", "norm_area", "cov_sigma", "out_rows", "out_cols"]
    sig = inspect.signature(fdr.Plan.richardson_lucy_blind).parameters
    assert list(sig)[:4] == ["self", "img", "psf_start", "iterations"]
    assert (sig["free_boundary"].default, sig["weights"].default, sig["psf_hold"].default, sig["norm_area"].default) == (False, None, 0, fdr.NORM_NONE)
    assert callable(fdr.Plan.richardson_lucy_blind_dev) and callable(fdr.Plan.blind_status)
    sig = inspect.signature(fdr.richardsonLucyBlind_myfft).parameters
    assert list(sig)[:6] == ["img", "psf_start", "psf_size", "iterations", "free_boundary", "mask"]
    assert sig["psf_start"].default is None


def test_refusals_that_need_no_device(fdr):
    ERR_ARG = -1
    buf = np.zeros((4, 4), dtype=np.float32)
    prm = fdr.BlindParams(1, 0, 0, fdr.NORM_NONE, 0.01, 0, 0)
    ptr = buf.ctypes.data
    # no plan: refused before anything is looked at
    assert fdr.lib.fdr_richardson_lucy_blind_f32(None, ptr, 4, 4, 4, None, 0, ptr, 3, 3, 3, ptr, 4, ctypes.byref(prm)) == ERR_ARG
    assert b"null argument" in fdr.lib.fdr_last_error()
    assert fdr.lib.fdr_richardson_lucy_blind_f32_dev(None, ptr, 4, 4, 4, None, 0, ptr, 3, 3, 3, ptr, 4, ctypes.byref(prm), None) == ERR_ARG
    assert fdr.lib.fdr_richardson_lucy_blind_status(None, None) == ERR_ARG
    # the Gaussian PSF
    assert fdr.lib.fdr_psf_gaussian(9, 0.0, None) == ERR_ARG
    for size, sigma in ((0, 0.0), (-3, 1.0), (257, 0.0), (9, -1.0), (9, float("nan")), (9, float("inf"))):
        assert fdr.lib.fdr_psf_gaussian(size, sigma, ptr) == ERR_ARG, (size, sigma)
        assert fdr.lib.fdr_psf_gaussian_dev(0, size, sigma, ptr, None) == ERR_ARG, (size, sigma)
    assert not buf.any()
    with pytest.raises(ValueError):
        fdr.richardsonLucyBlind_myfft(buf, mask=buf)
