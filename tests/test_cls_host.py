"""CPU tests of the constrained least-squares (CLS) filter (fdr_set_psf_cls*): the float64 model of tests/_cls_model.py, the
C ABI / Python surface without a GPU, and fault pins for the per-bin checker on the exact GPU cases of test_cls_gpu.py.

lap2 is pinned to |DFT|^2 of the 3 x 3 Laplacian placed anywhere in the plan (wrapping round), and cls_raw(gamma = 0) to
wiener_raw.  A complex64 restatement of the CLS operator must pass BIN_TOL on the GPU cases; the faults a CLS kernel is prone
to -- gamma dropped, |L| for L^2, u and v swapped, the packed Nyquist half given b_v of v = 0, the row frequency off by one (on
columns of up to 16 rows: beyond that a_{u+1} - a_u is too small to resolve) or taken in storage order -- must score more than
5x BIN_TOL there."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _cls_model import LAPLACIAN, SHAPES, cases, cls_raw, lap2
from _spectral import BIN_TOL, bin_error, normalize, tone_image, wiener_raw
from conftest import ROOT

CLS_FUNCS = ("fdr_set_psf_cls", "fdr_set_psf_cls_dev", "fdr_set_psf_motion_cls")


@pytest.mark.parametrize("M", [3, 4, 5, 8, 9, 30, 64])
@pytest.mark.parametrize("N", [3, 4, 5, 8, 9, 30, 64])
def test_lap2_is_the_laplacian_kernel_spectrum(M, N):
    want = lap2(M, N)
    for r0, c0 in ((0, 0), (1, 2), (M - 1, N - 1), (M // 2, 1)):
        k = np.zeros((M, N))
        for i in range(3):
            for j in range(3):
                k[(r0 + i) % M, (c0 + j) % N] += LAPLACIAN[i, j]
        assert np.abs(np.abs(np.fft.fft2(k)) ** 2 - want).max() <= 1e-10 * max(1.0, want.max()), (M, N, r0, c0)


@pytest.mark.parametrize("shape", [(64, 64), (45, 75), (32, 128)])
def test_cls_raw_gamma_zero_is_wiener_raw(oracle, shape):
    M, N = shape
    img = tone_image(M, N, 11)
    psf = oracle.motion_blur_kernel(15, 30.0)
    for K in (1e-4, 1e-2):
        assert np.abs(cls_raw(img, psf, K, 0.0, M, N) - wiener_raw(img, psf, K, M, N)).max() <= 1e-12


def test_header_library_and_python_surface(fdr):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fdr.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in CLS_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    import inspect
    for fn, kw in ((fdr.Plan.set_psf, "gamma"), (fdr.Plan.set_psf_dev, "gamma"), (fdr.Plan.set_psf_motion, "gamma"),
                   (fdr.wienerDeblur_myfft, "cls_gamma"), (fdr.wienerDeblur_myfft_unpadded, "cls_gamma"),
                   (fdr.wienerDeblur_RGB_optimized, "cls_gamma"), (fdr.wienerDeblur_RGB_naive, "cls_gamma")):
        p = inspect.signature(fn).parameters
        assert kw in p and p[kw].default == 0.0, (fn.__name__, kw)
    shim = open(os.path.join(ROOT, "include", "fft", "fft.hpp")).read()
    assert re.search(r"float cls_gamma = 0\.f;", shim)
    assert "--cls" in open(os.path.join(ROOT, "tools", "cli", "gpu.cpp")).read()


def test_null_plan_is_refused_without_a_gpu(fdr):
    L, f = fdr.lib, ctypes.c_float
    psf = np.ones((3, 3), dtype=np.float32)
    assert L.fdr_set_psf_cls(None, psf.ctypes.data, 3, 3, 3, f(0.01), f(0.5)) == -1
    assert b"null argument" in L.fdr_last_error()
    assert L.fdr_set_psf_cls_dev(None, None, 3, 3, 3, f(0.01), f(0.5), None) == -1
    assert L.fdr_set_psf_motion_cls(None, 15, 30.0, f(0.01), f(0.5), None) == -1


# ---- fault pins on the GPU cases ------------------------------------------------------------------------------------------
def _planes(img, psf, M, N):
    f = np.zeros((M, N))
    f[:img.shape[0], :img.shape[1]] = img
    h = np.zeros((M, N))
    h[:psf.shape[0], :psf.shape[1]] = psf
    return np.fft.fft2(f), np.fft.fft2(h)


def _out(G, W):
    return normalize(np.real(np.fft.ifft2(G * W))).astype(np.float32)


def _operator_c64(img, psf, K, gamma, M, N):
    """the CLS operator in single precision throughout (numpy transforms complex64 natively)"""
    f = np.zeros((M, N), dtype=np.complex64)
    f[:img.shape[0], :img.shape[1]] = img
    h = np.zeros((M, N), dtype=np.complex64)
    h[:psf.shape[0], :psf.shape[1]] = psf
    H = np.fft.fft2(h)
    den = np.abs(H) ** 2 + np.float32(K) + np.float32(gamma) * lap2(M, N).astype(np.float32)
    raw = np.real(np.fft.ifft2(np.fft.fft2(f) * (np.conj(H) / den)))
    lo, hi = raw.min(), raw.max()
    return ((raw - lo) / (hi - lo)).astype(np.float32)


def _faulty_filters(H, K, gamma, M, N):
    """name -> W with one CLS fault, full M x N plane"""
    a = 4.0 * np.sin(np.pi * np.arange(M) / M) ** 2
    b = 4.0 * np.sin(np.pi * np.arange(N) / N) ** 2
    L = a[:, None] + b[None, :]
    def q(reg):
        with np.errstate(divide="ignore", invalid="ignore"):
            den = np.abs(H) ** 2 + K + gamma * reg
            return np.where(den != 0, np.conj(H) / den, 0)
    out = {"gamma dropped": q(0.0), "|L| for L^2": q(L)}
    if M != N:
        # u and v swapped: a taken at the column frequency, b at the row frequency (the tables' roles exchanged)
        a_v = 4.0 * np.sin(np.pi * np.arange(N) / M) ** 2
        b_u = 4.0 * np.sin(np.pi * np.arange(M) / N) ** 2
        out["u and v swapped"] = q((b_u[:, None] + a_v[None, :]) ** 2)
    if N >= 32:
        # the packed column's Nyquist half (v = N/2) given b_0 = 0 instead of b_{N/2} = 4
        Ln = L.copy()
        Ln[:, N // 2] = a
        out["Nyquist column with b_0"] = q(Ln ** 2)
    if M <= 16:
        # a_{u+1} - a_u is O(1 / M): only on short columns does an off-by-one row frequency move the filter beyond what the
        # per-bin check resolves
        ap = 4.0 * np.sin(np.pi * ((np.arange(M) + 1) % M) / M) ** 2
        out["row frequency + 1"] = q((ap[:, None] + b[None, :]) ** 2)
    if M >= 4 and M & (M - 1) == 0:
        # a value's memory position (bit-reversed order) taken as its row frequency instead of Core::out_index
        bits = M.bit_length() - 1
        rev = np.array([int(format(u, "0%db" % bits)[::-1], 2) for u in range(M)])
        out["row frequency in storage order"] = q((a[rev][:, None] + b[None, :]) ** 2)
    return out


PIN_SHAPES = [(M, N, fl) for M, N, fl in SHAPES if M * N <= 1 << 18]


@pytest.mark.parametrize("M,N,flag", PIN_SHAPES)
def test_fault_pins_on_the_gpu_cases(oracle, M, N, flag):
    """On every (K, gamma, PSF) case of the GPU test at this shape: the complex64 operator passes BIN_TOL and every fault
    scores above 5x BIN_TOL (the faults are judged on the cases where they move the filter: a PSF whose faulty quotient equals
    the right one to 1e-9 everywhere is skipped for that fault)."""
    img = tone_image(M, N, M * 7919 + N)
    bad = []
    for name, psf, K, gamma in cases(oracle, M, N):
        raw = cls_raw(img, psf, K, gamma, M, N)
        what = "%dx%d %s K=%g gamma=%g" % (M, N, name, K, gamma)
        e, _ = bin_error(_operator_c64(img, psf, K, gamma, M, N), raw)
        if not e <= BIN_TOL:
            bad.append("%s: complex64 operator %.3g > BIN_TOL" % (what, e))
        G, H = _planes(img, psf, M, N)
        right = np.conj(H) / (np.abs(H) ** 2 + K + gamma * lap2(M, N))
        for fault, W in _faulty_filters(H, K, gamma, M, N).items():
            if np.abs(W - right).max() <= 1e-9 * np.abs(right).max():
                continue
            e, _ = bin_error(_out(G, W), raw)
            if not e > 5 * BIN_TOL:
                bad.append("%s: fault '%s' scores %.3g <= 5 x BIN_TOL" % (what, fault, e))
    assert not bad, "\n".join(bad[:20])
