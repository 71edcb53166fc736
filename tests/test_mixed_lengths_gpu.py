"""Every length and layout of FDR_FLAG_MIXED_RADIX on the MI355X.

All 167 lengths L = 2^a 3^b 5^c up to 8192 run as a row length (plan (45, L)) and as a column length (plans (L, 12), (L, 6),
(L, 15): panel widths 4, 2 and 1 where the plan's limits allow), with the layout (logP, B) of each plan taken from
tools/cli/mixed_plan_check and plans whose (L, role, logP, B) repeats dropped (_mixed_model.sweep_cases: 593 plans, all 15
(logP, B) pairs; test_mixed_plan_host.py asserts that reach).

  a. complex transforms (MIX_ROWS_C2C, MIX_COLS_C2C) against numpy's complex128 fft2 / ifft2, judged per line: the relative
     L2 error of every single row and column (LINE_TOL) and the largest |got - want| over rms(want) (PEAK_TOL), so that one
     wrong transform of a B-group or one wrong column of a panel cannot hide in a whole-plane norm.
  b. the operator (MIX_ROWS_FWD_REAL, MIX_COLS_FILTER, MIX_COLS_FUSED, MIX_ROWS_INV_REAL) on the same plans with both sides
     >= 5: full-plane tone image, motion PSF 15/30 (5/30 below 15), K = 1e-2 and 1e-4, bin by bin (_spectral.bin_error) and
     max-abs against the float64 model at BIN_TOL / SPATIAL_TOL.
  c. odd windows with strides of their own on plans of every B and P, both normalisation areas, the poison around the
     window intact; and a smaller window after a full-plane call equals the same call on a fresh plan bit for bit (the
     spectrum rows a call does not write are stale by design and must not be read).
  d. the CLS filter on panel widths 1, 2 and 4, odd and even M, bin by bin against _cls_model.cls_raw; gamma = 0 is the
     Wiener call byte for byte.

Each plan prints a `MIXLEN` (a) or `MIXOP` (b) line with its measured values (pytest -s).  LINE_TOL and PEAK_TOL in
_mixed_model.py are at most 4x the largest values of one such run on an MI355X:
  line 7.5e-7 at L = 1 (plan (45, 1), forward: its rows are single elements, so this is one element's relative error);
       over the lengths above 5, 5.8e-7 at L = 1000 (plan (1000, 6), inverse, a row of six elements); the plans (45, L) with
       L >= 64, whose worst lines are columns of 45 elements, stay at or below 3.1e-7 ((45, 7776), forward), about twice
       the 1.6e-7 of a float32 restatement of one transform's stages (each element passes through two transforms);
  peak 9.0e-7 of rms at L = 3888 (plan (3888, 15), inverse), 8.5e-7 at L = 1800 as a row length.
No length stands out from its neighbours in either figure.  The same run measured, against thresholds that were there
before (BIN_TOL 8e-4, SPATIAL_TOL 2e-5): operator per-bin 1.5e-4 ((4320, 12), K = 1e-4) and max-abs 3.6e-6 ((75, 12)); windows
max-abs 3.0e-7; CLS per-bin 9.2e-5 and max-abs 6.2e-7 (both (5000, 60))."""
import ctypes

import numpy as np
import pytest

import _mixed_model as mm
from _cls_model import cases, cls_raw, motion_psf
from _mixed_model import wiener_model, wiener_raw
from _spectral import BIN_TOL, SPATIAL_TOL, bin_error, failures, max_abs, normalize, tone_image

pytestmark = pytest.mark.gpu

# (role, partner, band of lengths): (L, 6) adds a plan only where (L, 12) has P = 4 (L <= 2496), (L, 15) only where one of
# them has P > 1 (L <= 4992); each id asserts that it has plans, so a changed limit shows here
IDS = [(role, n, b) for role, n in mm.ROLES for b, Ls in enumerate(mm.bands())
       if role == "row" or n == 12 or Ls[0] <= (2496 if n == 6 else 4992)]


def _plan(fdr, M, N):
    return fdr.Plan(M, N, fdr.MODE_FAST, 0, flags=fdr.FLAG_MIXED_RADIX)


def _cases(role, partner, band):
    Ls = set(mm.bands()[band])
    cs = [c for c in mm.sweep_cases() if c["role"] == role and c["partner"] == partner and c["L"] in Ls]
    assert cs, "no plan left for this id: the limits in IDS are stale"
    return cs


@pytest.mark.parametrize("role,partner,band", IDS)
def test_c2c_every_length_per_line(fdr, role, partner, band):
    bad = []
    for c in _cases(role, partner, band):
        M, N = c["M"], c["N"]
        rng = np.random.default_rng(M * 8209 + N)
        x = (rng.standard_normal((M, N)) + 1j * rng.standard_normal((M, N))).astype(np.complex64)
        with _plan(fdr, M, N) as p:
            fwd = p.fft2d(x)
            inv = p.fft2d(x, inverse=True)
        x128 = x.astype(np.complex128)
        for name, got, want in (("fwd", fwd, np.fft.fft2(x128)), ("inv", inv, np.fft.ifft2(x128) * (M * N))):
            line, peak, where = mm.line_errors(got, want)
            what = "%s L=%d %dx%d %s logP=%d B=%d" % (role, c["L"], M, N, name, c["logP"], c["B"])
            print("MIXLEN\t%s\tline=%.3g\tat=%s\tpeak=%.3g" % (what, line, where, peak))
            if not line <= mm.LINE_TOL:
                bad.append("%s: relative error %.3g > %.3g in %s" % (what, line, mm.LINE_TOL, where))
            if not peak <= mm.PEAK_TOL:
                bad.append("%s: largest error %.3g > %.3g of rms" % (what, peak, mm.PEAK_TOL))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("role,partner,band", IDS)
def test_operator_every_length_per_bin(fdr, oracle, role, partner, band):
    bad = []
    for c in _cases(role, partner, band):
        M, N = c["M"], c["N"]
        if min(M, N) < 5:
            continue
        img = tone_image(M, N, M * 7919 + N)
        psf = motion_psf(oracle, 15 if min(M, N) >= 15 else 5, 30.0, M, N)
        with _plan(fdr, M, N) as p:
            for K in (1e-2, 1e-4):
                K32 = float(np.float32(K))
                p.set_psf(psf, K32)
                got = p.wiener(img, fdr.NORM_PADDED)
                raw = wiener_raw(img, psf, K32, M, N)
                e, where = bin_error(got, raw)
                sp = max_abs(got, normalize(raw))
                what = "%s L=%d %dx%d logP=%d B=%d K=%g" % (role, c["L"], M, N, c["logP"], c["B"], K)
                print("MIXOP\t%s\tbin=%.3g\tat=%s\tspatial=%.3g" % (what, e, where, sp))
                bad += failures(what, M, N, e, where, sp, BIN_TOL, SPATIAL_TOL)
    assert not bad, "\n".join(bad)


def _odd_below(n):
    return n - 3 if (n - 3) % 2 else n - 4


def _window_call(fdr, p, img, norm):
    """wiener_dev on a window with strides of its own into a poisoned buffer two rows taller: the window, after checking that
    everything around it still holds the poison"""
    import torch
    rows, cols = img.shape
    stride, ostride = cols + 7, cols + 13
    big = np.zeros((rows, stride), dtype=np.float32)
    big[:, :cols] = img
    d_in = torch.from_numpy(big).cuda()
    d_out = torch.full((rows + 2, ostride), -7.0, dtype=torch.float32, device="cuda")
    p.wiener_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), ostride, norm)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[:rows, cols:] == -7.0) and np.all(out[rows:] == -7.0), "output written outside the window"
    return out[:rows, :cols]


@pytest.mark.parametrize("M,N", mm.WINDOW_PLANS)
def test_windows_strides_and_stale_spectra(fdr, oracle, M, N):
    logP, B = mm.plan_dump(tuple(mm.WINDOW_PLANS + mm.CLS_PLANS))[1][(M, N)][:2]
    rows, cols = _odd_below(M), _odd_below(N)
    assert rows % 2 == 1 and cols % 2 == 1 and rows % (2 * B) != 0
    img = tone_image(M, N, rows * 31 + cols, rows=rows, cols=cols)
    small = np.ascontiguousarray(img[:_odd_below(M // 2), :_odd_below(N // 2)])
    full = tone_image(M, N, M * 104729 + N)
    psf = oracle.motion_blur_kernel(15, 30.0)
    K32 = float(np.float32(0.01))
    norms = (fdr.NORM_CROPPED, fdr.NORM_PADDED)
    bad = []
    with _plan(fdr, M, N) as p:
        p.set_psf(psf, K32)
        for norm in norms:
            got = _window_call(fdr, p, img, norm)
            sp = max_abs(got, wiener_model(img, psf, K32, M, N, norm_cropped=norm == fdr.NORM_CROPPED))
            what = "%dx%d in %dx%d logP=%d B=%d norm=%d" % (rows, cols, M, N, logP, B, norm)
            print("MIXWIN\t%s\tspatial=%.3g" % (what, sp))
            bad += failures(what, M, N, None, None, sp, BIN_TOL, SPATIAL_TOL)
        # every spectrum row written once, then a window that writes and reads fewer of them
        p.wiener(full, fdr.NORM_PADDED)
        after_full = [_window_call(fdr, p, small, norm) for norm in norms]
    with _plan(fdr, M, N) as q:
        q.set_psf(psf, K32)
        fresh = [_window_call(fdr, q, small, norm) for norm in norms]
    for norm, a, b in zip(norms, after_full, fresh):
        if not np.array_equal(a, b):
            bad.append("%dx%d in %dx%d norm=%d: differs after a full-plane call (max %.3g): stale spectrum rows were read"
                       % (small.shape + (M, N, norm, max_abs(a, b))))
    assert not bad, "\n".join(bad)


def _filter_bytes(p):
    import torch
    n = p.filter_bytes()
    d = torch.empty(n, dtype=torch.uint8, device="cuda")
    p.export_filter_dev(d.data_ptr(), n)
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("M,N", mm.CLS_PLANS)
def test_cls_on_every_panel_width(fdr, oracle, M, N):
    logP = mm.plan_dump(tuple(mm.WINDOW_PLANS + mm.CLS_PLANS))[1][(M, N)][0]
    img = tone_image(M, N, M * 7919 + N)
    bad = []
    with _plan(fdr, M, N) as p:
        for name, psf, K, gamma in cases(oracle, M, N):
            K32, g32 = float(np.float32(K)), float(np.float32(gamma))
            p.set_psf(psf, K32, gamma=g32)
            got = p.wiener(img, fdr.NORM_PADDED)
            raw = cls_raw(img, psf, K32, g32, M, N)
            e, where = bin_error(got, raw)
            sp = max_abs(got, normalize(raw))
            what = "%dx%d logP=%d %s K=%g gamma=%g" % (M, N, logP, name, K, gamma)
            print("MIXCLS\t%s\tbin=%.3g\tat=%s\tspatial=%.3g" % (what, e, where, sp))
            bad += failures(what, M, N, e, where, sp, BIN_TOL, SPATIAL_TOL)
        # gamma = 0 through the CLS entry point: the filter bytes and the output of the Wiener call
        psf = np.ascontiguousarray(motion_psf(oracle, 15, 30.0, M, N), dtype=np.float32)
        K32 = float(np.float32(0.01))
        p.set_psf(psf, K32)
        fw, ow = _filter_bytes(p), p.wiener(img)
        rc = fdr.lib.fdr_set_psf_cls(p._h, psf.ctypes.data, psf.shape[0], psf.shape[1], psf.shape[1], ctypes.c_float(K32), ctypes.c_float(0.0))
        assert rc == 0, fdr.lib.fdr_last_error()
        fc, oc = _filter_bytes(p), p.wiener(img)
        if not (np.array_equal(fw, fc) and np.array_equal(ow, oc)):
            bad.append("%dx%d: gamma = 0 is not the Wiener call" % (M, N))
    assert not bad, "\n".join(bad)
