"""The fast Wiener operator (FDR_MODE_FAST) on the MI355X, bin by bin against the float64 model of tests/_spectral.py.

Full-plane images (rows = M, cols = N) restored with NORM_PADDED: the per-bin check (bin_error) and max-abs against the
normalised float64 model, over K in {1e-4, 1e-2, 1} and four PSFs (motion 15 / 30 deg, motion 50 / 123.4 deg, random
dense PSFs the size of the plan, zero-mean and non-negative).  The shapes put every row and column length from 2^3 to
2^13 through the fast kernels (rows4, the split / fused16 / persistent radix-8 column passes, half and full spectrum),
plus the benchmark size, the simple path, the long-row path and the mixed-radix plans, odd lengths included.  A delta
PSF has an exact answer without any transform (the shifted input); cropped images with strides are checked spatially
against the model.  Every case is judged by _spectral.failures(), which fails on NaN and inf as well.  Each case prints a `SPECTRAL` line with its measured values (pytest -s); the thresholds in _spectral.py come from those."""
import numpy as np
import pytest

from _mixed_model import wiener_model
from _spectral import (BIN_TOL, DC_BIN_TOL, DC_SPATIAL_TOL, SPATIAL_TOL, bin_error, delta_psf, delta_raw, failures, max_abs,
                       normalize, tone_image, wiener_raw)

pytestmark = pytest.mark.gpu

KS = (1e-4, 1e-2, 1.0)

# every row / column length 2^3 .. 2^13, M != N.  One image's column pass (launch_cols_panel) is the persistent radix-8
# kernel at LOGM 3..7, the split kernel at LOGM 8..11 and fused16 at LOGM 12..13; the half spectrum (Nyquist column packed
# into column 0) from N = 32
POW2_SHAPES = [(8, 8192), (16, 4096), (32, 2048), (64, 1024), (128, 512), (256, 256), (512, 128), (1024, 64), (2048, 32),
               (4096, 16), (8192, 8), (1024, 1024), (4096, 4096), (2048, 8192), (8192, 2048)]
SIMPLE_SHAPES = [(4, 64), (64, 4)]            # a dimension below 8: the reference-shaped simple path
LONG_SHAPES = [(16384, 64), (64, 16384)]      # a dimension above 8192: the long row pass
FULL_SPECTRUM_SHAPES = [(256, 256), (64, 1024)]
MIXED_SHAPES = [(45, 75), (75, 64), (125, 243), (2187, 40), (3125, 36), (40, 3125), (4320, 4320)]


def _log(cls, what, e, where, spatial):
    print("SPECTRAL\t%s\t%s\tbin=%.3g\tat=%s\tspatial=%.3g" % (cls, what, e, where, spatial))


def _fit(psf, M, N):
    """A PSF larger than the plan is cut to its central min(M) x min(N) window and renormalised (fdr_set_psf refuses a PSF
    larger than the padded image)."""
    r, c = psf.shape
    if r <= M and c <= N:
        return psf
    r0, c0 = (r - min(r, M)) // 2, (c - min(c, N)) // 2
    h = psf[r0:r0 + min(r, M), c0:c0 + min(c, N)].astype(np.float64)
    return (h / h.sum()).astype(np.float32)


def _motion_psfs(oracle, M, N):
    """(name, PSF): the motion PSFs, summing to 1"""
    return [("motion 15/30", _fit(oracle.motion_blur_kernel(15, 30.0), M, N)),
            ("motion 50/123.4", _fit(oracle.motion_blur_kernel(50, 123.4), M, N))]


def _psfs(oracle, M, N, seed):
    """(name, PSF, per-bin threshold, spatial threshold).  The dense PSFs are uniform noise / sqrt(M N), so that their
    non-DC bins have |H| ~ 0.3, where K decides the quotient: one shifted to zero mean, one non-negative, whose large
    H(0, 0) costs column 0 the accuracy described at DC_BIN_TOL (a smoke check only, see there)."""
    dense = np.random.default_rng(seed).random((M, N)) / np.sqrt(M * N)
    return [(name, psf, BIN_TOL, SPATIAL_TOL) for name, psf in _motion_psfs(oracle, M, N)] + [
        ("dense zero-mean", (dense - dense.mean()).astype(np.float32), BIN_TOL, SPATIAL_TOL),
        ("dense non-negative", dense.astype(np.float32), DC_BIN_TOL, DC_SPATIAL_TOL)]


def _sweep(fdr, oracle, cls, M, N, flags):
    """Every PSF x K on one full-plane tone image: per-bin check and max-abs against the model, all failures reported."""
    img = tone_image(M, N, M * 7919 + N)
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        for name, psf, bin_tol, sp_tol in _psfs(oracle, M, N, M + 31 * N):
            for K in KS:
                K32 = float(np.float32(K))
                p.set_psf(psf, K32)
                got = p.wiener(img, fdr.NORM_PADDED)
                raw = wiener_raw(img, psf, K32, M, N)
                e, where = bin_error(got, raw)
                sp = max_abs(got, normalize(raw))
                what = "%dx%d %s K=%g" % (M, N, name, K)
                _log(cls, what, e, where, sp)
                bad += failures(what, M, N, e, where, sp, bin_tol, sp_tol)
    assert not bad, "\n".join(bad)


def _deltas(fdr, cls, M, N, flags):
    """delta PSFs at (0, 0), (1, 1), (M/2, N/2) and (M-1, N-1): the output is the normalised input shifted back by the delta's
    position, computed without a transform (delta_raw)."""
    img = tone_image(M, N, M * 104729 + N)
    K = float(np.float32(0.01))
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        for r0, c0 in ((0, 0), (1 % M, 1 % N), (M // 2, N // 2), (M - 1, N - 1)):
            p.set_psf(delta_psf(r0, c0), K)
            got = p.wiener(img, fdr.NORM_PADDED)
            raw = delta_raw(img, r0, c0, K)
            e, where = bin_error(got, raw)
            sp = max_abs(got, normalize(raw))
            what = "%dx%d delta at (%d, %d)" % (M, N, r0, c0)
            _log(cls + " delta", what, e, where, sp)
            bad += failures(what, M, N, e, where, sp, BIN_TOL, SPATIAL_TOL)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", POW2_SHAPES + SIMPLE_SHAPES + LONG_SHAPES)
def test_pow2_bins_against_float64(fdr, oracle, shape):
    _sweep(fdr, oracle, "pow2", shape[0], shape[1], 0)


@pytest.mark.parametrize("shape", FULL_SPECTRUM_SHAPES)
def test_full_spectrum_bins_against_float64(fdr, oracle, shape):
    _sweep(fdr, oracle, "full", shape[0], shape[1], fdr.FLAG_FULL_SPECTRUM)


@pytest.mark.parametrize("shape", MIXED_SHAPES)
def test_mixed_radix_bins_against_float64(fdr, oracle, shape):
    _sweep(fdr, oracle, "mixed", shape[0], shape[1], fdr.FLAG_MIXED_RADIX)


@pytest.mark.parametrize("shape", POW2_SHAPES + SIMPLE_SHAPES + LONG_SHAPES)
def test_pow2_delta_psf_shifts_the_input(fdr, shape):
    _deltas(fdr, "pow2", shape[0], shape[1], 0)


@pytest.mark.parametrize("shape", FULL_SPECTRUM_SHAPES)
def test_full_spectrum_delta_psf_shifts_the_input(fdr, shape):
    _deltas(fdr, "full", shape[0], shape[1], fdr.FLAG_FULL_SPECTRUM)


@pytest.mark.parametrize("shape", MIXED_SHAPES)
def test_mixed_radix_delta_psf_shifts_the_input(fdr, shape):
    _deltas(fdr, "mixed", shape[0], shape[1], fdr.FLAG_MIXED_RADIX)


# plan M x N, image rows x cols (odd, smaller than the plan), flags
CROPPED = [(256, 512, 201, 375, 0), (1024, 64, 999, 33, 0), (64, 1024, 37, 1001, 0), (8, 8192, 7, 8191, 0),
           (8192, 8, 8191, 5, 0), (4096, 4096, 4001, 3999, 0), (4, 64, 3, 45, 0), (64, 4, 45, 3, 0), (16384, 64, 9001, 61, 0),
           (256, 512, 201, 375, "FLAG_FULL_SPECTRUM"), (45, 75, 43, 71, "FLAG_MIXED_RADIX"),
           (2187, 40, 2001, 39, "FLAG_MIXED_RADIX")]


@pytest.mark.parametrize("M,N,rows,cols,flag", CROPPED)
def test_cropped_strided_against_float64(fdr, oracle, M, N, rows, cols, flag):
    """Odd rows < M and cols < N, input and output rows with a stride of their own, both normalisation areas: spatially
    against the float64 model; the output's stride padding is left untouched."""
    import torch
    flags = getattr(fdr, flag) if flag else 0
    stride, ostride = cols + 7, cols + 13
    img = tone_image(M, N, rows * 31 + cols, rows=rows, cols=cols)
    big = np.zeros((rows, stride), dtype=np.float32)
    big[:, :cols] = img
    d_in = torch.from_numpy(big).cuda()
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        for name, psf in _motion_psfs(oracle, M, N):
            for K in (1e-4, 1e-2):
                K32 = float(np.float32(K))
                p.set_psf(psf, K32)
                for norm in (fdr.NORM_CROPPED, fdr.NORM_PADDED):
                    d_out = torch.full((rows, ostride), -7.0, dtype=torch.float32, device="cuda")
                    p.wiener_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), ostride, norm)
                    torch.cuda.synchronize()
                    out = d_out.cpu().numpy()
                    assert np.all(out[:, cols:] == -7.0)
                    want = wiener_model(img, psf, K32, M, N, norm_cropped=norm == fdr.NORM_CROPPED)
                    sp = max_abs(out[:, :cols], want)
                    what = "%dx%d in %dx%d %s K=%g norm=%d" % (rows, cols, M, N, name, K, norm)
                    _log("crop", what, float("nan"), "-", sp)
                    bad += failures(what, M, N, None, None, sp, BIN_TOL, SPATIAL_TOL)
    assert not bad, "\n".join(bad)
