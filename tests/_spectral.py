"""float64 reference of the Wiener operator's raw plane and a per-bin spectral checker for the fast paths.

A full-plane image (rows = M, cols = N) restored with NORM_PADDED comes back as an affine map of the raw plane
(min-max normalisation).  bin_error() fits that map, takes the residual back to the frequency domain and scores every bin
against the spectrum of the raw plane, so an error confined to one bin, one Hermitian pair or one spectral row stands out
instead of vanishing under a max-abs on the normalised output.  DC is not scored: min-max normalisation removes a DC error
exactly, so the output cannot show one.  Pinned against the CPU oracle and against injected faults in
test_spectral_host.py before it judges the GPU (test_fast_spectral_gpu.py)."""
import numpy as np

from _mixed_model import wiener_raw  # noqa: F401  (re-exported: the reference raw plane)

# Thresholds from one run of test_fast_spectral_gpu.py on an MI355X, at most 4x the largest value measured there.
# BIN_TOL bounds bin_error(), SPATIAL_TOL max-abs against the normalised model.  Measured over every shape, K, delta and
# the motion and zero-mean dense PSFs: bin_error 2.8e-4 (2048 x 8192, motion 50/123.4, K = 1), max-abs 5.5e-6 (same shape
# and PSF, K = 1e-4).  The single-precision numpy operator stays below BIN_TOL and every injected 1 % fault scores more
# than 5x above it (test_spectral_host.py).
BIN_TOL = 8e-4
SPATIAL_TOL = 2e-5
# A non-negative dense PSF puts nearly all of its energy into H(0, 0), and the fast transforms then leave the other bins of
# column 0 with an error that grows with |H(0, 0)|; where |H|^2 is near K the filter there is off by up to 0.5 %.
# Measured: bin_error 4.6e-3 (column 0 of 2048 x 8192, K = 1e-4), max-abs 6.8e-5 (8192 x 2048 and 8 x 8192), against
# 1.2e-4 and 7.6e-6 for numpy's complex64 FFT on the same inputs (about 38x).  Shifting the same PSF to zero mean brings
# the plans under the thresholds above; the full spectrum and a DC-free image do not change it, so the Nyquist packing and
# the image's own DC are not the cause.  These thresholds are above what a 1 % fault in one bin can score (e <= 0.01), so
# the non-negative dense case is a smoke check of that regime only: the faults are caught by the motion and zero-mean
# dense PSFs, which run on the same plans at BIN_TOL / SPATIAL_TOL.
DC_BIN_TOL = 1.5e-2
DC_SPATIAL_TOL = 2.5e-4


def edge_bins(n):
    """The frequencies where the fast kernels special-case or pack: 0, 1, n/2 - 1, n/2, n/2 + 1, n - 1 (mod n, unique)."""
    h = n // 2
    return sorted({b % n for b in (0, 1, h - 1, h, h + 1, n - 1)})


def tone_image(M, N, seed, rows=None, cols=None, amp=0.25):
    """float32 rows x cols: uniform noise in [0, 1) plus cosines of amplitude `amp` and random phase at every bin of
    edge_bins(M) x edge_bins(N) of the M x N plan, so that each of those bins (and its conjugate) carries far more energy
    than a bin of the noise and a fault there is well above the arithmetic's own error."""
    rows = M if rows is None else rows
    cols = N if cols is None else cols
    rng = np.random.default_rng(seed)
    img = rng.random((rows, cols))
    ks, ls = edge_bins(M), edge_bins(N)
    # sum over k, l of amp cos(2 pi (k r / M + l c / N) + phi_kl) = Re(Er . C . Ec), separable in r and c
    C = amp * np.exp(1j * rng.uniform(0, 2 * np.pi, (len(ks), len(ls))))
    Er = np.exp(2j * np.pi * np.outer(np.arange(rows), ks) / M)
    Ec = np.exp(2j * np.pi * np.outer(ls, np.arange(cols)) / N)
    img += np.real(Er @ (C @ Ec))
    return img.astype(np.float32)


def normalize(a):
    """min-max to [0, 1] in float64 (the operator's last step)"""
    a = np.asarray(a, dtype=np.float64)
    lo, hi = a.min(), a.max()
    return (a - lo) / (hi - lo)


def describe_bin(k, l, M, N):
    where = []
    if k == 0:
        where.append("row 0")
    if M % 2 == 0 and k == M // 2:
        where.append("row M/2")
    if l == 0:
        where.append("column 0")
    if N % 2 == 0 and l == N // 2:
        where.append("column N/2")
    return "bin (%d, %d) of %d x %d%s" % (k, l, M, N, " [%s]" % ", ".join(where) if where else "")


def bin_error(got, raw):
    """Per-bin error of `got` (the restored full plane) against the float64 raw plane `raw`.

    Fits got ~ a * raw + b by least squares, r = (got - a raw - b) / a, and returns (e, (k, l)) with
    e = max over non-DC bins of |R[k, l]| / (|Y[k, l]| + rms |Y|), R = fft2(r), Y = fft2(raw), rms over the non-DC bins.
    r and raw are real, so the half spectrum l <= N/2 holds every value of |R| and |Y|; (k, l) is the bin in that half.
    An output holding NaN or inf, or a flat one (a = 0), scores NaN."""
    got = np.asarray(got, dtype=np.float64)
    raw = np.asarray(raw, dtype=np.float64)
    assert got.shape == raw.shape
    M, N = raw.shape
    if not np.all(np.isfinite(got)):  # NaN / inf in the output: no fit, a NaN score (which fails every threshold)
        return float("nan"), (0, 0)
    rc = raw - raw.mean()
    a = float(np.sum(rc * (got - got.mean())) / np.sum(rc * rc))
    b = float(got.mean() - a * raw.mean())
    with np.errstate(divide="ignore", invalid="ignore"):  # a flat output (a = 0) scores inf / NaN: a failure
        R = np.abs(np.fft.rfft2((got - a * raw - b) / a))
    Y = np.abs(np.fft.rfft2(raw))
    P = M * N
    # Parseval: sum over the full spectrum of |Y|^2 = P * sum raw^2, minus the DC bin
    rms = np.sqrt(max(P * np.sum(raw * raw) - np.sum(raw) ** 2, 0.0) / (P - 1))
    e = R / (Y + rms)
    if not np.all(np.isfinite(e)):
        return float("nan"), (0, 0)
    e[0, 0] = 0.0
    k, l = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[k, l]), (int(k), int(l))


def failures(what, M, N, e, where, sp, bin_tol, sp_tol):
    """Failure messages of one case (an empty list: it passed).  e / where: bin_error(), or e = None when only the
    spatial error is judged; sp: max-abs against the reference.  Written as `not value <= tol`, so NaN fails."""
    bad = []
    if e is not None and not e <= bin_tol:
        at = describe_bin(where[0], where[1], M, N) if np.isfinite(e) else "(output not finite, or flat)"
        bad.append("%s: per-bin error %.3g > %.3g at %s" % (what, e, bin_tol, at))
    if not sp <= sp_tol:
        bad.append("%s: max-abs %.3g > %.3g against the reference" % (what, sp, sp_tol))
    return bad


def max_abs(got, want):
    """max |got - want| in float64; NaN when either holds a NaN (np.max propagates it)"""
    d = np.atleast_1d(np.subtract(got, want, dtype=np.float64))  # both sides cast to float64 first; one temporary (the windows reach 2^20 pixels)
    return float(np.max(np.abs(d, out=d)))


def check_bins(got, raw, tol, what=""):
    """Asserts bin_error(got, raw) <= tol; the message names the worst bin and the spectral edge it lies on."""
    e, (k, l) = bin_error(got, raw)
    M, N = np.shape(raw)
    assert e <= tol, "%s: per-bin error %.3g > %.3g at %s" % (what, e, tol, describe_bin(k, l, M, N))
    return e


def delta_psf(r0, c0):
    """(r0 + 1) x (c0 + 1) float32 PSF, one at (r0, c0), zero elsewhere."""
    h = np.zeros((r0 + 1, c0 + 1), dtype=np.float32)
    h[r0, c0] = 1.0
    return h


def delta_raw(img, r0, c0, K):
    """The raw plane for the PSF delta_psf(r0, c0) and a full-plane image, without an FFT: H = exp(-2 pi i (k r0 / M +
    l c0 / N)) has |H| = 1, so W = conj(H) / (1 + K) shifts the image back by (r0, c0) circularly:
    out[r, c] = img[(r + r0) mod M, (c + c0) mod N] / (1 + K)."""
    return np.roll(np.asarray(img, dtype=np.float64), (-r0, -c0), axis=(0, 1)) / (1.0 + K)
