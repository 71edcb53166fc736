"""CPU tests of the per-bin checker of tests/_spectral.py, which judges the fast operator in test_fast_spectral_gpu.py.

A complex64 restatement of the operator (numpy, single precision throughout) must pass the GPU thresholds; faults of the
kinds the fast kernels are prone to -- one Hermitian pair 1 % off at the spectral edges, a conjugated pair, the Nyquist row
or column 1 % off, K 1 % off -- injected into the float64 model's filtered spectrum must fail them by at least 5x.  Most of
those faults move the normalised output by less than 1e-4, the tolerance of the older fast-mode tests.  A DC shift and an
overall scale are invisible after min-max normalisation and must not be flagged.  The float64 model itself is pinned to the
CPU oracle, and the delta-PSF identities the GPU tests rely on are pinned in it."""
import numpy as np
import pytest

from _spectral import (BIN_TOL, SPATIAL_TOL, bin_error, check_bins, delta_psf, delta_raw, edge_bins, failures, max_abs,
                       normalize, tone_image, wiener_raw)


def _operator_c64(img, psf, K, M, N):
    """The whole operator in single precision (numpy transforms float32 / complex64 natively): the error a correct
    float32 implementation is expected to have."""
    f = np.zeros((M, N), dtype=np.complex64)
    f[:img.shape[0], :img.shape[1]] = img
    h = np.zeros((M, N), dtype=np.complex64)
    h[:psf.shape[0], :psf.shape[1]] = psf
    H = np.fft.fft2(h)
    W = np.conj(H) / (np.abs(H) ** 2 + np.float32(K))
    raw = np.real(np.fft.ifft2(np.fft.fft2(f) * W))
    lo, hi = raw.min(), raw.max()
    return ((raw - lo) / (hi - lo)).astype(np.float32)


def _spectrum(img, psf, K, M, N):
    """float64 G, H and the filtered spectrum Y = G W of the model on the full M x N plane"""
    f = np.zeros((M, N))
    f[:img.shape[0], :img.shape[1]] = img
    h = np.zeros((M, N))
    h[:psf.shape[0], :psf.shape[1]] = psf
    G, H = np.fft.fft2(f), np.fft.fft2(h)
    return G, H, G * np.conj(H) / (np.abs(H) ** 2 + K)


def _output(Y):
    """what the operator would return for the filtered spectrum Y: real inverse, min-max normalised, stored as float32"""
    return normalize(np.real(np.fft.ifft2(Y))).astype(np.float32)


def _scale_pair(Y, k, l, s):
    """bin (k, l) times s and its conjugate partner times conj(s): the spectrum stays Hermitian, the fault stays real"""
    Y = Y.copy()
    M, N = Y.shape
    k, l = k % M, l % N
    Y[k, l] *= s
    if ((-k) % M, (-l) % N) != (k, l):
        Y[-k, -l] *= np.conj(s)
    return Y


def _conjugate_pair(Y, k, l):
    Y = Y.copy()
    Y[k, l], Y[-k, -l] = Y[-k, -l], Y[k, l]
    return Y


# fault name -> (Y, G, H, K) -> faulty filtered spectrum; bins given as functions of the plan's M x N
PAIRS = {"(M/2, 1)": lambda M, N: (M // 2, 1), "(M/2, 0)": lambda M, N: (M // 2, 0), "(0, N/2)": lambda M, N: (0, N // 2),
         "(1, N/2)": lambda M, N: (1, N // 2), "(M/2, N/2)": lambda M, N: (M // 2, N // 2), "(1, N-1)": lambda M, N: (1, N - 1),
         "(M/2+1, N/2-1)": lambda M, N: (M // 2 + 1, N // 2 - 1), "(M/2-1, 1)": lambda M, N: (M // 2 - 1, 1)}
FAULTS = {"pair %s x 1.01" % name: (lambda Y, G, H, K, b=b: _scale_pair(Y, *b(*Y.shape), 1.01)) for name, b in PAIRS.items()}
FAULTS["conjugated pair (M/2+1, 1)"] = lambda Y, G, H, K: _conjugate_pair(Y, Y.shape[0] // 2 + 1, 1)
FAULTS["row M/2 x 1.01"] = lambda Y, G, H, K: Y * np.where(np.arange(Y.shape[0]) == Y.shape[0] // 2, 1.01, 1.0)[:, None]
FAULTS["column N/2 x 1.01"] = lambda Y, G, H, K: Y * np.where(np.arange(Y.shape[1]) == Y.shape[1] // 2, 1.01, 1.0)[None, :]
FAULTS["K x 1.01"] = lambda Y, G, H, K: G * np.conj(H) / (np.abs(H) ** 2 + 1.01 * K)


def test_edge_bins():
    assert edge_bins(64) == [0, 1, 31, 32, 33, 63]
    assert edge_bins(75) == [0, 1, 36, 37, 38, 74]
    assert edge_bins(4) == [0, 1, 2, 3]


@pytest.mark.parametrize("shape", [(64, 64), (256, 128), (1024, 1024)])
@pytest.mark.parametrize("K", [1e-4, 1e-2, 1.0])
def test_single_precision_operator_passes(oracle, shape, K):
    M, N = shape
    img = tone_image(M, N, M + N)
    psf = oracle.motion_blur_kernel(15, 30.0)
    got = _operator_c64(img, psf, K, M, N)
    raw = wiener_raw(img, psf, K, M, N)
    check_bins(got, raw, BIN_TOL, "complex64 operator %dx%d K=%g" % (M, N, K))
    assert np.abs(got - normalize(raw)).max() <= SPATIAL_TOL


@pytest.mark.parametrize("shape", [(64, 64), (256, 128), (1024, 1024)])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_injected_faults_fail_by_5x(oracle, shape, fault):
    M, N = shape
    img = tone_image(M, N, M + N)
    psf = oracle.motion_blur_kernel(15, 30.0)
    K = 0.01
    G, H, Y = _spectrum(img, psf, K, M, N)
    got = _output(FAULTS[fault](Y, G, H, K))
    e, _ = bin_error(got, wiener_raw(img, psf, K, M, N))
    assert e >= 5 * BIN_TOL, (fault, e)


def test_failure_message_names_the_spectral_edge(oracle):
    M, N = 256, 128
    img = tone_image(M, N, 5)
    psf = oracle.motion_blur_kernel(15, 30.0)
    G, H, Y = _spectrum(img, psf, 0.01, M, N)
    raw = wiener_raw(img, psf, 0.01, M, N)
    with pytest.raises(AssertionError, match=r"bin \(128, 1\) of 256 x 128 \[row M/2\]"):
        check_bins(_output(_scale_pair(Y, M // 2, 1, 1.01)), raw, BIN_TOL)
    with pytest.raises(AssertionError, match=r"bin \(0, 64\) of 256 x 128 \[row 0, column N/2\]"):
        check_bins(_output(_scale_pair(Y, 0, N // 2, 1.01)), raw, BIN_TOL)


@pytest.mark.parametrize("shape", [(64, 64), (1024, 1024)])
def test_dc_shift_and_scale_not_flagged(oracle, shape):
    M, N = shape
    img = tone_image(M, N, 9)
    psf = oracle.motion_blur_kernel(15, 30.0)
    G, H, Y = _spectrum(img, psf, 0.01, M, N)
    raw = wiener_raw(img, psf, 0.01, M, N)
    dc = Y.copy()
    dc[0, 0] += 0.5 * abs(Y[0, 0]) + M * N
    assert bin_error(_output(dc), raw)[0] <= BIN_TOL / 100
    assert bin_error(_output(Y * 1.37), raw)[0] <= BIN_TOL / 100
    assert bin_error(_output(Y), raw)[0] <= BIN_TOL / 100


def _corrupt(got, how):
    bad = got.copy()
    if how == "one NaN pixel":
        bad[17, 5] = np.nan
    elif how == "one inf pixel":
        bad[3, 40] = np.inf
    elif how == "all NaN":
        bad[:] = np.nan
    else:  # a degenerate min-max: the operator's normalisation of a flat plane
        bad[:] = 0.0
    return bad


@pytest.mark.parametrize("how", ["one NaN pixel", "one inf pixel", "all NaN", "constant"])
def test_non_finite_or_flat_output_fails(oracle, how):
    """The GPU tests' decision (_spectral.failures on bin_error and max_abs) must fail an output holding NaN or inf, or a
    flat one, for the per-bin and the spatial check alike (a NaN compares false with every threshold)."""
    M, N = 64, 128
    img = tone_image(M, N, 7)
    psf = oracle.motion_blur_kernel(15, 30.0)
    raw = wiener_raw(img, psf, 0.01, M, N)
    good = normalize(raw).astype(np.float32)
    e, where = bin_error(good, raw)
    assert failures("good", M, N, e, where, max_abs(good, normalize(raw)), BIN_TOL, SPATIAL_TOL) == []
    bad = _corrupt(good, how)
    e, where = bin_error(bad, raw)
    sp = max_abs(bad, normalize(raw))
    msgs = failures(how, M, N, e, where, sp, BIN_TOL, SPATIAL_TOL)
    assert len(msgs) == 2 and "per-bin" in msgs[0] and "max-abs" in msgs[1], msgs
    assert len(failures(how, M, N, None, None, sp, BIN_TOL, SPATIAL_TOL)) == 1  # the spatial-only judge of the cropped test
    with pytest.raises(AssertionError):
        check_bins(bad, raw, BIN_TOL)


@pytest.mark.parametrize("shape", [(64, 64), (100, 200), (128, 256), (32, 512), (256, 16)])
def test_model_matches_oracle_pow2(oracle, shape):
    """wiener_raw at power-of-two plans against the oracle's serial path (pad to powers of two, normalise over the padded
    area, crop), within the oracle's own float32 error."""
    rows, cols = shape
    img = np.random.default_rng(rows * 1000 + cols).random((rows, cols), dtype=np.float32)
    psf = oracle.motion_blur_kernel(5, 30.0)
    M, N = 1 << (rows - 1).bit_length(), 1 << (cols - 1).bit_length()
    want = oracle.serial_channel(img, psf, 0.01)
    raw = wiener_raw(img, psf, 0.01, M, N)
    lo, hi = raw.min(), raw.max()
    got = (raw[:rows, :cols] - lo) / (hi - lo)
    assert np.abs(got - want).max() <= 1e-5


@pytest.mark.parametrize("shape", [(64, 64), (32, 128), (45, 75)])
def test_delta_psf_identities(shape):
    M, N = shape
    img = tone_image(M, N, 3)
    K = 0.01
    # delta at the origin: H = 1, the output is the normalised input
    assert np.abs(normalize(wiener_raw(img, delta_psf(0, 0), K, M, N)) - normalize(img)).max() <= 1e-12
    for r0, c0 in ((1, 1), (M // 2, N // 2), (M - 1, N - 1), (3, 0)):
        raw = wiener_raw(img, delta_psf(r0, c0), K, M, N)
        assert np.abs(raw - delta_raw(img, r0, c0, K)).max() <= 1e-12
        # the sign of the shift: out[r, c] = img[r + r0, c + c0] (mod M, N)
        assert abs(raw[0, 0] * (1 + K) - img[r0, c0]) <= 1e-12
        assert abs(raw[M - r0 - 1, N - c0 - 1] * (1 + K) - img[M - 1, N - 1]) <= 1e-12
