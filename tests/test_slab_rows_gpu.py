"""fdr_slab_rows_fft_dev called directly on device memory, at the lengths where its dispatch turns: 4 points (the simple kernel),
8 (the smallest register kernel), 8192 (the largest row held on chip) and 16384 (8192-point blocks + global stages).  The
multi-process slab test reaches it with lengths from 64 to 2048 only.

Three rows, both directions, both dimensions of two non-square tables-only plans (16384 x 4 and 8 x 8192: dim 0 transforms rows
of N points, dim 1 rows of M points).  Parity mode: every row bit-equal to the oracle's 1-D transform.  Fast mode: relative L2
error below 5e-7 against numpy's float64 transform, the bound of test_fft1d_fast_close at every length (the inverse is the
conjugate of the forward transform of the conjugate, so the same bound holds for it).  A fourth row behind the three must stay
untouched."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 3
PLANS = ((16384, 4), (8, 8192))
FAST_TOL = 5e-7  # test_fft1d_fast_close


@functools.lru_cache(maxsize=None)
def _input(L):
    rng = np.random.default_rng(1000 + L)
    x = (rng.random((ROWS + 1, L), dtype=np.float32) - 0.5 + 1j * (rng.random((ROWS + 1, L), dtype=np.float32) - 0.5)).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _model64(L, inverse):
    x = _input(L)[:ROWS].astype(np.complex128)
    ref = np.fft.ifft(x, axis=1) * L if inverse else np.fft.fft(x, axis=1)  # unscaled, as the library
    ref.setflags(write=False)
    return ref


def slab_rows_fft(fdr, plan, x, dim, inverse):
    """x[:ROWS] through fdr_slab_rows_fft_dev on the current stream; returns all of x's rows as they stand afterwards"""
    import torch
    d = torch.from_numpy(np.array(x)).cuda()  # (a writable copy: the shared input stays as it is)
    st = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))
    fdr._check(fdr.lib.fdr_slab_rows_fft_dev(plan._h, ctypes.c_void_p(d.data_ptr()), ROWS, dim, int(inverse), st))
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("dim", [0, 1])
@pytest.mark.parametrize("shape", PLANS, ids=["%dx%d" % s for s in PLANS])
@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_slab_rows_fft_at_the_dispatch_lengths(fdr, oracle, mode, shape, dim, inverse):
    M, N = shape
    L = N if dim == 0 else M
    x = _input(L)
    with fdr.Plan(M, N, fdr.MODE_PARITY if mode == "parity" else fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        got = slab_rows_fft(fdr, p, x, dim, inverse)
    assert np.array_equal(got[ROWS], x[ROWS]), "the row behind the %d transformed rows was written" % ROWS
    if mode == "parity":
        for r in range(ROWS):
            want = oracle.fft_radix2(x[r], inverse)
            bad = np.count_nonzero(~(got[r] == want))
            assert bad == 0, "L=%d dim=%d inv=%d row %d: %d of %d values differ from the oracle" % (L, dim, inverse, r, bad, L)
    else:
        ref = _model64(L, inverse)
        for r in range(ROWS):
            err = np.linalg.norm(got[r] - ref[r]) / np.linalg.norm(ref[r])
            print("SLABROWS fast L=%d dim=%d inv=%d row %d: rel-L2 %.3g (bound %.3g)" % (L, dim, inverse, r, err, FAST_TOL))
            assert err < FAST_TOL, "L=%d dim=%d inv=%d row %d: rel-L2 %.3g >= %.3g" % (L, dim, inverse, r, err, FAST_TOL)
