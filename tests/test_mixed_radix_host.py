"""CPU tests of FDR_FLAG_MIXED_RADIX: the flag's value on both sides of the ABI, plan validation before any device work,
and the float64 model of the optimal-size operator (tests/_mixed_model.py) pinned against the CPU oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from _mixed_model import optimal_size, wiener_model


def _create(fdr, M, N, mode, flags):
    h = ctypes.c_void_p()
    rc = fdr.lib.fdr_plan_create(0, M, N, mode, flags, ctypes.byref(h))
    if rc == 0:
        fdr.lib.fdr_plan_destroy(h)
    return rc, fdr.lib.fdr_last_error().decode()


def test_flag_value_python_and_header(fdr):
    assert fdr.FLAG_MIXED_RADIX == 2048
    header = open(os.path.join(ROOT, "include", "fdr.h")).read()
    m = re.search(r"#define\s+FDR_FLAG_MIXED_RADIX\s+(\d+)u?", header)
    assert m and int(m.group(1)) == 2048


def test_plan_refuses_non_smooth_size(fdr):
    rc, msg = _create(fdr, 4097, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX)
    assert rc == -1
    assert "fdr_optimal_dft_size" in msg and "8192" in msg


def test_plan_refuses_smooth_size_above_8192(fdr):
    assert _create(fdr, 9000, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX)[0] == -1
    assert _create(fdr, 64, 9000, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX | fdr.FLAG_ANY_SIZE)[0] == -1


def test_plan_refuses_tables_only_and_simple_path(fdr):
    assert _create(fdr, 300, 200, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX | fdr.FLAG_TABLES_ONLY)[0] == -1
    assert _create(fdr, 300, 200, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX | fdr.FLAG_SIMPLE_PATH)[0] == -1


def test_parity_mode_ignores_the_flag(fdr):
    # parity keeps today's rule: a non-power-of-two plan needs FLAG_ANY_SIZE
    assert _create(fdr, 100, 64, fdr.MODE_PARITY, fdr.FLAG_MIXED_RADIX)[0] == -2


@pytest.mark.parametrize("shape", [(30, 50), (45, 100), (97, 33), (6, 10)])
def test_model_matches_oracle(oracle, shape):
    rows, cols = shape
    rng = np.random.default_rng(rows * 1000 + cols)
    img = rng.random((rows, cols), dtype=np.float32)
    psf = oracle.motion_blur_kernel(5, 30.0)
    M, N = optimal_size(rows), optimal_size(cols)
    assert (M, N) == (oracle.optimal_dft_size(rows), oracle.optimal_dft_size(cols))
    want = oracle.wiener(img, psf, 0.01)
    got = wiener_model(img, psf, 0.01, M, N, norm_cropped=True)
    assert np.abs(got - want).max() <= 1e-5
