"""CPU pins of tests/_tvframes_model.py, the float64 model of multi-frame TV deconvolution, before it judges the device
(test_tvframes_gpu.py): one frame as the single-frame models, copies of one frame, the normal equations of the x step, the objective
from two starts, injected faults, the quality table, the public surface and the refusals that need no device.  No GPU needed.  Cases
print a `TVM` line with their measured values (pytest -s)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from _frames_model import quality_case
from _rl_model import op_spectrum, psnr, rel_err
from _tv_model import dx, dxT, dy, dyT
from _tvframes_model import (FAULTS, LEAST_SQUARES, POISSON, QUALITY_MEASURED, QUALITY_MU, SHORT, SHORT_IDS, TVFR_TOL, frames_objective,
                             quality_psnr, short_frames, short_psfs, short_weights, tvframes_iterates, tvframes_model)
from _tvfree_model import tvfree_iterates
from _tvpoisson_model import tvpoisson_iterates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N, ROWS, COLS = 64, 128, 37, 101
TERMS = ((LEAST_SQUARES, 0.0, "ls"), (POISSON, 0.3, "poisson"))


def _need(fdr):
    assert hasattr(fdr.lib, "fdr_tv_deconv_frames_f32_dev"), "the library has no multi-frame TV deconvolution"


def _case(K, kind="dense", weights="per_frame", seed=5, positive=False):
    psfs = short_psfs(kind, K, M, N)
    return short_frames(M, N, ROWS, COLS, K, psfs, seed, positive), psfs, short_weights(weights, K, ROWS, COLS, seed)


@pytest.mark.parametrize("weights", ["none", "per_frame"])
def test_one_frame_is_the_single_frame_model(weights):
    """K = 1 equals tvfree_iterates and tvpoisson_iterates, every plane of every iteration, to 1e-12"""
    ds, psfs, w = _case(1, weights=weights)
    w1 = None if w is None else w[0]
    for aniso in (False, True):
        a = list(tvframes_iterates(ds, psfs, M, N, 50.0, 1.0, 4, w, 3.0, LEAST_SQUARES, 0.0, aniso))
        b = list(tvfree_iterates(ds[0], psfs[0], M, N, 50.0, 1.0, 4, w1, 3.0, aniso))
        c = list(tvframes_iterates(ds, psfs, M, N, 50.0, 1.0, 4, w, 3.0, POISSON, 0.3, aniso))
        d = list(tvpoisson_iterates(ds[0], psfs[0], M, N, 50.0, 1.0, 4, w1, 3.0, 0.3, aniso))
        for it in range(5):
            assert float(np.max(np.abs(a[it]["x"] - b[it]["x"]))) <= 1e-12, (it, aniso)
            assert float(np.max(np.abs(c[it]["x"] - d[it]["x"]))) <= 1e-12, (it, aniso)
            if it:
                assert float(np.max(np.abs(a[it]["q"][0] - b[it]["q"]))) <= 1e-12 and float(np.max(np.abs(a[it]["r"][0] - b[it]["r"]))) <= 1e-12
                assert float(np.max(np.abs(c[it]["q"][0] - d[it]["q"]))) <= 1e-12 and float(np.max(np.abs(c[it]["r"][0] - d[it]["r"]))) <= 1e-12
    assert rel_err(c[4]["x"], a[4]["x"]) > 1e-4  # and the two data terms differ


@pytest.mark.parametrize("K", [2, 4, 8])
def test_copies_of_one_frame_are_the_single_model_at_K_mu_K_nu(K):
    """K copies of one frame (same PSF, same weights): every q_k is the same plane, b and sum |H|^2 scale by K, so x is the single
    model's at (K mu, K nu), for both data terms"""
    ds, psfs, w = _case(1)
    for term, bg, name in TERMS:
        many = tvframes_model(ds * K, psfs * K, M, N, 20.0, 2.0, 6, w[0], 1.5, term, bg, out_shape=(M, N))
        one = tvframes_model(ds, psfs, M, N, K * 20.0, 2.0, 6, w[0], K * 1.5, term, bg, out_shape=(M, N))
        e = float(np.max(np.abs(one - many)))
        print("TVM\tcopies\tK=%d %s\tmax diff=%.3g" % (K, name, e))
        assert e <= 1e-12, (K, name, e)


@pytest.mark.parametrize("K", [1, 3, 5])
def test_normal_equations_of_the_x_step(K):
    """the x of an iteration solves (nu sum_k H_k^T H_k + rho D^T D) x = nu sum_k H_k^T r_k + rho D^T v, with the r_k and v of that
    iteration, for both data terms"""
    ds, psfs, w = _case(K)
    Hs = [op_spectrum(p, M, N) for p in psfs]
    nu, rho = 3.0, 2.0
    for term, bg, name in TERMS:
        for it, st in enumerate(tvframes_iterates(ds, psfs, M, N, 40.0, rho, 3, w, nu, term, bg)):
            if not it:
                continue
            x, (vx, vy) = st["x"], st["v"]
            X = np.fft.rfft2(x)
            lhs = rho * (dxT(dx(x)) + dyT(dy(x)))
            rhs = rho * (dxT(vx) + dyT(vy))
            for k in range(K):
                lhs = lhs + nu * np.fft.irfft2(X * np.abs(Hs[k]) ** 2, s=(M, N))
                rhs = rhs + nu * np.fft.irfft2(np.fft.rfft2(st["r"][k]) * np.conj(Hs[k]), s=(M, N))
            e = float(np.max(np.abs(lhs - rhs))) / float(np.max(np.abs(rhs)))
            print("TVM\tnormal equations\tK=%d %s it=%d\tdefect=%.3g" % (K, name, it, e))
            assert e <= 1e-11, (K, name, it, e)


@pytest.mark.parametrize("term,bg,name", TERMS)
def test_objective_decreases_to_the_same_value_from_two_starts(term, bg, name):
    """a convex problem: from pad(d_0) and from a flat plane the objective mu sum_k Phi_k + TV falls from checkpoint to checkpoint (n
    = 0, 100, 300, 1000; 32^2, window 28 x 30, K = 3, per-frame weights) and settles at one value.  ADMM's objective error falls like
    1 / n, with a constant nobody knows beforehand, so the bound scales itself: the two values at n = 1000 may differ by no more than
    either run still gained between n = 300 and n = 1000, and by no more than 1e-4 of the value."""
    M_, N_, R_, C_ = 32, 32, 28, 30
    psfs = short_psfs("motion", 3, M_, N_)
    ds = short_frames(M_, N_, R_, C_, 3, psfs, 5, positive=True)
    w = short_weights("per_frame", 3, R_, C_, 5)
    mu, rho = 30.0, 2.0
    runs = []
    for x0 in (None, np.full((M_, N_), float(np.mean(ds[0])))):
        f = [frames_objective(st["x"], ds, psfs, M_, N_, mu, w, term, bg)
             for it, st in enumerate(tvframes_iterates(ds, psfs, M_, N_, mu, rho, 1000, w, 0.0, term, bg, x0=x0)) if it in (0, 100, 300, 1000)]
        print("TVM\tobjective\t%s start %s\t%s" % (name, "pad(d0)" if x0 is None else "flat", " -> ".join("%.6f" % v for v in f)))
        assert f[0] > f[1] > f[2] > f[3], f
        runs.append(f)
    gap = abs(runs[0][3] - runs[1][3])
    assert gap <= max(r[2] - r[3] for r in runs), (gap, runs)
    assert gap <= 1e-4 * abs(runs[0][3]), (gap, runs)


@pytest.mark.parametrize("fault", FAULTS)
def test_faults_are_visible(fault):
    """every fault model moves every short case (K >= 2, per-frame weights, both data terms) by more than 100 times the device
    tolerance"""
    for (M_, N_, rows, cols, _s, _ws, _os, _outs), sid in zip(SHORT, SHORT_IDS):
        for K in (2, 3, 5):
            psfs = short_psfs("dense", K, M_, N_)
            ds = short_frames(M_, N_, rows, cols, K, psfs, 7)
            w = short_weights("per_frame", K, rows, cols, 7)
            for term, bg, name in TERMS:
                for n in (1, 3):
                    good = tvframes_model(ds, psfs, M_, N_, 50.0, 1.0, n, w, 3.0, term, bg, out_shape=(M_, N_))
                    bad = tvframes_model(ds, psfs, M_, N_, 50.0, 1.0, n, w, 3.0, term, bg, out_shape=(M_, N_), fault=fault)
                    e = rel_err(bad, good)
                    print("TVM\tfault\t%s %s K=%d %s n=%d\trel=%.3g" % (fault, sid, K, name, n, e))
                    assert e > 100 * TVFR_TOL, (fault, sid, K, name, n, e)


@pytest.fixture(scope="module")
def case():
    return quality_case()


@pytest.mark.parametrize("term,name", [(LEAST_SQUARES, "ls"), (POISSON, "poisson")])
def test_quality_joint_beats_the_best_single_frame(case, term, name):
    """the issue's table, re-measured by the model (float64) on quality_case(): n = 100, rho = nu = 2, every entry at the best mu of
    QUALITY_MU, whose best value must be interior; PSNR in dB.  Half of the measured gain of the joint call over the best single
    frame (QUALITY_MEASURED) is asserted."""
    grid = QUALITY_MU[term]
    best = []
    for frames in ([0], [1], [2], [0, 1, 2]):
        vals = [quality_psnr(case, frames, mu, term) for mu in grid]
        i = int(np.argmax(vals))
        print("TVM\tquality (model)\t%s frames %s\t%s\tbest mu %g" % (name, frames, " ".join("%g:%.2f" % t for t in zip(grid, vals)), grid[i]))
        assert 0 < i < len(grid) - 1, (name, frames, vals)
        best.append(vals[i])
    crops = [psnr(d, case["truth"]) for d in case["ds"]]
    measured = QUALITY_MEASURED[term]
    gain = measured[3] - max(measured[:3])
    print("TVM\tquality (model)\t%s: alone %s, jointly %.2f dB (recorded gain %.2f dB)" % (name, ", ".join("%.2f" % s for s in best[:3]), best[3], gain))
    assert np.allclose(best, measured, atol=0.05), (best, measured)
    assert best[3] >= max(best[:3]) + gain / 2, (best, gain)
    assert min(best[:3]) > max(crops)


FUNCS = ("fdr_tv_deconv_frames_f32", "fdr_tv_deconv_frames_f32_dev")
FIELDS = (("float", "mu"), ("float", "rho"), ("float", "nu"), ("float", "background"), ("int", "data_term"), ("int", "iterations"),
          ("int", "anisotropic"), ("int", "nonneg"), ("int", "norm_area"), ("int", "out_rows"), ("int", "out_cols"), ("void*", "stream"))


def test_symbols_and_surface(fdr):
    _need(fdr)
    header = open(os.path.join(ROOT, "include", "fdr.h")).read()
    m = re.search(r"typedef\s+struct\s+fdr_tv_frames_params\s*\{(.*?)\}\s*fdr_tv_frames_params\s*;", header, re.S)
    assert m, "fdr_tv_frames_params is not in the header"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = tuple((t.replace(" ", ""), n.strip()) for t, names in re.findall(r"\b(int|float|void\s*\*)\s*([^;]+);", body) for n in names.split(","))
    assert fields == FIELDS, fields
    P = fdr.TvFramesParams
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "void*": ctypes.c_void_p}
    assert [f[0] for f in P._fields_] == [n for _, n in FIELDS]
    assert [f[1] for f in P._fields_] == [ctype[t] for t, _ in FIELDS]
    # four floats, seven ints, four bytes of padding, the pointer
    assert ctypes.sizeof(P) == 56
    assert [getattr(P, n).offset for _, n in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48]
    assert re.search(r"#define\s+FDR_TV_FRAMES_LEAST_SQUARES\s+0\b", header) and fdr.TV_FRAMES_LEAST_SQUARES == LEAST_SQUARES == 0
    assert re.search(r"#define\s+FDR_TV_FRAMES_POISSON\s+1\b", header) and fdr.TV_FRAMES_POISSON == POISSON == 1
    assert re.search(r"#define\s+FDR_VERSION\s+300\b", header) and re.search(r"#define\s+FDR_MAX_PASSES\s+16\b", header)
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in FUNCS:
        d = re.search(r"\bint\s+%s\s*\(([^;{]*)\)\s*;" % name, code)
        assert d, name
        assert "stream" not in d.group(1), "the stream travels in the struct"
        assert d.group(1).count(",") == 12, name  # the argument list of fdr_richardson_lucy_frames_f32
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    sig = inspect.signature(fdr.Plan.tv_deconv_frames).parameters
    assert list(sig)[:7] == ["self", "frames", "mu", "iterations", "weights", "data_term", "background"]
    assert (sig["weights"].default, sig["data_term"].default, sig["norm_area"].default) == (None, 0, fdr.NORM_NONE)
    sig = inspect.signature(fdr.Plan.tv_deconv_frames_dev).parameters
    assert list(sig)[:11] == ["self", "d_imgs", "img_pitch", "count", "rows", "cols", "stride", "d_out", "out_stride", "mu", "iterations"]
    assert sig["stream"].default is None
    sig = inspect.signature(fdr.tvDeblurFrames_myfft).parameters
    assert list(sig)[:5] == ["frames", "psfs", "mu", "iterations", "weights"]
    assert callable(fdr.tvDeblurFrames_RGB)
    mk = open(os.path.join(os.path.dirname(fdr.LIB_PATH), "Makefile")).read()
    assert "csrc/fdr_tvframes.hip" in mk and "csrc/fdr_api_tvframes.hip" in mk
    hpp = open(os.path.join(ROOT, "include", "fft", "fft.hpp")).read()
    assert re.search(r"\btvDeblurFrames_RGB\s*\(", hpp)


def test_refusals_without_a_device(fdr):
    """null pointers are refused before a device is touched"""
    _need(fdr)
    L = fdr.lib
    img = np.ones((8, 32), dtype=np.float32)
    out = np.empty_like(img)
    prm = fdr.TvFramesParams(10.0, 2.0, 0.0, 0.0, 0, 1, 0, 0, 0, 8, 32, None)
    for h, i, o, q in ((None, img.ctypes.data, out.ctypes.data, ctypes.byref(prm)), (1, None, out.ctypes.data, ctypes.byref(prm)),
                       (1, img.ctypes.data, None, ctypes.byref(prm)), (1, img.ctypes.data, out.ctypes.data, None)):
        assert L.fdr_tv_deconv_frames_f32(h, i, 256, 1, 8, 32, 32, None, 0, 0, o, 32, q) == -1
        assert b"fdr_tv_deconv_frames_f32: null argument" in L.fdr_last_error()
        assert L.fdr_tv_deconv_frames_f32_dev(h, i, 256, 1, 8, 32, 32, None, 0, 0, o, 32, q) == -1
        assert b"fdr_tv_deconv_frames_f32_dev: null argument" in L.fdr_last_error()
