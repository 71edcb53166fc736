"""CPU pins of tests/_frames_model.py, the float64 model of multi-frame Richardson-Lucy, before it judges the device
(test_frames_gpu.py): one frame as the single-frame models, copies of one frame, the adjoint identity, the flux invariant, injected
faults, the quality claims, the public surface and the refusals that need no device.  No GPU needed.  Cases print an `RLM` line with
their measured values (pytest -s)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from _frames_model import (FAULTS, MAX_FRAMES, QUALITY_EPS, QUALITY_LAMBDA, QUALITY_N, best_plain_iterate, blur_frames, blur_frames_adjoint,
                           crop_quality_case, flux_defect, frames_model, frames_state, quality_case, quality_psnr, threshold)
from _rl_model import centred_psf, dense_psf, psnr, rel_err, smooth_image
from _rlfree_model import SIGMA, rlfree_state
from _rltv_model import line_psf, rltv_free_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N, ROWS, COLS = 64, 128, 37, 101


def _psfs(K, sums=(1.0, 0.5, 2.0)):
    """K different small PSFs, centred in the plan and then shifted as a registration offset would (no H_k is real), with unequal
    sums (relative exposures)"""
    out = []
    for k in range(K):
        base = dense_psf(5 + k, 5) if k % 3 == 0 else line_psf(7, 25.0 * k) if k % 3 == 1 else dense_psf(3 + k, 7)
        plane = np.roll(centred_psf(base, M, N).astype(np.float64), (k % 2 + 1, -(k % 3) - 1), axis=(0, 1))
        out.append((plane * sums[k % len(sums)]).astype(np.float32))
    return out


def _frames(K, seed=8):
    """K frames of one smooth scene, each blurred by its own PSF and with its own small noise, >= 0.05"""
    rng = np.random.default_rng(seed)
    scene = smooth_image(M, N, seed).astype(np.float64) + 0.1
    psfs = _psfs(K)
    ds = []
    for k in range(K):
        b = blur_frames(scene, [psfs[k]], M, N)[0]
        ds.append((np.maximum(b[:ROWS, :COLS], 0.05) + 0.01 * rng.random((ROWS, COLS))).astype(np.float32))
    return ds, psfs


def _weights(K, seed=3):
    return (np.random.default_rng(seed).random((K, ROWS, COLS)) >= 0.1).astype(np.float32)


def test_one_frame_is_the_single_frame_model():
    """K = 1 equals rlfree_state, and with a prior rltv_free_state, to 1e-12"""
    ds, psfs = _frames(1)
    w = _weights(1)[0]
    for n in (0, 1, 5):
        a = frames_state(ds, psfs, M, N, n, weights=w)
        b = rlfree_state(ds[0], psfs[0], M, N, n, weights=w)
        for key in ("u", "alpha", "wgt"):
            assert float(np.max(np.abs(a[key] - b[key]))) <= 1e-12, (n, key)
        c = frames_state(ds, psfs, M, N, n, weights=w, lam=0.02, eps=1e-2)
        d = rltv_free_state(ds[0], psfs[0], M, N, n, 0.02, 1e-2, weights=w)
        assert float(np.max(np.abs(c["u"] - d["u"]))) <= 1e-12, n
    assert rel_err(c["u"], a["u"]) > 1e-4  # and the prior changes the result


@pytest.mark.parametrize("K", [2, 4, 8])
def test_copies_of_one_frame_are_the_single_call(K):
    """K copies of one frame (same PSF, same weights): alpha and the ratio sum scale by K, the threshold by K, u is unchanged"""
    ds, psfs = _frames(1)
    w = _weights(1)[0]
    for lam in (0.0, 0.02):
        one = frames_state(ds, psfs, M, N, 6, weights=w, lam=lam, eps=1e-2)["u"]
        many = frames_state(ds * K, psfs * K, M, N, 6, weights=w, lam=lam, eps=1e-2)["u"]
        e = float(np.max(np.abs(one - many)))
        print("RLM\tcopies\tK=%d lambda=%g\tmax diff=%.3g" % (K, lam, e))
        assert e <= 1e-12, (K, lam, e)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_adjoint_identity(K):
    """sum_k <blur_k x, y_k> = <x, sum_k blur_k^T y_k> on the window"""
    rng = np.random.default_rng(K)
    psfs = _psfs(K)
    x = rng.standard_normal((ROWS, COLS))
    ys = [rng.standard_normal((ROWS, COLS)) for _ in range(K)]
    lhs = sum(float(np.sum(b * y)) for b, y in zip(blur_frames(x, psfs, M, N), ys))
    rhs = float(np.sum(x * blur_frames_adjoint(ys, psfs, M, N)))
    scale = sum(float(np.sum(np.abs(b * y))) for b, y in zip(blur_frames(x, psfs, M, N), ys))
    print("RLM\tadjoint\tK=%d\tdefect=%.3g" % (K, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-12 * scale


@pytest.mark.parametrize("K", [2, 5])
def test_flux_invariant(K):
    """sum(alpha u) = sum_k sum(dw_k) after every iteration at lambda = 0 (every c_k > tau here), per-frame weights included"""
    ds, psfs = _frames(K)
    for w in (None, _weights(K)):
        for n in (1, 3, 10):
            f = flux_defect(frames_state(ds, psfs, M, N, n, weights=w))
            print("RLM\tflux\tK=%d n=%d weights=%s\tdefect=%.3g" % (K, n, w is not None, f))
            assert f <= 1e-12, (K, n, f)


@pytest.mark.parametrize("fault", FAULTS)
def test_faults_are_visible(fault):
    """every fault model moves every short case by far more than the device tolerance (1e-3).  sigma = 0.2 puts coverage values of
    the rim between sigma and sigma K, where the two thresholds differ."""
    for K in (2, 3, 5):
        ds, psfs = _frames(K)
        w = _weights(K)
        for n in (1, 3):
            good = frames_model(ds, psfs, M, N, n, weights=w, sigma=0.2, out_shape=(M, N))
            bad = frames_model(ds, psfs, M, N, n, weights=w, sigma=0.2, out_shape=(M, N), fault=fault)
            e = rel_err(bad, good)
            print("RLM\tfault\t%s K=%d n=%d\trel=%.3g" % (fault, K, n, e))
            assert e > 2e-2, (fault, K, n, e)


def test_threshold_is_a_float32_product():
    for K in range(1, MAX_FRAMES + 1):
        assert threshold(SIGMA, K) == float(np.float32(SIGMA) * np.float32(K))
    assert threshold(SIGMA, 1) == SIGMA


@pytest.fixture(scope="module")
def case():
    return quality_case()


def test_quality_joint_beats_the_best_single_frame(case):
    """the issue's table, re-measured by the model (float64), PSNR in dB.  Measured: the crops 21.70, 20.71, 21.70; with the prior
    (lambda 0.01, eps 1e-3, n = 100) the frames alone 32.35, 30.20, 32.41 and all three jointly 37.17: a gain of 4.76 dB, of which
    half is asserted; the smallest |alpha - 3 sigma| is 0.0226"""
    crops = [psnr(d, case["truth"]) for d in case["ds"]]
    single = [quality_psnr(case, [k]) for k in range(3)]
    joint = quality_psnr(case, [0, 1, 2])
    print("RLM\tquality (model)\tcrops %s; with the prior: alone %s, jointly %.2f dB"
          % (", ".join("%.2f" % c for c in crops), ", ".join("%.2f" % s for s in single), joint))
    assert joint >= max(single) + 2.4, (joint, single)
    assert min(single) > max(crops)
    st = frames_state(case["ds"], case["psfs"], case["M"], case["N"], 0)
    margin = float(np.min(np.abs(st["alpha"] - threshold(SIGMA, 3))))
    print("RLM\tquality (model)\tmin |alpha - 3 sigma| = %.4f" % margin)
    assert margin >= 1e-3


def test_quality_best_plain_iterates(case):
    """without a prior: the best joint iterate lies above every frame's own best iterate (measured 27.72 at k = 21 against 24.68 at
    k = 14, 23.92 at k = 18 and 24.66 at k = 14: a gain of 3.04 dB, of which half is asserted), and the joint iteration fits the
    noise afterwards as plain RL does"""
    single = [best_plain_iterate(case, [k], 40) for k in range(3)]
    joint = best_plain_iterate(case, [0, 1, 2], 40)
    late = quality_psnr(case, [0, 1, 2], 100, lam=0.0)
    print("RLM\tquality (model)\tno prior: alone %s, jointly %.2f dB at k=%d, %.2f dB at n=100"
          % (", ".join("%.2f at k=%d" % (q, k) for k, q in single), joint[1], joint[0], late))
    assert joint[1] >= max(q for _, q in single) + 1.5, (joint, single)
    assert late < joint[1]


SMOOTH_GAIN = 8.7  # dB, measured by the model (below)


def test_quality_on_the_smooth_scene():
    """crop_scene with 15 px horizontal, vertical and diagonal lines at 2000 photons: the best joint iterate against the best single
    frame's (measured 41.65 dB at k = 5 against 32.94 at k = 8, 32.06 at k = 9 and 31.26 at k = 9: a gain of 8.7 dB, of which half
    is asserted)"""
    c = crop_quality_case()
    single = [best_plain_iterate(c, [k], 40) for k in range(3)]
    joint = best_plain_iterate(c, [0, 1, 2], 40)
    print("RLM\tquality (model)\tsmooth scene, no prior: alone %s, jointly %.2f dB at k=%d"
          % (", ".join("%.2f at k=%d" % (q, k) for k, q in single), joint[1], joint[0]))
    assert joint[1] >= max(q for _, q in single) + SMOOTH_GAIN / 2, (joint, single)



FRAMES_FUNCS = ("fdr_set_frame_psfs", "fdr_set_frame_psfs_dev", "fdr_frame_count", "fdr_spectrum_sum_f32_dev", "fdr_blur_frames_f32_dev",
                "fdr_richardson_lucy_frames_f32", "fdr_richardson_lucy_frames_f32_dev")
FIELDS = (("int", "iterations"), ("float", "sigma"), ("int", "norm_area"), ("int", "out_rows"), ("int", "out_cols"), ("float", "tv_lambda"),
          ("float", "tv_eps"))


def test_symbols_and_surface(fdr):
    header = open(os.path.join(ROOT, "include", "fdr.h")).read()
    m = re.search(r"typedef\s+struct\s+fdr_rl_frames_params\s*\{(.*?)\}\s*fdr_rl_frames_params\s*;", header, re.S)
    assert m, "fdr_rl_frames_params is not in the header"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = tuple((t, n.strip()) for t, names in re.findall(r"\b(int|float)\s+([^;]+);", body) for n in names.split(","))
    assert fields == FIELDS, fields
    assert [f[0] for f in fdr.RlFramesParams._fields_] == [n for _, n in FIELDS]
    assert [f[1] for f in fdr.RlFramesParams._fields_] == [ctypes.c_int if t == "int" else ctypes.c_float for t, _ in FIELDS]
    assert ctypes.sizeof(fdr.RlFramesParams) == 28
    assert re.search(r"#define\s+FDR_MAX_FRAMES\s+8\b", header) and fdr.MAX_FRAMES == MAX_FRAMES == 8
    assert re.search(r"#define\s+FDR_VERSION\s+300\b", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in FRAMES_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    sig = inspect.signature(fdr.Plan.richardson_lucy_frames).parameters
    assert list(sig)[:6] == ["self", "frames", "iterations", "weights", "tv_lambda", "tv_eps"]
    assert (sig["weights"].default, sig["tv_lambda"].default, sig["norm_area"].default) == (None, 0.0, fdr.NORM_NONE)
    sig = inspect.signature(fdr.Plan.richardson_lucy_frames_dev).parameters
    assert list(sig)[:10] == ["self", "d_imgs", "img_pitch", "count", "rows", "cols", "stride", "d_out", "out_stride", "iterations"]
    for name in ("set_frame_psfs", "set_frame_psfs_dev", "frame_count", "blur_frames_dev"):
        assert callable(getattr(fdr.Plan, name)), name
    sig = inspect.signature(fdr.richardsonLucyFrames_myfft).parameters
    assert list(sig)[:5] == ["frames", "psfs", "iterations", "weights", "tv_lambda"]
    assert (sig["weights"].default, sig["tv_lambda"].default) == (None, 0.0)
    assert callable(fdr.richardsonLucyFrames_RGB) and callable(fdr.spectrum_sum_dev)
    mk = open(os.path.join(os.path.dirname(fdr.LIB_PATH), "Makefile")).read()
    assert "csrc/fdr_frames.hip" in mk and "csrc/fdr_api_frames.hip" in mk


def test_refusals_without_a_device(fdr):
    """what the entry points refuse before they touch a device: null pointers, and for the sum every bad argument (its pointers are
    only compared, never followed, before the refusal)"""
    L = fdr.lib
    img = np.ones((8, 32), dtype=np.float32)
    out = np.empty_like(img)
    prm = fdr.RlFramesParams(1, 1e-2, 2, 8, 32, 0.0, 0.0)
    for h, i, o in ((None, img.ctypes.data, out.ctypes.data), (1, None, out.ctypes.data), (1, img.ctypes.data, None)):
        assert L.fdr_richardson_lucy_frames_f32(h, i, 256, 1, 8, 32, 32, None, 0, 0, o, 32, ctypes.byref(prm)) == -1
        assert L.fdr_richardson_lucy_frames_f32_dev(h, i, 256, 1, 8, 32, 32, None, 0, 0, o, 32, ctypes.byref(prm), None) == -1
        assert b"null argument" in L.fdr_last_error()
        assert L.fdr_blur_frames_f32_dev(h, i, 256, 8, 32, 32, o, 256, 32, 1, 0, None) == -1 and b"null argument" in L.fdr_last_error()
    assert L.fdr_set_frame_psfs(None, img.ctypes.data, 256, 1, 8, 32, 32) == -1 and b"null argument" in L.fdr_last_error()
    assert L.fdr_set_frame_psfs_dev(None, img.ctypes.data, 256, 1, 8, 32, 32, None) == -1
    n = ctypes.c_int(5)
    assert L.fdr_frame_count(None, ctypes.byref(n)) == -1 and L.fdr_frame_count(1, None) == -1

    base = 1 << 20  # made-up, 16-byte aligned device addresses

    def ssum(dst=base, srcs=(base + 4096,), n=None, n_floats=64, acc=0):
        arr = (ctypes.c_void_p * 8)(*srcs)
        return L.fdr_spectrum_sum_f32_dev(0, dst, arr, len(srcs) if n is None else n, n_floats, acc, None)

    assert ssum(dst=None) == -1 and L.fdr_spectrum_sum_f32_dev(0, base, None, 1, 64, 0, None) == -1
    assert ssum(n=0) == -1 and ssum(n=9) == -1 and b"1 .. 8" in L.fdr_last_error()
    for nf in (0, 1, 3, 65):
        assert ssum(n_floats=nf) == -1 and b"n_floats" in L.fdr_last_error(), nf
    assert ssum(dst=base + 4) == -1 and ssum(srcs=(base + 4096 + 8,)) == -1 and b"aligned" in L.fdr_last_error()
    assert ssum(srcs=(base + 4096, None), n=2) == -1
    assert ssum(srcs=(base + 16,)) == -1 and b"overlaps" in L.fdr_last_error()  # shifted by less than the length
    assert ssum(srcs=(base + 4096, base + 64 * 4 - 16)) == -1 and b"overlaps" in L.fdr_last_error()


def test_cli_refuses_frame_beside_anything_else():
    """tools/cli/gpu: --frame without --rl n --free-boundary, beside another leg or option, with a bad length or with more than 7 frames
    prints the usage text of the frames leg and fails before a picture is read (the paths do not exist)"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")
    frame = ["--frame", "none2.png", "15", "30"]
    ok = ["--rl", "5", "--free-boundary"]
    for args in (frame, ["--rl", "5"] + frame, ["--free-boundary"] + frame, ok + ["--accel"] + frame, ["--rl", "auto", "--free-boundary"] + frame,
                 ok + ["--tile", "64"] + frame, ok + ["--rl-tv", "0.01", "--rl-tv-color"] + frame, ok + ["--frame", "none2.png", "0", "30"],
                 ok + frame * 8, ["--tv", "5", "--free-boundary"] + frame):
        r = subprocess.run([gpu, "none.png", "15", "30"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" in r.stdout and "Cannot read" not in r.stdout, (args, r.stdout[-300:])
        if args is frame or "--accel" in args:  # (an earlier check of another option may answer with the short usage line)
            assert "--frame <img2> <L2> <A2>" in r.stdout, (args, r.stdout[-300:])
    for extra in (["--k", "0.02"], ["--sigma", "0.01"], ["--reg", "gcv"], ["--norm", "cropped"], ["--host-epilogue"], ["--rl-max", "50"],
                  ["--rl-stop", "kl"], ["--gain", "100"], ["--rl-check", "2"], ["--mode", "fast"], ["--pad", "zero"], ["--verify"]):
        r = subprocess.run([gpu, "none.png", "15", "30"] + ok + frame + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" in r.stdout and "Cannot read" not in r.stdout, (extra, r.stdout[-300:])
    for first in (["auto", "auto"], ["blind", "9"], ["defocus", "3"]):
        r = subprocess.run([gpu, "none.png"] + first + ok + frame, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" in r.stdout and "Cannot read" not in r.stdout, (first, r.stdout[-300:])
    r = subprocess.run([gpu, "none.png", "15", "30"] + ok + frame + ["--rl-tv", "0.01", "--rl-tv-eps", "0.01", "--mask", "m.png", "--out", "o.png", "--raw-out", "o.f32"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Cannot read image" in r.stdout  # accepted: it gets as far as the picture
