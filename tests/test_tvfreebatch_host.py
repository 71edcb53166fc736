"""CPU pins of tests/_tvfreebatch_model.py, the float64 model of free-boundary and noise-constrained TV deconvolution in groups,
before it judges the device (test_tvfreebatch_gpu.py): one image against the single models, uncoupled groups against the per-image
models, injected group faults far outside the device tolerance on the GPU test's coupled cases, the quality claim of the coupled
free form on a colour crop, and the public surface.  No GPU needed; the refusals that need a plan are in test_tvfreebatch_gpu.py.
Cases print a `TVFB` line with their measured values (pytest -s).

Quality, measured with the model (test_coupled_free_beats_channelwise): colour_blocks 256^2 blurred by the 15 x 15 line PSF, noise
0.05, the 200 x 200 window at (28, 40), 60 steps, rho 2, each form at its best mu of (20, 40, 80): channel-wise 29.54 dB (mu 40),
coupled 29.94 dB (mu 40; 29.94 at 20), a gain of 0.40 dB over a blurred crop of 19.84 dB.  Half of it, 0.20 dB, is asserted."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from _rl_model import centred_psf, psnr
from _tvauto_model import f32, tvauto_iterates
from _tvcolor_model import colour_blocks
from _tvfree_model import line_psf, tvf_image, tvf_weights, tvfree_iterates
from _tvfreebatch_model import (COUPLED, COUPLED_IDS, COUPLED_PLANS, COUPLED_SIGMAS, FAULTS, FREE_FAULTS, TVFB_AUTO_TOL, TVFB_TOL, coupled_case,
                                group_iterates, group_model, rel_err)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEASURED_GAIN_DB = 0.40  # see the header


@pytest.mark.parametrize("coupled", [False, True], ids=["uncoupled", "coupled"])
def test_one_image_is_the_single_model(coupled):
    """C = 1: every plane of every iteration equals tvfree_iterates / tvauto_iterates exactly, coupled or not (the joint norm of one
    channel is its own; anisotropic only uncoupled), in float64 and in float32"""
    M, N, rows, cols = 16, 32, 9, 30
    d = tvf_image(M, N, rows, cols, 3)
    psf = centred_psf(line_psf(), M, N)
    for kind in ("none", "fractional"):
        w = tvf_weights(kind, rows, cols, 3)
        for aniso in ((False,) if coupled else (False, True)):
            for dtype in (np.float64, np.float32):
                one = list(tvfree_iterates(d, psf, M, N, 50.0, 2.0, 4, w, 3.0, aniso, dtype))
                grp = list(group_iterates(d[None], psf, M, N, mu=50.0, rho=2.0, iterations=4, weights=w, nu=3.0, anisotropic=aniso, coupled=coupled,
                                          dtype=dtype))
                assert len(one) == len(grp) == 5
                for a, b in zip(one, grp):
                    assert np.array_equal(a["x"], b["x"][0])
                assert np.array_equal(one[-1]["q"], grp[-1]["q"][0])
                for sigma in (0.02, 0.3, 0.0):
                    one = list(tvauto_iterates(d, psf, M, N, f32(sigma), 2.0, 4, w, 1.2, 20.0, aniso, dtype))
                    grp = list(group_iterates(d[None], psf, M, N, sigmas=[f32(sigma)], rho=2.0, iterations=4, weights=w, tau=1.2, nu=20.0,
                                              anisotropic=aniso, coupled=coupled, dtype=dtype))
                    for a, b in zip(one, grp):
                        assert np.array_equal(a["x"], b["x"][0]) and a["sigma"] == b["sigma"][0]
                    for a, b in zip(one[1:], grp[1:]):
                        assert tuple(b["trace"][0]) == a["trace"]


def test_uncoupled_group_is_the_per_image_models():
    """three images, uncoupled: outputs and traces equal the single models image by image, exactly; every image with its own sigma"""
    M, N, rows, cols = 64, 128, 37, 101
    d, psf, w = coupled_case(M, N, rows, cols)
    out, _ = group_model(d, psf, M, N, mu=50.0, rho=2.0, iterations=3, weights=w, nu=3.0, nonneg=True, norm_area=1, out_shape=(M, N))
    from _tvauto_model import tvauto_model
    from _tvfree_model import tvfree_model
    for c in range(3):
        assert np.array_equal(out[c], tvfree_model(d[c], psf, M, N, 50.0, 2.0, 3, w, 3.0, nonneg=True, norm_area=1, out_shape=(M, N)))
    sig = [f32(s) for s in COUPLED_SIGMAS[:2]] + [0.0]
    out, tr = group_model(d, psf, M, N, sigmas=sig, rho=2.0, iterations=3, weights=w, anisotropic=True)
    for c in range(3):
        o, t = tvauto_model(d[c], psf, M, N, sig[c], 2.0, 3, w, anisotropic=True)
        assert np.array_equal(out[c], o) and np.array_equal(tr[c], t)


@pytest.mark.parametrize("plan", COUPLED_PLANS, ids=COUPLED_IDS)
def test_group_faults_are_far_outside_the_tolerance(plan):
    """every fault model moves an output of the coupled GPU cases (n = 3, fractional weights) by more than 10x the tolerance that
    test_tvfreebatch_gpu.py holds the device to there: free form for the faults it can have, auto form for all six"""
    M, N, rows, cols = plan
    d, psf, w = coupled_case(M, N, rows, cols)
    sig = [f32(s) for s in COUPLED_SIGMAS]
    free, _ = group_model(d, psf, M, N, mu=COUPLED["mu"], rho=COUPLED["rho"], iterations=3, weights=w, nu=COUPLED["nu_free"], coupled=True)
    auto, tr = group_model(d, psf, M, N, sigmas=sig, rho=COUPLED["rho"], iterations=3, weights=w, nu=COUPLED["nu_auto"], coupled=True)
    assert np.all(tr[:, :, 2] > 0), "the coupled auto cases must keep mu_k active, or the mu faults cannot show"
    for fault in FAULTS:
        if fault in FREE_FAULTS:
            got, _ = group_model(d, psf, M, N, mu=COUPLED["mu"], rho=COUPLED["rho"], iterations=3, weights=w, nu=COUPLED["nu_free"], coupled=True,
                                 fault=fault)
            e = max(rel_err(got[c], free[c]) for c in range(3))
            print("TVFB\tfault\t%dx%d win %dx%d free %s\terr=%.3g" % (M, N, rows, cols, fault, e))
            assert e > 10 * TVFB_TOL, (fault, e)
        got, _ = group_model(d, psf, M, N, sigmas=sig, rho=COUPLED["rho"], iterations=3, weights=w, nu=COUPLED["nu_auto"], coupled=True, fault=fault)
        e = max(rel_err(got[c], auto[c]) for c in range(3))
        print("TVFB\tfault\t%dx%d win %dx%d auto %s\terr=%.3g" % (M, N, rows, cols, fault, e))
        assert e > 10 * TVFB_AUTO_TOL, (fault, e)


def test_single_precision_class():
    """the coupled model in float32 / complex64 (sums in double) against its float64 form on the GPU test's cases: the arithmetic
    class the device is held to"""
    from _tvauto_model import trace_err
    for M, N, rows, cols in COUPLED_PLANS[:2]:
        d, psf, w = coupled_case(M, N, rows, cols)
        sig = [f32(s) for s in COUPLED_SIGMAS]
        for n in (3, 30):
            a, _ = group_model(d, psf, M, N, mu=COUPLED["mu"], rho=COUPLED["rho"], iterations=n, weights=w, nu=COUPLED["nu_free"], coupled=True)
            b, _ = group_model(d, psf, M, N, mu=COUPLED["mu"], rho=COUPLED["rho"], iterations=n, weights=w, nu=COUPLED["nu_free"], coupled=True,
                               dtype=np.float32)
            e = max(rel_err(b[c], a[c]) for c in range(3))
            a, ta = group_model(d, psf, M, N, sigmas=sig, rho=COUPLED["rho"], iterations=n, weights=w, nu=COUPLED["nu_auto"], coupled=True)
            b, tb = group_model(d, psf, M, N, sigmas=sig, rho=COUPLED["rho"], iterations=n, weights=w, nu=COUPLED["nu_auto"], coupled=True,
                                dtype=np.float32)
            ea = max(rel_err(b[c], a[c]) for c in range(3))
            et = max(trace_err(tb[c], ta[c]) for c in range(3))
            print("TVFB\tfloat32 model\t%dx%d win %dx%d n=%d\tfree %.3g auto %.3g trace %.3g" % (M, N, rows, cols, n, e, ea, et))
            assert 1e-8 < e < 1e-5 and 1e-8 < ea < 1e-5 and et < 1e-4


def test_coupled_free_beats_channelwise():
    """the colour crop of the header: the coupled free model at its best mu beats the channel-wise one at its best mu by at least
    half the measured gain"""
    S, rows, cols, noise, at = 256, 200, 200, 0.05, (28, 40)
    truth = colour_blocks(S, S, 3, 3)
    psf = centred_psf(line_psf(), S, S)
    Hs = np.fft.rfft2(psf.astype(np.float64))
    blurred = np.stack([np.fft.irfft2(np.fft.rfft2(truth[c]) * Hs, s=(S, S)) for c in range(3)])
    noisy = blurred + noise * np.random.default_rng(9).standard_normal(blurred.shape)
    d = noisy[:, at[0]:at[0] + rows, at[1]:at[1] + cols].astype(np.float32)
    tr = truth[:, at[0]:at[0] + rows, at[1]:at[1] + cols]
    best = {}
    for coupled in (False, True):
        best[coupled] = {mu: psnr(group_model(d, psf, S, S, mu=mu, rho=2.0, iterations=60, coupled=coupled)[0], tr) for mu in (20.0, 40.0, 80.0)}
    cw, cp = max(best[False].values()), max(best[True].values())
    print("TVFB\tquality (model)\tblurred %.2f dB, channel-wise %s, coupled %s, gain %.3f dB"
          % (psnr(d, tr), {k: round(v, 2) for k, v in best[False].items()}, {k: round(v, 2) for k, v in best[True].items()}, cp - cw))
    assert cp - cw >= MEASURED_GAIN_DB / 2


FUNCS = ("fdr_tv_deconv_free_batch_f32", "fdr_tv_deconv_free_batch_f32_dev", "fdr_tv_deconv_auto_batch_f32", "fdr_tv_deconv_auto_batch_f32_dev")


def _struct_fields(header, name):
    m = re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}\s*%s\s*;" % (name, name), header)
    assert m, name + " is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return re.findall(r"\b(float|int|double)\s+(\w+)\s*;", body)


def test_symbols_and_surface(fdr):
    header = open(os.path.join(ROOT, "include", "fdr.h")).read()
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int, "double": ctypes.c_double}
    fields = _struct_fields(header, "fdr_tv_free_batch_params")
    assert [(n, ctype[t]) for t, n in fields] == list(fdr.TvFreeBatchParams._fields_)
    assert [n for _, n in fields] == [n for n, _ in fdr.TvFreeParams._fields_] + ["coupling"]
    assert ctypes.sizeof(fdr.TvFreeBatchParams) == 40
    fields = _struct_fields(header, "fdr_tv_auto_batch_params")
    assert [(n, ctype[t]) for t, n in fields] == list(fdr.TvAutoBatchParams._fields_)
    assert [n for _, n in fields] == [n for n, _ in fdr.TvAutoParams._fields_] + ["coupling"]
    assert ctypes.sizeof(fdr.TvAutoBatchParams) == 44
    assert re.search(r"#define\s+FDR_VERSION\s+300\b", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    sig = inspect.signature(fdr.Plan.tv_deconv_free_batch).parameters
    assert list(sig) == ["self", "imgs", "mu", "rho", "iterations", "weights", "nu", "anisotropic", "nonneg", "norm_area", "full_plane", "coupled"]
    assert [sig[k].default for k in list(sig)[3:]] == [2.0, 50, None, 0.0, False, False, fdr.NORM_NONE, False, False]
    sig = inspect.signature(fdr.Plan.tv_deconv_auto_batch).parameters
    assert list(sig) == ["self", "imgs", "sigma", "rho", "iterations", "weights", "tau", "nu", "anisotropic", "nonneg", "norm_area", "full_plane",
                         "sigmas", "coupled"]
    assert [sig[k].default for k in list(sig)[2:]] == [0.0, 2.0, 100, None, 0.0, 0.0, False, False, fdr.NORM_NONE, False, None, False]
    sig = inspect.signature(fdr.Plan.tv_deconv_free_batch_dev).parameters
    assert list(sig)[:13] == ["self", "d_imgs", "img_pitch", "count", "rows", "cols", "stride", "d_out", "out_pitch", "out_stride", "mu", "rho",
                              "iterations"]
    assert (sig["d_weights"].default, sig["wstride"].default, sig["coupled"].default, sig["stream"].default) == (None, 0, False, None)
    sig = inspect.signature(fdr.Plan.tv_deconv_auto_batch_dev).parameters
    assert list(sig)[:13] == ["self", "d_imgs", "img_pitch", "count", "rows", "cols", "stride", "d_out", "out_pitch", "out_stride", "sigma", "rho",
                              "iterations"]
    assert (sig["sigmas"].default, sig["d_trace"].default, sig["trace_pitch"].default, sig["coupled"].default) == (None, None, 0, False)
    for f in (fdr.tvDeblurFree_RGB, fdr.tvDeblurAuto_RGB):
        sig = inspect.signature(f).parameters
        assert list(sig)[-1] == "coupled" and sig["coupled"].default is False
    cxx = open(os.path.join(ROOT, "include", "fft", "fft.hpp")).read()
    assert "fdr_tv_deconv_free_batch_f32(" in cxx and "fdr_tv_deconv_auto_batch_f32(" in cxx
    for name in ("tvDeblurFree_RGB", "tvDeblurAuto_RGB"):  # both overloads of each end with the new argument
        heads = re.findall(r"inline [^\n]*\b%s\((?:[^{;]|\n)*?\{" % name, cxx)
        assert len(heads) == 2 and all(re.search(r"bool coupled = false\) \{$", h) for h in heads), (name, heads)


def test_null_arguments_are_refused_before_any_device_work(fdr):
    """a null plan, images, output or params: FDR_ERR_ARG from all four entry points with the function's name, on a machine without
    a device too; a negative count is refused and count = 0 returns FDR_OK before anything else is looked at"""
    L = fdr.lib
    img = np.zeros((2, 8, 32), dtype=np.float32)
    out = np.zeros((2, 8, 32), dtype=np.float32)
    fp = fdr.TvFreeBatchParams(10.0, 2.0, 0.0, 1, 0, 0, 0, 8, 32, 0)
    ap = fdr.TvAutoBatchParams(0.01, 0.0, 2.0, 0.0, 1, 0, 0, 0, 8, 32, 0)

    def free(h, i, o, p, dev, count=2):
        if dev:
            return L.fdr_tv_deconv_free_batch_f32_dev(h, i, 256, count, 8, 32, 32, None, 0, o, 256, 32, p, None)
        return L.fdr_tv_deconv_free_batch_f32(h, i, 256, count, 8, 32, 32, None, 0, o, 256, 32, p)

    def auto(h, i, o, p, dev, count=2):
        if dev:
            return L.fdr_tv_deconv_auto_batch_f32_dev(h, i, 256, count, 8, 32, 32, None, 0, o, 256, 32, p, None, None, 0, None)
        return L.fdr_tv_deconv_auto_batch_f32(h, i, 256, count, 8, 32, 32, None, 0, o, 256, 32, p, None, None, None, 0)

    for call, prm, base in ((free, fp, "fdr_tv_deconv_free_batch_f32"), (auto, ap, "fdr_tv_deconv_auto_batch_f32")):
        for dev in (False, True):
            name = (base + "_dev" if dev else base).encode()
            for h, i, o, p in ((None, img.ctypes.data, out.ctypes.data, ctypes.byref(prm)), (1, None, out.ctypes.data, ctypes.byref(prm)),
                               (1, img.ctypes.data, None, ctypes.byref(prm)), (1, img.ctypes.data, out.ctypes.data, None)):
                assert call(h, i, o, p, dev) == -1
                assert name + b": null argument" in L.fdr_last_error()
            assert call(1, img.ctypes.data, out.ctypes.data, ctypes.byref(prm), dev, count=-1) == -1
            assert name + b": negative count" in L.fdr_last_error()
            assert call(1, None, None, ctypes.byref(prm), dev, count=0) == 0
