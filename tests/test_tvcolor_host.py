"""CPU checks of the colour / batched total-variation model (tests/_tvcolor_model.py) before it judges the GPU (test_tvcolor_gpu.py):
the uncoupled model is tv_model per channel and the coupled one with a single channel is tv_model, exactly; the joint shrinkage is
the proximal map of t ||.||_2 on R^(2C); the coupled objective falls and plateaus; the delta-PSF fixed point; the error class of single
precision; injected faults far outside the device tolerance on every shape the GPU test uses; the restoration margin of vectorial TV
over channel-wise TV; and the C ABI / Python surface of fdr_tv_deconv_batch_f32*."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, blur_model, centred_psf, dense_psf, op_spectrum, psnr, rel_err
from _tv_model import TV_TOL, blur_plane, tv_model
import _tvcolor_model as tc
from test_tv_host import line_psf

MU, RHO = 200.0, 10.0  # the GPU cases: threshold 0.1, below the texture of colour_images


def gpu_case(M, N, rows, cols, C):
    """(images [C, rows, cols] float32, psf) of a plan of _tvcolor_model.GPU_PLANS, shared with test_tvcolor_gpu.py: a dense 5 x 5
    PSF (it fits the smallest plan), centred for a cropped window as test_tv_gpu.py does"""
    full = rows is None
    rows, cols = (M, N) if full else (rows, cols)
    psf = dense_psf(5, 5)
    return tc.colour_images(M, N, rows, cols, C, M + 3 * N + C), psf if full else centred_psf(psf, M, N)


@pytest.mark.parametrize("aniso", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_uncoupled_is_tv_model_per_channel(aniso, dtype):
    imgs, psf = gpu_case(64, 256, 50, 200, 3)
    for area, nonneg in ((NORM_NONE, False), (NORM_CROPPED, True), (NORM_PADDED, False)):
        got = tc.tvcolor_model(imgs, psf, 64, 256, MU, RHO, 5, False, nonneg, area, dtype, anisotropic=aniso)
        for c in range(3):
            assert np.array_equal(got[c], tv_model(imgs[c], psf, 64, 256, MU, RHO, 5, aniso, nonneg, area, dtype)), (c, area)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_coupled_single_channel_is_tv_model(dtype):
    imgs, psf = gpu_case(64, 256, 50, 200, 1)
    for n in (0, 1, 5):
        assert np.array_equal(tc.tvcolor_model(imgs, psf, 64, 256, MU, RHO, n, True, dtype=dtype)[0], tv_model(imgs[0], psf, 64, 256, MU, RHO, n, dtype=dtype))


def test_joint_shrinkage_is_the_proximal_map():
    """argmin_z t ||z||_2 + ||z - g||^2 / 2 on R^(2C), C = 2, by brute force: the minimiser lies on the ray of g (any component
    across it only adds to both terms), so a fine grid of the plane spanned by g and one direction across it, around the closed
    form, finds it -- as test_tv_host.py does for the two components of one channel"""
    t = 0.5
    grid = np.linspace(-2.5, 2.5, 1001)
    a, b = np.meshgrid(grid, grid, indexing="ij")  # z = a e + b f, e = g / |g|, f across g
    rng = np.random.default_rng(3)
    for g in (np.array([1.3, -0.4, 0.2, 0.9]), np.array([0.2, 0.3, -0.1, 0.1]), np.array([-0.9, 1.1, 1.0, -1.2]), np.array([0.3, 0.0, 0.4, 0.0])):
        n = float(np.linalg.norm(g))
        e = g / n
        f = rng.standard_normal(4)
        f -= e * np.dot(f, e)
        f /= np.linalg.norm(f)
        cost = t * np.sqrt(a * a + b * b) + 0.5 * ((a - n) ** 2 + b * b)  # |z - g|^2 = (a - |g|)^2 + b^2 in this basis
        k = np.unravel_index(np.argmin(cost), cost.shape)
        brute = a[k] * e + b[k] * f
        gx, gy = g[0::2].reshape(2, 1, 1), g[1::2].reshape(2, 1, 1)
        zx, zy = tc.joint_shrink(gx, gy, t)
        z = np.array([zx[0, 0, 0], zy[0, 0, 0], zx[1, 0, 0], zy[1, 0, 0]])
        assert np.max(np.abs(z - brute)) <= 0.0051, (g, z, brute)
        assert abs(np.linalg.norm(z) - max(n - t, 0)) <= 1e-12  # shortened by t, or 0
    # and it is not the channel-wise map: the channels share the factor
    gx, gy = np.array([1.0, 0.1]).reshape(2, 1, 1), np.array([0.0, 0.0]).reshape(2, 1, 1)
    zx, _ = tc.joint_shrink(gx, gy, t)
    assert zx[1, 0, 0] > 0 and tc.joint_shrink(gx, gy, t, "channelwise")[0][1, 0, 0] == 0


def coupled_objective(x, d_pad, H, mu):
    r = np.stack([blur_plane(x[c], H) - d_pad[c] for c in range(x.shape[0])])
    return 0.5 * mu * float(np.sum(r * r)) + tc.vtv_value(x)


def test_coupled_objective_falls_and_plateaus():
    M, N, mu, rho = 64, 64, 300.0, 2.0
    truth = tc.colour_blocks(M, N, 3, 1)
    psf = centred_psf(line_psf(7, 30.0), M, N)
    d = np.stack([blur_model(truth[c], psf, M, N) for c in range(3)]) + np.random.default_rng(0).normal(0, 0.01, truth.shape)
    H = op_spectrum(psf, M, N)
    obj, res = [], []
    for x, zx, zy in tc.tvcolor_iterates(d, psf, M, N, mu, rho, 300, True):
        obj.append(coupled_objective(x, d, H, mu))
        if zx is not None:
            res.append(float(np.sqrt(sum(np.sum((tc.dx(x[c]) - zx[c]) ** 2 + (tc.dy(x[c]) - zy[c]) ** 2) for c in range(3)))))
    assert obj[300] < 0.5 * obj[0]
    assert abs(obj[300] - obj[250]) <= 1e-3 * obj[300]  # a plateau
    assert min(obj[200:]) >= obj[300] * (1 - 1e-3)
    assert res[-1] <= 1e-2 * max(res) and res[-1] <= 0.05
    # the channel-wise iteration ends higher in the coupled objective: the two minimise different things
    xc = None
    for xc, _, _ in tc.tvcolor_iterates(d, psf, M, N, mu, rho, 300, False):
        pass
    assert coupled_objective(xc, d, H, mu) > obj[300] * (1 + 1e-4)


def test_delta_psf_constant_channels_are_a_fixed_point():
    M, N = 32, 64
    c = np.empty((3, M, N))
    c[:] = np.array([0.37, 0.05, 0.9])[:, None, None]
    assert np.allclose(tc.tvcolor_model(c, np.ones((1, 1)), M, N, 10.0, 2.0, 20, True), c, atol=1e-13)
    assert np.array_equal(tc.tvcolor_model(c[:, :20, :33], np.ones((1, 1)), M, N, 10.0, 2.0, 0, True), c[:, :20, :33])  # n = 0: pad(d)


def test_single_precision_class():
    """the coupled model in float32 / complex64 against float64: the arithmetic class of the device, within TV_TOL itself"""
    worst = {}
    for M, N, rows, cols in ((256, 256, None, None), (128, 512, 100, 333)):
        imgs, psf = gpu_case(M, N, rows, cols, 3)
        for n in (3, 30, 100):
            e = rel_err(tc.tvcolor_model(imgs, psf, M, N, MU, RHO, n, True, dtype=np.float32), tc.tvcolor_model(imgs, psf, M, N, MU, RHO, n, True))
            worst[n] = max(worst.get(n, 0.0), e)
    print("TVC\tfloat32 coupled model against float64\t%s" % {n: "%.3g" % e for n, e in worst.items()})
    assert max(worst.values()) <= TV_TOL, worst


@pytest.mark.parametrize("M,N,rows,cols", tc.GPU_PLANS, ids=["%dx%d" % (p[0], p[1]) for p in tc.GPU_PLANS])
def test_faults_are_visible_on_every_gpu_shape(M, N, rows, cols):
    """each fault model moves the coupled result by more than 100x the device tolerance at every plan of the GPU test and every
    channel count above one used there -- the tile-edge fault too, at the one-tile plan (which wraps onto itself) and the two-tile
    one; the coupled and the uncoupled results are as far apart (the GPU test's guard against a silent fall-through)"""
    low = {}
    for C in (2, 3, 4, 8):
        imgs, psf = gpu_case(M, N, rows, cols, C)
        want = tc.tvcolor_model(imgs, psf, M, N, MU, RHO, 3, True)
        for fault in tc.FAULTS:
            e = rel_err(tc.tvcolor_model(imgs, psf, M, N, MU, RHO, 3, True, fault=fault), want)
            low[fault] = min(low.get(fault, 1e9), e)
            assert e > 100 * TV_TOL, (fault, C, e)
        assert rel_err(tc.tvcolor_model(imgs, psf, M, N, MU, RHO, 3, False), want) > 100 * TV_TOL
        assert rel_err(tc.tvcolor_model(imgs, psf, M, N, MU, RHO, 2, True), want) > 100 * TV_TOL  # one iteration fewer
    print("TVC\tfaults\t%dx%d\tsmallest shift %s" % (M, N, {f: "%.3g" % e for f, e in low.items()}))


def test_fault_models_are_what_they_say():
    imgs, psf = gpu_case(64, 256, None, None, 3)
    unc = tc.tvcolor_model(imgs, psf, 64, 256, MU, RHO, 3, False)
    assert np.array_equal(tc.tvcolor_model(imgs, psf, 64, 256, MU, RHO, 3, True, fault="channelwise"), unc)
    one = tc.tvcolor_model(imgs[:1], psf, 64, 256, MU, RHO, 3, True)
    assert np.array_equal(tc.tvcolor_model(imgs, psf, 64, 256, MU, RHO, 3, True, fault="first_channel")[0], one[0])
    assert tc.tile_shape(8, 32) == (8, 32) and tc.tile_shape(16, 512) == (16, 256) and tc.tile_shape(64, 256) == (16, 256)
    assert tc.tile_shape(256, 32) == (128, 32) and tc.tile_shape(128, 512) == (16, 256) and tc.tile_shape(4096, 4096) == (16, 256)
    # the tile-edge fault is gone where no second channel exists
    assert np.array_equal(tc.tvcolor_model(imgs[:1], psf, 64, 256, MU, RHO, 3, True, fault="halo_own_norm"), one)


QUALITY = dict(M=256, N=256, C=3, seed=0, psf=(11, 30.0), rho=2.0, n=100, mus=np.logspace(np.log10(5.0), np.log10(400.0), 13))
QUALITY_MARGIN_DB = 0.5


def quality_gain(sigma):
    """(best coupled PSNR, its mu, best channel-wise PSNR, its mu) over the mu grid, PSNR over all channels"""
    q = QUALITY
    truth = tc.colour_blocks(q["M"], q["N"], q["C"], q["seed"])
    psf = centred_psf(line_psf(*q["psf"]), q["M"], q["N"])
    d = np.stack([blur_model(truth[c], psf, q["M"], q["N"]) for c in range(q["C"])]) + np.random.default_rng(1).normal(0, sigma, truth.shape)
    out = []
    for coupled in (True, False):
        ps = [psnr(tc.tvcolor_model(d, psf, q["M"], q["N"], mu, q["rho"], q["n"], coupled), truth) for mu in q["mus"]]
        out += [max(ps), float(q["mus"][int(np.argmax(ps))])]
    return out


@pytest.mark.parametrize("sigma", [0.02, 0.05, 0.10])
def test_vectorial_tv_beats_channelwise_tv(sigma):
    """256 x 256, three channels of colour_blocks (shared rectangles, per-channel levels), an 11 px / 30 degree line PSF, Gaussian noise
    of deviation sigma, rho = 2, 100 iterations, mu on a 13-point log grid from 5 to 400: the best-mu PSNR (over all channels) of the
    coupled model must lie at least 0.5 dB above the best-mu PSNR of the channel-wise one.  Measured with this model: 1.23 dB at
    sigma 0.02 (38.38 against 37.14 dB, mu 92.8 and 133.7), 1.07 dB at 0.05 (32.74 against 31.68 dB, mu 31.0 both) and 0.84 dB at 0.10
    (29.09 against 28.25 dB, mu 10.4 and 15.0)."""
    pc, mc, pu, mu_u = quality_gain(sigma)
    print("TVC\tquality (model)\tsigma %.2f: coupled %.2f dB at mu %.1f, channel-wise %.2f dB at mu %.1f, gain %.2f dB" % (sigma, pc, mc, pu, mu_u, pc - pu))
    assert pc >= pu + QUALITY_MARGIN_DB, (sigma, pc, pu)
    assert mc <= mu_u  # the coupled optimum lies at a smaller mu


TVB_FUNCS = ("fdr_tv_deconv_batch_f32", "fdr_tv_deconv_batch_f32_dev")


def test_symbols_and_surface(fdr):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fdr.h")).read()
    assert re.search(r"typedef\s+struct\s+fdr_tv_batch_params\s*\{[^}]*float\s+mu;[^}]*float\s+rho;[^}]*int\s+iterations;[^}]*int\s+anisotropic;"
                     r"[^}]*int\s+nonneg;[^}]*int\s+norm_area;[^}]*int\s+coupling;[^}]*\}\s*fdr_tv_batch_params\s*;", header)
    assert re.search(r"#define\s+FDR_TV_COUPLE_NONE\s+0\b", header) and re.search(r"#define\s+FDR_TV_COUPLE_CHANNELS\s+1\b", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in TVB_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    assert ctypes.sizeof(fdr.TvBatchParams) == 28
    assert [f[0] for f in fdr.TvBatchParams._fields_] == ["mu", "rho", "iterations", "anisotropic", "nonneg", "norm_area", "coupling"]
    assert (fdr.TV_COUPLE_NONE, fdr.TV_COUPLE_CHANNELS) == (0, 1)
    for meth in ("tv_deconv_batch", "tv_deconv_batch_dev"):
        assert callable(getattr(fdr.Plan, meth)), meth
    sig = inspect.signature(fdr.Plan.tv_deconv_batch).parameters
    assert list(sig)[:3] == ["self", "imgs", "mu"]
    assert (sig["rho"].default, sig["iterations"].default, sig["anisotropic"].default, sig["nonneg"].default, sig["norm_area"].default,
            sig["coupled"].default) == (2.0, 50, False, False, fdr.NORM_NONE, False)
    sig = inspect.signature(fdr.Plan.tv_deconv_batch_dev).parameters
    assert list(sig)[:10] == ["self", "d_imgs", "img_pitch", "count", "rows", "cols", "stride", "d_out", "out_pitch", "out_stride"]
    assert sig["coupled"].default is False and sig["stream"].default is None
    sig = inspect.signature(fdr.tvDeblur_RGB).parameters
    assert list(sig)[:3] == ["channels", "psf", "mu"]
    assert (sig["rho"].default, sig["iterations"].default, sig["nonneg"].default, sig["device"].default, sig["norm_area"].default,
            sig["coupled"].default) == (2.0, 50, False, 0, fdr.NORM_NONE, False)
    # the two C++ overloads and the CLI option
    hpp = open(os.path.join(root, "include", "fft", "fft.hpp")).read()
    assert len(re.findall(r"inline void tvDeblur_RGB\([^)]*bool coupled = false\)", hpp)) == 2
    assert "--tv-color" in open(os.path.join(root, "tools", "cli", "gpu.cpp")).read()


def test_refusals_without_a_device(fdr):
    """a null plan is refused before anything else (the other refusals need a plan: test_tvcolor_gpu.py)"""
    L = fdr.lib
    prm = fdr.TvBatchParams(10.0, 2.0, 1, 0, 0, fdr.NORM_NONE, fdr.TV_COUPLE_NONE)
    buf = np.zeros(64, dtype=np.float32)
    assert L.fdr_tv_deconv_batch_f32(None, buf.ctypes.data, 64, 1, 8, 8, 8, buf.ctypes.data, 64, 8, ctypes.byref(prm)) == -1
    assert L.fdr_tv_deconv_batch_f32_dev(None, buf.ctypes.data, 64, 1, 8, 8, 8, buf.ctypes.data, 64, 8, ctypes.byref(prm), None) == -1
