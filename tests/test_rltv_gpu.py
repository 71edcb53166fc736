"""Richardson-Lucy with a total-variation prior (fdr_richardson_lucy_tv_f32*, fdr_rl_tv_factor_f32_dev) on the MI355X against the
float64 model of tests/_rltv_model.py: the factor kernel at the edges of its tile, the bits of the unregularised calls through the
new path, both forms against the model in the regime where a comparison step by step means something, restoration quality, and
hygiene (determinism, isolation from every other call of the plan, refusals, allocations, pass names, the CLI).  Each case prints
an `RLTV` line with its measured values (pytest -s)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, dense_psf, normalize, psnr, rel_err, smooth_image
from _rlfree_model import SIGMA, SIGMA_MARGIN, sigma_margin
from _rltv_model import (QUALITY_EPS, QUALITY_LAMBDA, QUALITY_N, RLTV_FACTOR_TOL, RLTV_FREE_TOL, RLTV_TOL, quality_case, quality_run,
                         rltv_free_state, rltv_model, tv_factor)
from _spectral import tone_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_EPS = float(np.finfo(np.float32).eps)


def _tile():
    """(Th, Tw): the pixels of one workgroup of the factor kernel, read from its source (a thread owns 4 x 4)"""
    src = open(os.path.join(ROOT, "parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd", "csrc", "fdr_rltv.hip")).read()
    m = re.search(r"kRltvTX\s*=\s*(\d+)\s*,\s*kRltvTY\s*=\s*(\d+)", src)
    return 4 * int(m.group(2)), 4 * int(m.group(1))


TH, TW = _tile()
SHAPES = [(1, 1), (1, 37), (37, 1), (3, 5), (TH - 1, TW + 1), (TH, TW), (TH + 1, 2 * TW - 1), (2 * TH + 1, 2 * TW + 1)]
PARAMS = [(0.125, 1e-3), (0.01, 1e-3), (0.01, 0.05), (0.125, 1e-6)]


def _planes(R, C, seed):
    """the inputs of the factor kernel: random, smooth, flat, a tiny-gradient plane and a counts-scale plane, float32"""
    rng = np.random.default_rng(seed)
    smooth = smooth_image(max(R, 2), max(C, 2), seed)[:R, :C]
    return {"random": rng.random((R, C)).astype(np.float32), "smooth": smooth, "flat": np.full((R, C), 0.37, dtype=np.float32),
            "tiny": (0.5 + 1e-3 * rng.random((R, C))).astype(np.float32), "counts": (1000 * rng.random((R, C))).astype(np.float32)}


def _factor_dev(fdr, u, w, lam, eps, stride, ostride, offset=0, side_stream=False):
    """fdr_rl_tv_factor_f32_dev on device copies of u (and w) with row stride `stride`, every pointer `offset` floats past a 256-byte
    boundary; the output window lies inside a NaN-filled buffer (one row above, one below, the columns beyond cols), which must
    stay NaN"""
    import torch
    R, C = u.shape

    def up(a):
        host = np.full(R * stride + offset, 7.0, dtype=np.float32)  # the padding must not matter
        view = host[offset:].reshape(R, stride)
        view[:, :C] = a
        return torch.from_numpy(host).cuda()

    d_u = up(u)
    d_w = up(w) if w is not None else None
    d_out = torch.full(((R + 2) * ostride + offset,), float("nan"), dtype=torch.float32, device="cuda")
    args = (d_u.data_ptr() + 4 * offset, R, C, stride, d_out.data_ptr() + 4 * (offset + ostride), ostride, lam, eps,
            d_w.data_ptr() + 4 * offset if d_w is not None else None)
    torch.cuda.synchronize()
    if side_stream:
        s = torch.cuda.Stream()
        fdr.rl_tv_factor_dev(*args, stream=s.cuda_stream)
        s.synchronize()
    else:
        fdr.rl_tv_factor_dev(*args)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()[offset:].reshape(R + 2, ostride)
    assert np.all(np.isnan(out[0])) and np.all(np.isnan(out[-1])) and np.all(np.isnan(out[1:-1, C:])), "a store landed outside the output window"
    return out[1:-1, :C]


def _factor_errors(fdr, u, w, lam, eps, got):
    """(device error, float32 CPU error) against the float64 model on the same float32 inputs, relative to max(w) (1 without w)"""
    want = tv_factor(u, lam, eps, w=w)
    scale = 1.0 if w is None else max(float(np.max(w)), 1e-30)
    cpu32 = float(np.max(np.abs(tv_factor(u, lam, eps, w=w, dtype=np.float32).astype(np.float64) - want))) / scale
    return float(np.max(np.abs(got.astype(np.float64) - want))) / scale, cpu32


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_factor_kernel_at_its_edges(fdr, shape):
    R, C = shape
    c4 = (C + 3) // 4 * 4
    layouts = [("tight", C, C, 0), ("loose", C + 3, C + 5, 0), ("loose, 16-byte rows", c4 + 4, c4 + 8, 0)]
    if shape == (TH + 1, 2 * TW - 1):
        layouts.append(("pointers offset by one float", c4, c4, 1))
    rng = np.random.default_rng(R * 1000 + C)
    wz = rng.random((R, C)).astype(np.float32)
    wz[rng.random((R, C)) < 0.2] = 0
    bad, worst, worst32 = [], 0.0, 0.0
    for kind, u in _planes(R, C, R + C).items():
        for what, stride, ostride, offset in layouts:
            for w in (None, wz):
                for k, (lam, eps) in enumerate(PARAMS):
                    side = what == "tight" and kind == "random" and k == 0
                    got = _factor_dev(fdr, u, w, lam, eps, stride, ostride, offset, side_stream=side)
                    e, cpu32 = _factor_errors(fdr, u, w, lam, eps, got)
                    worst, worst32 = max(worst, e), max(worst32, cpu32)
                    tag = "%dx%d %s %s w=%s lambda=%g eps=%g" % (R, C, kind, what, w is not None, lam, eps)
                    if w is not None and not np.all(got[w == 0] == 0):
                        bad.append("%s: a zero of w did not stay zero" % tag)
                    if kind == "flat" and not np.array_equal(got, np.ones_like(got) if w is None else w):
                        bad.append("%s: a flat plane must give the factor w exactly" % tag)
                    if not e <= RLTV_FACTOR_TOL:
                        bad.append("%s: error %.3g > %s" % (tag, e, RLTV_FACTOR_TOL))
                    if not e <= 10 * max(cpu32, F32_EPS):
                        bad.append("%s: error %.3g above 10x the float32 CPU run's %.3g" % (tag, e, cpu32))
    print("RLTV\tfactor\t%dx%d\tworst=%.3g\tcpu32 worst=%.3g" % (R, C, worst, worst32))
    assert not bad, "\n".join(bad[:20])


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def _mask(rows, cols, seed, zero=0.1):
    return (np.random.default_rng(seed).random((rows, cols)) >= zero).astype(np.float32)


def _case(fdr, name):
    """M, N, rows, cols, stride, psf, weights (free form only) of the named case"""
    motion = fdr.motionBlurKernel(15, 30.0)
    if name == "64x128 win 37x101 masked":
        return 64, 128, 37, 101, 103, dense_psf(5, 5), _mask(37, 101, 6)
    if name == "256 win 200x151":
        return 256, 256, 200, 151, 163, dense_psf(11), None
    if name == "512 full plane":
        return 512, 512, 512, 512, 512, centred_psf(motion, 512, 512), None
    if name == "2048x512 win 2000x500":
        return 2048, 512, 2000, 500, 500, centred_psf(motion, 2048, 512), None
    raise KeyError(name)


PLANS = ["64x128 win 37x101 masked", "256 win 200x151", "512 full plane"]


def _image(M, N, rows, cols):
    img = np.clip(tone_image(M, N, M + 17 * N, rows, cols), 0, None) + np.float32(0.05)
    img[: max(1, rows // 16), : max(1, cols // 16)] -= np.float32(0.5)  # negative pixels: the forms use d+
    return img


class _Dev:
    """device copies of one case's input (row stride `stride`) and weights (stride + 1), and a NaN-guarded output"""

    def __init__(self, img, weights, stride):
        import torch
        self.rows, self.cols, self.stride = img.shape[0], img.shape[1], stride
        src = np.zeros((self.rows, stride), dtype=np.float32)
        src[:, :self.cols] = img
        self.d_in = torch.from_numpy(src).cuda()
        self.d_w, self.ws = None, 0
        if weights is not None:
            self.ws = stride + 1
            w = np.full((self.rows, self.ws), 7.0, dtype=np.float32)  # the padding must not be read
            w[:, :self.cols] = weights
            self.d_w = torch.from_numpy(w).cuda()

    def run(self, call, out_rows, out_cols):
        """call(d_in, d_w, wstride, d_out, out_stride) -> the out_rows x out_cols window; the guard must stay NaN"""
        import torch
        out_stride = out_cols + 3
        d_out = torch.full((out_rows + 1, out_stride), float("nan"), dtype=torch.float32, device="cuda")
        call(self.d_in.data_ptr(), self.d_w.data_ptr() if self.d_w is not None else None, self.ws, d_out.data_ptr(), out_stride)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert np.all(np.isnan(out[:out_rows, out_cols:])) and np.all(np.isnan(out[out_rows:, :])), "a store landed outside the output window"
        return out[:out_rows, :out_cols]


def _tv(p, dev, n, lam, eps, free, area=NORM_NONE, orows=None, ocols=None):
    orows, ocols = dev.rows if orows is None else orows, dev.cols if ocols is None else ocols
    return dev.run(lambda i, w, ws, o, os_: p.richardson_lucy_tv_dev(i, dev.rows, dev.cols, dev.stride, o, os_, n, lam, eps, free_boundary=free,
                                                                     d_weights=w if free else None, wstride=ws if free else 0, norm_area=area,
                                                                     out_rows=orows, out_cols=ocols), orows, ocols)


def _plain(p, dev, n, area):
    return dev.run(lambda i, w, ws, o, os_: p.richardson_lucy_dev(i, dev.rows, dev.cols, dev.stride, o, os_, n, norm_area=area), dev.rows, dev.cols)


def _free(p, dev, n, area, orows, ocols):
    return dev.run(lambda i, w, ws, o, os_: p.richardson_lucy_free_dev(i, dev.rows, dev.cols, dev.stride, o, os_, n, d_weights=w, wstride=ws,
                                                                       norm_area=area, out_rows=orows, out_cols=ocols), orows, ocols)


@pytest.mark.parametrize("name", PLANS)
def test_the_new_path_gives_the_bits_of_the_old_calls(fdr, name):
    """lambda = 0.1 with eps = 1e18 makes g exactly 1 in float32, so the factor is exactly w: the regularised call, through the
    factor kernel and the weighted update, must return the bits of fdr_richardson_lucy_f32_dev and _free_f32_dev; lambda = 0, which
    calls those drivers, as well"""
    M, N, rows, cols, stride, psf, w = _case(fdr, name)
    img = _image(M, N, rows, cols)
    dev = _Dev(img, w, stride)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        for n in (0, 1, 2, 5, 30):
            for area in (NORM_NONE, NORM_CROPPED, NORM_PADDED):
                ref = _plain(p, dev, n, area)
                assert np.array_equal(ref, _tv(p, dev, n, 0.1, 1e18, False, area)), ("plain", n, area)
                assert np.array_equal(ref, _tv(p, dev, n, 0.0, 0.0, False, area)), ("plain, lambda 0", n, area)
                for orows, ocols in ((rows, cols), (M, N)):
                    ref = _free(p, dev, n, area, orows, ocols)
                    assert np.array_equal(ref, _tv(p, dev, n, 0.1, 1e18, True, area, orows, ocols)), ("free", n, area, orows, ocols)
                    assert np.array_equal(ref, _tv(p, dev, n, 0.0, 0.0, True, area, orows, ocols)), ("free, lambda 0", n, area, orows, ocols)
        # the host form takes the same route
        assert np.array_equal(p.richardson_lucy(img, 5), p.richardson_lucy_tv(img, 5, 0.1, 1e18))
        assert np.array_equal(p.richardson_lucy_free(img, 5, weights=w, full_plane=True),
                              p.richardson_lucy_tv(img, 5, 0.1, 1e18, free_boundary=True, weights=w, full_plane=True))


def _err(got, want, area):
    return rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(got.astype(np.float64) - want)))


def _against_model(fdr, name, runs):
    """both forms of one case against the model for every (lambda, eps, n) of `runs`; returns the failures"""
    M, N, rows, cols, stride, psf, w = _case(fdr, name)
    img = _image(M, N, rows, cols)
    dev = _Dev(img, w, stride)
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        for lam, eps, n in runs:
            # the plain form: the raw estimate on device pointers, the normalised one through the host form
            want = rltv_model(img, psf, M, N, n, lam, eps)
            cpu32 = rel_err(rltv_model(img, psf, M, N, n, lam, eps, dtype=np.float32), want)
            for area, got in ((NORM_NONE, _tv(p, dev, n, lam, eps, False)), (NORM_CROPPED, p.richardson_lucy_tv(img, n, lam, eps, norm_area=NORM_CROPPED))):
                e = _err(got, normalize(want, area, M, N), area)
                what = "%s plain lambda=%g eps=%g n=%d norm=%d" % (name, lam, eps, n, area)
                print("RLTV\tmodel\t%s\terr=%.3g\tcpu32=%.3g" % (what, e, cpu32))
                if not e <= RLTV_TOL:
                    bad.append("%s: error %.3g > %s" % (what, e, RLTV_TOL))
                if area == NORM_NONE and not e <= 10 * max(cpu32, F32_EPS):
                    bad.append("%s: error %.3g above 10x the float32 CPU run's %.3g" % (what, e, cpu32))
            # the free-boundary form: the whole plan raw on device pointers, the window normalised through the host form
            st = rltv_free_state(img, psf, M, N, n, lam, eps, weights=w)
            assert sigma_margin(st["alpha"], SIGMA) >= SIGMA_MARGIN, name
            cpu32 = rel_err(rltv_free_state(img, psf, M, N, n, lam, eps, weights=w, dtype=np.float32)["u"], st["u"])
            for area, got, ref in ((NORM_NONE, _tv(p, dev, n, lam, eps, True, NORM_NONE, M, N), st["u"]),
                                   (NORM_PADDED, p.richardson_lucy_tv(img, n, lam, eps, free_boundary=True, weights=w, norm_area=NORM_PADDED),
                                    st["u"][:rows, :cols])):
                e = _err(got, normalize(ref, area, M, N), area)
                what = "%s free lambda=%g eps=%g n=%d norm=%d" % (name, lam, eps, n, area)
                print("RLTV\tmodel\t%s\terr=%.3g\tcpu32=%.3g" % (what, e, cpu32))
                if not e <= RLTV_FREE_TOL:
                    bad.append("%s: error %.3g > %s" % (what, e, RLTV_FREE_TOL))
                if area == NORM_NONE and not e <= 10 * max(cpu32, F32_EPS):
                    bad.append("%s: error %.3g above 10x the float32 CPU run's %.3g" % (what, e, cpu32))
    return bad


@pytest.mark.parametrize("name", PLANS)
def test_against_model(fdr, name):
    """n <= 3 at eps = 1e-3, and 10 and 30 steps at eps = 0.05: the regime in which the model stays within 1e-6 of its own float32 run"""
    bad = _against_model(fdr, name, [(0.01, 1e-3, n) for n in (1, 2, 3)] + [(0.01, 0.05, n) for n in (10, 30)])
    assert not bad, "\n".join(bad)


def test_against_model_large_rows(fdr):
    """2048 x 512, window 2000 x 500, n = 3: the row kernels of the long plans"""
    bad = _against_model(fdr, "2048x512 win 2000x500", [(0.01, 1e-3, 3)])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("which", ["full", "crop"])
def test_quality_matches_the_model(fdr, which):
    """the two scenes of test_rltv_host.py at n = 100, lambda = 0.01, eps = 1e-3: step for step the arithmetics drift apart here, the
    PSNR must agree to 0.05 dB (the float32 CPU run of the model differs by 0.004 dB)"""
    case = quality_case(which)
    pm = psnr(quality_run(case, QUALITY_N, QUALITY_LAMBDA, QUALITY_EPS), case["truth"])
    with fdr.Plan(case["M"], case["N"], fdr.MODE_FAST) as p:
        p.set_operator_psf(case["psf"])
        got = p.richardson_lucy_tv(case["d"], QUALITY_N, QUALITY_LAMBDA, QUALITY_EPS, free_boundary=case["free"])
        pg = psnr(got, case["truth"])
        base = p.richardson_lucy_free(case["d"], QUALITY_N) if case["free"] else p.richardson_lucy(case["d"], QUALITY_N)
    print("RLTV\tquality\t%s\tmodel %.3f dB, GPU %.3f dB (blurred %.2f dB, without the prior on the GPU %.2f dB)"
          % (which, pm, pg, psnr(case["d"], case["truth"]), psnr(base, case["truth"])))
    assert abs(pg - pm) <= 0.05, (pm, pg)
    assert pg >= psnr(base, case["truth"]) + 3.0


# ---- hygiene --------------------------------------------------------------------------------------------------------------------
def test_determinism_and_forms(fdr):
    M, N, rows, cols, stride, psf, w = _case(fdr, "64x128 win 37x101 masked")
    img = _image(M, N, rows, cols)
    dev = _Dev(img, w, stride)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        for free in (False, True):
            kw = dict(free_boundary=True, weights=w) if free else {}
            a = p.richardson_lucy_tv(img, 7, 0.02, 1e-3, **kw)
            assert np.array_equal(a, p.richardson_lucy_tv(img, 7, 0.02, 1e-3, **kw)), "two runs differ"
            assert np.array_equal(a, _tv(p, dev, 7, 0.02, 1e-3, free)), "host and _dev forms differ"
            assert np.array_equal(a, p.richardson_lucy_tv(img, 7, 0.02, 0.0, **kw)), "eps = 0 is not FDR_RLTV_EPS"
            assert not np.array_equal(a, p.richardson_lucy_tv(img, 7, 0.0, **kw)), "the prior changes nothing"
        full = p.richardson_lucy_tv(img, 7, 0.02, free_boundary=True, weights=w, full_plane=True)
        assert np.array_equal(full[:rows, :cols], p.richardson_lucy_tv(img, 7, 0.02, free_boundary=True, weights=w))
    got = fdr.richardsonLucyTV_myfft(img, psf, 7, 0.02)
    assert fdr._rl_plan_size(rows, cols) == (M, N)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        assert np.array_equal(got, p.richardson_lucy_tv(img, 7, 0.02))


def test_isolation(fdr):
    """Wiener, blur, plain, free-boundary and accelerated RL and TV give the same bytes before and after regularised calls"""
    M, N, rows, cols = 256, 512, 200, 451
    img = tone_image(M, N, 21, rows, cols)
    w = _mask(rows, cols, 3, 0.02)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0)

        def others():
            p.set_psf_motion(15, 30.0, 0.01)
            return [p.wiener(img), p.blur(img), p.blur(img, adjoint=True), p.richardson_lucy(img, 3), p.richardson_lucy_free(img, 3, weights=w),
                    p.richardson_lucy(img, 5, accelerate=True), p.richardson_lucy_free(img, 5, weights=w, accelerate=True),
                    p.tv_deconv(img, 200.0, iterations=3)]

        before = others()  # allocates the other workspaces
        a = p.richardson_lucy_tv(img, 3, 0.02)
        b = p.richardson_lucy_tv(img, 3, 0.02, free_boundary=True, weights=w, norm_area=NORM_PADDED, full_plane=True)
        after = others()
        for k, (x, y) in enumerate(zip(before, after)):
            assert np.array_equal(x, y), "result %d changed after the regularised calls" % k
        assert np.array_equal(a, p.richardson_lucy_tv(img, 3, 0.02))
        assert np.array_equal(b, p.richardson_lucy_tv(img, 3, 0.02, free_boundary=True, weights=w, norm_area=NORM_PADDED, full_plane=True))


def test_later_calls_allocate_nothing(fdr):
    """the first regularised call of a plan makes the workspace (8 M N bytes), later ones nothing: the device's free memory, which the
    first call lowers by the workspace, stays where it is over calls of both forms (the free form's own workspace is made first)"""
    import torch
    M = N = 2048
    img = tone_image(M, N, 5, 2000, 2000)
    dev = _Dev(img, None, 2000)
    ws = 8 * M * N
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0)
        _free(p, dev, 1, NORM_CROPPED, 2000, 2000)
        _tv(p, dev, 1, 0.0, 0.0, False)  # lambda = 0 needs no workspace
        torch.cuda.synchronize()
        f0 = torch.cuda.mem_get_info()[0]
        _tv(p, dev, 1, 0.01, 1e-3, False)
        torch.cuda.synchronize()
        f1 = torch.cuda.mem_get_info()[0]
        _tv(p, dev, 2, 0.01, 1e-3, False, NORM_PADDED)
        _tv(p, dev, 2, 0.01, 1e-3, True, NORM_NONE)
        torch.cuda.synchronize()
        f2 = torch.cuda.mem_get_info()[0]
    print("RLTV\tallocations\tfirst call %d bytes (workspace %d), later calls %d bytes" % (f0 - f1, ws, f1 - f2))
    assert f0 - f1 >= ws // 2, "the first call did not allocate its workspace"
    assert f1 - f2 < ws // 2, "a later call allocated"


def test_refusals(fdr):
    import torch
    L = fdr.lib
    psf = fdr.motionBlurKernel(15, 30.0)
    img = tone_image(64, 64, 3)
    out = np.empty((64, 64), dtype=np.float32)
    w = np.ones((64, 64), dtype=np.float32)

    def prm(n=1, free=0, lam=0.01, eps=1e-3, area=2, sigma=1e-2, orows=8, ocols=8):
        return ctypes.byref(fdr.RlTvParams(n, free, lam, eps, area, sigma, orows, ocols))

    def call(p, rows=8, cols=8, stride=64, wp=None, ws=64, op=None, ostride=64, pr=None):
        return L.fdr_richardson_lucy_tv_f32(p._h, img.ctypes.data, rows, cols, stride, wp, ws, out.ctypes.data if op is None else op, ostride,
                                            prm() if pr is None else pr)

    for M, N, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (64, 64, fdr.MODE_FAST, fdr.FLAG_SIMPLE_PATH, "simple"),
                                    (64, 64, fdr.MODE_FAST, fdr.FLAG_FULL_SPECTRUM, "full spectrum"), (64, 16, fdr.MODE_FAST, 0, "N < 32")):
        with fdr.Plan(M, N, mode, flags=flags) as p:
            assert call(p) == -1 and call(p, pr=prm(free=1)) == -1, what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert call(p) == -4
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        p.profile(True)
        assert call(p) == -4 and b"operator PSF" in L.fdr_last_error()
        p.set_operator_psf(psf)
        p.pass_times()  # reads and clears the records of the PSF passes
        assert L.fdr_richardson_lucy_tv_f32(p._h, img.ctypes.data, 8, 8, 64, None, 0, out.ctypes.data, 64, None) == -1  # null params
        assert L.fdr_richardson_lucy_tv_f32(p._h, None, 8, 8, 64, None, 0, out.ctypes.data, 64, prm()) == -1
        for free in (0, 1):
            for lam in (-0.01, 0.1251, float("nan"), float("inf")):
                assert call(p, pr=prm(free=free, lam=lam)) == -1 and b"lambda" in L.fdr_last_error(), lam
            for eps in (-1e-3, float("nan"), float("inf")):
                assert call(p, pr=prm(free=free, eps=eps)) == -1 and b"eps" in L.fdr_last_error(), eps
            assert call(p, pr=prm(free=free, n=-1)) == -1
            for area in (3, -1):
                assert call(p, pr=prm(free=free, area=area)) == -1
            assert call(p, pr=prm(free=free), rows=65) == -1 and call(p, pr=prm(free=free), rows=0) == -1 and call(p, pr=prm(free=free), stride=4) == -1
            assert call(p, pr=prm(free=free), op=img.ctypes.data) == -1 and b"overlaps the input" in L.fdr_last_error()
        # the plain form: no weights, the input's window
        assert call(p, wp=w.ctypes.data) == -1 and b"weights" in L.fdr_last_error()
        for orows, ocols in ((9, 8), (8, 0), (64, 64)):
            assert call(p, pr=prm(orows=orows, ocols=ocols)) == -1, (orows, ocols)
        assert call(p, pr=prm(orows=0, ocols=0)) == 0
        # the free form: sigma, the output window, the weights
        for sigma in (0.0, 1.0, float("nan")):
            assert call(p, pr=prm(free=1, sigma=sigma)) == -1, sigma
        for orows, ocols in ((7, 8), (8, 65), (0, 0)):
            assert call(p, pr=prm(free=1, orows=orows, ocols=ocols)) == -1, (orows, ocols)
        assert call(p, wp=w.ctypes.data, ws=4, pr=prm(free=1)) == -1
        assert call(p, wp=w.ctypes.data, op=w.ctypes.data + 4 * 64 * 3, pr=prm(free=1)) == -1 and b"overlaps the weights" in L.fdr_last_error()
        p.pass_times()  # the one accepted call above
        d = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        base = d.data_ptr()
        for free in (0, 1):
            assert L.fdr_richardson_lucy_tv_f32_dev(p._h, ctypes.c_void_p(base), 64, 64, 64, None, 0, ctypes.c_void_p(base + 4 * 63 * 64), 64,
                                                    prm(free=free, orows=64, ocols=64), None) == -1
            assert L.fdr_richardson_lucy_tv_f32_dev(p._h, ctypes.c_void_p(base), 64, 64, 64, None, 0, ctypes.c_void_p(out.ctypes.data), 64,
                                                    prm(free=free, lam=0.2, orows=64, ocols=64), None) == -1
        # the factor entry on device pointers
        o = torch.empty(64 * 64, dtype=torch.float32, device="cuda")
        assert L.fdr_rl_tv_factor_f32_dev(0, base, 64, 64, 64, None, 0.01, 1e-3, base + 4 * 64, 64, None) == -1  # overlap
        assert L.fdr_rl_tv_factor_f32_dev(0, base, 64, 64, 64, o.data_ptr(), 0.01, 1e-3, o.data_ptr(), 64, None) == -1  # the output is w
        assert L.fdr_rl_tv_factor_f32_dev(0, base, 64, 64, 63, None, 0.01, 1e-3, o.data_ptr(), 64, None) == -1
        assert L.fdr_rl_tv_factor_f32_dev(0, base, 64, 64, 64, None, 0.3, 1e-3, o.data_ptr(), 64, None) == -1
        torch.cuda.synchronize()
        assert sum(c for _, _, c in p.pass_times()) == 0, "a refused call launched a pass"
        for free in (False, True):  # the plan still works
            want = rltv_free_state(img, psf, 64, 64, 3, 0.01)["u"] if free else rltv_model(img, psf, 64, 64, 3, 0.01)
            got = p.richardson_lucy_tv(img, 3, 0.01, free_boundary=free)
            assert rel_err(got, want) <= (RLTV_FREE_TOL if free else RLTV_TOL)


def test_pass_names(fdr):
    """a step is the form's step with one factor launch before it and the weighted update; lambda = 0 launches nothing new"""
    with fdr.Plan(256, 512, fdr.MODE_FAST) as p:
        p.profile(True)
        p.set_operator_psf_motion(15, 30.0)
        p.pass_times()
        img = tone_image(256, 512, 1, 200, 300)
        p.richardson_lucy_tv(img, 3, 0.01, norm_area=NORM_PADDED)
        names = {n: c for n, _, c in p.pass_times() if c}
        print("RLTV\tpasses\tplain\t%s" % names)
        want = {"RL init: u = max(d, 0)": 1, "RLTV factor: w / (1 - lambda div)": 3, "A op rows: pad+FFT (blur / RL)": 6, "B' op cols: FFT*H*IFFT": 3,
                "B' op cols: FFT*conj(H)*IFFT": 3, "C op rows: IFFT+RL ratio": 3, "C op rows: IFFT+RL update (factor)": 3, "E RL minmax+normalize": 1}
        assert names == want, names
        p.richardson_lucy_tv(img, 2, 0.01, free_boundary=True)
        names = {n: c for n, _, c in p.pass_times() if c}
        print("RLTV\tpasses\tfree\t%s" % names)
        want = {"RLF setup: dw, W, sums": 1, "RLF start: wgt = 1/alpha, u": 1, "RLTV factor: w / (1 - lambda div)": 2, "A op rows: pad+FFT (blur / RL)": 1 + 4,
                "B' op cols: FFT*H*IFFT": 2, "B' op cols: FFT*conj(H)*IFFT": 1 + 2, "C op rows: IFFT+crop (blur)": 1, "C op rows: IFFT+RL ratio (free)": 2,
                "C op rows: IFFT+RL update (weighted)": 2, "RLF out: crop": 1}
        assert names == want, names
        for free in (False, True):
            p.richardson_lucy_tv(img, 2, 0.0, free_boundary=free)
            assert not any(c and ("RLTV" in n or "(factor)" in n) for n, _, c in p.pass_times())


def test_cli_rl_tv(fdr, tmp_path):
    """tools/cli/gpu --rl n --rl-tv lambda [--rl-tv-eps e] [--free-boundary [--mask m.png]]: the planes (--raw-out) equal three
    richardson_lucy_tv(..., NORM_PADDED) calls on the plan the Python path uses, and are the written image; --rl-tv with --accel,
    --rl auto or blind is refused with a message, without --rl or with a lambda out of range with the usage line"""
    from PIL import Image
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")
    png = os.path.join(ROOT, "tests", "golden", "car_blurred.png")
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    keep = np.random.default_rng(8).random((h, w)) >= 0.02
    mask_png = str(tmp_path / "mask.png")
    Image.fromarray(np.repeat((keep * np.uint8(255))[:, :, None], 3, axis=2).astype(np.uint8), "RGB").save(mask_png)
    psf = fdr.motionBlurKernel(40, 45.0)
    legs = (("free masked", ["--rl-tv", "0.01", "--free-boundary", "--mask", mask_png], dict(lam=0.01, eps=0.0, free_boundary=True, weights=keep.astype(np.float32)),
             "richardson-lucy free-boundary 10 tv 0.01"),
            ("plain", ["--rl-tv", "0.02", "--rl-tv-eps", "0.01"], dict(lam=0.02, eps=0.01), "richardson-lucy 10 tv 0.02"))
    for tag, extra, kw, line in legs:
        out_png, out_raw = str(tmp_path / (tag.replace(" ", "_") + ".png")), str(tmp_path / (tag.replace(" ", "_") + ".f32"))
        r = subprocess.run([gpu, png, "40", "45", "--rl", "10"] + extra + ["--out", out_png, "--raw-out", out_raw], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Deblurring 3 channels took(gpu[%s]): " % line in r.stdout, r.stdout
        raw = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
        M, N = fdr._rlfree_plan_size(h, w, 40, 40) if kw.get("free_boundary") else fdr._rl_plan_size(h, w)
        planes = []
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            p.set_operator_psf(psf)
            for k, c in enumerate((2, 1, 0)):  # B, G, R
                want = p.richardson_lucy_tv(np.ascontiguousarray(rgb[:, :, c]), 10, norm_area=fdr.NORM_PADDED, **kw)
                assert np.array_equal(raw[k], want), (tag, k, float(np.abs(raw[k] - want).max()))
                planes.append(want)
        bgr = fdr.applyWhiteBalance_u8([np.ascontiguousarray(rgb[:, :, c]) for c in (2, 1, 0)], planes)
        assert np.array_equal(np.asarray(Image.open(out_png).convert("RGB")), bgr[:, :, ::-1]), tag
    for args in (["--rl", "10", "--rl-tv", "0.01", "--accel"], ["--rl", "auto", "--rl-tv", "0.01"]):
        r = subprocess.run([gpu, png, "40", "45"] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "--rl-tv has no accelerated, data-stopped or blind form" in r.stdout, (args, r.stdout[-300:])
    r = subprocess.run([gpu, png, "blind", "9", "--rl", "5", "--rl-tv", "0.01"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--rl-tv has no accelerated, data-stopped or blind form" in r.stdout, r.stdout[-300:]
    for args in (["--rl-tv", "0.01"], ["--rl", "10", "--rl-tv", "0.2"], ["--rl", "10", "--rl-tv-eps", "-1"], ["--rl", "10", "--rl-tv", "-0.1"]):
        r = subprocess.run([gpu, png, "40", "45"] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "Usage" in r.stdout, (args, r.returncode, r.stdout[-300:])
