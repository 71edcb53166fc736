"""Sectioned restoration (fdr_restore_tiled_f32*) on the MI355X.  Small shapes throughout: a 32 x 64 tile plan, 24 x 40 windows, PSFs
5 x 7 and 1 x 1, pictures from one tile to 100 x 300 (far larger than the plan), loose strides and pointers off 16-byte alignment,
overlaps 0, 8 and T / 2.  Bit for bit against the float32 model blend of the public single _dev calls' tile outputs; the launch
groups; determinism; the float64 model of tests/_tiled_model.py; normalisation; quality; refusals; the operator tables; the
neighbours on the plan; allocations; pass names; the upper layers.  Prints `TILED` lines with the measured values (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _tiled_model as tm
from _rl_model import NORM_CROPPED, NORM_NONE, centred_psf, psnr
from _rlfree_model import crop_scene
from _rltv_model import line_psf

pytestmark = pytest.mark.gpu

M, N = tm.PLAN
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(fdr, prm, norm_area=NORM_NONE):
    """the TiledParams of a model parameter dict"""
    return fdr.TiledParams.make(prm["method"], prm["tile"], prm["overlap"], prm["iterations"], prm.get("sigma", tm.SIGMA), prm.get("mu", 1.0),
                                prm.get("rho", 2.0), prm.get("nu", 0.0), prm.get("anisotropic", False), prm.get("nonneg", False), norm_area)


def _fenced(a, stride, shift):
    """device copy of the window a with row stride `stride`, `shift` floats behind a 16-byte aligned base, NaN everywhere else: a read
    outside the window poisons the result.  Returns (tensor, pointer of a[0, 0])."""
    import torch
    buf = np.full(shift + a.shape[0] * stride, np.nan, dtype=np.float32)
    view = buf[shift:].reshape(a.shape[0], stride)
    view[:, :a.shape[1]] = a
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + 4 * shift


class Run:
    """one tiled _dev call on device copies with their own strides and misalignments; .out is the picture, after checking that
    nothing was stored outside it"""

    def __init__(self, fdr, p, img, psfs, prm, weights=None, norm_area=NORM_NONE, pad=(3, 5, 2), shift=1, work_slack=0):
        import torch
        rows, cols = img.shape
        psfs = np.asarray(psfs, dtype=np.float32)
        psfs = psfs[None] if psfs.ndim == 2 else psfs
        count, prows, pcols = psfs.shape
        self.stride, self.out_stride, self.wstride = cols + pad[0], cols + pad[1], cols + pad[2]
        self.params = _params(fdr, prm, norm_area)
        lay = fdr.tiled_layout(rows, cols, prows, pcols, self.params)
        self.work_bytes = lay.work_bytes + 4 * (p.M * p.N - lay.min_M * lay.min_N) + work_slack
        self.keep = [_fenced(img, self.stride, shift)]
        self.d_img = self.keep[0][1]
        self.d_w = None
        if weights is not None:
            self.keep.append(_fenced(weights, self.wstride, shift))
            self.d_w = self.keep[-1][1]
        pstride, self.psf_pitch = pcols + 1, prows * (pcols + 1) + 3
        pbuf = np.full(count * self.psf_pitch, np.nan, dtype=np.float32)
        for k in range(count):
            pbuf[k * self.psf_pitch:k * self.psf_pitch + prows * pstride].reshape(prows, pstride)[:, :pcols] = psfs[k]
        self.d_psfs = torch.from_numpy(pbuf).cuda()
        self.psf_args = (self.d_psfs.data_ptr(), self.psf_pitch, count, prows, pcols, pstride)
        self.d_out = torch.full((shift + rows * self.out_stride,), float("nan"), dtype=torch.float32, device="cuda")
        self.out_ptr = self.d_out.data_ptr() + 4 * shift
        self.d_work = torch.empty(self.work_bytes + 256, dtype=torch.uint8, device="cuda")
        self.work_ptr = (self.d_work.data_ptr() + 255) & ~255
        self.shape, self.shift, self.p = (rows, cols), shift, p

    def call(self, stream=None):
        import torch
        rows, cols = self.shape
        self.p.restore_tiled_dev(self.d_img, rows, cols, self.stride, *self.psf_args, self.out_ptr, self.out_stride, self.params, self.work_ptr,
                                 self.work_bytes, self.d_w, self.wstride, stream)
        torch.cuda.synchronize()
        return self.result()

    def result(self):
        rows, cols = self.shape
        raw = self.d_out.cpu().numpy()
        assert np.all(np.isnan(raw[:self.shift])), "a store landed in front of the picture"
        out = raw[self.shift:].reshape(rows, self.out_stride)
        assert np.all(np.isnan(out[:, cols:])), "a store landed outside the picture"
        return out[:, :cols].copy()


def _single_tiles(fdr, p, img, psfs, prm, weights=None):
    """every tile by the public single _dev call of its method on the plan holding that tile's PSF centred: dict (a, b) -> window"""
    import torch
    rows, cols = img.shape
    ar, ac = tm.axis(rows, prm["tile"][0], prm["overlap"][0]), tm.axis(cols, prm["tile"][1], prm["overlap"][1])
    d_img = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    d_w = torch.from_numpy(np.ascontiguousarray(weights)).cuda() if weights is not None else None
    d_out = torch.empty((ar[1], ac[1]), dtype=torch.float32, device="cuda")
    tiles = {}
    for a in range(ar[0]):
        for b in range(ac[0]):
            y, x = tm.origin(ar, a), tm.origin(ac, b)
            plane = torch.from_numpy(centred_psf(tm.tile_psf(psfs, ac[0], a, b), M, N)).cuda()
            p.set_operator_psf_dev(plane.data_ptr(), M, N, N)
            off = 4 * (y * cols + x)
            wp = d_w.data_ptr() + off if d_w is not None else None
            if prm["method"] == tm.RL_FREE:
                p.richardson_lucy_free_dev(d_img.data_ptr() + off, ar[1], ac[1], cols, d_out.data_ptr(), ac[1], prm["iterations"], wp, cols, prm["sigma"])
            else:
                p.tv_deconv_free_dev(d_img.data_ptr() + off, ar[1], ac[1], cols, d_out.data_ptr(), ac[1], prm["mu"], prm["rho"], prm["iterations"], wp,
                                     cols, prm["nu"], prm["anisotropic"], prm["nonneg"])
            torch.cuda.synchronize()
            tiles[(a, b)] = d_out.cpu().numpy().copy()
    return tiles, ar, ac


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


METHODS = (tm.RL_FREE, tm.TV_FREE)
IDS = {tm.RL_FREE: "rl", tm.TV_FREE: "tv"}


@pytest.mark.parametrize("pic", tm.PICTURES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("method", METHODS, ids=lambda m: IDS[m])
def test_bit_for_bit_against_the_single_calls(fdr, method, pic):
    """the tiled picture is the float32 model blend of the single _dev calls' tiles: every overlap, with one PSF, with a mask, with
    a PSF per tile, with the 1 x 1 PSF; loose strides, pointers off 16-byte alignment and aligned ones"""
    rows, cols = pic
    img = tm.gpu_picture(rows, cols)
    wts = tm.gpu_weights(rows, cols)
    runs = 0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for ov in tm.OVERLAPS:
            prm = tm.method_params(method, 2, overlap=ov)
            lay = tm.layout(rows, cols, 5, 7, tm.TILE, ov)
            variants = [("one psf", tm.gpu_psf(5, 7), None, (3, 5, 2), 1), ("mask", tm.gpu_psf(5, 7), wts, (0, 0, 0), 0),
                        ("psf per tile", tm.gpu_psfs(lay[0] * lay[1], 5, 7), None, (1, 4, 0), 3)]
            if ov == (8, 8):
                variants.append(("delta", np.ones((1, 1), dtype=np.float32), wts, (2, 3, 1), 2))
            for what, psfs, w, pad, shift in variants:
                got = Run(fdr, p, img, psfs, prm, w, pad=pad, shift=shift).call()
                tiles, ar, ac = _single_tiles(fdr, p, img, psfs, prm, w)
                want = tm.blend(tiles, ar, ac, rows, cols)
                assert _bits_equal(got, want), (what, ov, float(np.abs(got - want).max()))
                runs += 1
    print("TILED\tbits\t%s %dx%d: %d runs equal the blend of their single calls" % (IDS[method], rows, cols, runs))


@pytest.mark.parametrize("method", METHODS, ids=lambda m: IDS[m])
def test_groups_and_determinism(fdr, method):
    """launch groups of 1, 3 and 4 give the same bits, and so do two calls"""
    for rows, cols, ov in ((61, 131, (12, 20)), (100, 300, (8, 8))):
        img = tm.gpu_picture(rows, cols)
        prm = tm.method_params(method, 3, overlap=ov)
        outs = []
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            for g in (1, 3, 4, 3):
                p.set_batching(1, g)
                outs.append(Run(fdr, p, img, tm.gpu_psf(5, 7), prm).call())
        for o in outs[1:]:
            assert _bits_equal(o, outs[0]), (rows, cols)


@pytest.mark.parametrize("n", (0, 1, 3))
@pytest.mark.parametrize("method", METHODS, ids=lambda m: IDS[m])
def test_against_the_float64_model(fdr, method, n):
    tol = tm.RLFREE_TOL if method == tm.RL_FREE else tm.TVF_TOL
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 4)
        for rows, cols, ov, masked, per_tile in ((50, 100, (8, 8), False, True), (61, 131, (12, 20), True, False), (100, 300, (8, 8), False, False),
                                                 (20, 33, (0, 0), False, False)):
            img = tm.gpu_picture(rows, cols)
            w = tm.gpu_weights(rows, cols) if masked else None
            prm = tm.method_params(method, n, overlap=ov)
            lay = tm.layout(rows, cols, 5, 7, tm.TILE, ov)
            psfs = tm.gpu_psfs(lay[0] * lay[1], 5, 7) if per_tile else tm.gpu_psf(5, 7)
            got = Run(fdr, p, img, psfs, prm, w).call()
            e = tm.rel_err(got, tm.tiled_model(img, psfs, M, N, prm, w))
            print("TILED\tmodel\t%s n=%d %dx%d overlap %s: err %.3g (tolerance %.3g)" % (IDS[method], n, rows, cols, ov, e, tol))
            assert e <= tol, (rows, cols, e)


@pytest.mark.parametrize("method", METHODS, ids=lambda m: IDS[m])
def test_normalisation(fdr, method):
    """FDR_NORM_CROPPED is the min-max of the FDR_NORM_NONE picture: one tile equals the single call's bits; several tiles equal
    the model's normalisation of the raw result; a stride beyond the plan's min/max partials (swept in bands) changes no bit"""
    import torch
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        img = tm.gpu_picture(24, 40)
        prm = tm.method_params(method, 2)
        psf = tm.gpu_psf(5, 7)
        got = Run(fdr, p, img, psf, prm, norm_area=NORM_CROPPED).call()
        plane = torch.from_numpy(centred_psf(psf, M, N)).cuda()
        p.set_operator_psf_dev(plane.data_ptr(), M, N, N)
        d_img, d_out = torch.from_numpy(img).cuda(), torch.empty((24, 40), dtype=torch.float32, device="cuda")
        if method == tm.RL_FREE:
            p.richardson_lucy_free_dev(d_img.data_ptr(), 24, 40, 40, d_out.data_ptr(), 40, 2, None, 0, prm["sigma"], NORM_CROPPED)
        else:
            p.tv_deconv_free_dev(d_img.data_ptr(), 24, 40, 40, d_out.data_ptr(), 40, prm["mu"], prm["rho"], 2, None, 0, prm["nu"], False, False, NORM_CROPPED)
        torch.cuda.synchronize()
        assert _bits_equal(got, d_out.cpu().numpy())
        img = tm.gpu_picture(100, 300)
        raw = Run(fdr, p, img, psf, prm).call()
        norm = Run(fdr, p, img, psf, prm, norm_area=NORM_CROPPED).call()
        want = (raw.astype(np.float64) - raw.min()) / (float(raw.max()) - float(raw.min()))
        e = float(np.abs(norm - want).max())
        # the device rounds the scale, the product v . scale (up to R = max |v| / (max - min)) and the sum with the shift, each to float
        bound = (4 * float(np.abs(raw).max()) / (float(raw.max()) - float(raw.min())) + 2) * 2.0 ** -24
        print("TILED\tnorm\t%s 100x300: |cropped - minmax(none)| = %.3g (bound %.3g)" % (IDS[method], e, bound))
        assert e <= bound
        wide = Run(fdr, p, img, psf, prm, norm_area=NORM_CROPPED, pad=(3, 21000, 2)).call()  # 100 rows x 84 partials > the plan's 8224
        assert _bits_equal(wide, norm)


def test_device_quality(fdr):
    """one small scene of the model: the device's PSNR equals the model's within 0.05 dB"""
    scene = crop_scene(256, 5)
    psf = line_psf(9, 30.0)
    blurred = np.fft.irfft2(np.fft.rfft2(scene) * np.fft.rfft2(centred_psf(psf, 256, 256).astype(np.float64)), s=scene.shape)
    truth = scene[40:160, 40:160]
    d = (blurred[40:160, 40:160] + np.random.default_rng(9).normal(0, 0.002, truth.shape)).astype(np.float32)
    prm = dict(method=tm.RL_FREE, tile=(64, 64), overlap=(16, 16), iterations=30, sigma=tm.SIGMA)
    model = tm.tiled_model(d, psf, 128, 128, prm)
    with fdr.Plan(128, 128, fdr.MODE_FAST) as p:
        p.set_batching(1, 3)
        got = Run(fdr, p, d, psf, prm).call()
    pm, pg = psnr(model, truth), psnr(got, truth)
    print("TILED\tquality\tblurred %.2f dB, model %.3f dB, device %.3f dB" % (psnr(d, truth), pm, pg))
    assert abs(pm - pg) <= 0.05 and pg > psnr(d, truth) + 2.0


def test_refusals(fdr):
    """every refusal comes before any device work (no pass recorded, the output untouched) and leaves the plan usable"""
    import torch
    L = fdr.lib
    rows, cols = 50, 100
    img = tm.gpu_picture(rows, cols)
    psf = tm.gpu_psf(5, 7)
    prm = tm.method_params(tm.RL_FREE, 2)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        good = Run(fdr, p, img, psf, prm).call()
        p.profile(True)
        p.pass_times()

        def refused(code=-1, **kw):
            r = Run(fdr, p, img, psf, dict(prm, **kw.pop("model", {})), kw.pop("weights", None))
            q = r.params
            for k in ("method", "tile_rows", "tile_cols", "overlap_rows", "overlap_cols", "sigma", "mu", "rho", "nu", "iterations", "norm_area"):
                if k in kw:
                    setattr(q, k, kw.pop(k))
            a = dict(plan=p._h, img=r.d_img, rows=rows, cols=cols, stride=r.stride, w=r.d_w, wstride=r.wstride, psfs=r.psf_args[0],
                     psf_pitch=r.psf_args[1], psf_count=r.psf_args[2], prows=r.psf_args[3], pcols=r.psf_args[4], pstride=r.psf_args[5], out=r.out_ptr,
                     out_stride=r.out_stride, prm=ctypes.byref(q), work=r.work_ptr, work_bytes=r.work_bytes)
            a.update({k: v(r) if callable(v) else v for k, v in kw.items()})
            rc = L.fdr_restore_tiled_f32_dev(a["plan"], a["img"], a["rows"], a["cols"], a["stride"], a["w"], a["wstride"], a["psfs"], a["psf_pitch"],
                                             a["psf_count"], a["prows"], a["pcols"], a["pstride"], a["out"], a["out_stride"], a["prm"], a["work"],
                                             a["work_bytes"], None)
            torch.cuda.synchronize()
            assert rc == code, (kw, rc, L.fdr_last_error())
            assert all(c == 0 for _, _, c in p.pass_times()), "a refused call launched a pass"
            assert np.all(np.isnan(r.d_out.cpu().numpy())), "a refused call wrote to the output"
            return L.fdr_last_error()

        nan, inf = float("nan"), float("inf")
        for kw in (dict(overlap_rows=13), dict(overlap_cols=21), dict(overlap_rows=-1), dict(overlap_cols=-2), dict(tile_rows=0), dict(tile_cols=-3),
                   dict(method=2), dict(iterations=-1), dict(sigma=0.0), dict(sigma=1.0), dict(sigma=nan), dict(norm_area=fdr.NORM_PADDED),
                   dict(norm_area=7), dict(psf_count=2), dict(psf_count=0), dict(psf_count=8), dict(prows=0), dict(pstride=6), dict(work_bytes=1024),
                   dict(stride=cols - 1), dict(out_stride=cols - 1), dict(weights=tm.gpu_weights(rows, cols), wstride=cols - 1), dict(rows=0),
                   dict(cols=-1), dict(img=None), dict(out=None), dict(psfs=None), dict(work=None), dict(prm=None), dict(plan=None),
                   dict(tile_rows=30), dict(tile_cols=60), dict(prows=10, psf_pitch=200), dict(pcols=26, pstride=26, psf_pitch=200)):
            refused(**kw)
        for kw in (dict(mu=0.0), dict(mu=nan), dict(rho=-1.0), dict(rho=inf), dict(nu=-1.0), dict(nu=nan), dict(iterations=-2)):
            refused(model=tm.method_params(tm.TV_FREE, 2), **kw)
        assert b"FDR_NORM_PADDED" in refused(norm_area=fdr.NORM_PADDED)
        assert b"aligned" in refused(work=lambda r: r.work_ptr + 16)
        assert b"overlaps the input" in refused(out=lambda r: r.d_img, out_stride=lambda r: r.stride)
        assert b"overlaps the workspace" in refused(out=lambda r: r.work_ptr)
        refused(img=lambda r: r.work_ptr)  # (the staging of tile (0, 0) on its own input: the single call's refusal)
        assert b"workspace overlaps" in refused(img=lambda r: r.work_ptr + 8192)
        assert b"workspace overlaps" in refused(psfs=lambda r: r.work_ptr + 4096)
        assert b"overlaps the PSFs" in refused(out=lambda r: r.psf_args[0])
        assert b"overlaps the weights" in refused(weights=tm.gpu_weights(rows, cols), out=lambda r: r.d_w, out_stride=lambda r: r.wstride)
        p.profile(False)
        assert _bits_equal(Run(fdr, p, img, psf, prm).call(), good)
    for PM, PN, mode, flags, code in ((32, 64, fdr.MODE_PARITY, 0, -1), (32, 64, fdr.MODE_FAST, fdr.FLAG_FULL_SPECTRUM, -1),
                                      (32, 64, fdr.MODE_FAST, fdr.FLAG_TABLES_ONLY, -4), (30, 60, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX, -1)):
        with fdr.Plan(PM, PN, mode, flags=flags) as q:
            r = Run(fdr, q, img, psf, prm)
            rc = L.fdr_restore_tiled_f32_dev(q._h, r.d_img, rows, cols, r.stride, None, 0, *r.psf_args, r.out_ptr, r.out_stride, ctypes.byref(r.params),
                                             r.work_ptr, r.work_bytes, None)
            assert rc == code, (PM, PN, mode, flags, rc)
    with fdr.Plan(M, N, fdr.MODE_FAST) as q:  # the host form
        out = np.full((rows, cols), np.nan, dtype=np.float32)
        bad = fdr.TiledParams.make(tm.RL_FREE, tm.TILE, (13, 8), 2)
        assert L.fdr_restore_tiled_f32(q._h, img.ctypes.data, rows, cols, cols, None, 0, psf.ctypes.data, 35, 1, 5, 7, 7, out.ctypes.data, cols,
                                       ctypes.byref(bad)) == -1 and np.all(np.isnan(out))
        with pytest.raises(ValueError):
            q.restore_tiled(img, psf, _params(fdr, prm), weights=img[:-1])
        assert _bits_equal(q.restore_tiled(img, psf, _params(fdr, prm)), good)


def test_operator_tables_are_the_last_tiles(fdr):
    import torch
    rows, cols = 50, 100
    img = tm.gpu_picture(rows, cols)
    prm = tm.method_params(tm.TV_FREE, 1)
    psfs = tm.gpu_psfs(9, 5, 7)
    probe = torch.from_numpy(tm.gpu_picture(24, 40, seed=4)).cuda()
    a, b = torch.empty_like(probe), torch.empty_like(probe)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        Run(fdr, p, img, psfs, prm).call()
        p.blur_dev(probe.data_ptr(), 24, 40, 40, a.data_ptr(), 40)
        plane = torch.from_numpy(centred_psf(psfs[8], M, N)).cuda()
        p.set_operator_psf_dev(plane.data_ptr(), M, N, N)
        p.blur_dev(probe.data_ptr(), 24, 40, 40, b.data_ptr(), 40)
        torch.cuda.synchronize()
        assert _bits_equal(a.cpu().numpy(), b.cpu().numpy())
        plane0 = torch.from_numpy(centred_psf(psfs[0], M, N)).cuda()
        p.set_operator_psf_dev(plane0.data_ptr(), M, N, N)
        p.blur_dev(probe.data_ptr(), 24, 40, 40, b.data_ptr(), 40)
        torch.cuda.synchronize()
        assert not _bits_equal(a.cpu().numpy(), b.cpu().numpy())


def test_other_results_unchanged(fdr):
    """Wiener, blur, Richardson-Lucy and TV on the same plan give the same bytes before and after tiled calls of both methods"""
    img = tm.gpu_picture(24, 40, seed=2)
    big = tm.gpu_picture(61, 131)
    psf = tm.gpu_psf(5, 7)

    def neighbours(p):
        p.set_operator_psf(psf)  # (a tiled call leaves the last tile's tables)
        return [p.wiener(img), p.blur(img), p.richardson_lucy(img, 3), p.richardson_lucy_free(img, 3), p.tv_deconv(img, 20.0, 2.0, 3),
                p.tv_deconv_free(img, 20.0, 2.0, 3)]

    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_psf(psf, 0.01)
        before = neighbours(p)
        for method in METHODS:
            p.set_batching(1, 3)
            Run(fdr, p, big, psf, tm.method_params(method, 2, overlap=(12, 20)), norm_area=NORM_CROPPED).call()
            p.set_batching(1, 1)
            for x, y in zip(before, neighbours(p)):
                assert np.array_equal(x, y), method


def test_second_call_allocates_nothing(fdr):
    import torch
    img = tm.gpu_picture(100, 300)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 4)
        runs = [Run(fdr, p, img, tm.gpu_psf(5, 7), tm.method_params(m, 2), norm_area=NORM_CROPPED) for m in METHODS]
        masked = Run(fdr, p, img, tm.gpu_psfs(60, 5, 7), tm.method_params(tm.TV_FREE, 1), tm.gpu_weights(100, 300))
        for r in runs:
            r.call()
        torch.cuda.synchronize()
        f1 = torch.cuda.mem_get_info()[0]
        for r in runs + [masked]:
            r.call()
        torch.cuda.synchronize()
        f2 = torch.cuda.mem_get_info()[0]
    assert f1 == f2, "a later call allocated device memory"


def test_pass_names(fdr):
    """a fresh profiled plan's pass names stay within MAX_PASSES after a tiled call in launch groups, the blend among them; the PSF
    roll is not recorded"""
    img = tm.gpu_picture(61, 131)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.profile(True)
        p.set_batching(1, 3)
        Run(fdr, p, img, tm.gpu_psf(5, 7), tm.method_params(tm.TV_FREE, 2), norm_area=NORM_CROPPED).call()
        names = {n: c for n, _, c in p.pass_times()}
    print("TILED\tpasses\t%s" % names)
    assert 0 < len(names) <= fdr.MAX_PASSES
    assert names["O rows: PSF pad+FFT (operator)"] == 1 and names["E tiled minmax+normalize"] == 1
    assert names["T blend: tiles -> picture"] == 1 and not any("centre" in n or "roll" in n for n in names)


def test_python_layers(fdr):
    """the host form equals the _dev form; restoreTiled_myfft and restoreTiled_RGB equal it on the layout's plan"""
    rows, cols = 61, 131
    img = tm.gpu_picture(rows, cols)
    w = tm.gpu_weights(rows, cols)
    for method in METHODS:
        prm = tm.method_params(method, 2, overlap=(12, 20))
        q = _params(fdr, prm, NORM_CROPPED)
        lay = fdr.tiled_layout(rows, cols, 5, 7, q)
        assert (lay.min_M, lay.min_N) == (M, N)
        psfs = tm.gpu_psfs(lay.tiles_r * lay.tiles_c, 5, 7)
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            dev = Run(fdr, p, img, psfs, prm, w, NORM_CROPPED).call()
            assert _bits_equal(p.restore_tiled(img, psfs, q, w), dev)
            one = p.restore_tiled(img, psfs[0], q)
        assert _bits_equal(fdr.restoreTiled_myfft(img, psfs, q, w), dev)
        chans = [img, np.ascontiguousarray(img[::-1]), img * np.float32(0.5)]
        want = [fdr.restoreTiled_myfft(c, psfs[0], q) for c in chans]
        assert _bits_equal(want[0], one)
        fdr.restoreTiled_RGB(chans, psfs[0], q)
        for k in range(3):
            assert _bits_equal(chans[k], want[k]), k


def test_cpp_wrapper(fdr, tmp_path):
    """fft_gpu::restoreTiled_RGB: the three planes equal the host call it is defined by, on the layout's plan"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "tiled_shim_test"])
    exe = os.path.join(ROOT, "tools", "cli", "tiled_shim_test")
    rows, cols = 61, 131
    ch = [tm.gpu_picture(rows, cols, seed=20 + k) for k in range(3)]
    np.stack(ch).tofile(str(tmp_path / "in.f32"))
    psf = fdr.motionBlurKernel(7, 30.0)
    for method in METHODS:
        r = subprocess.run([exe, str(tmp_path / "in.f32"), str(rows), str(cols), "7", "30", str(method), "40", "8", "3", str(tmp_path / "out.f32")],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(str(tmp_path / "out.f32"), dtype=np.float32).reshape(3, rows, cols)
        q = fdr.TiledParams.make(method, 40, 8, 3, fdr.RL_SIGMA, 200.0, 2.0, 0.0, False, True, NORM_CROPPED)
        for k in range(3):
            assert _bits_equal(got[k], fdr.restoreTiled_myfft(ch[k], psf, q)), (method, k)


def test_cli_tile(fdr, tmp_path):
    """tools/cli/gpu --rl n | --tv mu --free-boundary --tile T [--overlap O] [--mask m.png]: the planes (--raw-out) equal
    restoreTiled_myfft per channel, normalised over the picture; without --free-boundary --tile prints the usage text"""
    from PIL import Image
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")
    png = os.path.join(ROOT, "tests", "golden", "car_blurred.png")
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    keep = np.random.default_rng(8).random((h, w)) >= 0.02
    mask_png = str(tmp_path / "mask.png")
    Image.fromarray(np.repeat((keep * np.uint8(255))[:, :, None], 3, axis=2).astype(np.uint8), "RGB").save(mask_png)
    psf = fdr.motionBlurKernel(15, 30.0)
    legs = ((["--rl", "4"], fdr.TILED_RL_FREE, 4, ["--overlap", "32", "--mask", mask_png], 32, keep.astype(np.float32),
             "richardson-lucy free-boundary 4 tile 200 overlap 32"),
            (["--tv", "200", "--tv-iters", "4"], fdr.TILED_TV_FREE, 4, [], 25, None, "total-variation free-boundary mu 200 rho 2 n 4 tile 200 overlap 25"))
    for leg, method, n, extra, overlap, wt, says in legs:
        out_raw = str(tmp_path / "out.f32")
        r = subprocess.run([gpu, png, "15", "30"] + leg + ["--free-boundary", "--tile", "200"] + extra + ["--raw-out", out_raw, "--out",
                            str(tmp_path / "out.png")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Deblurring 3 channels took(gpu[%s]): " % says in r.stdout, r.stdout
        got = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
        q = fdr.TiledParams.make(method, 200, overlap, n, fdr.RL_SIGMA, 200.0, 2.0, 0.0, False, True, NORM_CROPPED)
        for k, c in enumerate((2, 1, 0)):  # B, G, R
            want = fdr.restoreTiled_myfft(np.ascontiguousarray(rgb[:, :, c]), psf, q, wt)
            assert _bits_equal(got[k], want), (says, k, float(np.abs(got[k] - want).max()))
    for bad in (["--rl", "4", "--tile", "200"], ["--rl", "4", "--free-boundary", "--tile", "200", "--overlap", "101"],
                ["--rl", "4", "--free-boundary", "--accel", "--tile", "200"], ["--tv", "auto", "--tile", "200"]):
        r = subprocess.run([gpu, png, "15", "30"] + bad, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "Usage" in r.stdout, bad
