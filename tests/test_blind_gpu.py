"""Blind Richardson-Lucy (fdr_richardson_lucy_blind_f32*) on the MI355X against the float64 model of tests/_blind_model.py: every
column length of the new column kernel, the row lengths and PSF windows, the free-boundary form with and without weights, the bit
identities (a held PSF is the non-blind call, determinism, the operator tables left behind, the untouched Wiener filter), the
invariants of the PSF, the restoration quality, the refusals with the status word, the CLI and the C++ wrapper.

The tolerance (bm.gpu_tol): the device's max-abs error over max |model|, image and PSF separately, may be 10 times that of the
float32 replay of the model on the same input, with a floor of 1e-5.  Each case prints a `BLIND` line with its values (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _blind_model as bm
from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, rel_err

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
# no coverage of a free-form model run may lie this close to sigma: a rounding flip of the threshold would void the comparison
# (10 times the 5e-7 absolute error of a float32 coverage that _rlfree_model.py records)
MARGIN = 5e-6


def _compare(name, got_u, got_p, img, p0, M, N, n, **kw):
    """device image and PSF against the model; returns the failures"""
    info = {}
    u, p = bm.blind_model(img, p0, M, N, n, info=info, **kw)
    u32, p32 = bm.blind_model(img, p0, M, N, n, dtype=np.float32, **kw)
    if "margin" in info:
        assert info["margin"] >= MARGIN, "%s: a model coverage lies %.3g from sigma" % (name, info["margin"])
    e32 = rel_err(u32, u), rel_err(p32, p)
    e = rel_err(got_u, u), rel_err(got_p, p)
    print("BLIND\t%s\timage err=%.3g cpu32=%.3g\tpsf err=%.3g cpu32=%.3g" % (name, e[0], e32[0], e[1], e32[1]))
    bad = []
    for what, err, err32 in (("image", e[0], e32[0]), ("psf", e[1], e32[1])):
        if not err <= bm.gpu_tol(err32):
            bad.append("%s %s: error %.3g > %.3g (float32 replay %.3g)" % (name, what, err, bm.gpu_tol(err32), err32))
    return bad


def _dev_call(p, img, p0, n, free=False, weights=None, out_shape=None, hold=0, area=NORM_NONE, stride_pad=5):
    """Plan.richardson_lucy_blind_dev on device copies with padded strides; NaN guards round the output and the PSF must stay NaN"""
    import torch
    rows, cols = img.shape
    stride = cols + stride_pad
    src = np.full((rows, stride), 9.0, dtype=np.float32)
    src[:, :cols] = img
    d_in = torch.from_numpy(src).cuda()
    d_w, ws = None, 0
    if weights is not None:
        ws = cols + 1
        w = np.full((rows, ws), 7.0, dtype=np.float32)
        w[:, :cols] = weights
        d_w = torch.from_numpy(w).cuda()
    prows, pcols = p0.shape
    ps = pcols + 2
    psf = np.full((prows + 1, ps), np.nan, dtype=np.float32)
    psf[:prows, :pcols] = p0
    d_psf = torch.from_numpy(psf).cuda()
    orows, ocols = out_shape or (rows, cols)
    os_ = ocols + 3
    d_out = torch.full((orows + 1, os_), float("nan"), dtype=torch.float32, device="cuda")
    p.richardson_lucy_blind_dev(d_in.data_ptr(), rows, cols, stride, d_psf.data_ptr(), prows, pcols, ps, d_out.data_ptr(), os_, n,
                                free_boundary=free, d_weights=d_w.data_ptr() if d_w is not None else None, wstride=ws, psf_hold=hold,
                                norm_area=area, out_rows=orows if free else None, out_cols=ocols if free else None)
    torch.cuda.synchronize()
    out, pn = d_out.cpu().numpy(), d_psf.cpu().numpy()
    assert np.all(np.isnan(out[:orows, ocols:])) and np.all(np.isnan(out[orows:, :])), "a store landed outside the output window"
    assert np.all(np.isnan(pn[:prows, pcols:])) and np.all(np.isnan(pn[prows:, :])), "a store landed outside the PSF"
    return out[:orows, :ocols], pn[:prows, :pcols]


@pytest.mark.parametrize("M", bm.COLUMN_M)
def test_every_column_length(fdr, M):
    """plain form, full-plane window, N = 32, 3 x 3 and 5 x 12 PSFs, 3 iterations; the host form and the device form"""
    bad = []
    img = bm.gpu_image(M, 32, M)
    with fdr.Plan(M, 32, fdr.MODE_FAST) as p:
        for k, (pr, pc) in enumerate(bm.COLUMN_PSFS):
            p0 = bm.start_psf(pr, pc, M + pr)
            if k == 0:
                u, pn = p.richardson_lucy_blind(img, p0, bm.COLUMN_N_ITER)
            else:
                u, pn = _dev_call(p, img, p0, bm.COLUMN_N_ITER)
            bad += _compare("col M=%d psf %dx%d" % (M, pr, pc), u, pn, img, p0, M, 32, bm.COLUMN_N_ITER)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("N", bm.ROW_N)
def test_row_lengths(fdr, N):
    img, p0 = bm.gpu_image(16, N, N), bm.start_psf(3, 3, N)
    with fdr.Plan(16, N, fdr.MODE_FAST) as p:
        u, pn = p.richardson_lucy_blind(img, p0, bm.COLUMN_N_ITER)
    bad = _compare("row N=%d" % N, u, pn, img, p0, 16, N, bm.COLUMN_N_ITER)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("N", (32, 8192))
def test_psf_windows_of_the_crop_pass(fdr, N):
    """1 x 1, 9 x 9 and 31 x 31 PSFs on the narrowest and the widest rows (32 rows: the 31-row PSF has to fit the plan)"""
    bad = []
    with fdr.Plan(32, N, fdr.MODE_FAST) as p:
        for pr, pc in bm.PSF_WINDOWS:
            img, p0 = bm.gpu_image(32, N, N + pr), bm.start_psf(pr, pc, pr)
            u, pn = _dev_call(p, img, p0, bm.COLUMN_N_ITER)
            if pr == 1:
                assert pn[0, 0] == 1.0, "a 1 x 1 PSF stays {1}"
            bad += _compare("win N=%d psf %dx%d" % (N, pr, pc), u, pn, img, p0, 32, N, bm.COLUMN_N_ITER)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", bm.FREE_CASES, ids=lambda c: "%dx%d" % c[:2])
def test_free_form(fdr, case):
    """9 x 9 PSF, with and without weights (2 % zeros), window and whole-plan output, 5 and 20 iterations"""
    M, N, rows, cols = case
    img, p0 = bm.gpu_image(rows, cols, M), bm.start_psf(9, 9, M)
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for w in (None, bm.gpu_mask(rows, cols, 7)):
            for n in bm.FREE_N_ITER:
                for shape in ((rows, cols), (M, N)):
                    name = "free %dx%d weights=%s n=%d out=%dx%d" % (M, N, w is not None, n, shape[0], shape[1])
                    if shape == (rows, cols):
                        u, pn = _dev_call(p, img, p0, n, free=True, weights=w, out_shape=shape)
                    else:
                        u, pn = p.richardson_lucy_blind(img, p0, n, free_boundary=True, weights=w, full_plane=True)
                    assert pn.min() >= 0 and abs(float(pn.sum(dtype=np.float64)) - 1) <= 1e-6, name
                    bad += _compare(name, u, pn, img, p0, M, N, n, free_boundary=True, weights=w, out_shape=shape)
    assert not bad, "\n".join(bad)


def test_plain_form_on_a_cropped_window(fdr):
    """iterations = 0 and the refusals only: the plain form's numbers are judged on full-plane windows ("limit of
    the model": a top-left PSF makes c ~ tau in the first rows of a crop)"""
    img, p0 = bm.gpu_image(50, 40, 1), bm.start_psf(5, 5, 1)
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        u, pn = p.richardson_lucy_blind(img, p0, 0)
        assert np.array_equal(u, np.maximum(img, 0)) and np.array_equal(pn, p0)
        u, pn = _dev_call(p, img, p0, 0, area=NORM_CROPPED)
        d = np.maximum(img, 0).astype(np.float64)
        assert np.max(np.abs(u - (d - d.min()) / (d.max() - d.min()))) < 1e-6 and np.array_equal(pn, p0)
        assert p.blind_status() == 0
        buf = np.zeros((64, 64), dtype=np.float32)
        out = np.zeros((64, 64), dtype=np.float32)
        psf = p0.copy()

        def call(rows=50, cols=40, stride=64, weights=None, prows=5, pcols=5, pstride=5, out_stride=64, psf_ptr=None, out_ptr=None,
                 prm=None):
            prm = prm or fdr.BlindParams(2, 0, 0, fdr.NORM_NONE, 0.01, 0, 0)
            return fdr.lib.fdr_richardson_lucy_blind_f32(p._h, buf.ctypes.data, rows, cols, stride, weights, 64,
                                                         psf.ctypes.data if psf_ptr is None else psf_ptr, prows, pcols, pstride,
                                                         out.ctypes.data if out_ptr is None else out_ptr, out_stride,
                                                         ctypes.byref(prm) if prm != "null" else None)
        gen = p.pass_times()  # clears the records
        refusals = {
            "null params": dict(prm="null"),
            "psf_hold < 0": dict(prm=fdr.BlindParams(2, 0, -1, fdr.NORM_NONE, 0.01, 0, 0)),
            "iterations < 0": dict(prm=fdr.BlindParams(-1, 0, 0, fdr.NORM_NONE, 0.01, 0, 0)),
            "norm_area": dict(prm=fdr.BlindParams(2, 0, 0, 7, 0.01, 0, 0)),
            "plain out window": dict(prm=fdr.BlindParams(2, 0, 0, fdr.NORM_NONE, 0.01, 64, 64)),
            "free sigma": dict(prm=fdr.BlindParams(2, 1, 0, fdr.NORM_NONE, 0.0, 50, 40)),
            "free out window": dict(prm=fdr.BlindParams(2, 1, 0, fdr.NORM_NONE, 0.01, 40, 40)),
            "weights in the plain form": dict(weights=buf.ctypes.data),
            "pstride < pcols": dict(pstride=4),
            "empty psf": dict(prows=0),
            "psf larger than the plan": dict(prows=65, pstride=5),
            "psf of more than 65536 entries": dict(prows=64, pcols=64, pstride=64),  # fits this plan: only a larger plan reaches the limit
            "window": dict(rows=65),
            "psf overlaps the input": dict(psf_ptr=buf.ctypes.data + 8),
            "psf overlaps the output": dict(psf_ptr=out.ctypes.data + 64),
            "output overlaps the input": dict(out_ptr=buf.ctypes.data),
        }
        for name, kw in refusals.items():
            if name == "psf of more than 65536 entries":
                continue
            assert call(**kw) == ERR_ARG, name
        # the start PSF of the host form
        for bad_psf in (-p0, p0 * 0, np.where(np.arange(25).reshape(5, 5) == 7, np.nan, p0), np.where(np.arange(25).reshape(5, 5) == 3, -1e-9, p0)):
            psf = np.ascontiguousarray(bad_psf, dtype=np.float32)
            assert call() == ERR_ARG, bad_psf
        assert sum(c for _, _, c in p.pass_times()) == 0, "a refused call launched a pass"
        assert not out.any() and gen is not None
        psf = p0.copy()
        assert call() == 0  # the plan is usable afterwards
    with fdr.Plan(512, 512, fdr.MODE_FAST) as p:  # the entry limit needs a plan a 257 x 256 PSF fits
        big = np.zeros((257, 256), dtype=np.float32)
        img = np.ones((512, 512), dtype=np.float32)
        prm = fdr.BlindParams(1, 0, 0, fdr.NORM_NONE, 0.01, 0, 0)
        o = np.zeros_like(img)
        assert fdr.lib.fdr_richardson_lucy_blind_f32(p._h, img.ctypes.data, 512, 512, 512, None, 0, big.ctypes.data, 257, 256, 256,
                                                     o.ctypes.data, 512, ctypes.byref(prm)) == ERR_ARG
        assert b"65536" in fdr.lib.fdr_last_error()
    with fdr.Plan(64, 64, fdr.MODE_PARITY) as p:
        with pytest.raises(fdr.FdrError) as e:
            p.richardson_lucy_blind(img[:64, :64], p0, 1)
        assert e.value.code == ERR_ARG


def test_dev_refusals_and_the_status_word(fdr):
    import torch
    img, p0 = bm.gpu_image(64, 64, 2), bm.start_psf(5, 5, 2)
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        with pytest.raises(fdr.FdrError) as e:
            p.blind_status()
        assert e.value.code == ERR_STATE
        d_in = torch.from_numpy(img).cuda()
        d_out = torch.zeros(64, 64, device="cuda")
        d_psf = torch.from_numpy(p0).cuda()

        def call(psf=d_psf.data_ptr(), out=d_out.data_ptr(), w=None, pstride=5, hold=0, free=False):
            p.richardson_lucy_blind_dev(d_in.data_ptr(), 64, 64, 64, psf, 5, 5, pstride, out, 64, 2, free_boundary=free, d_weights=w, wstride=64,
                                        psf_hold=hold)
        for kw in (dict(psf=None), dict(hold=-1), dict(pstride=4), dict(w=d_out.data_ptr()), dict(psf=d_in.data_ptr() + 16),
                   dict(psf=d_out.data_ptr() + 16), dict(out=d_in.data_ptr()), dict(free=True, w=d_psf.data_ptr())):
            with pytest.raises(fdr.FdrError) as e:
                call(**kw)
            assert e.value.code == ERR_ARG, kw
        torch.cuda.synchronize()
        assert not d_out.any().item() and np.array_equal(d_psf.cpu().numpy(), p0)
        call()
        assert p.blind_status() == 0
        good = d_psf.cpu().numpy()
        assert rel_err(good, p0) > 1e-3
        for bad in (-p0, p0 * 0, np.where(np.arange(25).reshape(5, 5) == 7, np.nan, p0).astype(np.float32)):
            d_bad = torch.from_numpy(np.ascontiguousarray(bad, dtype=np.float32)).cuda()
            call(psf=d_bad.data_ptr())
            assert p.blind_status() == 1
            back = d_bad.cpu().numpy()
            assert np.array_equal(back, bad, equal_nan=True), "a bad start PSF is left alone"
        d_psf2 = torch.from_numpy(p0).cuda()
        call(psf=d_psf2.data_ptr())
        assert p.blind_status() == 0 and np.array_equal(d_psf2.cpu().numpy(), good)


@pytest.mark.parametrize("free", (False, True))
def test_held_psf_is_the_non_blind_call(fdr, free):
    """psf_hold = iterations: bit for bit the non-blind call with p_0 in all three norm areas, the PSF unchanged; psf_hold = 2 of 4:
    the first two steps are the non-blind ones (checked through psf_hold > iterations of a 2-step call)"""
    M, N, rows, cols = (128, 128, 100, 90) if free else (128, 128, 128, 128)
    img, p0 = bm.gpu_image(rows, cols, 11), bm.start_psf(7, 9, 11)
    w = bm.gpu_mask(rows, cols, 12) if free else None
    with fdr.Plan(M, N, fdr.MODE_FAST) as p, fdr.Plan(M, N, fdr.MODE_FAST) as ref:
        ref.set_operator_psf(p0)
        for area in (NORM_NONE, NORM_CROPPED, NORM_PADDED):
            for hold in (6, 9):
                u, pn = p.richardson_lucy_blind(img, p0, 6, free_boundary=free, weights=w, psf_hold=hold, norm_area=area)
                want = ref.richardson_lucy_free(img, 6, weights=w, norm_area=area) if free else ref.richardson_lucy(img, 6, area)
                assert np.array_equal(u, want), (area, hold, float(np.abs(u - want).max()))
                assert np.array_equal(pn, p0)
        u, pn = _dev_call(p, img, p0, 6, free=free, weights=w, hold=6)
        want = ref.richardson_lucy_free(img, 6, weights=w) if free else ref.richardson_lucy(img, 6)
        assert np.array_equal(u, want) and np.array_equal(pn, p0)


def test_calls_repeat_and_leave_the_tables_of_the_result(fdr):
    img, p0 = bm.gpu_image(256, 128, 13), bm.start_psf(9, 9, 13)
    rnd = np.random.default_rng(14).random((256, 128)).astype(np.float32)
    win = np.ascontiguousarray(img[:200, :100])
    with fdr.Plan(256, 128, fdr.MODE_FAST) as p, fdr.Plan(256, 128, fdr.MODE_FAST) as fresh:
        p.set_psf(fdr.motionBlurKernel(9, 30.0), 0.01)
        wiener = p.wiener(rnd, fdr.NORM_PADDED)
        for free in (False, True):
            x = win if free else img
            a = p.richardson_lucy_blind(x, p0, 8, free_boundary=free)
            b = p.richardson_lucy_blind(x, p0, 8, free_boundary=free)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), "two blind calls differ"
            assert a[1].min() >= 0 and abs(float(a[1].sum(dtype=np.float64)) - 1) <= 1e-6
            fresh.set_operator_psf(a[1])
            for adjoint in (False, True):
                assert p.blur(rnd, adjoint).tobytes() == fresh.blur(rnd, adjoint).tobytes(), "the tables are not those of p_n"
            assert p.richardson_lucy(img, 3).tobytes() == fresh.richardson_lucy(img, 3).tobytes()
        assert p.wiener(rnd, fdr.NORM_PADDED).tobytes() == wiener.tobytes(), "the Wiener filter changed"


def test_pass_names_fit_the_timer(fdr):
    """a plan's pass timer remembers FDR_MAX_PASSES = 16 names: a fresh plan holds every pass of a free-boundary blind call, cropped
    and normalised, under its own name (an overflow would pile the launches onto the last name)"""
    img, p0, n = bm.gpu_image(50, 100, 5), bm.start_psf(9, 9, 5), 4
    with fdr.Plan(64, 128, fdr.MODE_FAST) as p:
        p.profile(True)
        p.richardson_lucy_blind(img, p0, n, free_boundary=True)
        p.richardson_lucy_blind(img, p0, n, free_boundary=True, norm_area=NORM_CROPPED)
        names = {name: c for name, _, c in p.pass_times() if c}
        p.profile(False)
    assert len(names) <= fdr.MAX_PASSES
    want = {"BL cols: FFT -> conj(U)/MN": 2 * n, "B' op cols: FFT*conj(U)*IFFT": 4 * n, "C op rows: IFFT+crop (PSF)": 4 * n,
            "BL PSF: start / project / wgt": 2 * (1 + n + n - 1), "C op rows: IFFT+RL update (weighted)": 2 * n,
            "C op rows: IFFT+RL ratio (free)": 2 * n, "O cols: FFT -> H/MN, conj(H)/MN": 2 * (1 + n), "RLF out: crop": 1, "E RLF minmax+normalize": 1}
    for name, count in want.items():
        assert names.get(name) == count, (name, names)
    with fdr.Plan(64, 128, fdr.MODE_FAST) as p:  # the plain form
        p.profile(True)
        p.richardson_lucy_blind(bm.gpu_image(64, 128, 5), p0, n, norm_area=NORM_PADDED)
        names = {name: c for name, _, c in p.pass_times() if c}
    assert names.get("C op rows: IFFT+RL update") == n and names.get("BL PSF: start / project / wgt") == 1 + n and names.get("E RL minmax+normalize") == 1


@pytest.mark.parametrize("free", (False, True))
def test_zeroed_border_stays_zero(fdr, free):
    M, N, rows, cols = (64, 128, 50, 100) if free else (64, 128, 64, 128)
    img = bm.gpu_image(rows, cols, 3)
    p0 = bm.start_psf(9, 9, 4)
    p0[0, :] = p0[-1, :] = p0[:, 0] = p0[:, -1] = 0
    p0 /= p0.sum()
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        _, pn = p.richardson_lucy_blind(img, p0, 20, free_boundary=free)
    assert pn.min() >= 0 and abs(float(pn.sum(dtype=np.float64)) - 1) <= 1e-6
    assert not pn[0, :].any() and not pn[-1, :].any() and not pn[:, 0].any() and not pn[:, -1].any()
    assert rel_err(pn, p0) > 1e-3


def test_quality(fdr):
    """the plain 128^2 scene and the free-form crop of test_blind_host.py, 80 iterations: the device's correlation within 0.01 of
    the model's, the image PSNR within 0.05 dB"""
    q = bm.QUALITY
    g = bm.psf_gaussian(q["psf"])
    truth, d, psf = bm.plain_case(1)
    img, p = fdr.richardsonLucyBlind_myfft(d, psf_size=q["psf"], iterations=q["n"])
    mi, mp = bm.blind_model(d, g, q["S"], q["S"], q["n"])
    c_dev, c_mod = bm.shift_corr(p, psf), bm.shift_corr(mp, psf)
    s_dev, s_mod = bm.shift_psnr(img, truth), bm.shift_psnr(mi, truth)
    print("BLIND\tquality plain\tcorr device=%.4f model=%.4f\tpsnr device=%.3f model=%.3f" % (c_dev, c_mod, s_dev, s_mod))
    assert abs(c_dev - c_mod) <= 0.01 and abs(s_dev - s_mod) <= 0.05
    c = q["crop"]
    tw, dc, psf = bm.crop_case(1)
    with fdr.Plan(c["M"], c["N"], fdr.MODE_FAST) as plan:
        img, p = plan.richardson_lucy_blind(dc, g, q["n"], free_boundary=True)
    mi, mp = bm.blind_model(dc, g, c["M"], c["N"], q["n"], free_boundary=True)
    c_dev, c_mod = bm.shift_corr(p, psf), bm.shift_corr(mp, psf)
    s_dev, s_mod = bm.shift_psnr(img, tw, margin=8), bm.shift_psnr(mi, tw, margin=8)
    print("BLIND\tquality crop\tcorr device=%.4f model=%.4f\tpsnr device=%.3f model=%.3f" % (c_dev, c_mod, s_dev, s_mod))
    assert abs(c_dev - c_mod) <= 0.01 and abs(s_dev - s_mod) <= 0.05


def test_psf_gaussian_dev(fdr):
    import torch
    for size, sigma in ((9, 0.0), (1, 0.0), (16, 1.3), (256, 40.0)):
        d = torch.full((size * size + 1,), float("nan"), device="cuda")
        assert fdr.lib.fdr_psf_gaussian_dev(0, size, sigma, ctypes.c_void_p(d.data_ptr()), None) == 0
        torch.cuda.synchronize()
        got = d.cpu().numpy()
        assert np.isnan(got[-1])
        want = bm.psf_gaussian(size, sigma).astype(np.float64).ravel()
        # evaluated in double on both sides; the exponential and the order of the sum may differ in the last bits of a double
        assert np.max(np.abs(got[:-1] - want)) <= want.max() * 2.0 ** -23, (size, sigma)


def test_cli_blind(fdr, tmp_path):
    """tools/cli/gpu <img> blind 9 --rl 5 --psf-out: runs, prints the line and writes both files"""
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(root, "tools", "cli", "gpu")
    png = os.path.join(root, "tests", "golden", "car_blurred.png")
    out_png, psf_png = str(tmp_path / "out.png"), str(tmp_path / "psf.png")
    r = subprocess.run([gpu, png, "blind", "9", "--rl", "5", "--psf-out", psf_png, "--out", out_png], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("blind: ")]
    assert len(line) == 1 and line[0].startswith("blind: size 9 iterations 5 psf-sum 1 psf-peak "), r.stdout
    assert " at (" in line[0]
    src = Image.open(png)
    assert Image.open(out_png).size == src.size
    k = np.asarray(Image.open(psf_png).convert("L"))
    assert k.shape == (9, 9) and k.min() == 0 and k.max() == 255
    r = subprocess.run([gpu, png, "blind", "9"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "Usage" in r.stdout  # blind needs --rl n


def test_cpp_wrapper(fdr, tmp_path):
    """fft_gpu::richardsonLucyBlind_RGB: the PSF from the mean of the channels with FDR_NORM_NONE, then each channel through the
    non-blind form with it -- the three planes equal the C calls it is defined by"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "blind_shim_test"])
    exe = os.path.join(root, "tools", "cli", "blind_shim_test")
    rows, cols, n = 60, 100, 6
    ch = [bm.gpu_image(rows, cols, 20 + k) for k in range(3)]
    np.stack(ch).tofile(str(tmp_path / "in.f32"))
    for free in (0, 1):
        r = subprocess.run([exe, str(tmp_path / "in.f32"), str(rows), str(cols), "9", str(n), str(free), str(tmp_path / "out.f32"),
                            str(tmp_path / "psf.f32")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(str(tmp_path / "out.f32"), dtype=np.float32).reshape(3, rows, cols)
        got_psf = np.fromfile(str(tmp_path / "psf.f32"), dtype=np.float32).reshape(9, 9)
        mean = ((ch[0] + ch[1] + ch[2]) / np.float32(3)).astype(np.float32)
        M, N = fdr._rlfree_plan_size(rows, cols, 9, 9) if free else fdr._rl_plan_size(rows, cols)
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            _, psf = p.richardson_lucy_blind(mean, fdr.psf_gaussian(9), n, free_boundary=bool(free))
            assert np.array_equal(got_psf, psf)
            for k in range(3):
                want = p.richardson_lucy_free(ch[k], n, norm_area=fdr.NORM_PADDED) if free else p.richardson_lucy(ch[k], n, fdr.NORM_PADDED)
                assert np.array_equal(got[k], want), (free, k)
