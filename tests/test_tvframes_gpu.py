"""Multi-frame TV deconvolution (fdr_tv_deconv_frames_f32*) on the MI355X: against the float64 model of tests/_tvframes_model.py on
the smallest shapes at which its kernels can go wrong, the table kernel seen through one iteration, the bit identities (one frame =
the single-frame calls, every launch group, two calls, the host form), isolation from the rest of the plan, allocation-free later
calls, every refusal, the pass names and the quality case.  Every output has NaN guard columns that must stay NaN.  Cases print a
`TVM` line with their measured values (pytest -s)."""
import ctypes

import numpy as np
import pytest

from _frames_model import quality_case
from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, psnr, rel_err
from _tvframes_model import (LEAST_SQUARES, POISSON, QUALITY_JOINT_MU, QUALITY_MEASURED, QUALITY_N, QUALITY_RHO, SHORT, SHORT_IDS, TVFR_TOL, WEIGHT_KINDS,
                             quality_psnr, short_frames, short_psfs, short_weights, tvframes_iterates, tvframes_model)
from _tvfree_model import finish

pytestmark = pytest.mark.gpu

F32_EPS = float(np.finfo(np.float32).eps)
ITERATIONS = (0, 1, 2, 10, 30)
KS = (1, 2, 3, 5, 8)


def _need(fdr):
    assert hasattr(fdr.lib, "fdr_tv_deconv_frames_f32_dev"), "the library has no multi-frame TV deconvolution"


def _to_dev(planes, stride, fill=0.0):
    """K planes rows x cols into one device buffer with row stride `stride` and one extra row between the planes; (tensor, pitch)"""
    import torch
    K, rows, cols = len(planes), planes[0].shape[0], planes[0].shape[1]
    buf = np.full((K, rows + 1, stride), fill, dtype=np.float32)
    for k in range(K):
        buf[k, :rows, :cols] = planes[k]
    return torch.from_numpy(buf).cuda(), (rows + 1) * stride


def _dev_call(p, ds, weights, stride, wstride, out_stride, out_rows, out_cols, mu, iterations, **kw):
    """Plan.tv_deconv_frames_dev on device copies (row strides as given, the padding of the weights 7.0: it must not be read); the
    output has NaN-filled guard columns and a guard row, which must stay NaN; returns the out_rows x out_cols window"""
    import torch
    K, (rows, cols) = len(ds), ds[0].shape
    d_in, pitch = _to_dev(ds, stride)
    d_w, wp = None, 0
    if weights is not None:
        w = np.asarray(weights, dtype=np.float32)
        d_w, wp = _to_dev([w] if w.ndim == 2 else list(w), wstride, 7.0)
        if w.ndim == 2:
            wp = 0
    out_stride = max(out_stride, out_cols + 3)
    d_out = torch.full((out_rows + 1, out_stride), float("nan"), dtype=torch.float32, device="cuda")
    p.tv_deconv_frames_dev(d_in.data_ptr(), pitch, K, rows, cols, stride, d_out.data_ptr(), out_stride, mu, iterations,
                           d_weights=d_w.data_ptr() if d_w is not None else None, weight_pitch=wp, wstride=wstride if d_w is not None else 0,
                           out_rows=out_rows, out_cols=out_cols, **kw)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(np.isnan(out[:out_rows, out_cols:])) and np.all(np.isnan(out[out_rows:, :])), "a store landed outside the output window"
    return out[:out_rows, :out_cols]


def _err(got, want, area):
    return rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(got.astype(np.float64) - want)))


def _model_planes(ds, psfs, M, N, mu, rho, nu, weights, term, bg, aniso, dtype):
    """x after every n of ITERATIONS, from one run of the model"""
    return {it: st["x"] for it, st in enumerate(tvframes_iterates(ds, psfs, M, N, mu, rho, max(ITERATIONS), weights, nu, term, bg, aniso, dtype))
            if it in ITERATIONS}


# the data terms of a case, with the parameters of the short cases of the single-frame forms: mu 5 .. 500, rho 1, 2, 10, nu = rho and
# not, both shrinkages, background 0 and > 0, the clamped output
COMBOS = (("ls mu50 rho1 nu3 aniso nonneg", LEAST_SQUARES, 0.0, 50.0, 1.0, 3.0, True, True),
          ("poisson b0 mu500 rho2 iso", POISSON, 0.0, 500.0, 2.0, 0.0, False, False),
          ("poisson b0.3 mu5 rho10 nu4 aniso nonneg", POISSON, 0.3, 5.0, 10.0, 4.0, True, True),
          ("ls mu500 rho2 iso", LEAST_SQUARES, 0.0, 500.0, 2.0, 0.0, False, False))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHORT, ids=SHORT_IDS)
def test_against_model(fdr, shape, K):
    """every n of ITERATIONS, both output windows and the three norm_area against the float64 model within TVFR_TOL and within 10x
    of the float32 CPU run of the model in the same metric; the weights kind, the PSF kind, the launch group and two of the four
    data-term combinations rotate with the case"""
    _need(fdr)
    M, N, rows, cols, stride, wstride, out_stride, outs = shape
    idx = SHORT.index(shape) + KS.index(K)
    kind = WEIGHT_KINDS[idx % 3]
    pkind = ("dense", "motion")[idx % 2]
    group = (1, 2, 3, 8)[idx % 4]
    psfs = short_psfs(pkind, K, M, N)
    ds = short_frames(M, N, rows, cols, K, psfs, 40 + idx)
    w = short_weights(kind, K, rows, cols, idx)
    bad, worst = [], (0.0, 0.0)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, group)
        p.set_frame_psfs(psfs)
        for name, term, bg, mu, rho, nu, aniso, nonneg in (COMBOS[idx % 4], COMBOS[(idx + 1) % 4]):
            x64 = _model_planes(ds, psfs, M, N, mu, rho, nu, w, term, bg, aniso, np.float64)
            x32 = _model_planes(ds, psfs, M, N, mu, rho, nu, w, term, bg, aniso, np.float32)
            for n in ITERATIONS:
                for orows, ocols in outs:
                    for area in (NORM_NONE, NORM_CROPPED, NORM_PADDED):
                        want = finish(x64[n], (orows, ocols), nonneg, area, M, N)
                        cpu32 = _err(finish(x32[n], (orows, ocols), nonneg, area, M, N), want, area)
                        kw = dict(data_term=term, background=bg, rho=rho, nu=nu, anisotropic=aniso, nonneg=nonneg, norm_area=area)
                        if (orows, ocols) == (rows, cols) and area == NORM_CROPPED:
                            got = p.tv_deconv_frames(ds, mu, n, weights=w, **kw)  # the host form
                        else:
                            got = _dev_call(p, ds, w, stride, wstride, out_stride, orows, ocols, mu, n, **kw)
                        e = _err(got, want, area)
                        worst = max(worst, (e, cpu32))
                        case = "%s K=%d %s weights=%s psf=%s group=%d n=%d out=%dx%d norm=%d" % (SHORT_IDS[SHORT.index(shape)], K, name, kind, pkind,
                                                                                                 group, n, orows, ocols, area)
                        print("TVM\tframes\t%s\terr=%.3g\tcpu32=%.3g" % (case, e, cpu32))
                        if not e <= TVFR_TOL:
                            bad.append("%s: error %.3g > %s" % (case, e, TVFR_TOL))
                        # (4 float32 roundings stand in where the CPU run happens to hit the model exactly: n = 0)
                        if not e <= 10 * max(cpu32, 4 * F32_EPS):
                            bad.append("%s: error %.3g above 10x the float32 CPU run's %.3g" % (case, e, cpu32))
    print("TVM\tworst\t%s K=%d\terr=%.3g\tcpu32=%.3g" % ((SHORT_IDS[SHORT.index(shape)], K) + worst))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("K", KS)
def test_table_kernel_through_one_iteration(fdr, K):
    """8 x 32, where the packed DC / Nyquist column is one of only sixteen and holds most of the table's case analysis:
    dense PSFs with unequal sums, whose Nyquist responses are not zero, n = 1, the whole plan, both data terms.  A table from frame
    0 alone (the model's fault) lies more than 100 TVFR_TOL away for K > 1, so the check has the power it claims."""
    _need(fdr)
    M, N = 8, 32
    psfs = short_psfs("dense", K, M, N)
    for p_ in psfs:  # the Nyquist responses: column N / 2 of the row transform, row M / 2 of the column transform
        plane = np.zeros((M, N))
        plane[:5, :5] = p_
        H = np.fft.fft2(plane)
        assert min(abs(H[0, N // 2]), abs(H[M // 2, 0]), abs(H[M // 2, N // 2])) > 1e-3
    ds = short_frames(M, N, M, N, K, psfs, 3)
    w = short_weights("per_frame", K, M, N, 3)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 3)
        p.set_frame_psfs(psfs)
        for term, bg in ((LEAST_SQUARES, 0.0), (POISSON, 0.2)):
            for nu, rho in ((3.0, 1.0), (0.0, 2.0)):
                want = tvframes_model(ds, psfs, M, N, 40.0, rho, 1, w, nu, term, bg, out_shape=(M, N))
                got = _dev_call(p, ds, w, N, N, N, M, N, 40.0, 1, data_term=term, background=bg, rho=rho, nu=nu)
                e = rel_err(got, want)
                print("TVM\ttable\tK=%d term=%d nu=%g rho=%g\terr=%.3g" % (K, term, nu, rho, e))
                assert e <= TVFR_TOL, (K, term, nu, rho, e)
                if K > 1:
                    bad = tvframes_model(ds, psfs, M, N, 40.0, rho, 1, w, nu, term, bg, out_shape=(M, N), fault="table_one")
                    assert rel_err(bad, want) > 100 * TVFR_TOL


# ---- bit identities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHORT, ids=SHORT_IDS)
def test_one_frame_has_the_bits_of_the_single_calls(fdr, shape):
    """K = 1: the bits of fdr_tv_deconv_free_f32_dev and fdr_tv_deconv_poisson_f32_dev under that PSF as the operator PSF"""
    _need(fdr)
    import torch
    M, N, rows, cols, stride, wstride, out_stride, outs = shape
    for pkind in ("dense", "motion"):
        psf = short_psfs(pkind, 2, M, N)[1]
        d = short_frames(M, N, rows, cols, 1, [psf], 9)[0]
        for wkind in ("none", "per_frame"):
            w = short_weights(wkind, 1, rows, cols, 2)
            d_in, _ = _to_dev([d], stride)
            d_w = _to_dev([w[0]], wstride, 7.0)[0] if w is not None else None
            with fdr.Plan(M, N, fdr.MODE_FAST) as p:
                p.set_operator_psf(psf)
                p.set_frame_psfs([psf])
                for n, area, aniso, nonneg, (orows, ocols) in ((0, NORM_NONE, False, False, outs[0]), (1, NORM_NONE, True, True, outs[-1]),
                                                               (5, NORM_PADDED, False, True, outs[0]), (10, NORM_CROPPED, True, False, outs[-1])):
                    for term, bg in ((LEAST_SQUARES, 0.0), (POISSON, 0.0), (POISSON, 0.3)):
                        ostr = max(out_stride, ocols + 3)
                        d_out = torch.full((orows + 1, ostr), float("nan"), dtype=torch.float32, device="cuda")
                        kw = dict(d_weights=d_w.data_ptr() if d_w is not None else None, wstride=wstride if d_w is not None else 0, nu=3.0,
                                  anisotropic=aniso, nonneg=nonneg, norm_area=area, out_rows=orows, out_cols=ocols)
                        if term == POISSON:
                            p.tv_deconv_poisson_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), ostr, 50.0, 1.0, n, background=bg, **kw)
                        else:
                            p.tv_deconv_free_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), ostr, 50.0, 1.0, n, **kw)
                        torch.cuda.synchronize()
                        want = d_out.cpu().numpy()[:orows, :ocols]
                        got = _dev_call(p, [d], w, stride, wstride, out_stride, orows, ocols, 50.0, n, data_term=term, background=bg, rho=1.0, nu=3.0,
                                        anisotropic=aniso, nonneg=nonneg, norm_area=area)
                        assert np.array_equal(got, want), "K = 1 %s %s term %d b %g n = %d norm %d: not the bits of the single call" % (
                            pkind, wkind, term, bg, n, area)


@pytest.mark.parametrize("K", [5, 8])
def test_same_bits_for_every_group_and_in_two_calls(fdr, K):
    """the plan groups 1 .. 8 (K = 5 in groups of 2, 3 and 4 has a tail), two consecutive calls and the host form: the same bytes"""
    _need(fdr)
    M, N, rows, cols, stride, wstride, out_stride, _ = SHORT[2]
    psfs = short_psfs("motion", K, M, N)
    ds = short_frames(M, N, rows, cols, K, psfs, 7)
    w = short_weights("per_frame", K, rows, cols, 9)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_frame_psfs(psfs)
        ref = {}
        for group in range(1, 9):
            p.set_batching(1, group)
            for term, bg in ((LEAST_SQUARES, 0.0), (POISSON, 0.1)):
                for wk in (w, w[0], None):
                    key = (term, wk is None, wk is not None and wk.ndim)
                    a = _dev_call(p, ds, wk, stride, wstride, out_stride, M, N, 30.0, 6, data_term=term, background=bg)
                    b = _dev_call(p, ds, wk, stride, wstride, out_stride, M, N, 30.0, 6, data_term=term, background=bg)
                    assert np.array_equal(a, b), "two consecutive calls differ (group %d)" % group
                    if group == 1:
                        ref[key] = a
                    assert np.array_equal(a, ref[key]), "group %d differs from group 1 (%s)" % (group, key)
        host = p.tv_deconv_frames(ds, 30.0, 6, weights=w, full_plane=True)
        assert np.array_equal(host, ref[(LEAST_SQUARES, False, 3)]), "the host form differs from the _dev form"
        assert not np.array_equal(ref[(LEAST_SQUARES, False, 3)], ref[(LEAST_SQUARES, False, 2)])  # the per-frame weights are read


def test_convenience_calls(fdr):
    """tvDeblurFrames_myfft is the plan's call on the plan it documents; tvDeblurFrames_RGB is that call per channel"""
    _need(fdr)
    M, N, rows, cols = 64, 128, 37, 101
    K = 3
    psfs = short_psfs("dense", K, M, N)
    ch = [short_frames(M, N, rows, cols, K, psfs, seed) for seed in (11, 12)]  # two channels of K frames each
    w = short_weights("per_frame", K, rows, cols, 1)
    assert fdr._frames_plan_size(rows, cols, psfs) == (M, N)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_frame_psfs(psfs)
        want = [p.tv_deconv_frames(c, 40.0, 4, weights=w, data_term=POISSON, background=0.1) for c in ch]
    got = [fdr.tvDeblurFrames_myfft(c, psfs, 40.0, 4, weights=w, data_term=POISSON, background=0.1) for c in ch]
    rgb = fdr.tvDeblurFrames_RGB([[ch[0][k], ch[1][k]] for k in range(K)], psfs, 40.0, 4, weights=w, data_term=POISSON, background=0.1)
    for c in range(2):
        assert np.array_equal(got[c], want[c]) and np.array_equal(rgb[c], want[c]), c


# ---- plan state and hygiene ----------------------------------------------------------------------------------------------------------------
def test_isolation(fdr):
    """free TV, Poisson TV, RL frames, blur, periodic TV and Wiener give their old bytes before and after frames calls (the shared solve
    table is rebuilt by whoever needs it, in both directions), the frame tables are untouched by them, and a new frame set
    invalidates the table"""
    _need(fdr)
    from _spectral import tone_image
    M, N, rows, cols = 64, 128, 37, 101
    img = tone_image(M, N, 21, rows, cols)
    K = 3
    psfs = short_psfs("motion", K, M, N)
    ds = short_frames(M, N, rows, cols, K, psfs, 3)
    w = short_weights("per_frame", K, rows, cols, 3)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 2)

        def others():
            p.set_psf_motion(7, 30.0, 0.01)
            return [p.wiener(img), p.blur(img), p.blur(img, adjoint=True), p.tv_deconv_free(img, 30.0, iterations=3, weights=w[0]),
                    p.tv_deconv_poisson(img, 30.0, iterations=3, weights=w[0], background=0.1), p.tv_deconv(img, 30.0, iterations=3),
                    p.richardson_lucy_frames(ds, 3, weights=w)]

        def frames_calls():
            return [p.tv_deconv_frames(ds, 30.0, 3, weights=w), p.tv_deconv_frames(ds, 30.0, 2, weights=w, data_term=POISSON, background=0.1,
                                                                                 norm_area=NORM_PADDED, full_plane=True)]

        p.set_operator_psf_motion(7, 30.0)
        p.set_frame_psfs(psfs)
        before = others()
        a = frames_calls()
        after = others()
        for k, (x, y) in enumerate(zip(before, after)):
            assert np.array_equal(x, y), "result %d changed after the frames calls" % k
        # the free call builds the operator's table for the (nu, rho) of the frames calls: neither may take the other's for its own
        assert np.array_equal(p.tv_deconv_free(img, 30.0, iterations=3, weights=w[0]), before[3])
        for x, y in zip(a, frames_calls()):
            assert np.array_equal(x, y), "a frames call right after a free call with the same nu and rho changed"
        assert np.array_equal(p.tv_deconv_free(img, 30.0, iterations=3, weights=w[0]), before[3]), "a free call right after a frames call changed"
        p.set_operator_psf_motion(9, 100.0)  # another operator PSF: the frame tables are their own
        for x, y in zip(a, frames_calls()):
            assert np.array_equal(x, y), "a frames call changed with the operator PSF"
        p.set_frame_psfs(psfs[::-1])  # another frame set: the table is built again
        c = p.tv_deconv_frames(ds, 30.0, 3, weights=w)
        assert not np.array_equal(c, a[0])
        p.set_frame_psfs(psfs)
        assert np.array_equal(p.tv_deconv_frames(ds, 30.0, 3, weights=w), a[0])


def test_later_calls_allocate_nothing(fdr):
    _need(fdr)
    import torch
    M, N, rows, cols, stride = 64, 128, 37, 101, 103
    K = 3
    psfs = short_psfs("motion", K, M, N)
    ds = short_frames(M, N, rows, cols, K, psfs, 3)
    d_in, pitch = _to_dev(ds, stride)
    d_out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 2)
        p.set_frame_psfs(psfs)

        def call(term):
            p.tv_deconv_frames_dev(d_in.data_ptr(), pitch, K, rows, cols, stride, d_out.data_ptr(), cols, 30.0, 2, data_term=term)

        call(LEAST_SQUARES)  # the first call makes the workspaces
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for term in (LEAST_SQUARES, POISSON, LEAST_SQUARES, POISSON):
            call(term)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "a later call allocated device memory"


def _prm(fdr, mu=10.0, rho=2.0, nu=0.0, bg=0.0, term=0, n=1, aniso=0, nonneg=0, area=0, orows=8, ocols=8):
    return fdr.TvFramesParams(mu, rho, nu, bg, term, n, aniso, nonneg, area, orows, ocols, None)


def test_refusals(fdr):
    """every refusal, host and _dev form alike, and a plan that still works afterwards"""
    _need(fdr)
    from _spectral import tone_image
    L = fdr.lib
    psf = fdr.motionBlurKernel(15, 30.0)
    imgs = np.stack([tone_image(64, 64, 3), tone_image(64, 64, 4)])
    out = np.empty((64, 64), dtype=np.float32)
    w = np.ones((2, 64, 64), dtype=np.float32)

    def call(p, pitch=4096, count=2, rows=8, cols=8, stride=64, wp=None, wpitch=0, ws=64, op=None, ostride=64, pr=None, dev=False):
        f = L.fdr_tv_deconv_frames_f32_dev if dev else L.fdr_tv_deconv_frames_f32
        return f(p._h, imgs.ctypes.data, pitch, count, rows, cols, stride, wp, wpitch, ws, out.ctypes.data if op is None else op, ostride,
                 ctypes.byref(_prm(fdr) if pr is None else pr))

    def both(p, **kw):
        """the code both forms give (every refusal comes before a pointer is followed, so the _dev form may see host pointers here)"""
        a, b = call(p, **kw), call(p, dev=True, **kw)
        assert a == b, (a, b, kw)
        return a

    for M, N, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (64, 64, fdr.MODE_FAST, fdr.FLAG_SIMPLE_PATH, "simple"),
                                    (64, 64, fdr.MODE_FAST, fdr.FLAG_FULL_SPECTRUM, "full spectrum"), (64, 16, fdr.MODE_FAST, 0, "N < 32"),
                                    (75, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX, "mixed radix")):
        with fdr.Plan(M, N, mode, flags=flags) as p:
            assert both(p) == -1, what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert both(p) == -4
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        p.profile(True)
        assert both(p) == -4 and b"frame PSFs" in L.fdr_last_error()  # no frame tables
        p.set_frame_psfs([psf, psf])
        p.pass_times()  # reads and clears the records of the PSF passes
        assert L.fdr_tv_deconv_frames_f32(p._h, imgs.ctypes.data, 4096, 2, 8, 8, 64, None, 0, 0, out.ctypes.data, 64, None) == -1  # null params
        for count in (1, 3, 0, 9):
            assert both(p, count=count) == -1, count
        # what the free call refuses
        for bad in (dict(mu=0.0), dict(mu=-1.0), dict(mu=float("nan")), dict(rho=0.0), dict(rho=float("inf")), dict(nu=-1.0), dict(nu=float("nan")),
                    dict(n=-1), dict(area=3), dict(area=-1), dict(orows=7), dict(ocols=7), dict(orows=65), dict(ocols=65), dict(orows=0, ocols=0)):
            assert both(p, pr=_prm(fdr, **bad)) == -1, bad
        assert both(p, ostride=32, pr=_prm(fdr, ocols=40)) == -1
        assert both(p, rows=65) == -1 and both(p, cols=65, stride=65) == -1 and both(p, rows=0) == -1 and both(p, stride=4) == -1
        assert both(p, wp=w.ctypes.data, ws=4) == -1
        # the data term and the background
        for term in (2, -1):
            assert both(p, pr=_prm(fdr, term=term)) == -1 and b"data_term" in L.fdr_last_error(), term
        for bg in (-0.1, float("nan"), float("inf")):
            assert both(p, pr=_prm(fdr, term=1, bg=bg)) == -1 and b"background" in L.fdr_last_error(), bg
        assert both(p, pr=_prm(fdr, term=0, bg=0.1)) == -1 and b"least-squares" in L.fdr_last_error()
        # the frames' and the weights' layout
        assert both(p, pitch=7 * 64 + 7) == -1 and b"img_pitch" in L.fdr_last_error()
        assert both(p, wp=w.ctypes.data, wpitch=7 * 64 + 7) == -1 and b"weight_pitch" in L.fdr_last_error()
        assert both(p, op=imgs.ctypes.data + 4 * 4096) == -1 and b"overlaps a frame" in L.fdr_last_error()  # the second frame
        assert both(p, wp=w.ctypes.data, wpitch=4096, op=w.ctypes.data + 4 * (4096 + 64 * 3)) == -1 and b"overlaps the weights" in L.fdr_last_error()
        assert sum(c for _, _, c in p.pass_times()) == 0, "a refused call launched a pass"
        assert call(p, wp=w.ctypes.data, op=w.ctypes.data + 4 * 4096) == 0  # one weights plane: the second is not read
        assert call(p, wp=w.ctypes.data, wpitch=4096) == 0  # the plan still works
        assert call(p, wp=w.ctypes.data, wpitch=4096, pr=_prm(fdr, term=1, bg=0.1)) == 0


def test_pass_names(fdr):
    """K = 3 on launch groups of 2 (a group of two and a tail of one), n = 2, clamped and normalised, on a fresh profiled plan: the
    passes by name and count -- the existing names wherever the pass is the existing kernel, one new name -- all within
    FDR_MAX_PASSES, the two passes of the frame setter included"""
    _need(fdr)
    M, N, rows, cols = 64, 128, 37, 101
    K, n = 3, 2
    psfs = short_psfs("dense", K, M, N)
    ds = short_frames(M, N, rows, cols, K, psfs, 1)
    w = short_weights("per_frame", K, rows, cols, 1)
    for term, data_name in ((LEAST_SQUARES, "TVF data: s, q, r = 2s-e (window)"), (POISSON, "TVP data: Poisson s, q, r = 2s-e (window)")):
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            p.set_batching(1, 2)
            p.profile(True)
            p.set_frame_psfs(psfs)
            p.tv_deconv_frames(ds, 30.0, n, weights=w, data_term=term, nonneg=True, norm_area=NORM_PADDED)
            names = {name: c for name, _, c in p.pass_times()}
        print("TVM\tpasses\t%s" % names)
        assert len(names) <= fdr.MAX_PASSES, "the names overflow FDR_MAX_PASSES"
        want = {"O rows: PSF pad+FFT (operator)": K, "O cols: FFT -> H/MN, conj(H)/MN": K,
                "TV table: 1/(nu sum|H_k|^2+rho L)/MN (frames)": 1, "TVF init: x = pad(d), w = q = 0": 1,
                "A op rows: pad+FFT (blur / RL), group": 2 * n, "A op rows: pad+FFT (blur / RL)": 3 * n,
                "B' op cols: FFT*H_k*IFFT (frame)": K * n, "B' op cols: FFT*conj(H_k)*IFFT (frame)": K * n, data_name: 2 * n,
                "S frames: sum of spectra": 2 * n, "C op rows: IFFT+crop (frames)": 3 * n, "TV spatial: shrink+dual+div (free)": n,
                "B' op cols: FFT*T*IFFT (TVF solve)": n, "C op rows: IFFT (TVF x)": n, "TVF out: crop+clamp": 1, "E TVF minmax+normalize": 1}
        for name, c in want.items():
            assert names.get(name) == c, (name, names.get(name), c)
        assert set(names) == set(want), set(names) ^ set(want)


def test_quality_matches_the_model(fdr):
    """the three-frame quality case of test_tvframes_host.py on the device at the model's best mu, n = 100, both data terms: within
    0.1 dB of the model's PSNR"""
    _need(fdr)
    case = quality_case()
    with fdr.Plan(case["M"], case["N"], fdr.MODE_FAST) as p:
        p.set_batching(1, 3)
        p.set_frame_psfs(case["psfs"])
        for term in (LEAST_SQUARES, POISSON):
            mu = QUALITY_JOINT_MU[term]
            pm = quality_psnr(case, [0, 1, 2], mu, term)
            pg = psnr(p.tv_deconv_frames(case["ds"], mu, QUALITY_N, data_term=term, rho=QUALITY_RHO), case["truth"])
            print("TVM\tquality\tterm %d mu %g: model %.3f dB, GPU %.3f dB" % (term, mu, pm, pg))
            assert abs(pm - QUALITY_MEASURED[term][3]) <= 0.05, (pm, QUALITY_MEASURED[term])
            assert abs(pg - pm) <= 0.1, (term, pm, pg)
