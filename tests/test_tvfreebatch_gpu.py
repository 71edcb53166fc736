"""Free-boundary and noise-constrained TV deconvolution in groups (fdr_tv_deconv_free_batch_f32*, fdr_tv_deconv_auto_batch_f32*) on
the MI355X.  Uncoupled: every image of a batch, and every entry of its trace, has the bits of the single _dev call on the same plan,
for 1, 3 and 5 images in groups of 1, 2, 3, 4 and 8 (tails 5 = 2 + 2 + 1 and 3 in 4), a loose odd pitch (the images differ in
16-byte alignment), odd strides, weights none / mask / fractional, both shrinkages, the three norm_area values and the M x N output
window; for the auto form a noise level per image, one of them estimated, and the common level.  Coupled: three channels against
the float64 model of tests/_tvfreebatch_model.py, outputs and traces.  Then the refusals, the workspaces, the pass list and the
wrappers.  Cases print a `TVFB` line with their measured values (pytest -s)."""
import ctypes

import numpy as np
import pytest

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, dense_psf
from _tvauto_model import f32, trace_err
from _tvfree_model import tvf_image, tvf_weights
from _tvfreebatch_model import (COUPLED, COUPLED_IDS, COUPLED_PLANS, COUPLED_SIGMAS, TVFB_AUTO_TOL, TVFB_TOL, TVFB_TRACE_TOL, coupled_case,
                                group_iterates, rel_err)

pytestmark = pytest.mark.gpu

N_IT = 2  # iterations of the bit cases: the second one reads every dual the first one wrote


class Batch:
    """`count` windows on the device, image i at i * pitch floats (NaN between the rows and between the images: a read outside a
    window poisons the result), the weights window with its own stride, and NaN-filled outputs and traces"""

    def __init__(self, imgs, stride, pitch, weights, wstride):
        import torch
        self.count, self.rows, self.cols = imgs.shape
        self.stride, self.pitch, self.wstride = stride, pitch, wstride
        src = np.full(((self.count - 1) * pitch + self.rows * stride,), np.nan, dtype=np.float32)
        for i in range(self.count):
            for r in range(self.rows):
                src[i * pitch + r * stride: i * pitch + r * stride + self.cols] = imgs[i, r]
        self.d_in = torch.from_numpy(src).cuda()
        self.d_w = None
        if weights is not None:
            w = np.full((self.rows, wstride), np.nan, dtype=np.float32)
            w[:, :self.cols] = weights
            self.d_w = torch.from_numpy(w).cuda()

    def img_ptr(self, i=0):
        return self.d_in.data_ptr() + 4 * i * self.pitch

    def w_ptr(self):
        return self.d_w.data_ptr() if self.d_w is not None else None


def _outputs(count, out_shape, out_stride, out_pitch):
    import torch
    return torch.full(((count - 1) * out_pitch + out_shape[0] * out_stride,), float("nan"), dtype=torch.float32, device="cuda")


def _read_outputs(d_out, count, out_shape, out_stride, out_pitch):
    """[count, out_shape] from the device, after checking that everything outside the output windows is still NaN"""
    flat = d_out.cpu().numpy()
    seen = np.zeros(flat.shape, dtype=bool)
    outs = np.empty((count,) + tuple(out_shape), dtype=np.float32)
    for i in range(count):
        for r in range(out_shape[0]):
            at = i * out_pitch + r * out_stride
            outs[i, r] = flat[at:at + out_shape[1]]
            seen[at:at + out_shape[1]] = True
    assert np.all(np.isnan(flat[~seen])), "a store landed outside the output windows"
    return outs


def _free_batch(p, b, count, out_shape, out_stride, out_pitch, mu, rho, n, nu=0.0, aniso=False, nonneg=False, area=NORM_NONE, coupled=False):
    import torch
    d_out = _outputs(count, out_shape, out_stride, out_pitch)
    p.tv_deconv_free_batch_dev(b.img_ptr(), b.pitch, count, b.rows, b.cols, b.stride, d_out.data_ptr(), out_pitch, out_stride, mu, rho, n, b.w_ptr(),
                               b.wstride, nu, aniso, nonneg, area, out_shape[0], out_shape[1], coupled)
    torch.cuda.synchronize()
    return _read_outputs(d_out, count, out_shape, out_stride, out_pitch)


def _auto_batch(p, b, count, out_shape, out_stride, out_pitch, sigma, sigmas, rho, n, nu=0.0, aniso=False, nonneg=False, area=NORM_NONE, tau=0.0,
                coupled=False):
    import torch
    tp = 3 * n + 1
    d_out = _outputs(count, out_shape, out_stride, out_pitch)
    d_tr = torch.full((count * tp + 2,), float("nan"), dtype=torch.float64, device="cuda")
    p.tv_deconv_auto_batch_dev(b.img_ptr(), b.pitch, count, b.rows, b.cols, b.stride, d_out.data_ptr(), out_pitch, out_stride, sigma, rho, n, b.w_ptr(),
                               b.wstride, tau, nu, aniso, nonneg, area, out_shape[0], out_shape[1], sigmas, d_tr.data_ptr(), tp, coupled)
    torch.cuda.synchronize()
    tr = d_tr.cpu().numpy()
    assert np.all(np.isnan(tr[count * tp:])) and np.all(np.isnan(tr[:count * tp].reshape(count, tp)[:, 3 * n:])), "a store landed outside the traces"
    return _read_outputs(d_out, count, out_shape, out_stride, out_pitch), tr[:count * tp].reshape(count, tp)[:, :3 * n].reshape(count, n, 3)


def _free_single(p, b, i, out_shape, out_stride, mu, rho, n, nu, aniso, nonneg, area):
    import torch
    d_out = _outputs(1, out_shape, out_stride, 0)
    p.tv_deconv_free_dev(b.img_ptr(i), b.rows, b.cols, b.stride, d_out.data_ptr(), out_stride, mu, rho, n, b.w_ptr(), b.wstride, nu, aniso, nonneg, area,
                         out_shape[0], out_shape[1])
    torch.cuda.synchronize()
    return _read_outputs(d_out, 1, out_shape, out_stride, 0)[0]


def _auto_single(p, b, i, out_shape, out_stride, sigma, rho, n, nu, aniso, nonneg, area, tau):
    import torch
    d_out = _outputs(1, out_shape, out_stride, 0)
    d_tr = torch.full((3 * n,), float("nan"), dtype=torch.float64, device="cuda")
    p.tv_deconv_auto_dev(b.img_ptr(i), b.rows, b.cols, b.stride, d_out.data_ptr(), out_stride, sigma, rho, n, b.w_ptr(), b.wstride, tau, nu, aniso, nonneg,
                         area, out_shape[0], out_shape[1], d_tr.data_ptr())
    torch.cuda.synchronize()
    return _read_outputs(d_out, 1, out_shape, out_stride, 0)[0], d_tr.cpu().numpy().reshape(n, 3)


def _images(M, N, rows, cols, count):
    """`count` different windows: tvf_image with a seed per image, scaled so that their noise levels and discrepancies differ"""
    return np.stack([tvf_image(M, N, rows, cols, 11 + 7 * i) * np.float32(1.0 - 0.1 * i) for i in range(count)])


# (M, N, rows, cols, stride, wstride, odd out_stride): the full window, strides 31 / 33 / 35, a window of a residue 1 mod 4, more than one workgroup
BIT_PLANS = [(8, 32, 8, 32, 32, 32, 32), (16, 32, 9, 30, 31, 33, 35), (64, 128, 37, 101, 103, 101, 131), (256, 256, 200, 151, 163, 152, 259)]
BIT_IDS = ["%dx%d-win%dx%d" % c[:4] for c in BIT_PLANS]
COUNTS_GROUPS = [(c, g) for c in (1, 3, 5) for g in (1, 2, 3, 4, 8)]
# a level per image, as the float parameter of the single call holds it: one estimated (0), one so large that mu_k clamps at 0
SIGMAS5 = tuple(f32(s) for s in (0.02, 0.05, 0.0, 0.03, 0.3))


def _settings(M, N, rows, cols):
    """(weights kind, anisotropic, nonneg, norm_area, output window, auto: (sigma, sigmas)): the three weights, both shrinkages, the
    three norm_area values with nonneg, the M x N output window; the common level, a level per image, and one image estimated"""
    return [("none", False, True, NORM_NONE, (rows, cols), (0.02, None)),
            ("mask", True, True, NORM_CROPPED, (M, N), (0.0, [s or f32(0.04) for s in SIGMAS5])),
            ("fractional", False, True, NORM_PADDED, (rows, cols), (0.5, list(SIGMAS5)))]


def _psf_for(fdr, M, N, rows, cols):
    motion = fdr.motionBlurKernel(15, 30.0)
    if motion.shape[0] > M or motion.shape[1] > N:
        return dense_psf(5, 5)
    return motion if (rows, cols) == (M, N) else centred_psf(motion, M, N)


@pytest.mark.parametrize("form", ["free", "auto"])
@pytest.mark.parametrize("plan", BIT_PLANS, ids=BIT_IDS)
def test_uncoupled_bits(fdr, plan, form):
    """np.array_equal against the single _dev call on the same plan, image by image, traces included"""
    M, N, rows, cols, stride, wstride, ostride = plan
    imgs = _images(M, N, rows, cols, 5)
    pitch = rows * stride + 5  # loose and odd: image 1 is not 16-byte aligned where image 0 is
    checked = 0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(_psf_for(fdr, M, N, rows, cols))
        for kind, aniso, nonneg, area, out_shape, (sigma, sigmas) in _settings(M, N, rows, cols):
            b = Batch(imgs, stride, pitch, tvf_weights(kind, rows, cols, 5), wstride)
            out_stride = ostride if ostride >= out_shape[1] else out_shape[1] + 3
            out_pitch = out_shape[0] * out_stride + 3
            p.set_batching(1, 1)
            if form == "free":
                want = [_free_single(p, b, i, out_shape, out_stride, 50.0, 2.0, N_IT, 3.0, aniso, nonneg, area) for i in range(5)]
            else:
                ref = [_auto_single(p, b, i, out_shape, out_stride, sigmas[i] if sigmas else sigma, 2.0, N_IT, 20.0, aniso, nonneg, area, 1.2) for i in range(5)]
                want, want_tr = [r[0] for r in ref], [r[1] for r in ref]
            assert all(np.all(np.isfinite(w)) for w in want) and not np.array_equal(want[0], want[1])
            for count, group in COUNTS_GROUPS:
                p.set_batching(1, group)
                if form == "free":
                    got = _free_batch(p, b, count, out_shape, out_stride, out_pitch, 50.0, 2.0, N_IT, 3.0, aniso, nonneg, area)
                else:
                    got, got_tr = _auto_batch(p, b, count, out_shape, out_stride, out_pitch, sigma, sigmas[:count] if sigmas else None, 2.0, N_IT, 20.0,
                                              aniso, nonneg, area, 1.2)
                for i in range(count):
                    what = (form, kind, "count %d group %d image %d" % (count, group, i))
                    assert np.array_equal(got[i], want[i]), what + (float(np.nanmax(np.abs(got[i] - want[i]))),)
                    if form == "auto":
                        assert np.array_equal(got_tr[i], want_tr[i]), what + (got_tr[i], want_tr[i])
                    checked += 1
    print("TVFB\tbits\t%dx%d win %dx%d %s\t%d images equal their single calls" % (M, N, rows, cols, form, checked))


@pytest.mark.parametrize("form", ["free", "auto"])
def test_uncoupled_bits_many_partials(fdr, form):
    """2048 x 512, window 2000 x 333, three images in one group, one iteration: every image has more than 256 partials of each sum,
    so the fold of image z strides over its own block"""
    M, N, rows, cols, stride, wstride = 2048, 512, 2000, 333, 347, 336
    rng = np.random.default_rng(3)
    imgs = rng.random((3, rows, cols), dtype=np.float32) - np.float32(0.1)
    b = Batch(imgs, stride, rows * stride + 5, (rng.random((rows, cols)) > 0.02).astype(np.float32), wstride)
    out_shape, out_stride = (rows, cols), 335
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(centred_psf(fdr.motionBlurKernel(15, 30.0), M, N))
        p.set_batching(1, 3)
        if form == "free":
            got = _free_batch(p, b, 3, out_shape, out_stride, rows * out_stride + 1, 50.0, 2.0, 1)
            for i in range(3):
                assert np.array_equal(got[i], _free_single(p, b, i, out_shape, out_stride, 50.0, 2.0, 1, 0.0, False, False, NORM_NONE)), i
        else:
            sig = [f32(0.02), f32(0.05), f32(0.03)]
            got, tr = _auto_batch(p, b, 3, out_shape, out_stride, rows * out_stride + 1, 0.0, sig, 2.0, 1)
            for i in range(3):
                o, t = _auto_single(p, b, i, out_shape, out_stride, sig[i], 2.0, 1, 0.0, False, False, NORM_NONE, 0.0)
                assert np.array_equal(got[i], o) and np.array_equal(tr[i], t), (i, tr[i], t)
            assert len({float(t[0, 2]) for t in tr}) == 3 and np.all(tr[:, 0, 2] > 0)


def _model_planes(d, psf, M, N, w, ns, auto):
    """({n: x [3, M, N]}, traces [3, max(ns), 3]) of the coupled float64 model, one run"""
    kw = dict(sigmas=[f32(s) for s in COUPLED_SIGMAS], nu=COUPLED["nu_auto"]) if auto else dict(mu=COUPLED["mu"], nu=COUPLED["nu_free"])
    planes, traces = {}, []
    for k, st in enumerate(group_iterates(d, psf, M, N, rho=COUPLED["rho"], iterations=max(ns), weights=w, coupled=True, **kw)):
        if k in ns:
            planes[k] = np.array(st["x"], dtype=np.float64)
        if "trace" in st:
            traces.append(st["trace"])
    return planes, np.array(traces).reshape(-1, 3, 3).transpose(1, 0, 2)


def _coupled_against_model(fdr, plan, ns):
    M, N, rows, cols = plan
    d, psf, w = coupled_case(M, N, rows, cols)
    stride, wstride, out_stride = cols + 3, cols + 1, N + 5
    b = Batch(d, stride, rows * stride + 5, w, wstride)
    bad, worst = [], dict(free=0.0, auto=0.0, trace=0.0)
    free_m, _ = _model_planes(d, psf, M, N, w, ns, False)
    auto_m, trace_m = _model_planes(d, psf, M, N, w, ns, True)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        p.set_batching(1, 3)
        for n in ns:
            for out_shape in ((rows, cols), (M, N)):
                op = out_shape[0] * out_stride + 3
                got = _free_batch(p, b, 3, out_shape, out_stride, op, COUPLED["mu"], COUPLED["rho"], n, COUPLED["nu_free"], coupled=True)
                e = max(rel_err(got[c], free_m[n][c, :out_shape[0], :out_shape[1]]) for c in range(3))
                got, tr = _auto_batch(p, b, 3, out_shape, out_stride, op, 0.0, [f32(s) for s in COUPLED_SIGMAS], COUPLED["rho"], n, COUPLED["nu_auto"], coupled=True)
                ea = max(rel_err(got[c], auto_m[n][c, :out_shape[0], :out_shape[1]]) for c in range(3))
                et = max(trace_err(tr[c], trace_m[c, :n]) for c in range(3))
                what = "%dx%d win %dx%d out %dx%d n=%d" % (M, N, rows, cols, out_shape[0], out_shape[1], n)
                print("TVFB\tcoupled\t%s\tfree=%.3g auto=%.3g trace=%.3g mu_k=%s" % (what, e, ea, et, " ".join("%.4g" % v for v in trace_m[:, n - 1, 2])))
                worst = dict(free=max(worst["free"], e), auto=max(worst["auto"], ea), trace=max(worst["trace"], et))
                if not e <= TVFB_TOL:
                    bad.append("%s: free error %.3g > %.3g" % (what, e, TVFB_TOL))
                if not ea <= TVFB_AUTO_TOL:
                    bad.append("%s: auto error %.3g > %.3g" % (what, ea, TVFB_AUTO_TOL))
                if not et <= TVFB_TRACE_TOL:
                    bad.append("%s: trace error %.3g > %.3g" % (what, et, TVFB_TRACE_TOL))
    print("TVFB\tworst\t%dx%d win %dx%d n<=%d\tfree %.3g auto %.3g trace %.3g" % (M, N, rows, cols, max(ns), worst["free"], worst["auto"], worst["trace"]))
    return bad


@pytest.mark.parametrize("plan", COUPLED_PLANS, ids=COUPLED_IDS)
def test_coupled_against_model(fdr, plan):
    bad = _coupled_against_model(fdr, plan, (1, 2, 3))
    assert not bad, "\n".join(bad)


def test_coupled_against_model_30_steps(fdr):
    bad = _coupled_against_model(fdr, COUPLED_PLANS[1], (30,))
    assert not bad, "\n".join(bad)


def test_coupled_one_channel_and_coupling_matters(fdr):
    """coupled with count = 1 gives the single call's bits (the joint norm of one channel is its own); coupled with three channels
    differs from uncoupled in every channel"""
    M, N, rows, cols = COUPLED_PLANS[1]
    d, psf, w = coupled_case(M, N, rows, cols)
    b = Batch(d, cols + 3, rows * (cols + 3) + 5, w, cols + 1)
    out_shape, out_stride = (rows, cols), cols + 2
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        p.set_batching(1, 3)
        one = _free_batch(p, b, 1, out_shape, out_stride, 0, 50.0, 2.0, 3, 3.0, coupled=True)[0]
        assert np.array_equal(one, _free_single(p, b, 0, out_shape, out_stride, 50.0, 2.0, 3, 3.0, False, False, NORM_NONE))
        one, tr = _auto_batch(p, b, 1, out_shape, out_stride, 0, 0.02, None, 2.0, 3, coupled=True)
        o, t = _auto_single(p, b, 0, out_shape, out_stride, 0.02, 2.0, 3, 0.0, False, False, NORM_NONE, 0.0)
        assert np.array_equal(one[0], o) and np.array_equal(tr[0], t)
        op = rows * out_stride + 1
        for coupled_auto in (False, True):
            if coupled_auto:
                a = _auto_batch(p, b, 3, out_shape, out_stride, op, 0.02, None, 2.0, 3, coupled=True)[0]
                u = _auto_batch(p, b, 3, out_shape, out_stride, op, 0.02, None, 2.0, 3, coupled=False)[0]
            else:
                a = _free_batch(p, b, 3, out_shape, out_stride, op, 50.0, 2.0, 3, 3.0, coupled=True)
                u = _free_batch(p, b, 3, out_shape, out_stride, op, 50.0, 2.0, 3, 3.0, coupled=False)
            for c in range(3):
                assert rel_err(a[c], u[c].astype(np.float64)) > 1e-3, (coupled_auto, c)


def test_refusals(fdr):
    """every refusal of the batched forms returns FDR_ERR_ARG before any device work and leaves the plan usable: a good call
    afterwards gives the bits of a fresh plan"""
    import torch
    L = fdr.lib
    M = N = 64
    rows, cols, count, n = 40, 48, 3, 2
    px = rows * cols
    psf = dense_psf(5, 5)
    imgs = _images(M, N, rows, cols, count)
    d = torch.from_numpy(imgs).cuda()
    dw = torch.from_numpy(tvf_weights("mask", rows, cols, 3)).cuda()
    do = torch.empty((count, rows, cols), dtype=torch.float32, device="cuda")
    dtr = torch.zeros(count * 3 * n + 8, dtype=torch.float64, device="cuda")
    sig = (ctypes.c_double * count)(0.02, 0.03, 0.04)

    def free(p, i=d.data_ptr(), w=dw.data_ptr(), o=do.data_ptr(), count=count, rows=rows, cols=cols, stride=cols, wstride=cols, out_stride=cols, pitch=px,
             opitch=px, mu=50.0, rho=2.0, nu=0.0, n=n, aniso=0, area=0, out_rows=rows, out_cols=cols, coupling=0, prm=True, plan=True, **_):
        q = fdr.TvFreeBatchParams(mu, rho, nu, n, aniso, 0, area, out_rows, out_cols, coupling)
        return L.fdr_tv_deconv_free_batch_f32_dev(p._h if plan else None, i, pitch, count, rows, cols, stride, w, wstride, o, opitch, out_stride,
                                                  ctypes.byref(q) if prm else None, None)

    def auto(p, i=d.data_ptr(), w=dw.data_ptr(), o=do.data_ptr(), count=count, rows=rows, cols=cols, stride=cols, wstride=cols, out_stride=cols, pitch=px,
             opitch=px, sigma=0.02, tau=0.0, rho=2.0, nu=0.0, n=n, aniso=0, area=0, out_rows=rows, out_cols=cols, coupling=0, prm=True, plan=True,
             sigmas=None, trace=None, tpitch=3 * n, **_):
        q = fdr.TvAutoBatchParams(sigma, tau, rho, nu, n, aniso, 0, area, out_rows, out_cols, coupling)
        return L.fdr_tv_deconv_auto_batch_f32_dev(p._h if plan else None, i, pitch, count, rows, cols, stride, w, wstride, o, opitch, out_stride,
                                                  ctypes.byref(q) if prm else None, sigmas, trace, tpitch, None)

    def good(p):
        p.set_batching(1, 2)
        a = p.tv_deconv_free_batch(imgs, 50.0, 2.0, n, dw.cpu().numpy())
        p.set_batching(1, 3)
        b, _, tr = p.tv_deconv_auto_batch(imgs, 0.02, 2.0, n, dw.cpu().numpy(), sigmas=[0.02, 0.0, 0.04], coupled=True)
        p.set_batching(1, 2)
        return a, b, tr

    with fdr.Plan(M, N, fdr.MODE_FAST) as fresh:
        fresh.set_operator_psf(psf)
        want = good(fresh)
    both = (dict(plan=False), dict(prm=False), dict(i=None), dict(o=None), dict(count=-1), dict(coupling=2), dict(coupling=-1),
            dict(coupling=1, aniso=1), dict(coupling=1, count=3),  # (group is 2)
            dict(rho=0.0), dict(rho=float("nan")), dict(nu=-1.0), dict(nu=float("inf")), dict(n=-1), dict(area=3), dict(rows=65), dict(rows=0),
            dict(stride=cols - 1), dict(wstride=cols - 1), dict(out_stride=cols - 1), dict(out_rows=rows - 1), dict(out_cols=cols - 1), dict(out_rows=M + 1),
            dict(o=d.data_ptr() + 4 * (2 * px + 5)),  # the first output overlaps the LAST input: not what a single call on image 0 sees
            dict(i=do.data_ptr() + 4 * px),  # the first input is the second output
            dict(w=do.data_ptr() + 4 * (2 * px + 8)))  # the weights lie in the last output
    nan, inf = float("nan"), float("inf")
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 2)
        assert free(p) == -4 and b"operator PSF" in L.fdr_last_error()
        p.set_operator_psf(psf)
        for kw in both + (dict(mu=0.0), dict(mu=nan)):
            assert free(p, **kw) == -1, ("free", kw)
        for kw in both + (dict(sigma=-1.0), dict(sigma=nan), dict(tau=-1.0), dict(tau=inf),
                          dict(sigmas=(ctypes.c_double * 3)(0.02, -0.01, 0.02)), dict(sigmas=(ctypes.c_double * 3)(0.02, 0.02, nan)),
                          dict(sigmas=(ctypes.c_double * 3)(0.02, inf, 0.02)),
                          dict(trace=dtr.data_ptr(), tpitch=3 * n - 1),
                          dict(trace=d.data_ptr() + 4 * (2 * px + 6)), dict(trace=do.data_ptr() + 4 * (2 * px + 6)), dict(trace=dw.data_ptr() + 8),
                          dict(sigmas=(ctypes.c_double * 3)(0.02, 0.0, 0.02), rows=2, stride=cols)):  # estimated on a window below 3 x 3
            assert auto(p, **kw) == -1, ("auto", kw)
        assert free(p, count=0, i=None, o=None) == 0 and auto(p, count=0, i=None, o=None) == 0
        assert free(p, w=None, wstride=0) == 0 and auto(p, sigmas=sig, trace=dtr.data_ptr()) == 0
        assert auto(p, count=1, trace=dtr.data_ptr(), tpitch=0) == 0  # one image: the pitch is not looked at
        assert auto(p, sigmas=(ctypes.c_double * 3)(0.02, 0.03, 0.02), rows=2, stride=cols, sigma=0.0) == 0  # every level given: nothing estimated
        torch.cuda.synchronize()
        got = good(p)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), "a refused call changed what a good one gives"
        with pytest.raises(fdr.FdrError):
            p.tv_deconv_free_batch(imgs, 50.0, coupled=True, anisotropic=True)
        with pytest.raises(ValueError):
            p.tv_deconv_auto_batch(imgs, sigmas=[0.02, 0.02])
        with pytest.raises(ValueError):
            p.tv_deconv_free_batch(imgs, 50.0, weights=np.ones((rows - 1, cols), dtype=np.float32))


def test_workspaces(fdr):
    """after a group-of-4 call has grown the workspaces the single free and auto calls give their earlier bits, and a second batched
    call allocates nothing"""
    import torch
    M, N, rows, cols = 512, 512, 400, 450
    imgs = _images(M, N, rows, cols, 4)
    w = tvf_weights("fractional", rows, cols, 1)
    b = Batch(imgs, cols, rows * cols, w, cols)
    out_shape = (rows, cols)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(centred_psf(fdr.motionBlurKernel(15, 30.0), M, N))
        f0 = _free_single(p, b, 1, out_shape, cols, 50.0, 2.0, 2, 3.0, False, True, NORM_PADDED)
        a0 = _auto_single(p, b, 1, out_shape, cols, 0.03, 2.0, 2, 0.0, False, True, NORM_PADDED, 0.0)
        p.set_batching(1, 4)
        free0 = _free_batch(p, b, 4, out_shape, cols, rows * cols, 50.0, 2.0, 2, 3.0, False, True, NORM_PADDED)
        auto0, tr0 = _auto_batch(p, b, 4, out_shape, cols, rows * cols, 0.03, None, 2.0, 2, 0.0, False, True, NORM_PADDED)
        assert np.array_equal(free0[1], f0) and np.array_equal(auto0[1], a0[0]) and np.array_equal(tr0[1], a0[1])
        assert np.array_equal(_free_single(p, b, 1, out_shape, cols, 50.0, 2.0, 2, 3.0, False, True, NORM_PADDED), f0)
        a1 = _auto_single(p, b, 1, out_shape, cols, 0.03, 2.0, 2, 0.0, False, True, NORM_PADDED, 0.0)
        assert np.array_equal(a1[0], a0[0]) and np.array_equal(a1[1], a0[1])
        d_out = _outputs(4, out_shape, cols, rows * cols)
        d_tr = torch.zeros(4 * 6, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        m0 = torch.cuda.mem_get_info()[0]
        for coupled in (False, True):
            p.tv_deconv_free_batch_dev(b.img_ptr(), b.pitch, 4, rows, cols, cols, d_out.data_ptr(), rows * cols, cols, 50.0, 2.0, 2, b.w_ptr(), cols,
                                       coupled=coupled)
            p.tv_deconv_auto_batch_dev(b.img_ptr(), b.pitch, 4, rows, cols, cols, d_out.data_ptr(), rows * cols, cols, 0.0, 2.0, 2, b.w_ptr(), cols,
                                       sigmas=[0.02, 0.0, 0.03, 0.04], d_trace=d_tr.data_ptr(), trace_pitch=6, coupled=coupled)
        p.set_batching(1, 2)
        p.tv_deconv_free_batch_dev(b.img_ptr(), b.pitch, 3, rows, cols, cols, d_out.data_ptr(), rows * cols, cols, 50.0, 2.0, 2)
        torch.cuda.synchronize()
        m1 = torch.cuda.mem_get_info()[0]
        print("TVFB\tallocations\tlater batched calls %d bytes" % (m0 - m1))
        assert m0 == m1, "a later batched call allocated device memory"


def test_pass_list(fdr):
    """a group of 3 makes the launches of one image per iteration (the forward rows under the group form's name), the window passes
    under names of their own"""
    M, N, rows, cols, n = 256, 512, 200, 300, 3
    imgs = _images(M, N, rows, cols, 3)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0)
        p.set_batching(1, 3)
        p.tv_deconv_free_batch(imgs, 50.0, 2.0, 1)  # the workspaces and the table
        p.profile(True)
        p.tv_deconv_free_batch(imgs, 50.0, 2.0, n)
        free = {k: c for k, _, c in p.pass_times()}
        p.tv_deconv_auto_batch(imgs, 0.02, 2.0, n, nu=2.0)  # (nu = rho: the table of the free call above)
        auto = {k: c for k, _, c in p.pass_times()}
        p.tv_deconv_free_batch(imgs, 50.0, 2.0, n, coupled=True)
        joint = {k: c for k, _, c in p.pass_times()}
    print("TVFB\tpasses\tfree %s\n\tauto %s\n\tcoupled %s" % (free, auto, joint))
    per_iteration = {"TVF data: s, q, r = 2s-e (window)": 1, "TV spatial: shrink+dual+div (free)": 1, "A op rows: pad+FFT (blur / RL), group": 3,
                     "B' op cols: FFT*H*IFFT": 1, "B' op cols: FFT*conj(H)*IFFT": 1, "C op rows: IFFT+crop (blur)": 2,
                     "B' op cols: FFT*T*IFFT (TVF solve)": 1, "C op rows: IFFT (TVF x)": 1}
    want = {k: n * c for k, c in per_iteration.items()}
    want.update({"TVF init: x = pad(d), w = q = 0": 1, "TVF out: crop+clamp": 1})
    assert {k: c for k, c in free.items() if c} == want, free
    want_auto = dict(want)
    del want_auto["TVF data: s, q, r = 2s-e (window)"]
    want_auto.update({"TVA norm+mu: res_e, res_c, S -> mu_k": n, "TVA data: s, q, r = 2s-e (mu_k)": n})
    assert {k: c for k, c in auto.items() if c} == want_auto, auto
    want_joint = dict(want)
    del want_joint["TV spatial: shrink+dual+div (free)"]
    want_joint["TV spatial: joint shrink+dual+div (free)"] = n
    assert {k: c for k, c in joint.items() if c} == want_joint, joint


def test_python_wrappers(fdr):
    """tvDeblurFree_RGB and tvDeblurAuto_RGB: uncoupled they equal three single calls bit for bit, coupled they equal the Plan's
    batched calls"""
    img = tvf_image(256, 512, 150, 350, 2)
    psf = fdr.motionBlurKernel(15, 30.0)
    w = tvf_weights("mask", 150, 350, 2)
    chans = [np.ascontiguousarray(img[::-1] * np.float32(0.75)), img, np.ascontiguousarray(img[:, ::-1] * np.float32(0.5))]
    M, N = fdr._rlfree_plan_size(150, 350, psf.shape[0], psf.shape[1])
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        free1 = [p.tv_deconv_free(c, 50.0, 2.0, 3, w, 0.0, False, True, NORM_PADDED) for c in chans]
        auto1 = [p.tv_deconv_auto(c, 0.0, 2.0, 3, w, 0.0, 0.0, False, True, NORM_PADDED) for c in chans]
        p.set_batching(1, 3)
        freec = p.tv_deconv_free_batch(np.stack(chans), 50.0, 2.0, 3, w, 0.0, False, True, NORM_PADDED, False, True)
        autoc = p.tv_deconv_auto_batch(np.stack(chans), 0.0, 2.0, 3, w, 0.0, 0.0, False, True, NORM_PADDED, False, None, True)
    for coupled in (False, True):
        c = list(chans)
        fdr.tvDeblurFree_RGB(c, psf, 50.0, iterations=3, nonneg=True, norm_area=NORM_PADDED, weights=w, coupled=coupled)
        for k in range(3):
            assert np.array_equal(c[k], freec[k] if coupled else free1[k]), ("free", coupled, k)
        c = list(chans)
        res = fdr.tvDeblurAuto_RGB(c, psf, 0.0, iterations=3, nonneg=True, norm_area=NORM_PADDED, weights=w, coupled=coupled)
        for k in range(3):
            assert np.array_equal(c[k], autoc[0][k] if coupled else auto1[k][0]), ("auto", coupled, k)
            assert res[k] == (autoc[1][k] if coupled else auto1[k][1]), ("auto result", coupled, k)
    assert not np.array_equal(freec[0], free1[0]) and len({r.sigma for r in autoc[1]}) == 3
