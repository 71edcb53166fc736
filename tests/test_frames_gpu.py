"""Multi-frame Richardson-Lucy (fdr_set_frame_psfs*, fdr_spectrum_sum_f32_dev, fdr_blur_frames_f32_dev,
fdr_richardson_lucy_frames_f32*) on the MI355X: the sum kernel against the numpy float32 loop bit for bit, the blur through the
frames against the single-PSF blur (bits) and the float64 sum of adjoints, the restoration's bit identities (one frame = the
single-frame calls, copies of one frame, every launch group, two calls) and its comparison with the float64 model of
tests/_frames_model.py, isolation from the rest of the plan, allocation-free later calls, the refusals, the pass names, the
quality case, the convenience calls and the CLI leg.  Every output has NaN guard columns that must stay NaN.  Cases print an `RLM` line with their measured values
(pytest -s).

The model comparison covers K in {2, 3, 5, 8}, the three kinds of weights, PSF sums 0.5 / 1 / 2, both output windows, the three
norm_area and n in {0, 1, 2, 10, 30} on 64 x 128, 256^2 and 1024 x 512; the last plan's cases take up to half a minute each, nearly
all of it the float64 and float32 CPU runs of the model."""
import ctypes

import numpy as np
import pytest

from _frames_model import (FRAMES_ADJ_TOL, FRAMES_TOL, QUALITY_EPS, QUALITY_LAMBDA, QUALITY_N, SIGMA_MARGIN, blur_frames, blur_frames_adjoint,
                           frames_state, quality_case, quality_psnr, sigma_margin)
from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, normalize, psnr, rel_err
from _rlfree_model import SIGMA
from _spectral import tone_image

pytestmark = pytest.mark.gpu

SUMS = (0.5, 1.0, 2.0)
F32_EPS = float(np.finfo(np.float32).eps)


# ---- the sum kernel alone -------------------------------------------------------------------------------------------------------------
def _sum_reference(dst0, srcs, accumulate):
    v = dst0.copy() if accumulate else srcs[0].copy()
    for s in (srcs if accumulate else srcs[1:]):
        v = (v + s).astype(np.float32)  # one float32 add per source, in ascending order
    return v


@pytest.mark.parametrize("n_floats", [2, 6, 1022, 1024, 1026, 65538])
def test_spectrum_sum_has_the_bits_of_the_float32_loop(fdr, n_floats):
    import torch
    rng = np.random.default_rng(n_floats)
    guard = 8  # floats before and after every buffer (32 bytes: the 16-byte alignment holds)
    for n in range(1, 9):
        for accumulate in (False, True):
            for alias in (False, True):  # dst equal to source 0
                host = [(rng.standard_normal(n_floats) * 10.0 ** rng.integers(-3, 4, n_floats)).astype(np.float32) for _ in range(n + 1)]
                bufs = []
                for h in host:
                    b = np.full(n_floats + 2 * guard, 12345.0, dtype=np.float32)
                    b[guard:guard + n_floats] = h
                    bufs.append(torch.from_numpy(b).cuda())
                d_dst = bufs[0] if alias else bufs[n]
                srcs = host[:n]
                dst0 = host[0] if alias else host[n]
                fdr.spectrum_sum_dev(d_dst.data_ptr() + 4 * guard, [b.data_ptr() + 4 * guard for b in bufs[:n]], n_floats, accumulate)
                torch.cuda.synchronize()
                got = d_dst.cpu().numpy()
                want = _sum_reference(dst0, srcs, accumulate)
                what = (n_floats, n, accumulate, alias)
                assert np.array_equal(got[guard:guard + n_floats].view(np.uint32), want.view(np.uint32)), what
                assert np.all(got[:guard] == 12345.0) and np.all(got[guard + n_floats:] == 12345.0), ("a store outside [0, n_floats)", what)
                for k in range(0 if not alias else 1, n):  # the sources are read only
                    assert np.array_equal(bufs[k].cpu().numpy()[guard:guard + n_floats], host[k]), what


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _psfs(fdr, K, M, N, centred):
    """K motion PSFs at different angles with the sums 0.5, 1, 2 in turn: centred M x N planes, or 15 x 15 top-left.  (The angles
    8 + 22 k keep every coverage value of the cases below at least 1.9 SIGMA_MARGIN K away from sigma K.)"""
    out = []
    for k in range(K):
        m = fdr.motionBlurKernel(15, 8.0 + 22.0 * k).astype(np.float64) * SUMS[k % 3]
        out.append(centred_psf(m.astype(np.float32), M, N) if centred else m.astype(np.float32))
    return out


def _small_psfs(K):
    """3 x 3 PSFs for the smallest plan"""
    rng = np.random.default_rng(2)
    return [((p / p.sum()) * SUMS[k % 3]).astype(np.float32) for k, p in enumerate(rng.random((K, 3, 3)) + 0.1)]


def _frames(psfs, M, N, rows, cols, seed):
    """K frames of one scene: the tone image blurred by each PSF, floored at 0.05, with a patch of negative pixels (dw uses d+)"""
    scene = np.clip(tone_image(M, N, seed, rows, cols), 0, None).astype(np.float64)
    ds = []
    for k, b in enumerate(blur_frames(scene, psfs, M, N)):
        d = (np.maximum(b, 0) + 0.05).astype(np.float32)
        d[: max(1, rows // 16), : max(1, cols // 16)] -= np.float32(0.5 + 0.1 * k)
        ds.append(d)
    return ds


def _mask(K, rows, cols, seed):
    return (np.random.default_rng(seed).random((K, rows, cols)) >= 0.02).astype(np.float32)


def _to_dev(planes, stride, fill=0.0):
    """K planes rows x cols into one device buffer with row stride `stride` and one extra row between the planes; (tensor, pitch)"""
    import torch
    K, rows, cols = len(planes), planes[0].shape[0], planes[0].shape[1]
    buf = np.full((K, rows + 1, stride), fill, dtype=np.float32)
    for k in range(K):
        buf[k, :rows, :cols] = planes[k]
    return torch.from_numpy(buf).cuda(), (rows + 1) * stride


def _dev_call(p, ds, weights, stride, out_rows, out_cols, iterations, area=NORM_NONE, lam=0.0, eps=0.0, sigma=SIGMA):
    """Plan.richardson_lucy_frames_dev on device copies (row stride `stride`, weights stride + 1, their padding 7.0: it must not be
    read); the output has NaN-filled guard columns and a guard row, which must stay NaN; returns the out_rows x out_cols window"""
    import torch
    K, (rows, cols) = len(ds), ds[0].shape
    d_in, pitch = _to_dev(ds, stride)
    d_w, wp, ws = None, 0, 0
    if weights is not None:
        ws = stride + 1
        w = np.asarray(weights, dtype=np.float32)
        d_w, wp = _to_dev([w] if w.ndim == 2 else list(w), ws, 7.0)
        if w.ndim == 2:
            wp = 0
    out_stride = out_cols + 3
    d_out = torch.full((out_rows + 1, out_stride), float("nan"), dtype=torch.float32, device="cuda")
    p.richardson_lucy_frames_dev(d_in.data_ptr(), pitch, K, rows, cols, stride, d_out.data_ptr(), out_stride, iterations,
                                 d_weights=d_w.data_ptr() if d_w is not None else None, weight_pitch=wp, wstride=ws, tv_lambda=lam, tv_eps=eps,
                                 sigma=sigma, norm_area=area, out_rows=out_rows, out_cols=out_cols)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(np.isnan(out[:out_rows, out_cols:])) and np.all(np.isnan(out[out_rows:, :])), "a store landed outside the output window"
    return out[:out_rows, :out_cols]


def _err(got, want, area):
    return rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(got.astype(np.float64) - want)))


# ---- blur through the frames --------------------------------------------------------------------------------------------------------------
BLUR_PLANS = [(8, 32, 5, 29, 31), (64, 128, 37, 101, 103), (256, 256, 201, 151, 163), (1024, 512, 999, 333, 347)]


@pytest.mark.parametrize("M,N,rows,cols,stride", BLUR_PLANS)
def test_blur_frames(fdr, M, N, rows, cols, stride):
    """forward: frame k has the bits of fdr_blur_f32_dev under PSF k; adjoint: within FRAMES_ADJ_TOL of the float64 sum of the K
    single adjoint blurs (and within 10x of the float32 CPU run), with the same bits for the launch groups 1, 2, 3 and 8"""
    import torch
    K = 5
    psfs = _small_psfs(K) if M == 8 else _psfs(fdr, K, M, N, centred=False)
    rng = np.random.default_rng(M + N)
    x = rng.random((rows, cols)).astype(np.float32)
    ys = [rng.random((rows, cols)).astype(np.float32) for _ in range(K)]
    d_x, _ = _to_dev([x], stride)
    d_ys, ypitch = _to_dev(ys, stride)
    ostride = cols + 3
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        assert p.frame_count() == 0
        p.set_frame_psfs(psfs)
        assert p.frame_count() == K
        adj = {}
        for group in (1, 2, 3, 8):
            p.set_batching(1, group)
            d_out = torch.full((K, rows + 1, ostride), float("nan"), dtype=torch.float32, device="cuda")
            p.blur_frames_dev(d_x.data_ptr(), 0, rows, cols, stride, d_out.data_ptr(), (rows + 1) * ostride, ostride, K)
            d_adj = torch.full((rows + 1, ostride), float("nan"), dtype=torch.float32, device="cuda")
            p.blur_frames_dev(d_ys.data_ptr(), ypitch, rows, cols, stride, d_adj.data_ptr(), 0, ostride, K, adjoint=True)
            torch.cuda.synchronize()
            fwd = d_out.cpu().numpy()
            a = d_adj.cpu().numpy()
            assert np.all(np.isnan(fwd[:, :rows, cols:])) and np.all(np.isnan(fwd[:, rows:, :])), "forward: a store outside the windows"
            assert np.all(np.isnan(a[:rows, cols:])) and np.all(np.isnan(a[rows:, :])), "adjoint: a store outside the window"
            adj[group] = (fwd[:, :rows, :cols].copy(), a[:rows, :cols].copy())
        p.set_batching(1, 1)
        for k in range(K):  # the single-PSF blur of the same plan
            p.set_operator_psf(psfs[k])
            d_one = torch.full((rows + 1, ostride), float("nan"), dtype=torch.float32, device="cuda")
            p.blur_dev(d_x.data_ptr(), rows, cols, stride, d_one.data_ptr(), ostride)
            torch.cuda.synchronize()
            one = d_one.cpu().numpy()[:rows, :cols]
            for group in adj:
                assert np.array_equal(adj[group][0][k], one), "forward frame %d, group %d: not the bits of fdr_blur_f32_dev" % (k, group)
        assert p.frame_count() == K  # the operator setter leaves the frame tables alone
    for group in (2, 3, 8):
        assert np.array_equal(adj[group][1], adj[1][1]), "adjoint: group %d differs from group 1" % group
    want = blur_frames_adjoint(ys, psfs, M, N)
    e = rel_err(adj[1][1], want)
    cpu32 = rel_err(blur_frames_adjoint(ys, psfs, M, N, dtype=np.float32), want)
    print("RLM\tblur adjoint\t%dx%d win %dx%d K=%d\terr=%.3g\tcpu32=%.3g" % (M, N, rows, cols, K, e, cpu32))
    assert e <= FRAMES_ADJ_TOL and e <= 10 * max(cpu32, 4 * F32_EPS), (e, cpu32)


# ---- the restoration: bit identities ------------------------------------------------------------------------------------------------------
def _identity_case(fdr):
    M, N, rows, cols, stride = 256, 256, 200, 151, 163
    psf = _psfs(fdr, 2, M, N, centred=True)[1]
    d = _frames([psf], M, N, rows, cols, 31)[0]
    d = np.maximum(d, np.float32(0.05))  # image >= 0.05
    w = _mask(1, rows, cols, 4)[0]
    return M, N, rows, cols, stride, psf, d, w


def test_one_frame_has_the_bits_of_the_single_calls(fdr):
    """K = 1: the bits of fdr_richardson_lucy_free_f32_dev, and with lambda > 0 of fdr_richardson_lucy_tv_f32_dev (free boundary)"""
    import torch
    M, N, rows, cols, stride, psf, d, w = _identity_case(fdr)
    src = np.zeros((rows, stride), dtype=np.float32)
    src[:, :cols] = d
    d_in = torch.from_numpy(src).cuda()
    d_w = torch.from_numpy(np.ascontiguousarray(w)).cuda()
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        p.set_frame_psfs([psf])
        for n, lam, area, (orows, ocols) in ((0, 0.0, NORM_NONE, (rows, cols)), (5, 0.0, NORM_NONE, (M, N)), (5, 0.0, NORM_PADDED, (rows, cols)),
                                             (5, 0.02, NORM_NONE, (M, N)), (3, 0.01, NORM_CROPPED, (rows, cols))):
            d_out = torch.full((orows, ocols), float("nan"), dtype=torch.float32, device="cuda")
            if lam == 0.0:
                p.richardson_lucy_free_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), ocols, n, d_weights=d_w.data_ptr(), wstride=cols,
                                           norm_area=area, out_rows=orows, out_cols=ocols)
            else:
                p.richardson_lucy_tv_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), ocols, n, lam, 0.0, True, d_weights=d_w.data_ptr(),
                                         wstride=cols, norm_area=area, out_rows=orows, out_cols=ocols)
            torch.cuda.synchronize()
            want = d_out.cpu().numpy()
            got = _dev_call(p, [d], w, stride, orows, ocols, n, area, lam)
            assert np.array_equal(got, want), "K = 1, n = %d, lambda = %g, norm %d: not the bits of the single call" % (n, lam, area)


@pytest.mark.parametrize("K", [2, 4])
def test_copies_of_one_frame_have_the_bits_of_the_single_call(fdr, K):
    """K = 2 and 4 copies of one frame (image >= 0.05, n <= 10): every rescaling involved is by a power of two (alpha, the sum of the
    spectra and the threshold by K, wgt by 1 / K), so the bits are those of the single call.  The float32 CPU model of this input
    meets no denormal, with and without the prior: the smallest non-zero magnitude of alpha, wgt, every iterate u_0 .. u_10 and every
    ratio plane r_k of the ten steps stays above 1e-30 (checked here)."""
    M, N, rows, cols, stride, psf, d, w = _identity_case(fdr)
    for lam in (0.0, 0.02):
        st = frames_state([d] * K, [psf] * K, M, N, 10, weights=w, lam=lam, dtype=np.float32, keep=range(11), keep_r=True)
        planes = [("alpha", st["alpha"]), ("wgt", st["wgt"])] + [("u_%d" % n, u) for n, u in st["us"].items()]
        planes += [("r_%d of step %d" % (k, it), r) for it, step in enumerate(st["rs"]) for k, r in enumerate(step)]
        assert len(st["us"]) == 11 and len(st["rs"]) == 10 and len(st["rs"][0]) == K
        for key, x in planes:
            assert x.dtype == np.float32
            nz = np.abs(x[x != 0])
            assert nz.size and float(nz.min()) > 1e-30, (lam, key, float(nz.min()) if nz.size else None)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, K)
        p.set_frame_psfs([psf])
        one = {(n, lam): _dev_call(p, [d], w, stride, M, N, n, NORM_NONE, lam) for n in (0, 1, 10) for lam in (0.0, 0.02)}
        p.set_frame_psfs([psf] * K)
        for (n, lam), want in one.items():
            got = _dev_call(p, [d] * K, w, stride, M, N, n, NORM_NONE, lam)
            assert np.array_equal(got, want), "K = %d copies, n = %d, lambda = %g: not the bits of the single call" % (K, n, lam)


def test_same_bits_for_every_group_and_in_two_calls(fdr):
    M, N, rows, cols, stride = 64, 128, 37, 101, 103
    K = 8
    psfs = _psfs(fdr, K, M, N, centred=True)
    ds = _frames(psfs, M, N, rows, cols, 7)
    w = _mask(K, rows, cols, 9)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_frame_psfs(psfs)
        ref = {}
        for group in range(1, 9):
            p.set_batching(1, group)
            for lam in (0.0, 0.02):
                a = _dev_call(p, ds, w, stride, M, N, 6, NORM_NONE, lam)
                b = _dev_call(p, ds, w, stride, M, N, 6, NORM_NONE, lam)
                assert np.array_equal(a, b), "two consecutive calls differ (group %d)" % group
                if group == 1:
                    ref[lam] = a
                assert np.array_equal(a, ref[lam]), "group %d differs from group 1 (lambda %g)" % (group, lam)
        host = p.richardson_lucy_frames(ds, 6, weights=w, full_plane=True)
        assert np.array_equal(host, ref[0.0]), "the host form differs from the _dev form"


def test_convenience_calls(fdr):
    """richardsonLucyFrames_myfft is the plan's call on the plan it documents; richardsonLucyFrames_RGB is that call per channel"""
    M, N, rows, cols = 64, 128, 37, 101
    K = 3
    psfs = _psfs(fdr, K, M, N, centred=False)
    ch = [_frames(psfs, M, N, rows, cols, seed) for seed in (11, 12)]  # two channels of K frames each
    w = _mask(K, rows, cols, 1)
    assert fdr._frames_plan_size(rows, cols, psfs) == (M, N)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_frame_psfs(psfs)
        want = [p.richardson_lucy_frames(c, 4, weights=w, tv_lambda=0.01) for c in ch]
    got = [fdr.richardsonLucyFrames_myfft(c, psfs, 4, weights=w, tv_lambda=0.01) for c in ch]
    rgb = fdr.richardsonLucyFrames_RGB([[ch[0][k], ch[1][k]] for k in range(K)], psfs, 4, weights=w, tv_lambda=0.01)
    for c in range(2):
        assert np.array_equal(got[c], want[c]) and np.array_equal(rgb[c], want[c]), c


# ---- the restoration against the float64 model -------------------------------------------------------------------------------------------
MODEL_PLANS = {"64x128": (64, 128, 37, 101, 103, True), "256": (256, 256, 200, 151, 163, True), "1024x512": (1024, 512, 1000, 333, 347, False)}
WEIGHT_KINDS = ("per frame", "one plane", "none")


ITERATIONS = (0, 1, 2, 10, 30)


def _weights_of(kind, K, rows, cols, seed):
    if kind == "none":
        return None
    m = _mask(K, rows, cols, seed)
    return m if kind == "per frame" else m[0]


def _compare(fdr, M, N, rows, cols, stride, psfs, ds, w, iterations, group, what, lam=0.0, eps=0.0):
    K = len(ds)
    bad, worst = [], (0.0, 0.0)
    st = frames_state(ds, psfs, M, N, max(iterations), weights=w, lam=lam, eps=eps if eps else 1e-3, keep=iterations)
    margin = sigma_margin(st["alpha"], SIGMA, K)
    assert margin >= SIGMA_MARGIN * K, "%s: a model alpha lies %.3g from sigma K" % (what, margin)
    us32 = frames_state(ds, psfs, M, N, max(iterations), weights=w, lam=lam, eps=eps if eps else 1e-3, keep=iterations, dtype=np.float32)["us"]
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, group)
        p.set_frame_psfs(psfs)
        for n in iterations:
            for orows, ocols in ((rows, cols), (M, N)):
                raw = st["us"][n][:orows, :ocols]
                for area in (NORM_NONE, NORM_CROPPED, NORM_PADDED):
                    cpu32 = _err(normalize(us32[n][:orows, :ocols], area, M, N), normalize(raw, area, M, N), area)  # the same metric
                    if (orows, ocols) == (rows, cols) and area == NORM_CROPPED:
                        got = p.richardson_lucy_frames(ds, n, weights=w, tv_lambda=lam, tv_eps=eps, norm_area=area)  # the host form
                    else:
                        got = _dev_call(p, ds, w, stride, orows, ocols, n, area, lam, eps)
                    e = _err(got, normalize(raw, area, M, N), area)
                    worst = max(worst, (e, cpu32))
                    case = "%s n=%d out=%dx%d norm=%d" % (what, n, orows, ocols, area)
                    print("RLM\tframes\t%s\terr=%.3g\tcpu32=%.3g\tmargin=%.3g" % (case, e, cpu32, margin))
                    if not e <= FRAMES_TOL:
                        bad.append("%s: error %.3g > %s" % (case, e, FRAMES_TOL))
                    # (4 float32 roundings stand in where the CPU run happens to hit the model exactly: n = 0)
                    if not e <= 10 * max(cpu32, 4 * F32_EPS):
                        bad.append("%s: error %.3g above 10x the float32 CPU run's %.3g" % (case, e, cpu32))
    print("RLM\tworst\t%s\terr=%.3g\tcpu32=%.3g" % ((what,) + worst))
    return bad


@pytest.mark.parametrize("K", [2, 3, 5, 8])
@pytest.mark.parametrize("plan", list(MODEL_PLANS))
def test_against_model(fdr, plan, K):
    M, N, rows, cols, stride, centred = MODEL_PLANS[plan]
    kind = WEIGHT_KINDS[(K + list(MODEL_PLANS).index(plan)) % 3]
    psfs = _psfs(fdr, K, M, N, centred)
    ds = _frames(psfs, M, N, rows, cols, 100 + K)
    w = _weights_of(kind, K, rows, cols, K)
    group = (1, 2, 3, 8)[(K + M) % 4]
    bad = _compare(fdr, M, N, rows, cols, stride, psfs, ds, w, ITERATIONS, group, "%s K=%d weights=%s group=%d" % (plan, K, kind, group))
    assert not bad, "\n".join(bad)


def test_against_model_with_the_prior(fdr):
    """lambda = 0.02 at eps = 0.05 (the regime in which the float32 and float64 runs of the explicit TV step agree; _rltv_model.py)"""
    M, N, rows, cols, stride, centred = MODEL_PLANS["256"]
    K = 3
    psfs = _psfs(fdr, K, M, N, centred)
    ds = _frames(psfs, M, N, rows, cols, 55)
    bad = _compare(fdr, M, N, rows, cols, stride, psfs, ds, _mask(K, rows, cols, 2), (1, 2, 10), 2, "256 K=3 prior", lam=0.02, eps=0.05)
    assert not bad, "\n".join(bad)


def test_against_model_4096(fdr):
    """one case on 4096^2, n = 1, K = 2, one weights plane"""
    M = N = 4096
    rows, cols = 4000, 3900
    psfs = _psfs(fdr, 2, M, N, centred=False)
    ds = _frames(psfs, M, N, rows, cols, 77)
    w = _mask(1, rows, cols, 5)[0]
    st = frames_state(ds, psfs, M, N, 1, weights=w)
    assert sigma_margin(st["alpha"], SIGMA, 2) >= SIGMA_MARGIN * 2
    u32 = frames_state(ds, psfs, M, N, 1, weights=w, dtype=np.float32)["u"]
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 2)
        p.set_frame_psfs(psfs)
        got = _dev_call(p, ds, w, cols, rows, cols, 1)
    e, cpu32 = rel_err(got, st["u"][:rows, :cols]), rel_err(u32[:rows, :cols], st["u"][:rows, :cols])
    print("RLM\tframes\t4096 K=2 n=1\terr=%.3g\tcpu32=%.3g" % (e, cpu32))
    assert e <= FRAMES_TOL and e <= 10 * max(cpu32, 4 * F32_EPS), (e, cpu32)


# ---- plan state and hygiene ----------------------------------------------------------------------------------------------------------------
def test_isolation(fdr):
    """blur, RL, free RL, RL with the prior, TV and Wiener give the same bytes before and after frames calls, and a frames call the
    same bytes after the operator PSF changed"""
    M, N, rows, cols = 256, 512, 200, 480
    img = tone_image(M, N, 21, rows, cols)
    K = 3
    psfs = _psfs(fdr, K, M, N, centred=True)
    ds = _frames(psfs, M, N, rows, cols, 3)
    w = _mask(K, rows, cols, 3)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 2)

        def others():
            p.set_psf_motion(15, 30.0, 0.01)
            return [p.wiener(img), p.blur(img), p.blur(img, adjoint=True), p.richardson_lucy(img, 3), p.richardson_lucy_free(img, 3, weights=w[0]),
                    p.richardson_lucy_tv(img, 3, 0.02, free_boundary=True), p.tv_deconv(img, 200.0, iterations=3)]

        p.set_operator_psf_motion(15, 30.0)
        before = others()
        p.set_frame_psfs(psfs)
        a = p.richardson_lucy_frames(ds, 3, weights=w)
        b = p.richardson_lucy_frames(ds, 2, weights=w, tv_lambda=0.02, norm_area=NORM_PADDED, full_plane=True)
        after = others()
        for k, (x, y) in enumerate(zip(before, after)):
            assert np.array_equal(x, y), "result %d changed after the frames calls" % k
        p.set_operator_psf_motion(9, 100.0)  # another operator PSF: the frame tables are their own
        assert np.array_equal(p.richardson_lucy_frames(ds, 3, weights=w), a)
        assert np.array_equal(p.richardson_lucy_frames(ds, 2, weights=w, tv_lambda=0.02, norm_area=NORM_PADDED, full_plane=True), b)


def test_later_calls_allocate_nothing(fdr):
    import torch
    M, N, rows, cols, stride = 256, 256, 200, 151, 163
    K = 3
    psfs = _psfs(fdr, K, M, N, centred=True)
    ds = _frames(psfs, M, N, rows, cols, 3)
    d_in, pitch = _to_dev(ds, stride)
    d_out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 2)
        p.set_frame_psfs(psfs)

        def call(lam):
            p.richardson_lucy_frames_dev(d_in.data_ptr(), pitch, K, rows, cols, stride, d_out.data_ptr(), cols, 2, tv_lambda=lam)

        call(0.0)
        call(0.02)  # the first calls make the workspaces
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for lam in (0.0, 0.02, 0.0, 0.02):
            call(lam)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "a later call allocated device memory"


def test_refusals(fdr):
    import torch
    L = fdr.lib
    psf = fdr.motionBlurKernel(15, 30.0)
    imgs = np.stack([tone_image(64, 64, 3), tone_image(64, 64, 4)])
    out = np.empty((64, 64), dtype=np.float32)
    w = np.ones((2, 64, 64), dtype=np.float32)

    def prm(n=1, sigma=1e-2, area=2, orows=8, ocols=8, lam=0.0, eps=0.0):
        return ctypes.byref(fdr.RlFramesParams(n, sigma, area, orows, ocols, lam, eps))

    def call(p, pitch=4096, count=2, rows=8, cols=8, stride=64, wp=None, wpitch=0, ws=64, op=None, ostride=64, pr=None):
        return L.fdr_richardson_lucy_frames_f32(p._h, imgs.ctypes.data, pitch, count, rows, cols, stride, wp, wpitch, ws,
                                                out.ctypes.data if op is None else op, ostride, prm() if pr is None else pr)

    def setp(p, pitch=225, count=2, prows=15, pcols=15, pstride=15):
        two = np.stack([psf, psf])
        return L.fdr_set_frame_psfs(p._h, two.ctypes.data, pitch, count, prows, pcols, pstride)

    for M, N, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (64, 64, fdr.MODE_FAST, fdr.FLAG_SIMPLE_PATH, "simple"),
                                    (64, 64, fdr.MODE_FAST, fdr.FLAG_FULL_SPECTRUM, "full spectrum"), (64, 16, fdr.MODE_FAST, 0, "N < 32"),
                                    (75, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX, "mixed radix")):
        with fdr.Plan(M, N, mode, flags=flags) as p:
            assert setp(p) == -1 and call(p) == -1, what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert setp(p) == -4 and call(p) == -4
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        p.profile(True)
        assert call(p) == -4 and b"frame PSFs" in L.fdr_last_error()  # no frame tables
        d8 = torch.zeros(64, device="cuda")
        assert L.fdr_blur_frames_f32_dev(p._h, d8.data_ptr(), 0, 2, 2, 2, d8.data_ptr() + 64, 16, 2, 2, 0, None) == -4
        for count in (0, 9, -1):
            assert setp(p, count=count) == -1, count
        assert setp(p, pitch=224) == -1 and b"psf_pitch" in L.fdr_last_error()
        assert setp(p, prows=0) == -1 and setp(p, pstride=14) == -1 and setp(p, prows=65, pitch=65 * 15) == -1
        assert p.frame_count() == 0
        assert setp(p) == 0 and p.frame_count() == 2
        p.pass_times()  # reads and clears the records of the PSF passes
        assert L.fdr_richardson_lucy_frames_f32(p._h, imgs.ctypes.data, 4096, 2, 8, 8, 64, None, 0, 0, out.ctypes.data, 64, None) == -1  # null params
        d_b = torch.zeros(4096, device="cuda")

        def blur(count=2, in_pitch=64, out_pitch=64, rows=8, cols=8, stride=8, ostride=8, adjoint=0):
            return L.fdr_blur_frames_f32_dev(p._h, d_b.data_ptr(), in_pitch, rows, cols, stride, d_b.data_ptr() + 4 * 2048, out_pitch, ostride, count,
                                             adjoint, None)

        assert blur(count=1) == -1 and blur(count=3) == -1 and b"fdr_frame_count" in L.fdr_last_error()
        assert blur(out_pitch=63) == -1 and blur(adjoint=1, in_pitch=63) == -1 and b"pitch" in L.fdr_last_error()
        assert blur(rows=65) == -1 and blur(stride=7) == -1 and blur(ostride=7) == -1 and blur(rows=0) == -1
        assert L.fdr_blur_frames_f32_dev(p._h, d_b.data_ptr(), 64, 8, 8, 8, d_b.data_ptr() + 4 * 32, 64, 8, 2, 0, None) == -1  # frame 0's output in the input window
        assert b"overlaps the input" in L.fdr_last_error()
        assert L.fdr_blur_frames_f32_dev(p._h, d_b.data_ptr(), 64, 8, 8, 8, d_b.data_ptr() + 4 * 100, 64, 8, 2, 1, None) == -1  # ... in the second window
        assert blur() == 0 and blur(adjoint=1) == 0 and blur(adjoint=1, out_pitch=0) == 0 and blur(in_pitch=0) == 0
        torch.cuda.synchronize()
        p.pass_times()
        for count in (1, 3, 0, 9):
            assert call(p, count=count) == -1, count
        assert call(p, pr=prm(n=-1)) == -1
        for sigma in (0.0, 1.0, -0.5, float("nan")):
            assert call(p, pr=prm(sigma=sigma)) == -1 and b"sigma" in L.fdr_last_error(), sigma
        for area in (3, -1):
            assert call(p, pr=prm(area=area)) == -1
        for orows, ocols in ((7, 8), (8, 7), (65, 8), (8, 65), (0, 0)):
            assert call(p, pr=prm(orows=orows, ocols=ocols)) == -1, (orows, ocols)
        assert call(p, ostride=32, pr=prm(orows=8, ocols=40)) == -1
        assert call(p, rows=65) == -1 and call(p, cols=65, stride=65) == -1 and call(p, rows=0) == -1 and call(p, stride=4) == -1
        assert call(p, pitch=7 * 64 + 7) == -1 and b"img_pitch" in L.fdr_last_error()
        assert call(p, wp=w.ctypes.data, ws=4) == -1
        assert call(p, wp=w.ctypes.data, wpitch=7 * 64 + 7) == -1 and b"weight_pitch" in L.fdr_last_error()
        for lam in (-0.01, 0.126, float("nan")):
            assert call(p, pr=prm(lam=lam)) == -1 and b"lambda" in L.fdr_last_error(), lam
        for eps in (-1e-3, float("nan"), float("inf")):
            assert call(p, pr=prm(eps=eps)) == -1 and b"eps" in L.fdr_last_error(), eps
        assert call(p, op=imgs.ctypes.data + 4 * 4096) == -1 and b"overlaps a frame" in L.fdr_last_error()  # the second frame
        assert call(p, wp=w.ctypes.data, wpitch=4096, op=w.ctypes.data + 4 * (4096 + 64 * 3)) == -1 and b"overlaps the weights" in L.fdr_last_error()
        assert call(p, wp=w.ctypes.data, op=w.ctypes.data + 4 * 4096) == 0  # one weights plane: the second is not read
        assert call(p, wp=w.ctypes.data, wpitch=4096) == 0  # the plan still works


def test_refused_calls_launch_nothing(fdr):
    L = fdr.lib
    psf = fdr.motionBlurKernel(15, 30.0)
    imgs = np.stack([tone_image(64, 64, 3), tone_image(64, 64, 4)])
    out = np.empty((64, 64), dtype=np.float32)
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        p.set_frame_psfs([psf, psf])
        p.profile(True)
        for pr in (fdr.RlFramesParams(1, 2.0, 2, 8, 8, 0.0, 0.0), fdr.RlFramesParams(1, 1e-2, 2, 8, 8, 0.5, 0.0), fdr.RlFramesParams(1, 1e-2, 2, 7, 8, 0.0, 0.0)):
            assert L.fdr_richardson_lucy_frames_f32(p._h, imgs.ctypes.data, 4096, 2, 8, 8, 64, None, 0, 0, out.ctypes.data, 64, ctypes.byref(pr)) == -1
        assert L.fdr_richardson_lucy_frames_f32(p._h, imgs.ctypes.data, 4096, 3, 8, 8, 64, None, 0, 0, out.ctypes.data, 64,
                                                ctypes.byref(fdr.RlFramesParams(1, 1e-2, 2, 8, 8, 0.0, 0.0))) == -1
        assert sum(c for _, _, c in p.pass_times()) == 0, "a refused call launched a pass"


def test_pass_names(fdr):
    """K = 3 on launch groups of 2 (a group of two and a tail of one), n = 2 with the prior, normalised: the passes by name and
    count, all within FDR_MAX_PASSES"""
    M, N, rows, cols = 256, 512, 200, 300
    K, n = 3, 2
    psfs = _psfs(fdr, K, M, N, centred=False)
    ds = _frames(psfs, M, N, rows, cols, 1)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_batching(1, 2)
        p.profile(True)
        p.set_frame_psfs(psfs)
        p.richardson_lucy_frames(ds, n, tv_lambda=0.01, norm_area=NORM_PADDED)
        names = {name: c for name, _, c in p.pass_times()}
    print("RLM\tpasses\t%s" % names)
    assert len(names) <= fdr.MAX_PASSES - 1, "the names overflow FDR_MAX_PASSES"
    want = {"O rows: PSF pad+FFT (operator)": K, "O cols: FFT -> H/MN, conj(H)/MN": K, "RLM setup: dw_k, W_k, sums": K,
            "RLM start: fold, wgt = 1/alpha, u": 1, "A op rows: pad+FFT (blur / RL), group": 1 + 2 * n, "A op rows: pad+FFT (blur / RL)": 1 + 2 * n,
            "B' op cols: FFT*H_k*IFFT (frame)": K * n, "B' op cols: FFT*conj(H_k)*IFFT (frame)": K * (1 + n), "S frames: sum of spectra": 2 * (1 + n),
            "C op rows: IFFT+crop (frames)": 1, "C op rows: IFFT+RL ratio (frames)": 2 * n, "C op rows: IFFT+RL update (frames)": n,
            "RLTV factor: w / (1 - lambda div)": n, "E RLF minmax+normalize": 1}
    for name, c in want.items():
        assert names.get(name) == c, (name, names.get(name), c)
    assert set(names) == set(want), set(names) ^ set(want)


def test_quality_matches_the_model(fdr):
    """the three-frame quality case of test_frames_host.py on the device, with the prior at n = 100: within 0.01 dB of the model, and
    above the best single frame by the asserted half of the measured gain"""
    case = quality_case()
    pm = quality_psnr(case, [0, 1, 2])
    with fdr.Plan(case["M"], case["N"], fdr.MODE_FAST) as p:
        p.set_batching(1, 3)
        p.set_frame_psfs(case["psfs"])
        pg = psnr(p.richardson_lucy_frames(case["ds"], QUALITY_N, tv_lambda=QUALITY_LAMBDA, tv_eps=QUALITY_EPS), case["truth"])
        single = []
        for k in range(3):
            p.set_frame_psfs([case["psfs"][k]])
            single.append(psnr(p.richardson_lucy_frames([case["ds"][k]], QUALITY_N, tv_lambda=QUALITY_LAMBDA, tv_eps=QUALITY_EPS), case["truth"]))
    print("RLM\tquality\tmodel %.3f dB, GPU %.3f dB; single frames on the GPU %s" % (pm, pg, ", ".join("%.2f" % s for s in single)))
    assert abs(pg - pm) <= 0.01, (pm, pg)
    assert pg >= max(single) + 2.4, (pg, single)


def test_cli_frames(fdr, tmp_path):
    """tools/cli/gpu <img> L A --rl n --free-boundary --frame <img2> L2 A2 --rl-tv lambda --mask m.png: the planes (--raw-out) equal three
    richardson_lucy_frames(..., NORM_PADDED) calls, one per channel, on the plan richardsonLucyFrames_myfft uses"""
    import os
    import subprocess
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(root, "tools", "cli", "gpu")
    png = os.path.join(root, "tests", "golden", "car_blurred.png")
    u8 = np.asarray(Image.open(png).convert("RGB"))
    h, w = u8.shape[:2]
    second = np.roll(u8, (2, -3), axis=(0, 1))  # a second exposure: the same picture, shifted (what the frames show does not matter here)
    png2, mask_png = str(tmp_path / "second.png"), str(tmp_path / "mask.png")
    Image.fromarray(second, "RGB").save(png2)
    keep = np.random.default_rng(8).random((h, w)) >= 0.02
    Image.fromarray(np.repeat((keep * np.uint8(255))[:, :, None], 3, axis=2).astype(np.uint8), "RGB").save(mask_png)
    out_png, out_raw = str(tmp_path / "out.png"), str(tmp_path / "out.f32")
    r = subprocess.run([gpu, png, "40", "45", "--rl", "5", "--free-boundary", "--frame", png2, "25", "120", "--rl-tv", "0.01", "--mask", mask_png,
                        "--out", out_png, "--raw-out", out_raw], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Deblurring 3 channels took(gpu[richardson-lucy free-boundary 5 frames 2 tv 0.01]): " in r.stdout, r.stdout
    got = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
    frames = [u8.astype(np.float32) / 255.0, second.astype(np.float32) / 255.0]
    psfs = fdr._frame_psfs([fdr.motionBlurKernel(40, 45.0), fdr.motionBlurKernel(25, 120.0)])
    M, N = fdr._frames_plan_size(h, w, psfs)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_frame_psfs(psfs)
        for k, c in enumerate((2, 1, 0)):  # B, G, R
            want = p.richardson_lucy_frames([np.ascontiguousarray(f[:, :, c]) for f in frames], 5, weights=keep.astype(np.float32), tv_lambda=0.01,
                                            norm_area=fdr.NORM_PADDED)
            assert np.array_equal(got[k], want), (k, float(np.abs(got[k] - want).max()))
    assert os.path.exists(out_png)
