"""Richardson-Lucy with the TV prior in groups, with vectorial coupling, on the MI355X (fdr_richardson_lucy_tv_batch_f32*,
fdr_rl_tv_factor_group_f32_dev) against tests/_rltv_batch_model.py.

Uncoupled, every plane of a factor launch and every image of a batched call must equal, bit for bit (np.array_equal), what the
single-image _dev call gives for it on the same plan, at every row length, pass-B' kernel kind, group size and tail, iteration
count, normalisation, form and layout, and lie within RLTV_TOL / RLTV_FREE_TOL of the float64 model.  Coupled, the factor and both
calls are held to the model by the constants of _rltv_model.py and to 10x the error of the float32 CPU run of the model, case by case;
one channel must give the single call's bits.  NaN fills every output buffer and must survive outside the windows.  Each case prints
an `RLTVB` line with its measured values (pytest -s).  test_rltv_batch_host.py proves that this judge flags the fault models."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _batch_model as bm
import _rl_batch_model as rb
import _rltv_batch_model as tb
from _batch_model import SENTINEL
from _rl_batch_model import AREA_NAME, AREAS, Case
from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, psnr, rel_err, smooth_image
from _rltv_model import RLTV_FACTOR_TOL, RLTV_FREE_TOL, RLTV_TOL, tv_factor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_EPS = float(np.finfo(np.float32).eps)
TOL = {"plain": RLTV_TOL, "free": RLTV_FREE_TOL}
LAM, EPS = 0.01, 1e-3
TH = TW = tb.TILE
SHAPES = [(1, 1), (1, 37), (37, 1), (3, 5), (TH - 1, TW + 1), (TH, TW), (TH + 1, 2 * TW - 1), (2 * TH + 1, 2 * TW + 1)]
PLANES = (1, 2, 3, 5, 8)


# ---- the factor group kernel --------------------------------------------------------------------------------------------------
def _planes(n, R, C, seed):
    """n float32 planes R x C: random, smooth and tiny-gradient ones in turn (never flat: that is its own check)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        kind = k % 3
        if kind == 0:
            out.append(rng.random((R, C)).astype(np.float32))
        elif kind == 1:
            out.append(smooth_image(max(R, 2), max(C, 2), seed + k)[:R, :C].astype(np.float32))
        else:
            out.append((0.5 + 1e-3 * rng.random((R, C))).astype(np.float32))
    return np.stack(out)


class _Factor:
    """device copies of n planes (row stride `stride`, `pitch` floats apart, every pointer `offset` floats past a 256-byte
    boundary) and of w, and NaN-filled output buffers (row stride ostride, opitch apart) which must stay NaN outside the windows"""

    def __init__(self, us, w, stride, ostride, gap, offset):
        import torch
        self.n, self.R, self.C = us.shape
        self.stride, self.ostride, self.offset = stride, ostride, offset
        self.pitch, self.opitch = self.R * stride + gap, self.R * ostride + gap
        host = np.full(offset + self.n * self.pitch, 7.0, dtype=np.float32)  # the padding and the gaps must not matter
        for k in range(self.n):
            host[offset + k * self.pitch:][:self.R * stride].reshape(self.R, stride)[:, :self.C] = us[k]
        self.d_u = torch.from_numpy(host).cuda()
        self.d_w = None
        if w is not None:
            hw = np.full(offset + self.R * stride, 7.0, dtype=np.float32)
            hw[offset:].reshape(self.R, stride)[:, :self.C] = w
            self.d_w = torch.from_numpy(hw).cuda()

    def _out(self):
        import torch
        return torch.full((self.offset + self.ostride + self.n * self.opitch,), float("nan"), dtype=torch.float32, device="cuda")

    def _read(self, d_out, what):
        import torch
        torch.cuda.synchronize()
        flat = d_out.cpu().numpy()
        inside = np.zeros(flat.shape, dtype=bool)
        base = self.offset + self.ostride
        got = []
        for k in range(self.n):
            win = flat[base + k * self.opitch:][:self.R * self.ostride].reshape(self.R, self.ostride)[:, :self.C]
            inside[base + k * self.opitch:][:self.R * self.ostride].reshape(self.R, self.ostride)[:, :self.C] = True
            got.append(win.copy())
        assert np.all(np.isnan(flat[~inside])), "%s: a store landed outside the output windows" % what
        return np.stack(got)

    def group(self, p, lam, eps, couple, what):
        d_out = self._out()
        p.rl_tv_factor_group_dev(self.d_u.data_ptr() + 4 * self.offset, self.pitch, self.n, self.R, self.C, self.stride,
                                 d_out.data_ptr() + 4 * (self.offset + self.ostride), self.opitch, self.ostride, lam, eps,
                                 d_w=self.d_w.data_ptr() + 4 * self.offset if self.d_w is not None else None, couple=couple)
        return self._read(d_out, what)

    def alone(self, p, lam, eps, what):
        d_out = self._out()
        for k in range(self.n):
            p.rl_tv_factor_dev(self.d_u.data_ptr() + 4 * (self.offset + k * self.pitch), self.R, self.C, self.stride,
                               d_out.data_ptr() + 4 * (self.offset + self.ostride + k * self.opitch), self.ostride, lam, eps,
                               d_w=self.d_w.data_ptr() + 4 * self.offset if self.d_w is not None else None)
        return self._read(d_out, what)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_factor_group_kernel_at_its_edges(fdr, shape):
    R, C = shape
    c4 = (C + 3) // 4 * 4
    layouts = [("tight", C, C, 0, 0), ("loose", C + 3, C + 5, 7, 0), ("16-byte rows and pitches", c4 + 4, c4 + 8, 8, 0)]
    if shape == (TH + 1, 2 * TW - 1):
        layouts.append(("pointers offset by one float", c4, c4, 0, 1))
    rng = np.random.default_rng(R * 1000 + C)
    wz = rng.random((R, C)).astype(np.float32)
    wz[rng.random((R, C)) < 0.2] = 0
    bad, worst, worst32 = [], 0.0, 0.0
    with fdr.Plan(8, 32, fdr.MODE_FAST) as p:  # (the plan names the device; the factor needs none of its tables)
        for n in PLANES:
            us = _planes(n, R, C, R + C + n)
            flat = np.stack([np.full((R, C), 0.1 + 0.1 * k, dtype=np.float32) for k in range(n)])
            for what, stride, ostride, gap, offset in layouts:
                for w in (None, wz):
                    for lam, eps in ((0.125, 1e-3), (0.01, 0.05)):
                        tag = "%dx%d %d planes %s w=%s lambda=%g eps=%g" % (R, C, n, what, w is not None, lam, eps)
                        f = _Factor(us, w, stride, ostride, gap, offset)
                        ones = f.alone(p, lam, eps, tag)
                        # uncoupled: every plane has the bits of the single launch on it
                        if not np.array_equal(f.group(p, lam, eps, fdr.TV_COUPLE_NONE, tag), ones):
                            bad.append("%s: a plane of the group differs from the single launch on it" % tag)
                        # coupled: the model, 10x the float32 CPU run, the zeros of w
                        got = f.group(p, lam, eps, fdr.TV_COUPLE_CHANNELS, tag)
                        want = np.stack(tb.tv_factor_coupled(us, lam, eps, w))
                        scale = 1.0 if w is None else max(float(np.max(w)), 1e-30)
                        e = float(np.max(np.abs(got.astype(np.float64) - want))) / scale
                        cpu32 = float(np.max(np.abs(np.stack(tb.tv_factor_coupled(us, lam, eps, w, dtype=np.float32)).astype(np.float64) - want))) / scale
                        worst, worst32 = max(worst, e), max(worst32, cpu32)
                        if not e <= RLTV_FACTOR_TOL:
                            bad.append("%s: coupled error %.3g > %s" % (tag, e, RLTV_FACTOR_TOL))
                        if not e <= 10 * max(cpu32, F32_EPS):
                            bad.append("%s: coupled error %.3g above 10x the float32 CPU run's %.3g" % (tag, e, cpu32))
                        if w is not None and not np.all(got[:, w == 0] == 0):
                            bad.append("%s: a zero of w did not stay zero" % tag)
                        if n == 1 and not np.array_equal(got, ones):
                            bad.append("%s: one coupled channel differs from the single launch" % tag)
                    # a flat picture gives exactly w, coupled or not
                    ff = _Factor(flat, w, stride, ostride, gap, offset)
                    for couple in (fdr.TV_COUPLE_NONE, fdr.TV_COUPLE_CHANNELS):
                        got = ff.group(p, 0.125, 1e-3, couple, "flat")
                        if not all(np.array_equal(x, np.ones_like(x) if w is None else w) for x in got):
                            bad.append("%dx%d %d planes %s: a flat picture must give the factor w exactly (couple %d)" % (R, C, n, what, couple))
    print("RLTVB\tfactor\t%dx%d\tcoupled worst=%.3g\tcpu32 worst=%.3g" % (R, C, worst, worst32))
    assert not bad, "%d failures, the first:\n%s" % (len(bad), "\n".join(bad[:12]))


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def _nan_guard(out, olay):
    """NaN must survive everywhere outside the output windows; returns the buffer with the guard turned into the judge's SENTINEL"""
    inside = np.zeros(out.shape, dtype=bool)
    for i in range(olay.count):
        bm._window(inside, bm.out_base(olay, i), olay.rows, olay.cols, olay.out_stride)[...] = True
    ok = bool(np.all(np.isnan(out[~inside])))
    fixed = out.copy()
    fixed[~inside] = SENTINEL if ok else 0.0
    return fixed


class _Batch:
    """images, device buffers and the verdicts of one (plan shape, window, layout), shared by the calls of a case"""

    def __init__(self, fdr, M, N, rows, cols, count, loose=False):
        import torch
        self.fdr, self.M, self.N = fdr, M, N
        motion = bm.fit_psf(fdr.motionBlurKernel(15, 30.0), M, N)
        self.psf = motion if (rows, cols) == (M, N) else centred_psf(motion, M, N)
        self.lay = (bm.loose_layout if loose else bm.tight_layout)(rows, cols, count)
        self.imgs = rb.images(M, N, rows, cols, count, 1000 * bm.log2(M) + bm.log2(N))
        self.d_in = torch.from_numpy(bm.pack_inputs(self.imgs, self.lay)).cuda()
        self.mask = rb.mask(rows, cols, M + N)
        self.wstride = cols + 5 if loose else cols
        w = np.full((rows, self.wstride), 7.0, dtype=np.float32)  # the padding must not be read
        w[:, :cols] = self.mask
        self.d_w = torch.from_numpy(w).cuda()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.bad, self.worst, self.calls = [], 0.0, 0

    def plan(self):
        p = self.fdr.Plan(self.M, self.N, self.fdr.MODE_FAST)
        p.set_operator_psf(self.psf)
        return p

    def olay(self, case):
        return rb.out_layout(self.lay, self.M, self.N) if case.full_out else self.lay

    def fresh(self, olay):
        import torch
        return torch.full((bm.out_size(olay),), float("nan"), dtype=torch.float32, device="cuda")

    def _weights(self, case):
        return (self.d_w.data_ptr(), self.wstride) if case.masked else (None, 0)

    def alone(self, p, case, lam=LAM, eps=EPS):
        """every image through fdr_richardson_lucy_tv_f32_dev, read from and stored to the places it has in the batch:
        ([count, out_rows, out_cols], their errors against the model, the model)"""
        import torch
        lay, olay = self.lay, self.olay(case)
        d_one = self.fresh(olay)
        dw, ws = self._weights(case)
        free = case.form == "free"
        for i in range(lay.count):
            src, dst = self.d_in.data_ptr() + 4 * i * lay.img_pitch, d_one.data_ptr() + 4 * bm.out_base(olay, i)
            p.richardson_lucy_tv_dev(src, lay.rows, lay.cols, lay.stride, dst, olay.out_stride, case.iterations, lam, eps, free_boundary=free,
                                     d_weights=dw if free else None, wstride=ws if free else 0, norm_area=case.area, out_rows=olay.rows,
                                     out_cols=olay.cols, stream=self.stream)
        torch.cuda.synchronize()
        one = _nan_guard(d_one.cpu().numpy(), olay)
        if not bm.outside_untouched(one, olay):
            self.bad.append("%s: the single-image call wrote outside its window" % self.name(case))
        ones = bm.unpack(one, olay)
        refs = tb.references(case.form, self.imgs, self.psf, self.M, self.N, case.iterations, lam, eps, case.area, self.mask if case.masked else None,
                             out_shape=(olay.rows, olay.cols))
        return ones, rb.model_errors(ones, refs, case.area), refs

    def call(self, p, case, n, lam=LAM, eps=EPS, couple=0):
        """one batched call of the first n images into a NaN-filled buffer: (the flat output with the guard checked, its layout)"""
        import torch
        lay, olay = self.lay._replace(count=n), self.olay(case)._replace(count=n)
        d_out = self.fresh(olay)
        dw, ws = self._weights(case)
        free = case.form == "free"
        p.richardson_lucy_tv_batch_dev(self.d_in.data_ptr(), lay.img_pitch, n, lay.rows, lay.cols, lay.stride, d_out.data_ptr() + 4 * olay.lead,
                                       olay.out_pitch, olay.out_stride, case.iterations, lam, eps, free_boundary=free, d_weights=dw if free else None,
                                       wstride=ws if free else 0, norm_area=case.area, out_rows=olay.rows if free else None,
                                       out_cols=olay.cols if free else None, couple=couple, stream=self.stream)
        torch.cuda.synchronize()
        return _nan_guard(d_out.cpu().numpy(), olay), olay

    def batch(self, p, case, what, ones, count=None):
        n = self.lay.count if count is None else count
        out, olay = self.call(p, case, n)
        v = tb.judge("%s %s" % (self.name(case), what), out, olay, ones[0][:n], ones[2][:n], TOL[case.form], case.area, ones_err=ones[1][:n])
        self.bad += v.bad
        self.worst = max(self.worst, v.worst) if v.worst == v.worst and self.worst == self.worst else float("nan")
        self.calls += 1
        return out

    def name(self, case):
        return "%dx%d window %dx%d %s n=%d %s%s%s" % (self.M, self.N, self.lay.rows, self.lay.cols, case.form, case.iterations, AREA_NAME[case.area],
                                                     " masked" if case.masked else "", " out MxN" if case.full_out else "")

    def run(self, p, cases, groups, counts=(None,)):
        for case in cases:
            ones = self.alone(p, case)
            for group in groups:
                p.set_batching(1, group)
                for count in counts:
                    self.batch(p, case, "groups of %d, %s images" % (group, count or self.lay.count), ones, count)
        p.set_batching(1, 1)

    def finish(self, lst):
        print("RLTVB\t%s\t%dx%d window %dx%d\tworst error=%.3g\tbatch calls=%d" % (lst, self.M, self.N, self.lay.rows, self.lay.cols, self.worst, self.calls))
        assert not self.bad, "%d failures, the first:\n%s" % (len(self.bad), "\n".join(self.bad[:12]))


# one instantiation of the changed update kernel per length, in both forms: the plain form's factor at row stride cols on a cropped
# window (the last update routed to the raw plane under a normalisation), the free form's on the whole plan
LENGTH_CASES = [Case("plain", 1, NORM_CROPPED, False, False), Case("free", 1, NORM_NONE, True, False)]
ROW_PLANS = [(16, 1 << l) for l in range(5, 14)] + [(2048, 256)]


@pytest.mark.parametrize("M,N", ROW_PLANS, ids=["%dx%d" % s for s in ROW_PLANS])
def test_groups_at_every_row_length(fdr, M, N):
    """N = 2^5 .. 2^13: ROW_OUT_RL_UPDATE_W of the packed inverse kernel exists per length and now reads image k's own factor plane;
    at 2048 x 256 one image takes the split kernels and a group the packed ones.  5 images in groups of 2 (2, 2, 1) and 3 (3, 2)"""
    assert (M, N) != (2048, 256) or (bm.rows4_use_split(N, M, 1, True) and not bm.rows4_use_split(N, M, 2, True))
    rows, cols = bm.short_window(M, N)
    b = _Batch(fdr, M, N, rows, cols, 3 if M * N >= (1 << 19) else 5)
    with b.plan() as p:
        b.run(p, LENGTH_CASES, (2, 3))
    b.finish("rows")


@pytest.mark.parametrize("M,N", rb.COLUMN_PLANS, ids=["%dx%d" % s for s in rb.COLUMN_PLANS])
def test_groups_at_every_column_kernel(fdr, M, N):
    """every pass-B' kernel kind that bm.cols_kernel names, with a short row; 5 images in groups of 2, 3, 4 and 5"""
    rows, cols = bm.short_window(M, N)
    b = _Batch(fdr, M, N, rows, cols, rb.LENGTH_COUNT)
    with b.plan() as p:
        b.run(p, LENGTH_CASES[:1], rb.LENGTH_GROUPS)
    b.finish("columns")


FORM_CASES = [Case(form, n, area, masked, full_out)
              for form, masked, full_out in (("plain", False, False), ("free", False, False), ("free", True, False), ("free", False, True))
              for n in rb.ITERATIONS for area in AREAS]


def test_iterations_normalisations_forms_and_tails(fdr):
    """iterations 0, 1, 3 x FDR_NORM_NONE, _CROPPED, _PADDED x the plain form, the free form with NULL weights, with a mask that has
    zeros and with the M x N output, on an odd window with loose pitch and stride; 5 images in groups of 2 (2, 2, 1), 3 (3, 2), 4
    (4, 1), 8 (one group of 5) and 1 (the loop of the single calls)"""
    M, N = 32, 256
    rows, cols = bm.short_window(M, N)
    b = _Batch(fdr, M, N, rows, cols, 5, loose=True)
    with b.plan() as p:
        b.run(p, FORM_CASES, (2, 3, 4, 8, 1))
        b.run(p, FORM_CASES[4:5], (4,), counts=(1,))  # a batch of one image on a group of 4
    b.finish("forms")


def test_lambda_zero_is_the_batch_without_the_prior(fdr):
    """byte for byte, in both forms and coupled or not, and nothing of the prior is launched"""
    M, N = 32, 256
    rows, cols = bm.short_window(M, N)
    b = _Batch(fdr, M, N, rows, cols, 5, loose=True)
    import torch
    with b.plan() as p:
        p.set_batching(1, 3)
        p.profile(True)
        for case in (Case("plain", 3, NORM_PADDED, False, False), Case("free", 3, NORM_CROPPED, True, False), Case("free", 2, NORM_NONE, False, True)):
            lay, olay = b.lay, b.olay(case)
            d_out = b.fresh(olay)
            dw, ws = b._weights(case)
            free = case.form == "free"
            p.richardson_lucy_batch_dev(b.d_in.data_ptr(), lay.img_pitch, lay.count, lay.rows, lay.cols, lay.stride, d_out.data_ptr() + 4 * olay.lead,
                                        olay.out_pitch, olay.out_stride, case.iterations, case.area, free_boundary=free, d_weights=dw, wstride=ws,
                                        out_rows=olay.rows if free else None, out_cols=olay.cols if free else None)
            torch.cuda.synchronize()
            want = d_out.cpu().numpy()
            p.pass_times()
            for couple in (0, 1):
                got, _ = b.call(p, case, 3 if couple else lay.count, lam=0.0, eps=0.0, couple=couple)
                names = [n for n, _, c in p.pass_times() if c]
                assert not any("RLTV" in n or "(factor)" in n for n in names), names
                if not couple:
                    assert np.array_equal(_nan_guard(want, olay), got), b.name(case)


# ---- coupled calls against the model ----------------------------------------------------------------------------------------------
def _coupled_case(fdr, name):
    motion = fdr.motionBlurKernel(15, 30.0)
    if name == "64x128 win 37x101":
        M, N, rows, cols = 64, 128, 37, 101
    else:
        M, N, rows, cols = 256, 256, 200, 151
    imgs = rb.images(M, N, rows, cols, 3, M + N)
    return M, N, rows, cols, centred_psf(bm.fit_psf(motion, M, N), M, N), imgs, rb.mask(rows, cols, 11)


@pytest.mark.parametrize("name", ["64x128 win 37x101", "256 win 200x151"])
def test_coupled_calls_against_model(fdr, name):
    """3 channels; n = 1, 2, 3 at eps = 1e-3 and n = 10, 30 at eps = 0.05 (the regime in which a comparison step by step means
    something, _rltv_model.py); both forms (the free one masked, its M x N output); within the constants of _rltv_model.py and 10x
    the float32 CPU run of the model"""
    M, N, rows, cols, psf, imgs, w = _coupled_case(fdr, name)
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        p.set_batching(1, 3)
        for lam, eps, n in [(0.01, 1e-3, k) for k in (1, 2, 3)] + [(0.01, 0.05, k) for k in (10, 30)]:
            for form in ("plain", "free"):
                if form == "plain":
                    want = tb.rltv_coupled_model(imgs, psf, M, N, n, lam, eps)
                    cpu32 = rel_err(tb.rltv_coupled_model(imgs, psf, M, N, n, lam, eps, dtype=np.float32), want)
                    got = p.richardson_lucy_tv_batch(imgs, n, lam, eps, couple=fdr.TV_COUPLE_CHANNELS)
                else:
                    want = tb.rltv_free_coupled_model(imgs, psf, M, N, n, lam, eps, w, out_shape=(M, N))
                    cpu32 = rel_err(tb.rltv_free_coupled_model(imgs, psf, M, N, n, lam, eps, w, out_shape=(M, N), dtype=np.float32), want)
                    got = p.richardson_lucy_tv_batch(imgs, n, lam, eps, free_boundary=True, weights=w, full_plane=True, couple=fdr.TV_COUPLE_CHANNELS)
                e = max(rel_err(got[c], want[c]) for c in range(3))
                what = "%s %s lambda=%g eps=%g n=%d" % (name, form, lam, eps, n)
                print("RLTVB\tcoupled\t%s\terr=%.3g\tcpu32=%.3g" % (what, e, cpu32))
                if not e <= TOL[form]:
                    bad.append("%s: error %.3g > %s" % (what, e, TOL[form]))
                if not e <= 10 * max(cpu32, F32_EPS):
                    bad.append("%s: error %.3g above 10x the float32 CPU run's %.3g" % (what, e, cpu32))
                if n == 3:  # coupling is not a no-op, and a normalised output is the model's too
                    alone = p.richardson_lucy_tv_batch(imgs, n, lam, eps, free_boundary=form == "free", weights=w if form == "free" else None,
                                                       full_plane=form == "free")
                    assert not np.array_equal(alone, got), what
        # one channel, coupled, is the single call
        one = p.richardson_lucy_tv_batch(imgs[:1], 3, 0.01, 1e-3, couple=fdr.TV_COUPLE_CHANNELS)
        assert np.array_equal(one[0], p.richardson_lucy_tv(imgs[0], 3, 0.01, 1e-3))
    assert not bad, "\n".join(bad)


def test_coupled_quality_matches_the_model(fdr):
    """the colour quality scene at 1000 photons, n = 100, eps = 1e-3: step for step the arithmetics drift apart here
    (_rltv_model.py), the PSNR must agree with the model's to 0.05 dB, coupled and channel-wise"""
    case = tb.colour_quality_case(1000.0)
    with fdr.Plan(case["M"], case["N"], fdr.MODE_FAST) as p:
        p.set_operator_psf(case["psf"])
        p.set_batching(1, 3)
        for coupled, lam in ((True, 0.015), (False, 0.01)):
            pm = tb.colour_quality_run(case, (100,), lam, coupled)[100]
            got = p.richardson_lucy_tv_batch(case["d"], 100, lam, tb.QUALITY_EPS, couple=fdr.TV_COUPLE_CHANNELS if coupled else fdr.TV_COUPLE_NONE)
            pg = psnr(got, case["truth"])
            print("RLTVB\tquality\tcoupled=%s lambda=%g\tmodel %.3f dB, GPU %.3f dB" % (coupled, lam, pm, pg))
            assert abs(pg - pm) <= 0.05, (coupled, pm, pg)


# ---- hygiene --------------------------------------------------------------------------------------------------------------------
def test_determinism_forms_and_python_layers(fdr):
    """two calls give the same bits; the host and the _dev form agree; Plan.richardson_lucy_tv_batch and richardsonLucyTV_RGB give the
    single calls' bits uncoupled and the coupled call's bits coupled"""
    M, N, rows, cols = 64, 128, 50, 100
    psf = centred_psf(bm.fit_psf(fdr.motionBlurKernel(15, 30.0), M, N), M, N)
    b = _Batch(fdr, M, N, rows, cols, 3)
    imgs, w = b.imgs, b.mask
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        want_p = np.stack([p.richardson_lucy_tv(x, 3, 0.02, norm_area=NORM_CROPPED) for x in imgs])
        want_f = np.stack([p.richardson_lucy_tv(x, 3, 0.02, free_boundary=True, weights=w, norm_area=NORM_PADDED) for x in imgs])
        want_m = np.stack([p.richardson_lucy_tv(x, 2, 0.02, free_boundary=True, full_plane=True) for x in imgs])
        for group in (1, 3):
            p.set_batching(1, group)
            assert np.array_equal(p.richardson_lucy_tv_batch(imgs, 3, 0.02, norm_area=NORM_CROPPED), want_p)
            assert np.array_equal(p.richardson_lucy_tv_batch(imgs, 3, 0.02, free_boundary=True, weights=w, norm_area=NORM_PADDED), want_f)
            assert np.array_equal(p.richardson_lucy_tv_batch(imgs, 2, 0.02, free_boundary=True, full_plane=True), want_m)
        for free in (False, True):
            kw = dict(free_boundary=True, weights=w) if free else {}
            a = p.richardson_lucy_tv_batch(imgs, 5, 0.02, couple=fdr.TV_COUPLE_CHANNELS, **kw)
            assert np.array_equal(a, p.richardson_lucy_tv_batch(imgs, 5, 0.02, couple=fdr.TV_COUPLE_CHANNELS, **kw)), "two runs differ"
            assert np.array_equal(a, p.richardson_lucy_tv_batch(imgs, 5, 0.02, 1e-3, couple=fdr.TV_COUPLE_CHANNELS, **kw)), "eps = 0 is not FDR_RLTV_EPS"
            case = Case("free" if free else "plain", 5, NORM_NONE, free, False)
            with b.plan() as q:
                q.set_batching(1, 3)
                out, olay = b.call(q, case, 3, lam=0.02, eps=0.0, couple=fdr.TV_COUPLE_CHANNELS)
            assert np.array_equal(bm.unpack(out, olay), a), "host and _dev forms differ"
    small = fdr.motionBlurKernel(7, 30.0)
    ch = [x.copy() for x in imgs]
    fdr.richardsonLucyTV_RGB(ch, small, 3, 0.02)
    assert all(np.array_equal(c, fdr.richardsonLucyTV_myfft(x, small, 3, 0.02)) for c, x in zip(ch, imgs))
    ch = [x.copy() for x in imgs]
    fdr.richardsonLucyTV_RGB(ch, small, 3, 0.02, free_boundary=True, weights=w)
    assert all(np.array_equal(c, fdr.richardsonLucyTV_myfft(x, small, 3, 0.02, free_boundary=True, weights=w)) for c, x in zip(ch, imgs))
    ch = [x.copy() for x in imgs]
    fdr.richardsonLucyTV_RGB(ch, small, 3, 0.02, coupled=True)
    Mp, Np = fdr._rl_plan_size(rows, cols)
    with fdr.Plan(Mp, Np, fdr.MODE_FAST) as p:
        p.set_operator_psf(small)
        p.set_batching(1, 3)
        assert np.array_equal(np.stack(ch), p.richardson_lucy_tv_batch(imgs, 3, 0.02, couple=fdr.TV_COUPLE_CHANNELS))


def test_other_results_survive_and_later_calls_allocate_nothing(fdr):
    """Wiener, single RL-TV, batched RL and TV results on the same plan are byte-identical before a batched RL-TV call, after it, and
    after the workspace has grown again; once the workspace holds the group, calls of both forms allocate nothing"""
    import torch
    M, N, rows, cols = 256, 512, 200, 451
    b = _Batch(fdr, M, N, rows, cols, 4)
    img = b.imgs[1]
    with b.plan() as p:
        p.set_psf(bm.fit_psf(fdr.motionBlurKernel(15, 30.0), M, N), bm.K32)

        def others():
            p.set_batching(1, 2)
            r = (p.wiener(img), p.richardson_lucy_tv(img, 3, 0.02), p.richardson_lucy_tv(img, 3, 0.02, free_boundary=True, weights=b.mask),
                 p.richardson_lucy_batch(b.imgs, 2), p.richardson_lucy_batch(b.imgs, 2, free_boundary=True, weights=b.mask),
                 p.tv_deconv(img, 200.0, iterations=3), p.tv_deconv_batch(b.imgs[:2], 200.0, iterations=2))
            return r

        before = others()
        cases = (Case("plain", 2, NORM_PADDED, False, False), Case("free", 2, NORM_CROPPED, True, False))
        p.set_batching(1, 2)
        first = [b.call(p, c, 4)[0] for c in cases]
        mid = others()
        p.set_batching(1, 4)  # the workspace grows again: 2 -> 4 images
        grown = [b.call(p, c, 4)[0] for c in cases]
        torch.cuda.synchronize()
        f0 = torch.cuda.mem_get_info()[0]
        again = [b.call(p, c, 4, couple=k) [0] for c in cases for k in (0, 1)]
        torch.cuda.synchronize()
        f1 = torch.cuda.mem_get_info()[0]
        after = others()
        for k, (x, y, z) in enumerate(zip(before, mid, after)):
            assert np.array_equal(x, y) and np.array_equal(x, z), "result %d changed around the batched calls" % k
        for x, y, z in zip(first, grown, again[::2]):
            assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True), "the group size changed an image"
        # the NaN-filled output buffers of `again` are torch's, freed and reused: the library itself took nothing
        print("RLTVB\tallocations\tlater calls %d bytes (one M x N plane: %d)" % (f0 - f1, 4 * M * N))
        assert f0 - f1 < 4 * M * N, "a later call allocated"


def test_refusals_leave_the_plan_usable(fdr):
    """every refusal returns its code with no pass launched, and a valid call afterwards gives the single calls' bits"""
    import torch
    L = fdr.lib
    M, N, rows, cols, count = 32, 64, 31, 61, 3
    psf = centred_psf(bm.fit_psf(fdr.motionBlurKernel(15, 30.0), M, N), M, N)
    imgs = rb.images(M, N, rows, cols, count, 3)
    px = rows * cols
    d_in = torch.from_numpy(imgs.reshape(-1)).cuda()
    d_out = torch.zeros(count * M * N, dtype=torch.float32, device="cuda")
    d_w = torch.ones(px, dtype=torch.float32, device="cuda")
    vp = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)

    def prm(n=2, free=0, lam=0.01, eps=1e-3, area=NORM_NONE, sigma=0.01, orows=0, ocols=0, couple=0):
        return ctypes.byref(fdr.RlTvBatchParams(n, free, lam, eps, area, sigma, orows, ocols, couple))

    def rl(p, src=None, dst=None, w=None, ws=cols, pr=None, cnt=count, stride=cols, ostride=cols, r=rows, c=cols, opitch=px):
        return L.fdr_richardson_lucy_tv_batch_f32_dev(p._h, vp(d_in) if src is None else src, px, cnt, r, c, stride, w, ws,
                                                      vp(d_out) if dst is None else dst, opitch, ostride, prm() if pr is None else pr, None)

    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        assert rl(p) == -4  # FDR_ERR_STATE: no operator PSF yet
        p.set_operator_psf(psf)
        want = np.stack([p.richardson_lucy_tv(x, 2, 0.01) for x in imgs])
        p.set_batching(1, 2)
        p.profile(True)
        p.pass_times()

        def works():
            d_out.zero_()
            assert rl(p) == 0
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy()[:count * px].reshape(count, rows, cols), want)
            p.pass_times()

        for bad in (lambda: rl(p, cnt=-1), lambda: rl(p, src=ctypes.c_void_p(0)), lambda: rl(p, dst=ctypes.c_void_p(0)),
                    lambda: L.fdr_richardson_lucy_tv_batch_f32_dev(p._h, vp(d_in), px, count, rows, cols, cols, None, 0, vp(d_out), px, cols, None, None),
                    lambda: rl(p, r=M + 1), lambda: rl(p, stride=cols - 1), lambda: rl(p, ostride=cols - 1),  # what the single call refuses
                    lambda: rl(p, pr=prm(n=-1)), lambda: rl(p, pr=prm(area=7)),
                    lambda: rl(p, pr=prm(lam=-0.01)), lambda: rl(p, pr=prm(lam=0.1251)), lambda: rl(p, pr=prm(lam=float("nan"))),  # the prior's own
                    lambda: rl(p, pr=prm(eps=-1e-3)), lambda: rl(p, pr=prm(eps=float("inf"))),
                    lambda: rl(p, pr=prm(couple=2)), lambda: rl(p, pr=prm(couple=-1)), lambda: rl(p, pr=prm(couple=2, lam=0.0)),
                    lambda: rl(p, pr=prm(couple=1)),                                                   # 3 coupled channels on groups of 2
                    lambda: rl(p, pr=prm(couple=1, lam=0.0)),
                    lambda: rl(p, w=vp(d_w)),                                                          # weights with the plain form
                    lambda: rl(p, pr=prm(orows=rows + 1, ocols=cols)),                                 # the plain form's output window
                    lambda: rl(p, pr=prm(free=1, sigma=0.0, orows=rows, ocols=cols)), lambda: rl(p, pr=prm(free=1, sigma=1.0, orows=rows, ocols=cols)),
                    lambda: rl(p, pr=prm(free=1, orows=rows - 1, ocols=cols)), lambda: rl(p, pr=prm(free=1, orows=M + 1, ocols=cols)),
                    lambda: rl(p, pr=prm(free=1, orows=rows, ocols=cols), w=vp(d_w), ws=cols - 1),
                    lambda: rl(p, pr=prm(free=1, orows=M, ocols=N), ostride=N - 1, opitch=M * N),
                    lambda: rl(p, dst=vp(d_in, 2 * px + 5)), lambda: rl(p, dst=vp(d_in, -2 * px - 7))):  # overlap over the span of the batch
            assert bad() == -1, L.fdr_last_error()
            torch.cuda.synchronize()
            assert sum(c for _, _, c in p.pass_times()) == 0, "a refused call launched a pass"
            works()
        big = torch.zeros(4 * px, dtype=torch.float32, device="cuda")
        assert rl(p, pr=prm(free=1, orows=rows, ocols=cols), dst=vp(big), w=vp(big, 2 * px + 9)) == -1 and b"weights" in L.fdr_last_error()
        assert rl(p, cnt=0, src=ctypes.c_void_p(0)) == 0  # nothing to do
        assert sum(c for _, _, c in p.pass_times()) == 0
        works()
        p.set_batching(1, 3)
        assert rl(p, pr=prm(couple=1)) == 0  # one launch group now
        # the factor entry on device pointers
        o = torch.empty(3 * 64 * 64, dtype=torch.float32, device="cuda")
        u = torch.rand(3 * 64 * 64, dtype=torch.float32, device="cuda")
        fac = lambda **k: L.fdr_rl_tv_factor_group_f32_dev(0, k.get("u", u.data_ptr()), 4096, k.get("n", 3), 64, 64, k.get("stride", 64), k.get("w"),
                                                           k.get("lam", 0.01), 1e-3, k.get("couple", 1), k.get("o", o.data_ptr()), k.get("opitch", 4096), 64, None)
        assert fac() == 0
        assert fac(n=9) == -1 and fac(n=0) == -1 and fac(stride=63) == -1 and fac(lam=0.3) == -1 and fac(couple=3) == -1 and fac(opitch=4095) == -1
        assert fac(o=u.data_ptr() + 4 * 2 * 4096 + 64) == -1 and fac(w=o.data_ptr() + 4 * 4096) == -1  # overlap in the span of the planes
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_FULL_SPECTRUM) as q:  # not the operator's path
        assert rl(q) == -1


def test_launch_census_of_a_grouped_call(fdr):
    """one factor launch and the six passes per group and iteration; the group launches have their own pass names (pass A names
    its group launches too; a tail of one image makes the launches of the single call but for the factor's name)"""
    M, N, rows, cols = 256, 512, 200, 300
    b = _Batch(fdr, M, N, rows, cols, 5)
    it = 3
    with b.plan() as p:
        p.set_batching(1, 2)  # 5 images: groups of 2, 2, 1
        p.profile(True)
        p.pass_times()
        b.call(p, Case("plain", it, NORM_PADDED, False, False), 5)
        names = {n: c for n, _, c in p.pass_times() if c}
        print("RLTVB\tpasses\tplain\t%s" % names)
        g = 3
        a1, ag = "A op rows: pad+FFT (blur / RL)", "A op rows: pad+FFT (blur / RL), group"  # the tail of one image, the two groups of two
        want = {"RL init: u = max(d, 0)": 5, "RLTV factor (group): w / (1 - lambda div)": g * it, a1: 2 * it, ag: 2 * 2 * it,
                "B' op cols: FFT*H*IFFT": g * it, "B' op cols: FFT*conj(H)*IFFT": g * it, "C op rows: IFFT+RL ratio": g * it,
                "C op rows: IFFT+RL update (factor)": g * it, "E RL minmax+normalize": 5}
        assert names == want, names
        b.call(p, Case("free", it, NORM_NONE, False, False), 5)
        names = {n: c for n, _, c in p.pass_times() if c}
        print("RLTVB\tpasses\tfree\t%s" % names)
        want = {"RLF setup: dw, W, sums": 5, "RLF start: wgt = 1/alpha, u": 5, "RLTV factor (group): w / (1 - lambda div)": g * it,
                a1: 1 + 2 * it, ag: 2 * 2 * it, "B' op cols: FFT*H*IFFT": g * it, "B' op cols: FFT*conj(H)*IFFT": 1 + g * it,
                "C op rows: IFFT+crop (blur)": 1, "C op rows: IFFT+RL ratio (free)": g * it, "C op rows: IFFT+RL update (weighted)": g * it,
                "RLF out: crop": 5}
        assert names == want, names
        p.set_batching(1, 3)
        b.call(p, Case("plain", it, NORM_NONE, False, False), 3, couple=fdr.TV_COUPLE_CHANNELS)
        names = {n: c for n, _, c in p.pass_times() if c}
        assert names.get("RLTV factor (coupled): w / (1 - lambda div p_c)") == it and not any("(group)" in n for n in names), names


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_cli_rl_tv_runs_batched(fdr, tmp_path):
    """tools/cli/gpu --rl 4 --rl-tv 0.01, with and without --free-boundary --mask: the planes (--raw-out) are the bytes of the
    per-channel Python loop; --rl-tv-color: those of Plan.richardson_lucy_tv_batch(..., couple=TV_COUPLE_CHANNELS); --rl-tv-color
    without --rl-tv prints the usage text"""
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
    bgr = np.stack([np.ascontiguousarray(rgb[:, :, c]) for c in (2, 1, 0)])
    legs = (("plain", [], dict(), False), ("free masked", ["--free-boundary", "--mask", mask_png], dict(free_boundary=True, weights=keep.astype(np.float32)), False),
            ("colour", ["--rl-tv-color"], dict(), True))
    for tag, extra, kw, coupled in legs:
        out_png, out_raw = str(tmp_path / "o.png"), str(tmp_path / "o.f32")
        r = subprocess.run([gpu, png, "40", "45", "--rl", "4", "--rl-tv", "0.01"] + extra + ["--out", out_png, "--raw-out", out_raw], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Deblurring 3 channels took(gpu[richardson-lucy " in r.stdout, r.stdout
        raw = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
        M, N = fdr._rlfree_plan_size(h, w, 40, 40) if kw.get("free_boundary") else fdr._rl_plan_size(h, w)
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            p.set_operator_psf(psf)
            if coupled:
                p.set_batching(1, 3)
                want = p.richardson_lucy_tv_batch(bgr, 4, 0.01, norm_area=fdr.NORM_PADDED, couple=fdr.TV_COUPLE_CHANNELS)
                assert not np.array_equal(want, first_plain), "coupling changed nothing"
            else:
                want = np.stack([p.richardson_lucy_tv(x, 4, 0.01, norm_area=fdr.NORM_PADDED, **kw) for x in bgr])
        if tag == "plain":
            first_plain = want
        assert np.array_equal(raw, want), (tag, float(np.abs(raw - want).max()))
    r = subprocess.run([gpu, png, "40", "45", "--rl", "4", "--rl-tv-color"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "Usage" in r.stdout, (r.returncode, r.stdout[-300:])
