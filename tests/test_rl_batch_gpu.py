"""Batched blur and Richardson-Lucy on the MI355X (fdr_blur_batch_f32_dev, fdr_richardson_lucy_batch_f32*) at every row and column
length, group size and tail, iteration count, normalisation, window and layout, in all four forms: blur, adjoint blur, plain RL and
free-boundary RL (NULL weights, a mask with zeros, the M x N output).

Every image of every batch must equal, bit for bit (np.array_equal), the same image through the single-image _dev call on the same
plan, read from and written to the places it has in the batch, and lie within the tolerance that test_rl_gpu.py / test_rlfree_gpu.py
apply to the float64 model (BLUR_TOL, RL_TOL, RLFREE_TOL of their model files); NaN and inf fail; the sentinel that fills the output
buffer must survive in the stride padding, the pitch gaps and the slack around the images.  Cropped windows use a centred PSF, as
test_rl_gpu.py does (a top-left PSF leaves c = 0 rows that the float64 model cannot judge).  Each case prints an `RLB` line with its
largest error (pytest -s).  The shapes are the smallest that reach the code; test_rl_batch_host.py proves the coverage of the lists
and that this judge flags the fault models of a batched call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _batch_model as bm
import _rl_batch_model as rb
from _batch_model import SENTINEL
from _rl_batch_model import AREA_NAME, AREAS, Case
from _rl_model import BLUR_TOL, NORM_CROPPED, NORM_NONE, NORM_PADDED, RL_TOL, centred_psf, rel_err, rl_model
from _rlfree_model import RLFREE_TOL, SIGMA, SIGMA_MARGIN, rlfree_state, sigma_margin

pytestmark = pytest.mark.gpu

TOL = {"blur": BLUR_TOL, "adjoint": BLUR_TOL, "plain": RL_TOL, "free": RLFREE_TOL}


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
        alpha = rlfree_state(self.imgs[0], self.psf, M, N, 0, weights=self.mask)["alpha"]  # (masked: the smaller coverage)
        assert sigma_margin(alpha, SIGMA) >= SIGMA_MARGIN, "a model alpha lies at the threshold: the case cannot be judged"

    def plan(self):
        p = self.fdr.Plan(self.M, self.N, self.fdr.MODE_FAST)
        p.set_operator_psf(self.psf)
        return p

    def olay(self, case):
        return rb.out_layout(self.lay, self.M, self.N) if case.full_out else self.lay

    def fresh(self, olay):
        import torch
        return torch.full((bm.out_size(olay),), SENTINEL, dtype=torch.float32, device="cuda")

    def _weights(self, case):
        return (self.d_w.data_ptr(), self.wstride) if case.masked else (None, 0)

    def alone(self, p, case):
        """every image through the single-image _dev call, read from and stored to the places it has in the batch:
        ([count, out_rows, out_cols], their errors against the model, the model)"""
        import torch
        lay, olay = self.lay, self.olay(case)
        d_one = self.fresh(olay)
        dw, ws = self._weights(case)
        for i in range(lay.count):
            src, dst = self.d_in.data_ptr() + 4 * i * lay.img_pitch, d_one.data_ptr() + 4 * bm.out_base(olay, i)
            if case.form in ("blur", "adjoint"):
                p.blur_dev(src, lay.rows, lay.cols, lay.stride, dst, olay.out_stride, adjoint=case.form == "adjoint", stream=self.stream)
            elif case.form == "plain":
                p.richardson_lucy_dev(src, lay.rows, lay.cols, lay.stride, dst, olay.out_stride, case.iterations, case.area, stream=self.stream)
            else:
                p.richardson_lucy_free_dev(src, lay.rows, lay.cols, lay.stride, dst, olay.out_stride, case.iterations, d_weights=dw, wstride=ws,
                                           norm_area=case.area, out_rows=olay.rows, out_cols=olay.cols, stream=self.stream)
        torch.cuda.synchronize()
        one = d_one.cpu().numpy()
        if not bm.outside_untouched(one, olay):
            self.bad.append("%s: the single-image call wrote outside its window" % self.name(case))
        ones = bm.unpack(one, olay)
        refs = rb.references(case.form, self.imgs, self.psf, self.M, self.N, case.iterations, case.area, self.mask if case.masked else None,
                             out_shape=(olay.rows, olay.cols))
        return ones, rb.model_errors(ones, refs, case.area), refs

    def batch(self, p, case, what, ones, count=None):
        """one batched call of the first `count` images into a sentinel-filled buffer, judged; returns the flat output"""
        import torch
        n = self.lay.count if count is None else count
        lay, olay = self.lay._replace(count=n), self.olay(case)._replace(count=n)
        d_out = self.fresh(olay)
        dst = d_out.data_ptr() + 4 * olay.lead
        dw, ws = self._weights(case)
        if case.form in ("blur", "adjoint"):
            p.blur_batch_dev(self.d_in.data_ptr(), lay.img_pitch, n, lay.rows, lay.cols, lay.stride, dst, olay.out_pitch, olay.out_stride,
                             adjoint=case.form == "adjoint", stream=self.stream)
        else:
            free = case.form == "free"
            p.richardson_lucy_batch_dev(self.d_in.data_ptr(), lay.img_pitch, n, lay.rows, lay.cols, lay.stride, dst, olay.out_pitch, olay.out_stride,
                                        case.iterations, case.area, free_boundary=free, d_weights=dw, wstride=ws,
                                        out_rows=olay.rows if free else None, out_cols=olay.cols if free else None, stream=self.stream)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        v = rb.judge("%s %s" % (self.name(case), what), out, olay, ones[0][:n], ones[2][:n], TOL[case.form], case.area, ones_err=ones[1][:n])
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
        print("RLB\t%s\t%dx%d window %dx%d\tworst error=%.3g\tbatch calls=%d" % (lst, self.M, self.N, self.lay.rows, self.lay.cols, self.worst, self.calls))
        assert not self.bad, "%d failures, the first:\n%s" % (len(self.bad), "\n".join(self.bad[:12]))


def _length_case(fdr, lst, M, N):
    count, groups = (rb.BIG_COUNT, rb.BIG_GROUPS) if M * N >= rb.BIG_PIXELS else (rb.LENGTH_COUNT, rb.LENGTH_GROUPS)
    rows, cols = bm.short_window(M, N)
    b = _Batch(fdr, M, N, rows, cols, count)
    with b.plan() as p:
        b.run(p, rb.LENGTH_CASES, groups)
    b.finish(lst)


# ---- 1. row lengths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", rb.ROW_PLANS, ids=["%dx%d" % s for s in rb.ROW_PLANS])
def test_groups_at_every_row_length(fdr, M, N):
    """N = 2^5 .. 2^13, half spectrum: one instantiation of each changed kind of the inverse packed kernel per length, with
    blockIdx.y = image; at 256 .. 2048 columns (and up to 2048 rows) one image takes the split kernels and a group the packed ones"""
    _length_case(fdr, "rows", M, N)


# ---- 2. column lengths --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", rb.COLUMN_PLANS, ids=["%dx%d" % s for s in rb.COLUMN_PLANS])
def test_groups_at_every_column_kernel(fdr, M, N):
    """every pass-B' kernel kind that bm.cols_kernel names (split, persistent radix-8, fused16 flat and 2-d), now with an operator
    table as its filter"""
    _length_case(fdr, "columns", M, N)


# ---- 3. groups and tails, iterations, normalisations, windows and layouts -----------------------------------------------------------
FORM_CASES = [Case(form, n, area, masked, full_out)
              for form, masked, full_out in (("plain", False, False), ("free", False, False), ("free", True, False), ("free", False, True))
              for n in rb.ITERATIONS for area in AREAS]
BLUR_CASES = [Case("blur", 0, NORM_NONE, False, False), Case("adjoint", 0, NORM_NONE, False, False)]


@pytest.mark.parametrize("full,loose", [(False, True), (True, False)], ids=["odd-window-loose", "full-plane-tight"])
def test_iterations_normalisations_forms(fdr, full, loose):
    """iterations 0, 1, 3 (the start alone, the last update routed to the raw plane under a normalisation, the in-place update) x
    FDR_NORM_NONE, _CROPPED, _PADDED x plain RL, free RL with NULL weights, with a mask that has zeros and with the M x N output, on
    an odd window with loose pitch and stride and on the full plane; 5 images in groups of 2 (2, 2, 1) and 4 (4, 1)"""
    M, N = 32, 256
    rows, cols = (M, N) if full else bm.short_window(M, N)
    b = _Batch(fdr, M, N, rows, cols, 5, loose=loose)
    with b.plan() as p:
        b.run(p, BLUR_CASES + FORM_CASES, (2, 4))
    b.finish("forms")


TAIL_CASES = BLUR_CASES + [Case("plain", 3, NORM_PADDED, False, False), Case("free", 3, NORM_CROPPED, True, False)]


def test_groups_and_tails(fdr):
    """11 images in groups of 2, 3, 4, 5 and 8 (tails of 1, 2 and 3), groups of 1 (the loop of the single calls) and a batch of one
    image on a group of 4; odd window, loose pitch and stride"""
    M, N = 64, 512
    rows, cols = bm.short_window(M, N)
    b = _Batch(fdr, M, N, rows, cols, rb.COUNT, loose=True)
    with b.plan() as p:
        b.run(p, TAIL_CASES, (1,) + rb.GROUPS)
        b.run(p, TAIL_CASES, (4,), counts=(1,))
    b.finish("tails")


def test_host_form_and_python_layers(fdr):
    """Plan.richardson_lucy_batch (host arrays) and the module-level RGB functions give the per-image single calls' bits"""
    M, N, rows, cols = 64, 128, 50, 100
    psf = centred_psf(bm.fit_psf(fdr.motionBlurKernel(15, 30.0), M, N), M, N)
    imgs = rb.images(M, N, rows, cols, 3, 5)
    w = rb.mask(rows, cols, 9)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        want_p = [p.richardson_lucy(x, 3, NORM_CROPPED) for x in imgs]
        want_f = [p.richardson_lucy_free(x, 3, weights=w, norm_area=NORM_PADDED) for x in imgs]
        want_m = [p.richardson_lucy_free(x, 2, full_plane=True) for x in imgs]
        for group in (1, 3):
            p.set_batching(1, group)
            assert np.array_equal(p.richardson_lucy_batch(imgs, 3, norm_area=NORM_CROPPED), np.stack(want_p))
            assert np.array_equal(p.richardson_lucy_batch(imgs, 3, free_boundary=True, weights=w, norm_area=NORM_PADDED), np.stack(want_f))
            assert np.array_equal(p.richardson_lucy_batch(imgs, 2, free_boundary=True, full_plane=True), np.stack(want_m))
    small = fdr.motionBlurKernel(7, 30.0)
    ch = [x.copy() for x in imgs]
    fdr.richardsonLucy_RGB(ch, small, 3)
    assert all(np.array_equal(c, fdr.richardsonLucy_myfft(x, small, 3)) for c, x in zip(ch, imgs))
    ch = [x.copy() for x in imgs]
    fdr.richardsonLucyFree_RGB(ch, small, 3, weights=w)
    assert all(np.array_equal(c, fdr.richardsonLucyFree_myfft(x, small, 3, weights=w)) for c, x in zip(ch, imgs))


# ---- 4. the slots are shared ----------------------------------------------------------------------------------------------------
def test_other_results_survive_a_batched_call(fdr):
    """the Wiener result of the plan and a single-image RL of either form after a batched call are byte-identical to before it (the
    batch runs on the slots of the Wiener batches and regrows the free-boundary workspace)"""
    M, N, rows, cols = 64, 256, 63, 253
    b = _Batch(fdr, M, N, rows, cols, 5)
    with b.plan() as p:
        p.set_psf(bm.fit_psf(fdr.motionBlurKernel(15, 30.0), M, N), bm.K32)
        img = b.imgs[1]

        def others():
            return (p.wiener(img), p.wiener_batch(b.imgs), p.richardson_lucy(img, 3, NORM_PADDED),
                    p.richardson_lucy_free(img, 3, weights=b.mask, norm_area=NORM_CROPPED), p.blur(img))

        before = others()
        p.set_batching(2, 4)
        for case in TAIL_CASES:
            b.batch(p, case, "groups of 4 on two streams", b.alone(p, case))
        p.set_option(fdr.OPT_BATCH_GRAPH, 1)  # accepted, changes nothing
        b.batch(p, TAIL_CASES[2], "graph option set", b.alone(p, TAIL_CASES[2]))
        p.set_option(fdr.OPT_BATCH_GRAPH, 0)
        after = others()
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
    b.finish("shared slots")


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_plan_usable(fdr):
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

    def prm(n=2, area=NORM_NONE, free=0, sigma=SIGMA, orows=0, ocols=0):
        return ctypes.byref(fdr.RlBatchParams(n, area, free, sigma, orows, ocols))

    def rl(p, src=None, dst=None, w=None, ws=cols, pr=None, cnt=count, stride=cols, ostride=cols, r=rows, c=cols, opitch=px):
        return L.fdr_richardson_lucy_batch_f32_dev(p._h, vp(d_in) if src is None else src, px, cnt, r, c, stride, w, ws, vp(d_out) if dst is None else dst,
                                                   opitch, ostride, prm() if pr is None else pr, None)

    def blur(p, cnt=count, src=None, dst=None, r=rows, stride=cols):
        return L.fdr_blur_batch_f32_dev(p._h, vp(d_in) if src is None else src, px, cnt, r, cols, stride, vp(d_out) if dst is None else dst, px, cols, 0, None)

    want = np.stack([rl_model(x, psf, M, N, 2) for x in imgs])

    def works(p):
        d_out.zero_()
        assert rl(p) == 0
        torch.cuda.synchronize()
        assert rel_err(d_out.cpu().numpy()[:count * px].reshape(count, rows, cols), want) <= RL_TOL

    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        assert rl(p) == -4 and blur(p) == -4  # FDR_ERR_STATE: no operator PSF yet
        p.set_operator_psf(psf)
        p.set_batching(1, 2)
        for bad in (lambda: rl(p, cnt=-1), lambda: blur(p, cnt=-1),                                   # negative count
                    lambda: rl(p, src=ctypes.c_void_p(0)), lambda: rl(p, dst=ctypes.c_void_p(0)),     # null pointers
                    lambda: blur(p, src=ctypes.c_void_p(0)), lambda: blur(p, dst=ctypes.c_void_p(0)),
                    lambda: L.fdr_richardson_lucy_batch_f32_dev(p._h, vp(d_in), px, count, rows, cols, cols, None, 0, vp(d_out), px, cols, None, None),
                    lambda: rl(p, r=M + 1), lambda: rl(p, stride=cols - 1), lambda: rl(p, ostride=cols - 1),  # what the single call refuses
                    lambda: blur(p, r=M + 1), lambda: blur(p, stride=cols - 1),
                    lambda: rl(p, pr=prm(n=-1)), lambda: rl(p, pr=prm(area=7)),
                    lambda: rl(p, w=vp(d_w)),                                                          # weights with the plain form
                    lambda: rl(p, pr=prm(orows=rows + 1, ocols=cols)),                                 # the plain form's output window
                    lambda: rl(p, pr=prm(free=1, sigma=0.0, orows=rows, ocols=cols)),
                    lambda: rl(p, pr=prm(free=1, sigma=1.0, orows=rows, ocols=cols)),
                    lambda: rl(p, pr=prm(free=1, orows=rows - 1, ocols=cols)), lambda: rl(p, pr=prm(free=1, orows=M + 1, ocols=cols)),
                    lambda: rl(p, pr=prm(free=1, orows=rows, ocols=cols), w=vp(d_w), ws=cols - 1),
                    lambda: rl(p, pr=prm(free=1, orows=M, ocols=N), ostride=N - 1, opitch=M * N)):
            assert bad() == -1, L.fdr_last_error()
            works(p)  # every refusal leaves the plan as it was
        # overlap over the whole span of the batch: the output of image 0 on the input of image 2; the last output on the weights
        assert rl(p, dst=vp(d_in, 2 * px + 5)) == -1 and b"overlap" in L.fdr_last_error()
        works(p)
        assert rl(p, dst=vp(d_in, -2 * px - 7)) == -1 and b"overlap" in L.fdr_last_error()
        works(p)
        big = torch.zeros(4 * px, dtype=torch.float32, device="cuda")
        assert rl(p, pr=prm(free=1, orows=rows, ocols=cols), dst=vp(big), w=vp(big, 2 * px + 9)) == -1 and b"weights" in L.fdr_last_error()
        works(p)
        assert rl(p, cnt=0, src=ctypes.c_void_p(0)) == 0 and blur(p, cnt=0) == 0  # nothing to do
        works(p)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_FULL_SPECTRUM) as q:  # not the operator's path
        assert rl(q) == -1 and blur(q) == -1


# ---- 6. the command line --------------------------------------------------------------------------------------------------------
def test_cli_rl_runs_batched_with_the_loops_bytes(fdr, tmp_path):
    """tools/cli/gpu --rl 3 and --rl 3 --free-boundary on tests/golden/car_blurred.png: the planes (--raw-out) are the bytes of the
    per-channel loop of the Python single calls on the same padded plan"""
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(root, "tools", "cli", "gpu")
    png = os.path.join(root, "tests", "golden", "car_blurred.png")
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    psf = fdr.motionBlurKernel(40, 45.0)
    for extra, size in (([], fdr._rl_plan_size(h, w)), (["--free-boundary"], fdr._rlfree_plan_size(h, w, 40, 40))):
        out_png, out_raw = str(tmp_path / "rlb.png"), str(tmp_path / "rlb.f32")
        r = subprocess.run([gpu, png, "40", "45", "--rl", "3"] + extra + ["--out", out_png, "--raw-out", out_raw], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert os.path.getsize(out_png) > 0
        planes = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
        with fdr.Plan(size[0], size[1], fdr.MODE_FAST) as p:
            p.set_operator_psf(psf)
            for k, c in enumerate((2, 1, 0)):  # B, G, R
                ch = np.ascontiguousarray(rgb[:, :, c])
                want = p.richardson_lucy_free(ch, 3, norm_area=fdr.NORM_PADDED) if extra else p.richardson_lucy(ch, 3, fdr.NORM_PADDED)
                assert np.array_equal(planes[k], want), (extra, k, float(np.abs(planes[k] - want).max()))
