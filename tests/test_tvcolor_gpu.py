"""Batched and colour total-variation deconvolution (fdr_tv_deconv_batch_f32*) on the MI355X, on the smallest plans that reach each
tile geometry of the spatial kernels (_tvcolor_model.GPU_PLANS).

Uncoupled, every image of every batch must equal, bit for bit (np.array_equal), the same image through fdr_tv_deconv_f32_dev on the
same plan, read from and written to the places it has in the batch, and lie within TV_TOL of the float64 model; the sentinel that
fills the output buffer must survive in the stride padding, the pitch gaps and the slack around the images.  Coupled (vectorial TV),
every channel must lie within TV_TOL of the coupled float64 model of _tvcolor_model.py, one channel must give the single call's
bits, two calls must give equal bits, and the result must lie far from the uncoupled one.  NaN and inf fail everywhere.  Then the
refusals, the growth of the workspace, the pass names and the wrappers.  Each case prints a `TVC` line with its largest error
(pytest -s); test_tvcolor_host.py proves that this judge flags the fault models of the coupled kernel on these very shapes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _batch_model as bm
import _tvcolor_model as tc
from _batch_model import SENTINEL
from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, normalize, rel_err
from _tv_model import TV_TOL
from test_tvcolor_host import MU, RHO, gpu_case

pytestmark = pytest.mark.gpu

AREAS = (NORM_NONE, NORM_CROPPED, NORM_PADDED)
PLAN_IDS = ["%dx%d" % (p[0], p[1]) for p in tc.GPU_PLANS]
COUNTS, GROUPS = (1, 2, 3, 5, 8), (1, 2, 3, 4, 8)
PAIRS = [(c, g) for c in COUNTS for g in GROUPS]  # tails: 3 in 2s, 5 in 2s, 3s and 4s, 8 in 3s, a batch below its group, ...


def _err(got, want, area):
    """rel_err for raw outputs, max-abs for normalised ones (as test_tv_gpu.py); NaN or inf in `got` gives NaN"""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return float("nan")
    return rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(got - want)))


def _finish(raw, nonneg, area, M, N):
    """the output of a call from the raw windows [C, rows, cols] of the model"""
    out = np.maximum(raw, 0) if nonneg else raw
    return np.stack([normalize(o, area, M, N) for o in out])


def _raws(imgs, psf, M, N, ns, coupled, aniso=False):
    """{n: raw float64 windows [C, rows, cols]} from one run of the model's iteration"""
    _, rows, cols = imgs.shape
    out = {}
    for k, (x, _, _) in enumerate(tc.tvcolor_iterates(imgs, psf, M, N, MU, RHO, max(ns), coupled, anisotropic=aniso)):
        if k in ns:
            out[k] = np.array(x[:, :rows, :cols], dtype=np.float64)
    return out


class _Batch:
    """images, device buffers and the verdicts of one (plan shape, window, layout)"""

    def __init__(self, fdr, M, N, rows, cols, count, loose):
        import torch
        self.fdr, self.M, self.N = fdr, M, N
        self.imgs, self.psf = gpu_case(M, N, rows, cols, count)
        _, r, c = self.imgs.shape
        self.lay = (bm.loose_layout if loose else bm.tight_layout)(r, c, count)
        self.d_in = torch.from_numpy(bm.pack_inputs(self.imgs, self.lay)).cuda()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.bad, self.worst, self.calls = [], 0.0, 0

    def plan(self):
        p = self.fdr.Plan(self.M, self.N, self.fdr.MODE_FAST)
        p.set_operator_psf(self.psf)
        return p

    def _read(self, d_out, lay, what):
        import torch
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        if not bm.outside_untouched(out, lay):
            self.bad.append("%s: a store landed outside the output windows" % what)
        return bm.unpack(out, lay)

    def fresh(self, lay):
        import torch
        return torch.full((bm.out_size(lay),), SENTINEL, dtype=torch.float32, device="cuda")

    def alone(self, p, n, aniso, nonneg, area, what):
        """every image through the single-image _dev call, read from and stored to the places it has in the batch"""
        lay = self.lay
        d_one = self.fresh(lay)
        for i in range(lay.count):
            p.tv_deconv_dev(self.d_in.data_ptr() + 4 * i * lay.img_pitch, lay.rows, lay.cols, lay.stride, d_one.data_ptr() + 4 * bm.out_base(lay, i),
                            lay.out_stride, MU, RHO, n, aniso, nonneg, area, stream=self.stream)
        return self._read(d_one, lay, what + " (single calls)")

    def batch(self, p, count, n, aniso, nonneg, area, coupled, what):
        lay = self.lay._replace(count=count)
        d_out = self.fresh(lay)
        p.tv_deconv_batch_dev(self.d_in.data_ptr(), lay.img_pitch, count, lay.rows, lay.cols, lay.stride, d_out.data_ptr() + 4 * lay.lead,
                              lay.out_pitch, lay.out_stride, MU, RHO, n, aniso, nonneg, area, coupled, stream=self.stream)
        self.calls += 1
        return self._read(d_out, lay, what)

    def judge(self, got, want, area, what):
        for i in range(len(got)):
            e = _err(got[i], want[i], area)
            self.worst = max(self.worst, e) if e == e and self.worst == self.worst else float("nan")
            if not e <= TV_TOL:
                self.bad.append("%s image %d: error %.3g > %.3g" % (what, i, e, TV_TOL))

    def finish(self, lst):
        print("TVC\t%s\t%dx%d window %dx%d\tworst error=%.3g\tbatch calls=%d" % (lst, self.M, self.N, self.lay.rows, self.lay.cols, self.worst, self.calls))
        assert self.worst == self.worst, "NaN or inf in an output"
        assert not self.bad, "%d failures, the first:\n%s" % (len(self.bad), "\n".join(self.bad[:12]))


# ---- 1. uncoupled: the bits of the single calls ---------------------------------------------------------------------------------
@pytest.mark.parametrize("loose", [False, True], ids=["tight", "loose"])
@pytest.mark.parametrize("M,N,rows,cols", tc.GPU_PLANS, ids=PLAN_IDS)
def test_uncoupled_groups_give_the_single_calls_bits(fdr, M, N, rows, cols, loose):
    """n = 0 .. 3 x isotropic, anisotropic x nonneg x the three norm_area values (and one n = 30), each on all 25 (count, group)
    pairs of 1, 2, 3, 5, 8 images in groups of 1, 2, 3, 4, 8"""
    b = _Batch(fdr, M, N, rows, cols, max(COUNTS), loose)
    combos = [(n, aniso, nonneg, area) for n in (0, 1, 2, 3) for aniso in (False, True) for nonneg in (False, True) for area in AREAS]
    combos.append((30, False, True, NORM_CROPPED))
    raws = {aniso: _raws(b.imgs, b.psf, M, N, (0, 1, 2, 3, 30) if not aniso else (0, 1, 2, 3), False, aniso) for aniso in (False, True)}
    with b.plan() as p:
        for n, aniso, nonneg, area in combos:
            what = "n=%d %s%s norm=%d" % (n, "aniso" if aniso else "iso", " nonneg" if nonneg else "", area)
            ones = b.alone(p, n, aniso, nonneg, area, what)
            b.judge(ones, _finish(raws[aniso][n], nonneg, area, M, N), area, what)
            for count, group in PAIRS:
                p.set_batching(1, group)
                got = b.batch(p, count, n, aniso, nonneg, area, False, "%s, %d images in groups of %d" % (what, count, group))
                if not np.array_equal(got, ones[:count]):
                    b.bad.append("%s, %d images in groups of %d: not the bits of the single calls (max diff %.3g)"
                                 % (what, count, group, float(np.nanmax(np.abs(got - ones[:count])))))
        p.set_batching(1, 1)
    b.finish("uncoupled %s" % ("loose" if loose else "tight"))


# ---- 2. coupled: vectorial TV against its model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,rows,cols", tc.GPU_PLANS, ids=PLAN_IDS)
def test_coupled_channels_against_the_model(fdr, M, N, rows, cols):
    """1, 2, 3, 4 and 8 channels on a group of their number and on a group of 8, n = 0 .. 3 (and 30 for three channels), nonneg and
    the three norm_area values in rotation, loose layout for the odd counts: within TV_TOL of the coupled float64 model, equal bits
    from two calls, one channel = the single call's bits, and far from the uncoupled result"""
    worst_all = 0.0
    k = 0
    for count in (1, 2, 3, 4, 8):
        b = _Batch(fdr, M, N, rows, cols, count, loose=bool(count & 1))
        ns = (0, 1, 2, 3, 30) if count == 3 else (0, 1, 2, 3)
        raws = _raws(b.imgs, b.psf, M, N, ns, True)
        with b.plan() as p:
            for group in sorted({count, 8}):
                p.set_batching(1, group)
                for n in ns:
                    nonneg, area = bool(k & 1), AREAS[k % 3]
                    k += 1
                    what = "coupled %d channels on a group of %d, n=%d%s norm=%d" % (count, group, n, " nonneg" if nonneg else "", area)
                    got = b.batch(p, count, n, False, nonneg, area, True, what)
                    b.judge(got, _finish(raws[n], nonneg, area, M, N), area, what)
                    if not np.array_equal(got, b.batch(p, count, n, False, nonneg, area, True, what + " (again)")):
                        b.bad.append("%s: two calls differ" % what)
                    if count == 1 and not np.array_equal(got, b.alone(p, n, False, nonneg, area, what)):
                        b.bad.append("%s: not the bits of the single call" % what)
                    if count > 1 and n == 3:  # no silent fall-through to the channel-wise kernel
                        unc = b.batch(p, count, n, False, nonneg, area, False, what + " (uncoupled)")
                        if not _err(unc, got, area) > 100 * TV_TOL:
                            b.bad.append("%s: the coupled result is the uncoupled one to %.3g" % (what, _err(unc, got, area)))
            p.set_batching(1, 1)
        b.finish("coupled C=%d" % count)
        worst_all = max(worst_all, b.worst)
    print("TVC\tcoupled worst\t%dx%d\t%.3g" % (M, N, worst_all))


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_plan_usable(fdr):
    import torch
    L = fdr.lib
    M, N, rows, cols, count = 32, 64, 31, 61, 3
    imgs, psf = gpu_case(M, N, rows, cols, count)
    px = rows * cols
    d_in = torch.from_numpy(imgs.reshape(-1)).cuda()
    d_out = torch.zeros(count * M * N, dtype=torch.float32, device="cuda")
    vp = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)

    def prm(mu=MU, rho=RHO, n=2, aniso=0, nonneg=0, area=NORM_NONE, coupling=0):
        return ctypes.byref(fdr.TvBatchParams(mu, rho, n, aniso, nonneg, area, coupling))

    def tv(p, src=None, dst=None, pr=None, cnt=count, stride=cols, ostride=cols, r=rows, c=cols, opitch=px):
        return L.fdr_tv_deconv_batch_f32_dev(p._h, vp(d_in) if src is None else src, px, cnt, r, c, stride, vp(d_out) if dst is None else dst, opitch,
                                             ostride, prm() if pr is None else pr, None)

    want = tc.tvcolor_model(imgs, psf, M, N, MU, RHO, 2, False)
    want_c = tc.tvcolor_model(imgs, psf, M, N, MU, RHO, 2, True)

    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        assert tv(p) == -4 and b"operator PSF" in L.fdr_last_error()  # FDR_ERR_STATE: no operator PSF yet
        p.set_operator_psf(psf)
        single = p.tv_deconv(imgs[1], MU, RHO, 2)

        def works():
            d_out.zero_()
            assert tv(p) == 0
            torch.cuda.synchronize()
            assert rel_err(d_out.cpu().numpy()[:count * px].reshape(count, rows, cols), want) <= TV_TOL
            assert np.array_equal(p.tv_deconv(imgs[1], MU, RHO, 2), single), "the single call changed"

        p.set_batching(1, 2)
        for bad in (lambda: tv(p, cnt=-1),                                                             # negative count
                    lambda: tv(p, src=ctypes.c_void_p(0)), lambda: tv(p, dst=ctypes.c_void_p(0)),      # null pointers
                    lambda: L.fdr_tv_deconv_batch_f32_dev(p._h, vp(d_in), px, count, rows, cols, cols, vp(d_out), px, cols, None, None),
                    lambda: tv(p, r=M + 1), lambda: tv(p, r=0), lambda: tv(p, stride=cols - 1), lambda: tv(p, ostride=cols - 1),  # the single call's
                    lambda: tv(p, pr=prm(mu=0.0)), lambda: tv(p, pr=prm(mu=float("nan"))), lambda: tv(p, pr=prm(rho=-1.0)),
                    lambda: tv(p, pr=prm(rho=float("inf"))), lambda: tv(p, pr=prm(n=-1)), lambda: tv(p, pr=prm(area=7)),
                    lambda: tv(p, pr=prm(coupling=2)), lambda: tv(p, pr=prm(coupling=-1)),             # unknown coupling
                    lambda: tv(p, pr=prm(coupling=1, aniso=1)),                                        # coupled is isotropic
                    lambda: tv(p, pr=prm(coupling=1))):                                                # 3 channels on a group of 2
            assert bad() == -1, L.fdr_last_error()
            works()  # every refusal leaves the plan as it was
        assert tv(p, pr=prm(coupling=1)) == -1 and b"group" in L.fdr_last_error()
        # overlap over the whole span of the batch: the output of image 0 on the input of image 2, and in front of the inputs
        assert tv(p, dst=vp(d_in, 2 * px + 5)) == -1 and b"overlap" in L.fdr_last_error()
        works()
        assert tv(p, dst=vp(d_in, -2 * px - 7)) == -1 and b"overlap" in L.fdr_last_error()
        works()
        assert tv(p, dst=vp(d_in)) == -1  # in place, which the single call allows
        works()
        assert tv(p, cnt=0, src=ctypes.c_void_p(0)) == 0  # nothing to do
        works()
        p.set_batching(1, 3)  # and with room for the channels the coupled call runs
        d_out.zero_()
        assert tv(p, pr=prm(coupling=1)) == 0
        torch.cuda.synchronize()
        assert rel_err(d_out.cpu().numpy()[:count * px].reshape(count, rows, cols), want_c) <= TV_TOL
        p.set_batching(1, 2)
        works()
        with pytest.raises(fdr.FdrError):
            p.tv_deconv_batch(imgs, -1.0)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_FULL_SPECTRUM) as q:  # not the operator's path
        assert tv(q) == -1
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as q:
        assert tv(q) == -4


# ---- 4. the workspace grows and the single call keeps its bits --------------------------------------------------------------------
def test_workspace_growth_keeps_the_single_calls_bits(fdr):
    M, N, rows, cols = 64, 256, 63, 253
    imgs, psf = gpu_case(M, N, rows, cols, 5)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        single = [p.tv_deconv(x, MU, RHO, 3, False, True, NORM_PADDED) for x in imgs]
        other = p.tv_deconv(imgs[0], 50.0, 2.0, 2, True)
        for group in (1, 3, 1):
            p.set_batching(1, group)
            assert np.array_equal(p.tv_deconv_batch(imgs, MU, RHO, 3, False, True, NORM_PADDED), np.stack(single)), group
            assert np.array_equal(p.tv_deconv(imgs[2], MU, RHO, 3, False, True, NORM_PADDED), single[2]), group
            assert np.array_equal(p.tv_deconv(imgs[0], 50.0, 2.0, 2, True), other), group  # another mu, rho: the table again
        p.set_batching(1, 8)
        c1 = p.tv_deconv_batch(imgs, MU, RHO, 3, coupled=True)
        assert np.array_equal(p.tv_deconv(imgs[2], MU, RHO, 3, False, True, NORM_PADDED), single[2])
        assert np.array_equal(p.tv_deconv_batch(imgs, MU, RHO, 3, coupled=True), c1)


# ---- 5. the pass names ------------------------------------------------------------------------------------------------------------
def test_pass_names_of_a_coupled_call(fdr):
    """a fresh plan, one coupled, clamped, normalised call on three channels, 4 iterations: one spatial, one forward-row, one
    solve-column and one x-row launch per iteration for the group, within FDR_MAX_PASSES names"""
    M, N = 64, 256
    imgs, psf = gpu_case(M, N, 50, 200, 3)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.profile(True)
        p.set_operator_psf(psf)
        p.set_batching(1, 3)
        p.tv_deconv_batch(imgs, MU, RHO, 4, False, True, NORM_PADDED, coupled=True)
        names = {n: c for n, _, c in p.pass_times()}
    print("TVC\tpasses\t%s" % names)
    assert len(names) <= fdr.MAX_PASSES == 16
    want = {"TV table: 1/(mu|H|^2+rho L)/MN": 1, "TV init: x = pad(d), w = 0": 1, "TV spatial: joint shrink+dual+div": 4,
            "A op rows: pad+FFT (blur / RL), group": 5, "B' op cols: FFT*conj(H)*IFFT": 1, "C op rows: IFFT+crop (blur)": 1,
            "B' op cols: FFT*T*IFFT (TV solve)": 4, "C op rows: IFFT (TV x)": 4, "TV out: crop+clamp": 1, "E TV minmax+normalize": 3}
    for n, c in want.items():
        assert names.get(n) == c, (n, names.get(n), c)
    assert "TV spatial: shrink+dual+div" not in names and "A op rows: pad+FFT (blur / RL)" not in names


# ---- 6. the wrappers --------------------------------------------------------------------------------------------------------------
def test_python_layers(fdr):
    rows, cols = 50, 100
    imgs = tc.colour_images(64, 128, rows, cols, 3, 7)
    psf = fdr.motionBlurKernel(7, 30.0)
    assert fdr._rl_plan_size(rows, cols) == (64, 128)
    ch = [x.copy() for x in imgs]
    fdr.tvDeblur_RGB(ch, psf, 50.0, iterations=3, nonneg=True, coupled=True)
    want = tc.tvcolor_model(imgs, psf, 64, 128, 50.0, 2.0, 3, True, nonneg=True)
    e = rel_err(np.stack(ch), want)
    print("TVC\ttvDeblur_RGB coupled\t50x100 in 64x128\terr=%.3g" % e)
    assert e <= TV_TOL
    ch = [x.copy() for x in imgs]
    fdr.tvDeblur_RGB(ch, psf, 50.0, iterations=3, nonneg=True)  # uncoupled: the bits of the one-channel call
    assert all(np.array_equal(c, fdr.tvDeblur_myfft(x, psf, 50.0, iterations=3, nonneg=True)) for c, x in zip(ch, imgs))
    with fdr.Plan(64, 128, fdr.MODE_FAST) as p:  # the host form is the _dev form
        import torch
        p.set_operator_psf(psf)
        p.set_batching(1, 3)
        host = p.tv_deconv_batch(imgs, 50.0, 2.0, 3, coupled=True)
        d_in = torch.from_numpy(imgs).cuda()
        d_out = torch.zeros_like(d_in)
        p.tv_deconv_batch_dev(d_in.data_ptr(), rows * cols, 3, rows, cols, cols, d_out.data_ptr(), rows * cols, cols, 50.0, 2.0, 3, coupled=True)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), host)


def test_cli_tv_color(fdr, tmp_path):
    """tools/cli/gpu --tv mu --tv-color: the planes (--raw-out) are Plan.tv_deconv_batch(coupled=True, nonneg, NORM_PADDED) on the
    B, G, R planes of the picture, bit for bit; --tv-color without --tv is refused"""
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(root, "tools", "cli", "gpu")
    png = os.path.join(root, "tests", "golden", "car_blurred.png")
    out_png, out_raw = str(tmp_path / "tvc.png"), str(tmp_path / "tvc.f32")
    r = subprocess.run([gpu, png, "40", "45", "--tv", "200", "--tv-iters", "10", "--tv-rho", "5", "--tv-color", "--out", out_png, "--raw-out", out_raw],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Deblurring 3 channels took(gpu[total-variation mu 200 rho 5 n 10 colour]): " in r.stdout, r.stdout
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    planes = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
    M, N = fdr._rl_plan_size(h, w)
    bgr = np.stack([np.ascontiguousarray(rgb[:, :, c]) for c in (2, 1, 0)])
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(fdr.motionBlurKernel(40, 45.0))
        p.set_batching(1, 3)
        want = p.tv_deconv_batch(bgr, 200.0, 5.0, 10, False, True, fdr.NORM_PADDED, coupled=True)
        unc = p.tv_deconv_batch(bgr, 200.0, 5.0, 10, False, True, fdr.NORM_PADDED)
    assert np.array_equal(planes, want), float(np.abs(planes - want).max())
    assert not np.array_equal(planes, unc)
    r = subprocess.run([gpu, png, "40", "45", "--tv-color"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "Usage" in r.stdout, (r.returncode, r.stdout[-300:])
