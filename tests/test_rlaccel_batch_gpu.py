"""Batched accelerated Richardson-Lucy on the MI355X (fdr_richardson_lucy_batch_accel_f32*): 5 images in groups of 2, 3, 4, 8 and 1
for 0, 1, 2, 3, 4 and 7 iterations with the three normalisations, in both forms, on the scenes of tests/_rlaccel_batch_model.py (the
tile of the acceleration kernels is 1024 columns x 8 rows: two column tiles with a 3-column tail and the scalar path, one tile with the
16-byte path, a plan where a single image takes the split row kernels and a group the packed ones; the free form, whose sums run over
the whole plan, with NULL weights, a mask with zeros and the M x N output).

Every image and every alpha of every batch must equal, bit for bit (np.array_equal), what the single-image accelerated _dev call
gives on the same plan, reading from and writing to the image's place in the batch and in the alphas; the output lies within RLA_TOL /
RLA_FREE_TOL of the float64 model and the alphas within RLA_ALPHA_TOL (the tolerances of test_rlaccel_gpu.py); NaN and inf fail; the
sentinel survives in the stride padding, the pitch gaps, the slack and the alphas' pitch gaps; iterations <= 2 give the bytes of
richardson_lucy_batch_dev.  Then the refusals, the neighbours on the plan, the launch census, the host form with the Python layers
and the command line.  test_rlaccel_batch_host.py proves the coverage of the case list and that the judge flags the fault models of
a batched accelerated call.  Each scene prints an `RLAB` line with its largest errors (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _batch_model as bm
import _rl_batch_model as rb
import _rlaccel_batch_model as ab
from _batch_model import SENTINEL
from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf
from _rlaccel_model import RLA_ALPHA_TOL, RLA_FREE_TOL, RLA_TOL
from _rlfree_model import SIGMA

pytestmark = pytest.mark.gpu

TOL = {"plain": RLA_TOL, "free": RLA_FREE_TOL}


@pytest.fixture(autouse=True)
def _needs_the_feature(fdr):
    assert "fdr_richardson_lucy_batch_accel_f32_dev" in fdr.EXPORTED_SYMBOLS, "the library has no batched accelerated Richardson-Lucy"


class _Scene:
    """images, device buffers and the float64 model of one scene, shared by its calls"""

    def __init__(self, fdr, sc):
        import torch
        self.fdr, self.sc = fdr, sc
        self.psf = ab.scene_psf(fdr.motionBlurKernel(15, 30.0), sc)
        self.lay, self.olay = ab.scene_layouts(sc)
        self.imgs = ab.scene_images(sc)
        self.mask = ab.scene_mask(sc)
        self.d_in = torch.from_numpy(bm.pack_inputs(self.imgs, self.lay)).cuda()
        self.d_w, self.wstride = None, 0
        if sc.masked:
            self.wstride = sc.cols + 5
            w = np.full((sc.rows, self.wstride), 7.0, dtype=np.float32)  # the padding must not be read
            w[:, :sc.cols] = self.mask
            self.d_w = torch.from_numpy(w).cuda()
        self.stream = torch.cuda.current_stream().cuda_stream
        # the model: one run per image to the largest count, every smaller count on the way
        runs = [ab.single_path(sc.form, d, self.psf, sc.M, sc.N, ab.ITERATIONS, self.mask) for d in self.imgs]
        self.paths, self.ref_alphas = [r[0] for r in runs], [r[1] for r in runs]
        self.bad, self.worst, self.worst_alpha, self.calls = [], 0.0, 0.0, 0

    def plan(self):
        p = self.fdr.Plan(self.sc.M, self.sc.N, self.fdr.MODE_FAST)
        p.set_operator_psf(self.psf)
        return p

    def refs(self, n, area):
        return np.stack([ab.output_of(path[n], self.olay, area, self.sc.M, self.sc.N) for path in self.paths])

    def fresh(self, n):
        import torch
        al = ab.alpha_layout(n, self.lay.count, self.sc.loose)
        return (torch.full((bm.out_size(self.olay),), SENTINEL, dtype=torch.float32, device="cuda"),
                torch.full((ab.alpha_size(al),), SENTINEL, dtype=torch.float32, device="cuda"), al)

    def _kw(self):
        sc, free = self.sc, self.sc.form == "free"
        return dict(d_weights=self.d_w.data_ptr() if self.d_w is not None else None, wstride=self.wstride), free

    def alone(self, p, n, area):
        """every image through the single accelerated _dev call at its place in the batch: ([count, rows, cols], [count, n])"""
        import torch
        lay, olay = self.lay, self.olay
        d_out, d_al, al = self.fresh(n)
        kw, free = self._kw()
        for i in range(lay.count):
            src, dst = self.d_in.data_ptr() + 4 * i * lay.img_pitch, d_out.data_ptr() + 4 * bm.out_base(olay, i)
            dal = d_al.data_ptr() + 4 * (al.lead + i * al.pitch)
            if free:
                p.richardson_lucy_free_dev(src, lay.rows, lay.cols, lay.stride, dst, olay.out_stride, n, norm_area=area, out_rows=olay.rows,
                                           out_cols=olay.cols, stream=self.stream, accelerate=True, d_alphas=dal, **kw)
            else:
                p.richardson_lucy_dev(src, lay.rows, lay.cols, lay.stride, dst, olay.out_stride, n, area, stream=self.stream, accelerate=True,
                                      d_alphas=dal)
        torch.cuda.synchronize()
        one, one_al = d_out.cpu().numpy(), d_al.cpu().numpy()
        if not bm.outside_untouched(one, olay) or not ab.alphas_outside_untouched(one_al, al):
            self.bad.append("%s n=%d: the single-image call wrote outside its window or its alphas" % (self.sc.name, n))
        return bm.unpack(one, olay), ab.unpack_alphas(one_al, al)

    def batch(self, p, n, area, accelerate=True, count=None):
        """one batched call into sentinel-filled buffers: (flat output, flat alphas, alpha layout)"""
        import torch
        cnt = self.lay.count if count is None else count
        lay, olay = self.lay, self.olay
        d_out, d_al, al = self.fresh(n)
        kw, free = self._kw()
        if accelerate:
            kw.update(accelerate=True, d_alphas=d_al.data_ptr() + 4 * al.lead, alpha_pitch=al.pitch)
        p.richardson_lucy_batch_dev(self.d_in.data_ptr(), lay.img_pitch, cnt, lay.rows, lay.cols, lay.stride, d_out.data_ptr() + 4 * olay.lead,
                                    olay.out_pitch, olay.out_stride, n, area, free_boundary=free, out_rows=olay.rows if free else None,
                                    out_cols=olay.cols if free else None, stream=self.stream, **kw)
        torch.cuda.synchronize()
        self.calls += 1
        return d_out.cpu().numpy(), d_al.cpu().numpy(), al

    def run(self, p):
        sc = self.sc
        for n in ab.ITERATIONS:
            for area in ab.AREAS:
                ones, one_al = self.alone(p, n, area)
                refs = self.refs(n, area)
                for group in ab.GROUPS:
                    p.set_batching(1, group)
                    what = "%s n=%d %s groups of %d" % (sc.name, n, ab.AREA_NAME[area], group)
                    out, alphas, al = self.batch(p, n, area)
                    v = ab.judge(what, out, self.olay, alphas, al, ones, one_al, refs, self.ref_alphas, TOL[sc.form], RLA_ALPHA_TOL, area)
                    self.bad += v.bad
                    self.worst, self.worst_alpha = max(self.worst, v.worst), max(self.worst_alpha, v.worst_alpha)
                    if n <= 2:  # alpha_0 = alpha_1 = 0: the plain batch's bytes, and nothing but zeros in the alphas
                        plain = self.batch(p, n, area, accelerate=False)[0]
                        if not np.array_equal(out, plain):
                            self.bad.append("%s: differs from richardson_lucy_batch_dev" % what)
                        if np.any(ab.unpack_alphas(alphas, al) != 0):
                            self.bad.append("%s: alpha_0 or alpha_1 is not 0" % what)
                p.set_batching(1, 1)

    def finish(self):
        print("RLAB\t%s\tworst error=%.3g\tworst alpha error=%.3g\tbatch calls=%d" % (self.sc.name, self.worst, self.worst_alpha, self.calls))
        assert self.worst == self.worst and self.worst_alpha == self.worst_alpha, "NaN in an error"
        assert not self.bad, "%d failures, the first:\n%s" % (len(self.bad), "\n".join(self.bad[:12]))


# ---- 1. every scene: groups and tails x iterations x normalisations ---------------------------------------------------------
@pytest.mark.parametrize("sc", ab.SCENES, ids=ab.SCENE_IDS)
def test_groups_iterations_normalisations(fdr, sc):
    s = _Scene(fdr, sc)
    with s.plan() as p:
        s.run(p)
    s.finish()


def test_batch_of_fewer_images_than_the_group_and_null_alphas(fdr):
    """one and three images on groups of 4; a call without alphas gives the same bytes"""
    for sc in (ab.SCENES[1], ab.SCENES[7]):
        s = _Scene(fdr, sc)
        with s.plan() as p:
            ones, one_al = s.alone(p, 4, NORM_CROPPED)
            p.set_batching(1, 4)
            for cnt in (1, 3):
                out, alphas, al = s.batch(p, 4, NORM_CROPPED, count=cnt)
                got, got_al = bm.unpack(out, s.olay), ab.unpack_alphas(alphas, al)
                assert np.array_equal(got[:cnt], ones[:cnt]) and np.array_equal(got_al[:cnt], one_al[:cnt]), (sc.name, cnt)
                assert np.all(got[cnt:] == SENTINEL) and np.all(got_al[cnt:] == SENTINEL), (sc.name, cnt)
            out, alphas, al = s.batch(p, 4, NORM_CROPPED)
            import torch
            lay, olay = s.lay, s.olay
            d_out = s.fresh(4)[0]
            kw, free = s._kw()
            p.richardson_lucy_batch_dev(s.d_in.data_ptr(), lay.img_pitch, lay.count, lay.rows, lay.cols, lay.stride, d_out.data_ptr() + 4 * olay.lead,
                                        olay.out_pitch, olay.out_stride, 4, NORM_CROPPED, free_boundary=free, out_rows=olay.rows if free else None,
                                        out_cols=olay.cols if free else None, stream=s.stream, accelerate=True, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), out), sc.name


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_plan_usable(fdr):
    import torch
    L = fdr.lib
    M, N, rows, cols, count, n = 32, 64, 31, 61, 3, 4
    psf = centred_psf(bm.fit_psf(fdr.motionBlurKernel(15, 30.0), M, N), M, N)
    imgs = rb.images(M, N, rows, cols, count, 3)
    px = rows * cols
    d_in = torch.from_numpy(imgs.reshape(-1)).cuda()
    d_out = torch.zeros(count * M * N, dtype=torch.float32, device="cuda")
    d_w = torch.ones(px, dtype=torch.float32, device="cuda")
    d_al = torch.zeros(count * (n + 2), dtype=torch.float32, device="cuda")
    vp = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)

    def prm(it=n, area=NORM_NONE, free=0, sigma=SIGMA, orows=0, ocols=0):
        return ctypes.byref(fdr.RlBatchParams(it, area, free, sigma, orows, ocols))

    def rl(p, src=None, dst=None, w=None, ws=cols, pr=None, cnt=count, stride=cols, ostride=cols, r=rows, c=cols, opitch=px, al=0, ap=n + 2):
        return L.fdr_richardson_lucy_batch_accel_f32_dev(p._h, vp(d_in) if src is None else src, px, cnt, r, c, stride, w, ws,
                                                         vp(d_out) if dst is None else dst, opitch, ostride, prm() if pr is None else pr,
                                                         vp(d_al) if al == 0 else al, ap, None)

    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        assert rl(p) == -4  # FDR_ERR_STATE: no operator PSF yet
        p.set_operator_psf(psf)
        want, want_al = [], []
        for i in range(count):
            o, a = p.richardson_lucy(imgs[i], n, accelerate=True, return_alphas=True)
            want.append(o)
            want_al.append(a)
        p.set_batching(1, 2)

        def works():
            d_out.zero_()
            d_al.fill_(SENTINEL)
            assert rl(p) == 0, L.fdr_last_error()
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy()[:count * px].reshape(count, rows, cols), np.stack(want))
            assert np.array_equal(d_al.cpu().numpy().reshape(count, n + 2)[:, :n], np.stack(want_al))

        free = dict(free=1, orows=rows, ocols=cols)
        for bad in (lambda: rl(p, cnt=-1),                                                             # everything the plain batch refuses
                    lambda: rl(p, src=ctypes.c_void_p(0)), lambda: rl(p, dst=ctypes.c_void_p(0)),
                    lambda: L.fdr_richardson_lucy_batch_accel_f32_dev(p._h, vp(d_in), px, count, rows, cols, cols, None, 0, vp(d_out), px, cols, None,
                                                                      vp(d_al), n, None),
                    lambda: rl(p, r=M + 1), lambda: rl(p, stride=cols - 1), lambda: rl(p, ostride=cols - 1),
                    lambda: rl(p, pr=prm(it=-1)), lambda: rl(p, pr=prm(area=7)),
                    lambda: rl(p, w=vp(d_w)), lambda: rl(p, pr=prm(orows=rows + 1, ocols=cols)),
                    lambda: rl(p, pr=prm(sigma=0.0, **free)), lambda: rl(p, pr=prm(sigma=1.0, **free)),
                    lambda: rl(p, pr=prm(free=1, orows=rows - 1, ocols=cols)), lambda: rl(p, pr=prm(free=1, orows=M + 1, ocols=cols)),
                    lambda: rl(p, pr=prm(**free), w=vp(d_w), ws=cols - 1),
                    lambda: rl(p, pr=prm(free=1, orows=M, ocols=N), ostride=N - 1, opitch=M * N),
                    lambda: rl(p, dst=vp(d_in, 2 * px + 5)),                                            # outputs on the inputs
                    lambda: rl(p, ap=n - 1), lambda: rl(p, pr=prm(**free), ap=n - 1)):                   # alpha_pitch < iterations
            assert bad() == -1, L.fdr_last_error()
            works()  # every refusal leaves the plan as it was
        assert b"alpha_pitch" in (rl(p, ap=n - 1), L.fdr_last_error())[1]
        # the alphas' range over the whole batch: image 2's alphas on the outputs, image 0's on the last input, on the weights
        assert rl(p, al=vp(d_out, -2 * (n + 2) - 1)) == -1 and b"alphas overlap the outputs" in L.fdr_last_error()
        works()
        assert rl(p, al=vp(d_out, count * px - 1)) == -1 and b"alphas overlap the outputs" in L.fdr_last_error()
        works()
        assert rl(p, al=vp(d_in, count * px - 1)) == -1 and b"alphas overlap the inputs" in L.fdr_last_error()
        works()
        assert rl(p, pr=prm(**free), w=vp(d_w), al=vp(d_w, px - 1)) == -1 and b"alphas overlap the weights" in L.fdr_last_error()
        works()
        # nothing to write: no refusal for a pitch of 0 with no iterations, null alphas with any pitch, an empty batch
        assert rl(p, pr=prm(it=0), ap=0) == 0 and rl(p, al=None, ap=0) == 0 and rl(p, cnt=0, src=ctypes.c_void_p(0)) == 0
        works()
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_FULL_SPECTRUM) as q:  # not the operator's path
        assert rl(q) == -1


# ---- 3. the neighbours on the plan ------------------------------------------------------------------------------------------------
def test_other_results_survive_a_batched_accelerated_call(fdr):
    """a Wiener call and the single accelerated calls give the same bytes before a batched accelerated call (workspace for one image),
    after it (grown to groups of 2) and after it has grown again (groups of 4)"""
    M, N, rows, cols = 64, 256, 63, 253
    sc = ab.Scene("neighbours", "free", M, N, rows, cols, False, True, False)
    s = _Scene(fdr, sc)
    plain = _Scene(fdr, sc._replace(form="plain", masked=False))
    with s.plan() as p:
        p.set_psf(bm.fit_psf(fdr.motionBlurKernel(15, 30.0), M, N), bm.K32)
        img = s.imgs[1]

        def others():
            return (p.wiener(img), p.richardson_lucy(img, 5, NORM_PADDED, accelerate=True, return_alphas=True),
                    p.richardson_lucy_free(img, 4, weights=s.mask, norm_area=NORM_CROPPED, accelerate=True, return_alphas=True),
                    p.richardson_lucy(img, 3), p.wiener_batch(s.imgs))

        def same(a, b):
            return all(np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else np.array_equal(a, b)

        before = others()
        for group in (2, 4):
            p.set_batching(1, group)
            for t in (s, plain):
                ones, one_al = t.alone(p, 4, NORM_PADDED)
                out, alphas, al = t.batch(p, 4, NORM_PADDED)
                assert np.array_equal(bm.unpack(out, t.olay), ones) and np.array_equal(ab.unpack_alphas(alphas, al), one_al), (group, t.sc.form)
            p.set_batching(1, 1)
            for k, (x, y) in enumerate(zip(before, others())):
                assert same(x, y), "result %d changed after a batched accelerated call on groups of %d" % (k, group)


# ---- 4. the launch census -----------------------------------------------------------------------------------------------------------
def _census(p, call):
    import torch
    p.profile(True)
    call()
    torch.cuda.synchronize()
    got = {}
    for name, _, c in p.pass_times():
        if c:
            got[name] = got.get(name, 0) + c
    p.profile(False)
    return got


@pytest.mark.parametrize("form", ("plain", "free"))
def test_census_a_group_launches_what_one_image_launches(fdr, form):
    """5 images in groups of 2, 2, 1 at 4 iterations: per group 2 extrapolations and 3 directions, as for one image; the transform
    passes are those of the plain batch; and one image alone launches the same acceleration passes per group"""
    sc = ab.Scene("census", form, 32, 256, 29, 250, False, False, False)
    s = _Scene(fdr, sc)
    ext, dirn = "RLA extrapolate", "RLA direction + alpha"
    with s.plan() as p:
        p.set_batching(1, 2)
        accel = _census(p, lambda: s.batch(p, 4, NORM_CROPPED))
        plain = _census(p, lambda: s.batch(p, 4, NORM_CROPPED, accelerate=False))
        one = _census(p, lambda: s.batch(p, 4, NORM_CROPPED, count=1))
    assert one[ext] == 2 and one[dirn] == 3, one
    assert accel[ext] == 3 * one[ext] and accel[dirn] == 3 * one[dirn], accel  # three groups, each with the launches of one image
    assert {k: v for k, v in accel.items() if k not in (ext, dirn)} == plain and ext not in plain and dirn not in plain, (accel, plain)


# ---- 5. the host form and the Python layers ---------------------------------------------------------------------------------------
def test_host_form_and_python_layers(fdr):
    M, N, rows, cols = 64, 128, 50, 100
    psf = centred_psf(bm.fit_psf(fdr.motionBlurKernel(15, 30.0), M, N), M, N)
    imgs = rb.images(M, N, rows, cols, 3, 5)
    w = rb.mask(rows, cols, 9)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        want_p = [p.richardson_lucy(x, 5, NORM_CROPPED, accelerate=True, return_alphas=True) for x in imgs]
        want_f = [p.richardson_lucy_free(x, 4, weights=w, norm_area=NORM_PADDED, accelerate=True, return_alphas=True) for x in imgs]
        want_m = [p.richardson_lucy_free(x, 3, full_plane=True, accelerate=True) for x in imgs]
        for group in (1, 3):
            p.set_batching(1, group)
            out, al = p.richardson_lucy_batch(imgs, 5, norm_area=NORM_CROPPED, accelerate=True, return_alphas=True)
            assert np.array_equal(out, np.stack([x[0] for x in want_p])) and np.array_equal(al, np.stack([x[1] for x in want_p]))
            out, al = p.richardson_lucy_batch(imgs, 4, free_boundary=True, weights=w, norm_area=NORM_PADDED, accelerate=True, return_alphas=True)
            assert np.array_equal(out, np.stack([x[0] for x in want_f])) and np.array_equal(al, np.stack([x[1] for x in want_f]))
            assert np.array_equal(p.richardson_lucy_batch(imgs, 3, free_boundary=True, full_plane=True, accelerate=True), np.stack(want_m))
        with pytest.raises(ValueError):
            p.richardson_lucy_batch(imgs, 3, return_alphas=True)
    small = fdr.motionBlurKernel(7, 30.0)
    ch = [x.copy() for x in imgs]
    fdr.richardsonLucy_RGB(ch, small, 5, accelerate=True)
    assert all(np.array_equal(c, fdr.richardsonLucy_myfft(x, small, 5, accelerate=True)) for c, x in zip(ch, imgs))
    assert not np.array_equal(ch[0], fdr.richardsonLucy_myfft(imgs[0], small, 5))
    ch = [x.copy() for x in imgs]
    fdr.richardsonLucyFree_RGB(ch, small, 5, weights=w, accelerate=True)
    assert all(np.array_equal(c, fdr.richardsonLucyFree_myfft(x, small, 5, weights=w, accelerate=True)) for c, x in zip(ch, imgs))


# ---- 6. the command line --------------------------------------------------------------------------------------------------------
def test_cli_accel_runs_batched_with_the_loops_bytes(fdr, tmp_path):
    """tools/cli/gpu --rl 4 --accel and --rl 4 --accel --free-boundary on tests/golden/car_blurred.png: the planes (--raw-out) are the
    bytes of the per-channel loop of the Python single accelerated calls on the same padded plan"""
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(root, "tools", "cli", "gpu")
    png = os.path.join(root, "tests", "golden", "car_blurred.png")
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    psf = fdr.motionBlurKernel(40, 45.0)
    for extra, size in (([], fdr._rl_plan_size(h, w)), (["--free-boundary"], fdr._rlfree_plan_size(h, w, 40, 40))):
        out_png, out_raw = str(tmp_path / "rlab.png"), str(tmp_path / "rlab.f32")
        r = subprocess.run([gpu, png, "40", "45", "--rl", "4", "--accel"] + extra + ["--out", out_png, "--raw-out", out_raw], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert os.path.getsize(out_png) > 0
        planes = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
        with fdr.Plan(size[0], size[1], fdr.MODE_FAST) as p:
            p.set_operator_psf(psf)
            for k, c in enumerate((2, 1, 0)):  # B, G, R
                ch = np.ascontiguousarray(rgb[:, :, c])
                want = (p.richardson_lucy_free(ch, 4, norm_area=fdr.NORM_PADDED, accelerate=True) if extra
                        else p.richardson_lucy(ch, 4, fdr.NORM_PADDED, accelerate=True))
                assert np.array_equal(planes[k], want), (extra, k, float(np.abs(planes[k] - want).max()))
