"""Every entry point of include/fdr.h with a `void* stream` parameter behind the stream fence of tests/_stream_fence.py (DESIGN.md
section 39): on a non-blocking side stream whose inputs arrive on that stream, behind a delay, and whose outputs are read on it.

CASES is the table: one Case per fenced sequence, with the C entry points it covers, the Python wrappers it goes through, the plan it
runs on and -- where fdr.h lets the entry wait for its stream -- the sentence of fdr.h that says so.  Two verdicts per case:

  ordered         the results (every output buffer byte for byte, host values as numbers) equal those of the quiet run of the same
                  sequence; judged for every case
  does not wait   the delay was still running when the call returned; judged for every case without an `exempt` sentence

test_stream_order_host.py holds the table against fdr.h: every entry with a stream parameter has a case, every exemption is a quote.
The shapes are the smallest the family tests use to reach each path.  Every case prints a `STREAM` line (pytest -s)."""
import collections
import ctypes
import functools
import types

import numpy as np
import pytest

import _stream_fence as sf
from _rl_model import centred_psf, dense_psf, smooth_image

pytestmark = pytest.mark.gpu

M, N = 64, 128                       # the operator plan (FDR_MODE_FAST)
ROWS, COLS, STRIDE, OSTRIDE = 37, 101, 103, 101
ITER = 3
TAIL = 64                            # elements behind every output, which keep the sentinel
COUNT, PITCH, OPITCH = 5, ROWS * STRIDE + 6, ROWS * OSTRIDE + 4   # the batch forms: 5 images, odd pitches
OP_PLAN = (M, N, "MODE_FAST", ())

Case = collections.namedtuple("Case", "id entries wrappers plan build exempt batching options")


def case(id, entries, wrappers, plan, build, exempt=None, batching=None, options=()):
    return Case(id, tuple(entries), tuple(wrappers), plan, build, exempt, batching, tuple(options))


# the sentences of include/fdr.h that let an entry wait for its stream (whitespace and the comment's line starts aside)
Q_RL_RULE = "With a rule it is synchronous, as fdr_choose_reg_f32_dev is"
Q_TV_AUTO = "with sigma = 0 it waits for `stream` once, before the first iteration, to read the noise sum back"
Q_TV_AUTO_BATCH = "an entry of 0 is estimated from that image as the single call does (one wait on the stream before its group's first iteration)"
Q_MOTION = "The _dev form is SYNCHRONOUS: it reads the table back, so it returns after its work on `stream` is done."
Q_DEFOCUS = "into profile when it is not NULL. The _dev form is SYNCHRONOUS."
Q_BLUR = "The _dev form is SYNCHRONOUS as well: it returns both estimates to the host."
Q_REG = ("Every _dev form takes the picture from device memory and is SYNCHRONOUS: it reads its results back, so it returns after its "
         "work on `stream` is done.")


# ---- data (numpy only: the table is imported on machines without a GPU) ----------------------------------------------------------
def window(a, stride):
    """the rows x cols array a as rows x stride floats with NaN in the padding, flat"""
    a = np.asarray(a, dtype=np.float32)
    h = np.full((a.shape[0], stride), np.nan, dtype=np.float32)
    h[:, :a.shape[1]] = a
    return h.reshape(-1)


def pitched(windows, stride, pitch):
    """several windows, `pitch` floats apart, NaN everywhere else"""
    h = np.full(len(windows) * pitch, np.nan, dtype=np.float32)
    for k, a in enumerate(windows):
        w = window(a, stride)
        h[k * pitch:k * pitch + w.size] = w
    return h


@functools.lru_cache(maxsize=None)
def picture(k=0, rows=ROWS, cols=COLS):
    return (smooth_image(rows, cols, 11 + k) * (1.0 + 0.1 * k)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def weights(rows=ROWS, cols=COLS):
    w = np.ones((rows, cols), dtype=np.float32)
    w[3:6, 10:20] = 0.0
    w[rows // 2, :] = 0.5
    return w


def noise(n, seed):
    return np.random.default_rng(seed).random(n, dtype=np.float32)


def noise_picture(k, rows, cols):
    return noise(rows * cols, 20 + k).reshape(rows, cols)


@functools.lru_cache(maxsize=None)
def motion_plane(fdr):
    """the centred motion PSF 15 / 30 as an M x N plane"""
    return centred_psf(fdr.motionBlurKernel(15, 30.0), M, N).reshape(-1)


class Bufs:
    """the device buffers of one case, in the roles the fence knows"""

    def __init__(self):
        self.inputs, self.outputs = [], []

    def inp(self, a):
        import torch
        s = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).cuda()
        b = torch.empty_like(s)
        self.inputs.append((b, s))
        return b

    def out(self, n, dtype=None):
        import torch
        o = torch.empty(n + TAIL, dtype=dtype or torch.float32, device="cuda")
        self.outputs.append(o)
        return o

    def inout(self, a):
        """read and written by the call -- or written only, by an entry without inputs: the copy over the poison then undoes a
        store that came too early"""
        b = self.inp(a)
        self.outputs.append(b)
        return b


def _ptr(t):
    return ctypes.c_void_p(int(t.data_ptr())) if t is not None else None


def _st(st):
    return ctypes.c_void_p(int(st))


def _dp(t):
    return t.data_ptr() if t is not None else None


# ---- the operator families: plan 64 x 128, window 37 x 101, the PSF set inside the fenced sequence -------------------------------
def operator(make, with_weights=False, out_elems=ROWS * OSTRIDE):
    def build(fdr, p, b):
        psf = b.inp(motion_plane(fdr))
        d = types.SimpleNamespace(img=b.inp(window(picture(), STRIDE)).data_ptr(),
                                  w=b.inp(window(weights(), STRIDE)).data_ptr() if with_weights else None,
                                  ws=STRIDE if with_weights else 0, out=b.out(out_elems).data_ptr())
        go = make(fdr, p, b, d)

        def call(st):
            p.set_operator_psf_dev(psf.data_ptr(), M, N, N, stream=st)
            return go(st)
        return call
    return build


def batch_operator(make, with_weights=False, count=COUNT):
    def build(fdr, p, b):
        psf = b.inp(motion_plane(fdr))
        d = types.SimpleNamespace(imgs=b.inp(pitched([picture(k) for k in range(count)], STRIDE, PITCH)).data_ptr(), count=count,
                                  w=b.inp(window(weights(), STRIDE)).data_ptr() if with_weights else None,
                                  ws=STRIDE if with_weights else 0, out=b.out(count * OPITCH).data_ptr())
        go = make(fdr, p, b, d)

        def call(st):
            p.set_operator_psf_dev(psf.data_ptr(), M, N, N, stream=st)
            return go(st)
        return call
    return build


CASES = []


def op(id, entry, wrapper, make, with_weights=False, exempt=None):
    CASES.append(case(id, ("fdr_set_operator_psf_dev", entry), ("Plan.set_operator_psf_dev", wrapper), OP_PLAN,
                      operator(make, with_weights), exempt))


def op_w(id, entry, wrapper, make, exempt=None):
    """the entry takes weights: with and without them"""
    op(id, entry, wrapper, make, False, exempt)
    op(id + "-weights", entry, wrapper, make, True, exempt)


def bop(id, entry, wrapper, make, with_weights=False, exempt=None, count=COUNT, group=2):
    CASES.append(case(id, ("fdr_set_operator_psf_dev", entry), ("Plan.set_operator_psf_dev", wrapper), OP_PLAN,
                      batch_operator(make, with_weights, count), exempt, batching=(1, group)))


def bop_w(id, entry, wrapper, make, exempt=None, count=COUNT, group=2):
    bop(id, entry, wrapper, make, False, exempt, count, group)
    bop(id + "-weights", entry, wrapper, make, True, exempt, count, group)


W = (ROWS, COLS, STRIDE)  # the window arguments of the single calls

op("blur", "fdr_blur_f32_dev", "Plan.blur_dev", lambda fdr, p, b, d: lambda st: p.blur_dev(d.img, *W, d.out, OSTRIDE, stream=st))
op("blur-adjoint", "fdr_blur_f32_dev", "Plan.blur_dev",
   lambda fdr, p, b, d: lambda st: p.blur_dev(d.img, *W, d.out, OSTRIDE, adjoint=True, stream=st))
op("rl", "fdr_richardson_lucy_f32_dev", "Plan.richardson_lucy_dev",
   lambda fdr, p, b, d: lambda st: p.richardson_lucy_dev(d.img, *W, d.out, OSTRIDE, ITER, stream=st))
op("rl-normalised", "fdr_richardson_lucy_f32_dev", "Plan.richardson_lucy_dev",
   lambda fdr, p, b, d: lambda st: p.richardson_lucy_dev(d.img, *W, d.out, OSTRIDE, ITER, norm_area=fdr.NORM_CROPPED, stream=st))
op_w("rl-free", "fdr_richardson_lucy_free_f32_dev", "Plan.richardson_lucy_free_dev",
     lambda fdr, p, b, d: lambda st: p.richardson_lucy_free_dev(d.img, *W, d.out, OSTRIDE, ITER, d.w, d.ws, stream=st))


def _accel(fdr, p, b, d):
    al = b.out(ITER)
    return lambda st: p.richardson_lucy_dev(d.img, *W, d.out, OSTRIDE, ITER, stream=st, accelerate=True, d_alphas=al.data_ptr())


def _free_accel(fdr, p, b, d):
    al = b.out(ITER)
    return lambda st: p.richardson_lucy_free_dev(d.img, *W, d.out, OSTRIDE, ITER, d.w, d.ws, stream=st, accelerate=True, d_alphas=al.data_ptr())


op("rl-accel", "fdr_richardson_lucy_accel_f32_dev", "Plan.richardson_lucy_dev", _accel)
op_w("rl-free-accel", "fdr_richardson_lucy_free_accel_f32_dev", "Plan.richardson_lucy_free_dev", _free_accel)


def _rl_auto(rule, free, accelerate=False, sigma=0.0):
    def make(fdr, p, b, d):
        tr = b.out(2 * ITER, dtype=_f64())
        return lambda st: tuple(p.richardson_lucy_auto_dev(d.img, *W, d.out, OSTRIDE, ITER, rule=rule, sigma=sigma, free_boundary=free,
                                                           accelerate=accelerate, d_weights=d.w, wstride=d.ws, d_trace=tr.data_ptr(), stream=st))
    return make


def _f64():
    import torch
    return torch.float64


op("rl-auto-none", "fdr_richardson_lucy_auto_f32_dev", "Plan.richardson_lucy_auto_dev", _rl_auto(0, False))
op("rl-auto-none-accel", "fdr_richardson_lucy_auto_f32_dev", "Plan.richardson_lucy_auto_dev", _rl_auto(0, False, True))
op_w("rl-auto-none-free", "fdr_richardson_lucy_auto_f32_dev", "Plan.richardson_lucy_auto_dev", _rl_auto(0, True))
op("rl-auto-residual", "fdr_richardson_lucy_auto_f32_dev", "Plan.richardson_lucy_auto_dev", _rl_auto(1, False, sigma=0.05), exempt=Q_RL_RULE)
op("rl-auto-residual-estimated", "fdr_richardson_lucy_auto_f32_dev", "Plan.richardson_lucy_auto_dev", _rl_auto(1, True), True, exempt=Q_RL_RULE)


def _rltv(free):
    return lambda fdr, p, b, d: lambda st: p.richardson_lucy_tv_dev(d.img, *W, d.out, OSTRIDE, ITER, 0.01, free_boundary=free, d_weights=d.w,
                                                                    wstride=d.ws, stream=st)


op("rl-tv", "fdr_richardson_lucy_tv_f32_dev", "Plan.richardson_lucy_tv_dev", _rltv(False))
op_w("rl-tv-free", "fdr_richardson_lucy_tv_f32_dev", "Plan.richardson_lucy_tv_dev", _rltv(True))


def _blind(free, with_weights):
    def build(fdr, p, b):
        img = b.inp(window(picture(), STRIDE))
        w = b.inp(window(weights(), STRIDE)) if with_weights else None
        psf = b.inout(window(fdr.psf_gaussian(9), 10))
        out = b.out(ROWS * OSTRIDE)
        return lambda st: p.richardson_lucy_blind_dev(img.data_ptr(), *W, psf.data_ptr(), 9, 9, 10, out.data_ptr(), OSTRIDE, ITER, free_boundary=free,
                                                      d_weights=_dp(w), wstride=STRIDE if with_weights else 0, stream=st)
    return build


for _id, _free, _w in (("blind", False, False), ("blind-free", True, False), ("blind-free-weights", True, True)):
    CASES.append(case(_id, ("fdr_richardson_lucy_blind_f32_dev",), ("Plan.richardson_lucy_blind_dev",), OP_PLAN, _blind(_free, _w)))


# multi-frame: K = 3 PSFs in frame tables of their own, set inside the sequence
K_FRAMES, FP = 3, (5, 7, 8, 5 * 8 + 3)   # prows, pcols, pstride, pitch


def _frames(make, with_weights=False, out_elems=ROWS * OSTRIDE):
    def build(fdr, p, b):
        h = np.full(K_FRAMES * FP[3], np.nan, dtype=np.float32)
        for k in range(K_FRAMES):
            h[k * FP[3]:k * FP[3] + FP[0] * FP[2]] = window(dense_psf(70 + k, 7)[:FP[0], :FP[1]], FP[2])
        psfs = b.inp(h)
        d = types.SimpleNamespace(imgs=b.inp(pitched([picture(k) for k in range(K_FRAMES)], STRIDE, PITCH)).data_ptr(),
                                  w=b.inp(window(weights(), STRIDE)).data_ptr() if with_weights else None,
                                  ws=STRIDE if with_weights else 0, out=b.out(out_elems).data_ptr())
        go = make(fdr, p, b, d)

        def call(st):
            p.set_frame_psfs_dev(psfs.data_ptr(), FP[3], K_FRAMES, FP[0], FP[1], FP[2], stream=st)
            return go(st)
        return call
    return build


def frames(id, entry, wrapper, make, with_weights=False, out_elems=ROWS * OSTRIDE):
    CASES.append(case(id, ("fdr_set_frame_psfs_dev", entry), ("Plan.set_frame_psfs_dev", wrapper), OP_PLAN, _frames(make, with_weights, out_elems)))


def _rl_frames(lam):
    return lambda fdr, p, b, d: lambda st: p.richardson_lucy_frames_dev(d.imgs, PITCH, K_FRAMES, *W, d.out, OSTRIDE, ITER, d_weights=d.w,
                                                                        weight_pitch=0, wstride=d.ws, tv_lambda=lam, stream=st)


frames("frames-blur", "fdr_blur_frames_f32_dev", "Plan.blur_frames_dev",
       lambda fdr, p, b, d: lambda st: p.blur_frames_dev(d.imgs, 0, *W, d.out, OPITCH, OSTRIDE, K_FRAMES, stream=st), out_elems=K_FRAMES * OPITCH)
frames("frames-blur-adjoint", "fdr_blur_frames_f32_dev", "Plan.blur_frames_dev",
       lambda fdr, p, b, d: lambda st: p.blur_frames_dev(d.imgs, PITCH, *W, d.out, 0, OSTRIDE, K_FRAMES, adjoint=True, stream=st))
frames("frames-rl", "fdr_richardson_lucy_frames_f32_dev", "Plan.richardson_lucy_frames_dev", _rl_frames(0.0))
frames("frames-rl-weights", "fdr_richardson_lucy_frames_f32_dev", "Plan.richardson_lucy_frames_dev", _rl_frames(0.0), True)
frames("frames-rl-tv", "fdr_richardson_lucy_frames_f32_dev", "Plan.richardson_lucy_frames_dev", _rl_frames(0.01))


# TV by ADMM
op("tv", "fdr_tv_deconv_f32_dev", "Plan.tv_deconv_dev",
   lambda fdr, p, b, d: lambda st: p.tv_deconv_dev(d.img, *W, d.out, OSTRIDE, 200.0, 2.0, ITER, stream=st))
op("tv-nonneg-normalised", "fdr_tv_deconv_f32_dev", "Plan.tv_deconv_dev",
   lambda fdr, p, b, d: lambda st: p.tv_deconv_dev(d.img, *W, d.out, OSTRIDE, 200.0, 2.0, ITER, nonneg=True, norm_area=fdr.NORM_CROPPED, stream=st))
op_w("tv-free", "fdr_tv_deconv_free_f32_dev", "Plan.tv_deconv_free_dev",
     lambda fdr, p, b, d: lambda st: p.tv_deconv_free_dev(d.img, *W, d.out, OSTRIDE, 200.0, 2.0, ITER, d.w, d.ws, stream=st))
op_w("tv-poisson", "fdr_tv_deconv_poisson_f32_dev", "Plan.tv_deconv_poisson_dev",
     lambda fdr, p, b, d: lambda st: p.tv_deconv_poisson_dev(d.img, *W, d.out, OSTRIDE, 20.0, 2.0, ITER, d.w, d.ws, background=0.01, stream=st))


def _tv_auto(sigma):
    def make(fdr, p, b, d):
        tr = b.out(3 * ITER, dtype=_f64())
        return lambda st: p.tv_deconv_auto_dev(d.img, *W, d.out, OSTRIDE, sigma, 2.0, ITER, d.w, d.ws, d_trace=tr.data_ptr(), stream=st)
    return make


op_w("tv-auto", "fdr_tv_deconv_auto_f32_dev", "Plan.tv_deconv_auto_dev", _tv_auto(0.02))
op("tv-auto-estimated", "fdr_tv_deconv_auto_f32_dev", "Plan.tv_deconv_auto_dev", _tv_auto(0.0), exempt=Q_TV_AUTO)


# the Poisson data step alone: dense M x N planes c and q in place
def _poisson_step(count, with_weights):
    def build(fdr, p, b):
        c = b.inout(0.05 + noise(count * M * N, 31))
        q = b.inout(noise(count * M * N, 32) - 0.5)
        imgs = b.inp(pitched([picture(k) for k in range(count)], STRIDE, PITCH))
        w = b.inp(window(weights(), STRIDE)) if with_weights else None
        if count == 1:
            return lambda st: p.tv_poisson_step_dev(c.data_ptr(), q.data_ptr(), imgs.data_ptr(), *W, 20.0, 2.0, 0.01, _dp(w),
                                                    STRIDE if with_weights else 0, stream=st)
        return lambda st: p.tv_poisson_step_group_dev(c.data_ptr(), M * N, q.data_ptr(), M * N, imgs.data_ptr(), PITCH, count, *W, 20.0, 2.0, 0.01,
                                                      _dp(w), STRIDE if with_weights else 0, stream=st)
    return build


for _w in (False, True):
    CASES.append(case("tv-poisson-step" + ("-weights" if _w else ""), ("fdr_tv_poisson_step_f32_dev",), ("Plan.tv_poisson_step_dev",), OP_PLAN,
                      _poisson_step(1, _w)))
    CASES.append(case("tv-poisson-step-group" + ("-weights" if _w else ""), ("fdr_tv_poisson_step_group_f32_dev",),
                      ("Plan.tv_poisson_step_group_dev",), OP_PLAN, _poisson_step(3, _w)))


# the TV factor of one Richardson-Lucy step, single and in a group; the spectrum sum
def _factor(count, with_weights, couple):
    def build(fdr, p, b):
        u = b.inp(pitched([picture(k) for k in range(count)], STRIDE, PITCH))
        w = b.inp(window(weights(), STRIDE)) if with_weights else None
        out = b.out(count * OPITCH)
        if count == 1:
            return lambda st: p.rl_tv_factor_dev(u.data_ptr(), *W, out.data_ptr(), OSTRIDE, 0.01, 0.0, _dp(w), stream=st)
        return lambda st: p.rl_tv_factor_group_dev(u.data_ptr(), PITCH, count, *W, out.data_ptr(), OPITCH, OSTRIDE, 0.01, 0.0, _dp(w),
                                                   fdr.TV_COUPLE_CHANNELS if couple else fdr.TV_COUPLE_NONE, stream=st)
    return build


for _w in (False, True):
    _s = "-weights" if _w else ""
    CASES.append(case("rl-tv-factor" + _s, ("fdr_rl_tv_factor_f32_dev",), ("Plan.rl_tv_factor_dev", "rl_tv_factor_dev"), OP_PLAN, _factor(1, _w, False)))
    CASES.append(case("rl-tv-factor-group" + _s, ("fdr_rl_tv_factor_group_f32_dev",), ("Plan.rl_tv_factor_group_dev",), OP_PLAN, _factor(3, _w, False)))
CASES.append(case("rl-tv-factor-group-coupled", ("fdr_rl_tv_factor_group_f32_dev",), ("Plan.rl_tv_factor_group_dev",), OP_PLAN, _factor(3, False, True)))


def _spectrum_sum(accumulate):
    def build(fdr, p, b):
        n = 2 * 1000 + 2
        srcs = [b.inp(noise(n, 40 + k)) for k in range(3)]
        dst = b.inout(noise(n, 50)) if accumulate else b.out(n)
        return lambda st: fdr.spectrum_sum_dev(dst.data_ptr(), [s.data_ptr() for s in srcs], n, accumulate, stream=st)
    return build


CASES.append(case("spectrum-sum", ("fdr_spectrum_sum_f32_dev",), ("spectrum_sum_dev",), None, _spectrum_sum(False)))
CASES.append(case("spectrum-sum-accumulate", ("fdr_spectrum_sum_f32_dev",), ("spectrum_sum_dev",), None, _spectrum_sum(True)))


# sectioned restoration: a 50 x 150 picture in 2 x 2 tiles of 37 x 101 on the operator plan, the 15 x 15 motion PSF for all tiles
T_ROWS, T_COLS, T_STRIDE, T_OSTRIDE = 50, 150, 153, 151


def _tiled(method, with_weights):
    def build(fdr, p, b):
        prm = fdr.TiledParams.make(method, (ROWS, COLS), (8, 8), ITER, fdr.RL_SIGMA, 200.0, 2.0, 0.0, False, False, fdr.NORM_CROPPED)
        lay = fdr.tiled_layout(T_ROWS, T_COLS, 15, 15, prm)
        assert (lay.tiles_r, lay.tiles_c, lay.min_M, lay.min_N) == (2, 2, M, N)
        img = b.inp(window(picture(0, T_ROWS, T_COLS), T_STRIDE))
        w = b.inp(window(weights(T_ROWS, T_COLS), T_STRIDE)) if with_weights else None
        psf = b.inp(window(fdr.motionBlurKernel(15, 30.0), 16))
        out = b.out(T_ROWS * T_OSTRIDE)
        import torch
        work = torch.zeros(lay.work_bytes + 256, dtype=torch.uint8, device="cuda")
        b.keep = work
        wp = (work.data_ptr() + 255) & ~255
        return lambda st: p.restore_tiled_dev(img.data_ptr(), T_ROWS, T_COLS, T_STRIDE, psf.data_ptr(), 0, 1, 15, 15, 16, out.data_ptr(), T_OSTRIDE, prm,
                                              wp, lay.work_bytes, _dp(w), T_STRIDE if with_weights else 0, stream=st)
    return build


def _tiled_twice(fdr, p, b):
    """two calls with different tiles (origins 0, 13 / 0, 49 and 0, 20 / 0, 70), one behind the other on the stream: the cover tables of
    the first are made on the host, and the second call makes its own before the first one's have been used"""
    import torch
    prms = [fdr.TiledParams.make(0, tile, (8, 8), ITER, fdr.RL_SIGMA, 200.0, 2.0, 0.0, False, False, fdr.NORM_NONE) for tile in ((ROWS, COLS), (30, 80))]
    lays = [fdr.tiled_layout(T_ROWS, T_COLS, 15, 15, q) for q in prms]
    assert all((l.min_M, l.min_N, l.tiles_r, l.tiles_c) == (M, N, 2, 2) for l in lays)
    img = b.inp(window(picture(0, T_ROWS, T_COLS), T_STRIDE))
    psf = b.inp(window(fdr.motionBlurKernel(15, 30.0), 16))
    outs = [b.out(T_ROWS * T_OSTRIDE) for _ in prms]
    works = [torch.zeros(l.work_bytes + 256, dtype=torch.uint8, device="cuda") for l in lays]
    b.keep = works

    def call(st):
        for q, l, o, w in zip(prms, lays, outs, works):
            p.restore_tiled_dev(img.data_ptr(), T_ROWS, T_COLS, T_STRIDE, psf.data_ptr(), 0, 1, 15, 15, 16, o.data_ptr(), T_OSTRIDE, q,
                                (w.data_ptr() + 255) & ~255, l.work_bytes, stream=st)
    return call


CASES.append(case("tiled-rl-two-layouts", ("fdr_restore_tiled_f32_dev",), ("Plan.restore_tiled_dev",), OP_PLAN, _tiled_twice))
for _name, _method in (("rl", 0), ("tv", 1)):
    for _w in (False, True):
        CASES.append(case("tiled-%s%s" % (_name, "-weights" if _w else ""), ("fdr_restore_tiled_f32_dev",), ("Plan.restore_tiled_dev",), OP_PLAN,
                          _tiled(_method, _w)))


# ---- the batch forms: 5 images, groups 2, 2, 1 ------------------------------------------------------------------------------------
def _ba(d):
    return (d.imgs, PITCH, d.count, ROWS, COLS, STRIDE, d.out, OPITCH, OSTRIDE)


bop("batch-blur", "fdr_blur_batch_f32_dev", "Plan.blur_batch_dev", lambda fdr, p, b, d: lambda st: p.blur_batch_dev(*_ba(d), stream=st))
bop("batch-rl", "fdr_richardson_lucy_batch_f32_dev", "Plan.richardson_lucy_batch_dev",
    lambda fdr, p, b, d: lambda st: p.richardson_lucy_batch_dev(*_ba(d), ITER, stream=st))
bop_w("batch-rl-free", "fdr_richardson_lucy_batch_f32_dev", "Plan.richardson_lucy_batch_dev",
      lambda fdr, p, b, d: lambda st: p.richardson_lucy_batch_dev(*_ba(d), ITER, free_boundary=True, d_weights=d.w, wstride=d.ws, stream=st))


def _batch_accel(free):
    def make(fdr, p, b, d):
        al = b.out(COUNT * ITER)
        return lambda st: p.richardson_lucy_batch_dev(*_ba(d), ITER, free_boundary=free, d_weights=d.w, wstride=d.ws, stream=st, accelerate=True,
                                                      d_alphas=al.data_ptr())
    return make


bop("batch-rl-accel", "fdr_richardson_lucy_batch_accel_f32_dev", "Plan.richardson_lucy_batch_dev", _batch_accel(False))
bop_w("batch-rl-free-accel", "fdr_richardson_lucy_batch_accel_f32_dev", "Plan.richardson_lucy_batch_dev", _batch_accel(True))


def _batch_rltv(free, couple=False):
    return lambda fdr, p, b, d: lambda st: p.richardson_lucy_tv_batch_dev(*_ba(d), ITER, 0.01, free_boundary=free, d_weights=d.w, wstride=d.ws,
                                                                          couple=fdr.TV_COUPLE_CHANNELS if couple else fdr.TV_COUPLE_NONE, stream=st)


bop("batch-rl-tv", "fdr_richardson_lucy_tv_batch_f32_dev", "Plan.richardson_lucy_tv_batch_dev", _batch_rltv(False))
bop_w("batch-rl-tv-free", "fdr_richardson_lucy_tv_batch_f32_dev", "Plan.richardson_lucy_tv_batch_dev", _batch_rltv(True))
bop("batch-rl-tv-coupled", "fdr_richardson_lucy_tv_batch_f32_dev", "Plan.richardson_lucy_tv_batch_dev", _batch_rltv(False, True), count=3, group=3)
bop_w("batch-rl-tv-free-coupled", "fdr_richardson_lucy_tv_batch_f32_dev", "Plan.richardson_lucy_tv_batch_dev", _batch_rltv(True, True), count=3, group=3)


def _batch_tv(coupled):
    return lambda fdr, p, b, d: lambda st: p.tv_deconv_batch_dev(*_ba(d), 200.0, 2.0, ITER, coupled=coupled, stream=st)


def _batch_tv_free(coupled):
    return lambda fdr, p, b, d: lambda st: p.tv_deconv_free_batch_dev(*_ba(d), 200.0, 2.0, ITER, d.w, d.ws, coupled=coupled, stream=st)


def _batch_tv_poisson(coupled):
    return lambda fdr, p, b, d: lambda st: p.tv_deconv_poisson_batch_dev(*_ba(d), 20.0, 2.0, ITER, d.w, d.ws, background=0.01, coupled=coupled, stream=st)


def _batch_tv_auto(sigmas, coupled):
    def make(fdr, p, b, d):
        tr = b.out(d.count * 3 * ITER, dtype=_f64())
        return lambda st: p.tv_deconv_auto_batch_dev(*_ba(d), 0.02, 2.0, ITER, d.w, d.ws, sigmas=sigmas(d.count) if sigmas else None,
                                                     d_trace=tr.data_ptr(), trace_pitch=3 * ITER, coupled=coupled, stream=st)
    return make


bop("batch-tv", "fdr_tv_deconv_batch_f32_dev", "Plan.tv_deconv_batch_dev", _batch_tv(False))
bop("batch-tv-coupled", "fdr_tv_deconv_batch_f32_dev", "Plan.tv_deconv_batch_dev", _batch_tv(True), count=3, group=3)
bop_w("batch-tv-free", "fdr_tv_deconv_free_batch_f32_dev", "Plan.tv_deconv_free_batch_dev", _batch_tv_free(False))
bop_w("batch-tv-free-coupled", "fdr_tv_deconv_free_batch_f32_dev", "Plan.tv_deconv_free_batch_dev", _batch_tv_free(True), count=3, group=3)
bop_w("batch-tv-poisson", "fdr_tv_deconv_poisson_batch_f32_dev", "Plan.tv_deconv_poisson_batch_dev", _batch_tv_poisson(False))
bop_w("batch-tv-poisson-coupled", "fdr_tv_deconv_poisson_batch_f32_dev", "Plan.tv_deconv_poisson_batch_dev", _batch_tv_poisson(True), count=3, group=3)
bop_w("batch-tv-auto", "fdr_tv_deconv_auto_batch_f32_dev", "Plan.tv_deconv_auto_batch_dev", _batch_tv_auto(None, False))
bop("batch-tv-auto-sigmas", "fdr_tv_deconv_auto_batch_f32_dev", "Plan.tv_deconv_auto_batch_dev",
    _batch_tv_auto(lambda n: [0.01 + 0.005 * k for k in range(n)], False))
bop_w("batch-tv-auto-coupled", "fdr_tv_deconv_auto_batch_f32_dev", "Plan.tv_deconv_auto_batch_dev", _batch_tv_auto(None, True), count=3, group=3)
bop("batch-tv-auto-estimated", "fdr_tv_deconv_auto_batch_f32_dev", "Plan.tv_deconv_auto_batch_dev",
    _batch_tv_auto(lambda n: [0.02 if k % 2 else 0.0 for k in range(n)], False), exempt=Q_TV_AUTO_BATCH)


# ---- Wiener / CLS: fdr_wiener_f32_dev once on every plan path, the filter setters in front of it ----------------------------------
WIENER_PLANS = [("simple", (8, 8, "MODE_PARITY", ("FLAG_SIMPLE_PATH",))), ("parity", (8, 8, "MODE_PARITY", ())),
                ("fast-full", (8, 32, "MODE_FAST", ("FLAG_FULL_SPECTRUM",))), ("fast-half", (8, 32, "MODE_FAST", ())),
                ("mixed", (75, 64, "MODE_FAST", ("FLAG_MIXED_RADIX",))), ("any-size", (12, 20, "MODE_PARITY", ("FLAG_ANY_SIZE",))),
                ("long-rows", (16384, 8, "MODE_FAST", ()))]
SETTERS = {
    "dev": (("fdr_set_psf_dev",), ("Plan.set_psf_dev",)),
    "cls-dev": (("fdr_set_psf_dev", "fdr_set_psf_cls_dev"), ("Plan.set_psf_dev",)),
    "motion": (("fdr_set_psf_dev", "fdr_set_psf_motion"), ("Plan.set_psf_dev", "Plan.set_psf_motion")),
    "motion-cls": (("fdr_set_psf_dev", "fdr_set_psf_motion_cls"), ("Plan.set_psf_dev", "Plan.set_psf_motion")),
    "disk": (("fdr_set_psf_dev", "fdr_set_psf_disk"), ("Plan.set_psf_dev", "Plan.set_psf_disk")),
    "disk-cls": (("fdr_set_psf_dev", "fdr_set_psf_disk_cls"), ("Plan.set_psf_dev", "Plan.set_psf_disk")),
}


def _wiener(setter, norm_area=1):
    """The generated setters take no data: a filter built too early would still be right.  So a data setter (the poisoned 3 x 3 PSF)
    comes first on the stream: a generated filter that did not wait for its turn is overwritten by it."""
    def build(fdr, p, b):
        rows, cols = p.M - 1, p.N - 3
        psf = b.inp(window(dense_psf(5, 3), 4))
        img = b.inp(window(noise_picture(1, rows, cols), cols + 2))
        out = b.out(rows * (cols + 1))

        def call(st):
            if setter == "cls-dev":
                p.set_psf_dev(psf.data_ptr(), 3, 3, 4, 0.01, stream=st, gamma=0.05)
            else:
                p.set_psf_dev(psf.data_ptr(), 3, 3, 4, 0.01, stream=st)
            if setter.startswith("motion"):
                p.set_psf_motion(5, 30.0, 0.01, stream=st, gamma=0.05 if setter.endswith("cls") else 0.0)
            elif setter.startswith("disk"):
                p.set_psf_disk(2.0, 0.01, 0.05 if setter.endswith("cls") else 0.0, stream=st)
            p.wiener_dev(img.data_ptr(), rows, cols, cols + 2, out.data_ptr(), cols + 1, norm_area, stream=st)
        return call
    return build


for _name, _plan in WIENER_PLANS:
    CASES.append(case("wiener-" + _name, SETTERS["dev"][0] + ("fdr_wiener_f32_dev",), SETTERS["dev"][1] + ("Plan.wiener_dev",), _plan, _wiener("dev")))
for _setter in ("cls-dev", "motion", "motion-cls", "disk", "disk-cls"):
    for _name, _plan in (WIENER_PLANS[3], WIENER_PLANS[4]) if _setter == "cls-dev" else (WIENER_PLANS[3],):
        CASES.append(case("wiener-%s-set-%s" % (_name, _setter), SETTERS[_setter][0] + ("fdr_wiener_f32_dev",),
                          SETTERS[_setter][1] + ("Plan.wiener_dev",), _plan, _wiener(_setter, 0)))
CASES.append(case("wiener-parity-set-motion", SETTERS["motion"][0] + ("fdr_wiener_f32_dev",), SETTERS["motion"][1] + ("Plan.wiener_dev",),
                  WIENER_PLANS[1][1], _wiener("motion")))


def _export(fdr, p, b):
    psf = b.inp(window(dense_psf(5, 3), 4))
    nbytes = p.filter_bytes()
    blk = b.out(nbytes // 4)

    def call(st):
        p.set_psf_dev(psf.data_ptr(), 3, 3, 4, 0.02, stream=st)
        p.export_filter_dev(blk.data_ptr(), nbytes, stream=st)
    return call


def _import(fdr, p, b):
    import torch
    rows, cols = p.M - 1, p.N - 3
    nbytes = p.filter_bytes()
    first = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    p.set_psf(dense_psf(6, 3), 0.02)
    p.export_filter_dev(first.data_ptr(), nbytes)
    torch.cuda.synchronize()
    blk = b.inp(first.cpu().numpy())
    psf = b.inp(window(dense_psf(5, 3), 4))
    img = b.inp(window(noise_picture(1, rows, cols), cols + 2))
    out = b.out(rows * (cols + 1))

    def call(st):
        p.set_psf_dev(psf.data_ptr(), 3, 3, 4, 0.01, stream=st)   # (another filter first: an import that came too early is overwritten)
        p.import_filter_dev(blk.data_ptr(), nbytes, 0.02, stream=st)
        p.wiener_dev(img.data_ptr(), rows, cols, cols + 2, out.data_ptr(), cols + 1, stream=st)
    return call


for _name, _plan in (WIENER_PLANS[3], WIENER_PLANS[1]):
    CASES.append(case("filter-export-" + _name, ("fdr_set_psf_dev", "fdr_plan_export_filter_dev"), ("Plan.set_psf_dev", "Plan.export_filter_dev"), _plan, _export))
    CASES.append(case("filter-import-" + _name, ("fdr_set_psf_dev", "fdr_plan_import_filter_dev", "fdr_wiener_f32_dev"),
                      ("Plan.set_psf_dev", "Plan.import_filter_dev", "Plan.wiener_dev"), _plan, _import))


# fdr_wiener_batch_f32_dev: 5 images, two internal streams (fork from and join into the caller's stream), groups of two
def _wiener_batch(recapture):
    def build(fdr, p, b):
        import torch
        rows, cols = p.M - 1, p.N - 3
        stride, ostride = cols + 2, cols + 1
        pitch, opitch = rows * stride + 3, rows * ostride + 5
        psf = b.inp(window(dense_psf(5, 3), 4))
        imgs = b.inp(pitched([noise_picture(k, rows, cols) for k in range(COUNT)], stride, pitch))
        out = b.out(COUNT * opitch)

        def call(st):
            p.set_psf_dev(psf.data_ptr(), 3, 3, 4, 0.01, stream=st)
            p.wiener_batch_dev(imgs.data_ptr(), pitch, COUNT, rows, cols, stride, out.data_ptr(), opitch, ostride, fdr.NORM_PADDED, stream=st)
        if recapture:
            # one argument changes between the runs (on idle streams, synchronised): the fenced call finds another graph and captures anew
            other = torch.zeros(COUNT * pitch, dtype=torch.float32, device="cuda")
            scratch = torch.zeros(COUNT * opitch, dtype=torch.float32, device="cuda")
            p.set_psf(dense_psf(5, 3), 0.01)

            def prepare():
                p.wiener_batch_dev(other.data_ptr(), pitch, COUNT, rows, cols, stride, scratch.data_ptr(), opitch, ostride, fdr.NORM_CROPPED)
                torch.cuda.synchronize()
            b.prepare = prepare
        return call
    return build


_WB = (("fdr_set_psf_dev", "fdr_wiener_batch_f32_dev"), ("Plan.set_psf_dev", "Plan.wiener_batch_dev"))
for _name, _plan in (WIENER_PLANS[3], WIENER_PLANS[2], WIENER_PLANS[1]):
    CASES.append(case("wiener-batch-%s-streams" % _name, *_WB, _plan, _wiener_batch(False), batching=(2, 2)))
CASES.append(case("wiener-batch-graph-replay", *_WB, WIENER_PLANS[3][1], _wiener_batch(False), batching=(2, 2), options=(("OPT_BATCH_GRAPH", 1),)))
CASES.append(case("wiener-batch-graph-capture", *_WB, WIENER_PLANS[3][1], _wiener_batch(True), batching=(2, 2), options=(("OPT_BATCH_GRAPH", 1),)))


# ---- the rest ---------------------------------------------------------------------------------------------------------------------
def _generated_operator(kind):
    def build(fdr, p, b):
        psf = b.inp(motion_plane(fdr))
        img = b.inp(window(picture(), STRIDE))
        out = b.out(ROWS * OSTRIDE)

        def call(st):
            p.set_operator_psf_dev(psf.data_ptr(), M, N, N, stream=st)   # (overwrites a generated PSF that came too early)
            if kind == "motion":
                p.set_operator_psf_motion(15, 30.0, stream=st)
            else:
                p.set_operator_psf_disk(3.5, stream=st)
            p.blur_dev(img.data_ptr(), *W, out.data_ptr(), OSTRIDE, stream=st)
        return call
    return build


CASES.append(case("operator-psf-motion", ("fdr_set_operator_psf_dev", "fdr_set_operator_psf_motion", "fdr_blur_f32_dev"),
                  ("Plan.set_operator_psf_dev", "Plan.set_operator_psf_motion", "Plan.blur_dev"), OP_PLAN, _generated_operator("motion")))
CASES.append(case("operator-psf-disk", ("fdr_set_operator_psf_dev", "fdr_set_operator_psf_disk", "fdr_blur_f32_dev"),
                  ("Plan.set_operator_psf_dev", "Plan.set_operator_psf_disk", "Plan.blur_dev"), OP_PLAN, _generated_operator("disk")))


def _estimator(which):
    def build(fdr, p, b):
        img = b.inp(window(picture(), STRIDE))
        if which == "cepstrum":
            out = b.out(M * N)
            return lambda st: p.cepstrum_dev(img.data_ptr(), *W, out.data_ptr(), stream=st)
        if which == "motion":
            out = b.out(36 * 7)
            return lambda st: tuple(p.estimate_motion_dev(img.data_ptr(), *W, 3, 9, 5.0, out.data_ptr(), stream=st))
        if which == "defocus":
            out = b.out(7)
            return lambda st: tuple(p.estimate_defocus_dev(img.data_ptr(), *W, 3, 9, 5.0, out.data_ptr(), stream=st))

        def call(st):
            e = p.estimate_blur_dev(img.data_ptr(), *W, 3, 9, 5.0, 3, 9, 5.0, stream=st)
            return (e.kind,) + tuple(e.motion) + tuple(e.defocus)
        return call
    return build


CASES.append(case("cepstrum", ("fdr_cepstrum_f32_dev",), ("Plan.cepstrum_dev",), OP_PLAN, _estimator("cepstrum")))
CASES.append(case("estimate-motion", ("fdr_estimate_motion_f32_dev",), ("Plan.estimate_motion_dev",), OP_PLAN, _estimator("motion"), exempt=Q_MOTION))
CASES.append(case("estimate-defocus", ("fdr_estimate_defocus_f32_dev",), ("Plan.estimate_defocus_dev",), OP_PLAN, _estimator("defocus"), exempt=Q_DEFOCUS))
CASES.append(case("estimate-blur", ("fdr_estimate_blur_f32_dev",), ("Plan.estimate_blur_dev",), OP_PLAN, _estimator("blur"), exempt=Q_BLUR))

op("reg-curve", "fdr_reg_curve_f32_dev", "Plan.reg_curve_dev",
   lambda fdr, p, b, d: lambda st: np.concatenate(p.reg_curve_dev(d.img, *W, [1e-3, 1e-2, 1e-1], [0.0, 1e-2, 1.0], stream=st)), exempt=Q_REG)
op("choose-reg-gcv", "fdr_choose_reg_f32_dev", "Plan.choose_regularisation_dev",
   lambda fdr, p, b, d: lambda st: tuple(p.choose_regularisation_dev(d.img, *W, n_grid=8, refine=1, stream=st)), exempt=Q_REG)
op("choose-reg-discrepancy", "fdr_choose_reg_f32_dev", "Plan.choose_regularisation_dev",
   lambda fdr, p, b, d: lambda st: tuple(p.choose_regularisation_dev(d.img, *W, method=fdr.REG_DISCREPANCY, n_grid=8, refine=1, stream=st)), exempt=Q_REG)


def _noise_sigma(fdr, p, b):
    img = b.inp(window(picture() + 0.05 * noise(ROWS * COLS, 3).reshape(ROWS, COLS), STRIDE))
    return lambda st: (p.noise_sigma_dev(img.data_ptr(), *W, stream=st),)


CASES.append(case("noise-sigma", ("fdr_noise_sigma_f32_dev",), ("Plan.noise_sigma_dev",), OP_PLAN, _noise_sigma, exempt=Q_REG))


def _generator(which):
    """no inputs: the output doubles as an input (see Bufs.inout)"""
    def build(fdr, p, b):
        L = fdr.lib
        if which == "synth":
            out = b.inout(np.full(5000, -7.0))
            return lambda st: fdr.synth_image_dev(out.data_ptr(), 5000, 0x5EED0002, first_index=17, stream=st)
        out = b.inout(np.full(15 * 15, -7.0))
        if which == "motion":
            return lambda st: fdr._check(L.fdr_psf_motion_dev(0, 15, 30.0, _ptr(out), _st(st)))
        if which == "gaussian":
            return lambda st: fdr._check(L.fdr_psf_gaussian_dev(0, 15, 2.5, _ptr(out), _st(st)))
        return lambda st: fdr._check(L.fdr_psf_disk_dev(0, 15, 5.25, _ptr(out), _st(st)))
    return build


CASES.append(case("psf-motion", ("fdr_psf_motion_dev",), (), None, _generator("motion")))
CASES.append(case("psf-gaussian", ("fdr_psf_gaussian_dev",), (), None, _generator("gaussian")))
CASES.append(case("psf-disk", ("fdr_psf_disk_dev",), (), None, _generator("disk")))
CASES.append(case("synth", ("fdr_synth_image_dev",), ("synth_image_dev",), None, _generator("synth")))


def _white_balance(fdr, p, b):
    import torch
    rows, cols, stride, ostride = 19, 45, 50, 3 * 45 + 7
    planes = [b.inp(window(noise(rows * cols, 60 + k).reshape(rows, cols), stride)) for k in range(6)]
    out = b.out(rows * ostride, dtype=torch.uint8)
    po = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in planes[:3]])
    pr = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in planes[3:]])
    return lambda st: fdr._check(fdr.lib.fdr_white_balance_u8_dev(0, po, pr, rows, cols, stride, _ptr(out), ostride, _st(st)))


CASES.append(case("white-balance", ("fdr_white_balance_u8_dev",), (), None, _white_balance))


def _fft2d(inverse):
    def build(fdr, p, b):
        data = b.inout(noise(2 * p.M * p.N, 80) - 0.5)
        return lambda st: p.fft2d_dev(data.data_ptr(), inverse, stream=st)
    return build


for _name, _plan in (WIENER_PLANS[3], WIENER_PLANS[1], WIENER_PLANS[4]):
    CASES.append(case("fft2d-" + _name, ("fdr_fft2d_c2c_dev",), ("Plan.fft2d_dev",), _plan, _fft2d(False)))
CASES.append(case("fft2d-fast-half-inverse", ("fdr_fft2d_c2c_dev",), ("Plan.fft2d_dev",), WIENER_PLANS[3][1], _fft2d(True)))

# the slab primitives of the single-image multi-GPU mode, on a tables-only plan
SLAB_PLAN = (64, 128, "MODE_PARITY", ("FLAG_TABLES_ONLY",))


def _slab(which):
    def build(fdr, p, b):
        L = fdr.lib
        if which == "pad":
            src = b.inp(window(noise(3 * 37, 90).reshape(3, 37), 41))
            dst = b.out(5 * 128 * 2)
            return lambda st: fdr._check(L.fdr_slab_pad_dev(_ptr(src), 3, 37, 41, _ptr(dst), 5, 128, _st(st)))
        if which in ("rows-fft", "rows-fft-dim1"):
            dim = 1 if which.endswith("dim1") else 0
            data = b.inout(noise(5 * (64 if dim else 128) * 2, 91) - 0.5)
            return lambda st: fdr._check(L.fdr_slab_rows_fft_dev(p._h, _ptr(data), 5, dim, 0, _st(st)))
        if which == "pack":
            src = b.inp(noise(33 * 300, 92))
            dst = b.out(33 * 300)
            counts = (ctypes.c_int * 3)(100, 57, 143)
            return lambda st: fdr._check(L.fdr_slab_pack_dev(_ptr(src), 33, 300, 3, counts, 4, _ptr(dst), _st(st)))
        if which == "transpose":
            src = b.inp(noise(33 * 65 * 2, 93))
            dst = b.out(33 * 65 * 2)
            return lambda st: fdr._check(L.fdr_slab_transpose_dev(_ptr(src), _ptr(dst), 33, 65, 8, _st(st)))
        if which == "wiener":
            g = b.inout(noise(2 * 1000, 94) - 0.5)
            h = b.inp(noise(2 * 1000, 95) - 0.5)
            return lambda st: fdr._check(L.fdr_slab_wiener_dev(p._h, _ptr(g), _ptr(h), 1000, ctypes.c_float(0.01), _st(st)))
        if which == "real":
            src = b.inp(noise(2 * 1000, 96))
            dst = b.out(1000)
            return lambda st: fdr._check(L.fdr_slab_real_dev(_ptr(src), _ptr(dst), 1000, _st(st)))
        real = b.inp(noise(9 * 128, 97) - 0.5)
        if which == "minmax":
            mm = b.inout(np.array([np.inf, -np.inf], dtype=np.float32))
            return lambda st: fdr._check(L.fdr_slab_minmax_dev(p._h, _ptr(real), 9, 128, 7, 101, _ptr(mm), _st(st)))
        mm = b.inp(np.array([-0.5, 0.5], dtype=np.float32))
        out = b.out(7 * 103)
        return lambda st: fdr._check(L.fdr_slab_normalize_dev(_ptr(real), 128, _ptr(mm), _ptr(out), 7, 101, 103, _st(st)))
    return build


for _which, _entry in (("pad", "fdr_slab_pad_dev"), ("rows-fft", "fdr_slab_rows_fft_dev"), ("rows-fft-dim1", "fdr_slab_rows_fft_dev"),
                       ("pack", "fdr_slab_pack_dev"), ("transpose", "fdr_slab_transpose_dev"), ("wiener", "fdr_slab_wiener_dev"),
                       ("real", "fdr_slab_real_dev"), ("minmax", "fdr_slab_minmax_dev"), ("normalize", "fdr_slab_normalize_dev")):
    CASES.append(case("slab-" + _which, (_entry,), (), SLAB_PLAN, _slab(_which)))

assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"
ENTRIES = frozenset(e for c in CASES for e in c.entries)


# ---- the tests --------------------------------------------------------------------------------------------------------------------
def _flags(fdr, names):
    f = 0
    for n in names:
        f |= getattr(fdr, n)
    return f


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_entry_is_ordered_on_its_stream_and_does_not_wait(fdr, c):
    import torch
    b = Bufs()
    p = None
    if c.plan is not None:
        p = fdr.Plan(c.plan[0], c.plan[1], getattr(fdr, c.plan[2]), flags=_flags(fdr, c.plan[3]))
    try:
        if c.batching:
            p.set_batching(*c.batching)
        for opt, val in c.options:
            p.set_option(getattr(fdr, opt), val)
        call = c.build(fdr, p, b)
        v = sf.judge(fdr, c.id, call, b.inputs, b.outputs, exempt=c.exempt, prepare=getattr(b, "prepare", None))
        assert v.ordered, ("%s: the results behind the fence differ from the quiet run's: part of the call did not run in order on its stream "
                           "(%s)" % (c.id, ", ".join(c.entries)))
        if c.exempt is None:
            assert not v.waits, ("%s: the call returned after the delay on its stream had ended: it waited for the stream, and include/fdr.h has "
                                 "no sentence that lets it (%s)" % (c.id, ", ".join(c.entries)))
    finally:
        torch.cuda.synchronize()
        if p is not None:
            p.close()


def test_the_fence_sees_what_it_is_for(fdr):
    """stand-in entries made of torch copies: issued on a second non-blocking stream and on the null stream (both unordered), a correct
    copy followed by a wait for the stream (waits), and a correct copy (passes)"""
    import torch
    side = sf.side_stream()
    second = sf.pick_stream((torch.cuda.default_stream(), side))
    assert sf.runs_beside(side, second) and sf.runs_beside(side, torch.cuda.default_stream())
    assert sf.stream_flags(fdr, second) & sf.HIP_STREAM_NON_BLOCKING
    b = Bufs()
    src = b.inp(noise(4096, 1))
    dst = b.out(4096)

    def copy_on(stream):
        with torch.cuda.stream(stream):
            dst[:4096].copy_(src, non_blocking=True)

    def correct(st):
        copy_on(torch.cuda.ExternalStream(st))

    def on_second_stream(st):
        copy_on(second)

    def on_null_stream(st):
        copy_on(torch.cuda.default_stream())

    def waits(st):
        copy_on(torch.cuda.ExternalStream(st))
        side.synchronize()

    assert int(torch.cuda.default_stream().cuda_stream) == 0
    got = {f.__name__: sf.judge(fdr, "stand-in " + f.__name__, f, b.inputs, b.outputs, side) for f in (correct, on_second_stream, on_null_stream, waits)}
    second.synchronize()
    torch.cuda.synchronize()
    assert got["correct"].ordered and not got["correct"].waits
    assert not got["on_second_stream"].ordered, "the fence missed a copy on another non-blocking stream"
    assert not got["on_null_stream"].ordered, "the fence missed a copy on the null stream"
    assert got["waits"].ordered and got["waits"].waits, "the fence missed a wait for the stream"
