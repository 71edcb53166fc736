"""Batched blur and Richardson-Lucy (fdr_blur_batch_f32_dev, fdr_richardson_lucy_batch_f32*): a float64 model of a batched call
with the structure of the device's, built from the functions of _rl_model.py and _rlfree_model.py over the buffer layouts of
_batch_model.py; fault models of such a call; the images, the judge and the case lists of test_rl_batch_gpu.py.
test_rl_batch_host.py turns the fault models against the judge before it judges the GPU.

A call cuts `count` images into launch groups of `group` (the last may be smaller); a group runs to completion on the slots
0 .. g - 1: the start of every image, then per iteration ONE launch per pass over the group, then the normalisation of every image.
Image k of a group keeps its estimate u in its own output window (plain form) or its own dense M x N plane (free-boundary form) and
its ratio r in slot k; the free-boundary form computes the coverage and wgt = 1 / alpha once per call."""
import collections

import numpy as np

import _batch_model as bm
from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, TAU, blur_model, normalize, op_spectrum, rel_err, rl_model
from _rlfree_model import SIGMA, fullblur, rlfree_model

AREAS = (NORM_NONE, NORM_CROPPED, NORM_PADDED)
AREA_NAME = {NORM_NONE: "NONE", NORM_CROPPED: "CROPPED", NORM_PADDED: "PADDED"}
FORMS = ("blur", "adjoint", "plain", "free")
FAULTS = ("ratio_reads_image0", "update_reads_previous_group", "ignore_out_pitch", "wgt_image0_only", "drop_last_group")


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def images(M, N, rows, cols, count, seed):
    """float32 [count, rows, cols]: bm.batch_images (a range and extreme positions of its own per image) made positive, as the
    pictures of test_rl_gpu.py are (clipped at 0, plus 0.05), with a negative patch at the top-left corner: RL starts from d+"""
    imgs = np.clip(bm.batch_images(M, N, rows, cols, count, seed), 0, None) + np.float32(0.05)
    imgs[:, : max(1, rows // 16), : max(1, cols // 16)] -= np.float32(0.5)
    return imgs.astype(np.float32)


def mask(rows, cols, seed, zero=0.03):
    """weights in {0, 1}, about 3 % zeros (at least one)"""
    m = (np.random.default_rng(seed).random((rows, cols)) >= zero).astype(np.float32)
    m[rows // 2, cols // 2] = 0
    return m


def out_layout(lay, out_rows, out_cols):
    """the output side of a call whose output window differs from the input's (free-boundary form): the same kind of layout"""
    loose = lay.stride != lay.cols
    return (bm.loose_layout if loose else bm.tight_layout)(out_rows, out_cols, lay.count)


# ---- float64 model of one image (the reference of the GPU test) -----------------------------------------------------------
def single(form, d, psf, M, N, iterations, area, weights=None, sigma=SIGMA, out_shape=None):
    if form == "blur" or form == "adjoint":
        return blur_model(d, psf, M, N, adjoint=form == "adjoint")
    if form == "plain":
        return rl_model(d, psf, M, N, iterations, area)
    return rlfree_model(d, psf, M, N, iterations, weights, sigma, out_shape, area)


def references(form, imgs, psf, M, N, iterations, area, weights=None, sigma=SIGMA, out_shape=None):
    return np.stack([single(form, d, psf, M, N, iterations, area, weights, sigma, out_shape) for d in imgs])


# ---- float64 batched call with fault models -------------------------------------------------------------------------------
def batched_call(form, flat_in, lay, olay, psf, M, N, iterations, area, group, weights=None, sigma=SIGMA, fault=None):
    """The batched call in float64: image i read through img_pitch and stride, the groups of bm.launches, per group the start, the
    iterations pass by pass over the group, the normalisation, the store through out_pitch and out_stride into a SENTINEL-filled
    buffer (olay: the output side).  `fault`: one of FAULTS.
      ratio_reads_image0           the ratio of image k >= 1 of a group divides the group's first datum
      update_reads_previous_group  from the second group on, the update multiplies the estimate the slot held for the previous group
      ignore_out_pitch             image i is stored at i * out_rows * out_stride
      wgt_image0_only              free-boundary form: images k >= 1 of a group are updated without wgt
      drop_last_group              a last group smaller than `group` is not run"""
    assert form in ("plain", "free") and (fault is None or fault in FAULTS)
    rows, cols = lay.rows, lay.cols
    H = op_spectrum(psf, M, N)
    out = bm.new_output(olay, np.float64)
    win = np.zeros((M, N), dtype=bool)
    win[:rows, :cols] = True
    if form == "free":
        m = np.ones((rows, cols)) if weights is None else np.asarray(weights, dtype=np.float64)
        W = np.zeros((M, N))
        W[:rows, :cols] = m
        alpha = fullblur(W, H, adjoint=True)  # once per call
        seen = alpha > sigma
        wgt = np.where(seen, 1 / np.where(seen, alpha, 1), 0)
        sw = float(np.sum(W))
    held = {}  # slot -> the estimate it held when the previous group ended
    i0 = 0
    for n in bm.launches(lay.count, group):
        if fault == "drop_last_group" and n < group and i0 > 0:
            break
        d = [np.asarray(bm._window(flat_in, (i0 + k) * lay.img_pitch, rows, cols, lay.stride), dtype=np.float64) for k in range(n)]
        dp = [np.maximum(x, 0) for x in d]
        if form == "plain":
            u = [x.copy() for x in dp]
        else:
            dw = []
            for k in range(n):
                p = np.zeros((M, N))
                p[:rows, :cols] = m * dp[k]
                dw.append(p)
            u = [np.where(seen, (float(np.sum(dw[k])) / sw if sw > 0 else 0.0), 0.0) for k in range(n)]
        for _ in range(iterations):
            c, r, g = [], [], []
            for k in range(n):  # pass A, B', C (ratio) over the group
                c.append(blur_model(u[k], psf, M, N, H=H) if form == "plain" else fullblur(u[k], H))
            for k in range(n):
                src = 0 if fault == "ratio_reads_image0" else k
                if form == "plain":
                    ok = c[k] > TAU
                    r.append(np.where(ok, dp[src] / np.where(ok, c[k], 1), 0))
                else:
                    ok = win & (c[k] > TAU)
                    r.append(np.where(ok, dw[src] / np.where(ok, c[k], 1), 0))
            for k in range(n):  # pass A, B', C (update) over the group
                g.append(blur_model(r[k], psf, M, N, adjoint=True, H=H) if form == "plain" else fullblur(r[k], H, adjoint=True))
            for k in range(n):
                prev = held[k] if fault == "update_reads_previous_group" and k in held else u[k]
                if form == "plain":
                    u[k] = np.maximum(prev * g[k], 0)
                else:
                    u[k] = np.maximum(prev * (1 if fault == "wgt_image0_only" and k >= 1 else wgt) * g[k], 0)
        for k in range(n):
            held[k] = u[k]
            res = normalize(u[k][:olay.rows, :olay.cols], area, M, N)
            base = olay.lead + (i0 + k) * olay.rows * olay.out_stride if fault == "ignore_out_pitch" else bm.out_base(olay, i0 + k)
            bm._window(out, base, olay.rows, olay.cols, olay.out_stride)[...] = res
        i0 += n
    return out


# ---- the judge ------------------------------------------------------------------------------------------------------------
def error(got, want, area):
    """what test_rl_gpu.py and test_rlfree_gpu.py measure: max |got - model| / max |model| (raw outputs: blur, FDR_NORM_NONE), max-abs
    (normalised outputs)"""
    return rel_err(got, want) if area == NORM_NONE else float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)))


def model_errors(imgs, refs, area):
    return [error(a, b, area) for a, b in zip(imgs, refs)]


def judge(what, out, olay, ones, refs, tol, area, ones_err=None):
    """One batch result (the flat output buffer) against the one-by-one results `ones` (bit for bit) and the float64 model `refs`
    (error() within tol, per image); NaN and inf fail; everything outside the output windows must hold SENTINEL.  ones_err:
    model_errors(ones, refs, area) where the caller has them -- an image that equals `ones` bit for bit has that error."""
    got = bm.unpack(out, olay)
    bad, checks, worst = [], set(), 0.0
    if not bm.outside_untouched(out, olay):
        bad.append("%s: a value outside the output windows was overwritten" % what)
        checks.add("layout")
    for i in range(olay.count):
        if not np.all(np.isfinite(got[i])):
            bad.append("%s: image %d holds NaN or inf" % (what, i))
            checks.add("finite")
        same = np.array_equal(got[i], ones[i])
        if not same:
            bad.append("%s: image %d: %d of %d values differ from the image through the single call" % (what, i, int(np.count_nonzero(~(got[i] == ones[i]))),
                                                                                                       got[i].size))
            checks.add("bits")
        e = ones_err[i] if same and ones_err is not None else error(got[i], refs[i], area)
        worst = max(worst, e) if e == e and worst == worst else float("nan")
        if not e <= tol:
            bad.append("%s: image %d: error %.3g > %.3g against the float64 model" % (what, i, e, tol))
            checks.add("model")
    return bm.Verdict(worst, bad, checks)


# ---- the case lists of test_rl_batch_gpu.py -------------------------------------------------------------------------------
ROW_PLANS = bm.ROW_PLANS                                  # 16 x 2^5 .. 2^13, 2048 x 256, 2048 x 2048
COLUMN_PLANS = [(M, 64) for M in (8, 256, 512, 1024, 8192)]
COUNT = bm.COUNT                                          # 11 images ...
GROUPS = (2, 3, 4, 5, 8)                                  # ... in launches of 2, 3, 4, 5 and 8 with tails of 1, 2 and 3
ITERATIONS = (0, 1, 3)
LENGTH_COUNT = 5                                          # the length sweeps: 5 images in groups of 2 (2, 2, 1), 3 (3, 2), 4 (4, 1) and 5
LENGTH_GROUPS = (2, 3, 4, 5)
BIG_PIXELS = 1 << 21                                      # plans from here on: 3 images in groups of 2 (2, 1) and 3
BIG_COUNT, BIG_GROUPS = 3, (2, 3)

Case = collections.namedtuple("Case", "form iterations area masked full_out")
# one instantiation of each changed kind per length: blur and adjoint (ROW_OUT_BLUR), plain (RATIO, UPDATE; the last update routed to
# the raw plane under a normalisation), free (RATIO, UPDATE_W)
LENGTH_CASES = [Case("blur", 0, NORM_NONE, False, False), Case("adjoint", 0, NORM_NONE, False, False),
                Case("plain", 1, NORM_CROPPED, False, False), Case("free", 1, NORM_NONE, False, False)]
