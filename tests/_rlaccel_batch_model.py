"""Batched accelerated Richardson-Lucy (fdr_richardson_lucy_batch_accel_f32*): a float64 model of a batched accelerated call, built
from the steps and the recursion of _rlaccel_model.py (accelerate, rl_step_fn, rlfree_step_fn) over the buffer layouts of
_batch_model.py; fault models of such a call; the judge and the case list of test_rlaccel_batch_gpu.py.  test_rlaccel_batch_host.py
turns the fault models against the judge and proves what the case list covers before the GPU is judged.

A call cuts `count` images into launch groups of `group` (the last may be smaller).  A group runs to completion: the start of every
image, then per iteration ONE extrapolation, ONE step, ONE direction and ONE alpha launch over the group -- every image with its own
planes u, y, g, its own inner products and its own alpha -- then the normalisation of every image.  Image i's alphas lie at
i * alpha_pitch in the alphas buffer."""
import collections

import numpy as np

import _batch_model as bm
import _rl_batch_model as rb
from _batch_model import SENTINEL
from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, dense_psf, normalize
from _rlaccel_model import ACCEL_MAX, accelerate, rl_step_fn, rlfree_step_fn
from _rlfree_model import SIGMA

AREAS = rb.AREAS
AREA_NAME = rb.AREA_NAME
FAULTS = ("alpha_of_image0", "sums_over_group", "shared_g_plane", "previous_group_u", "ignore_alpha_pitch", "drop_last_group")
ALPHA_SLACK = 8  # floats in front of and behind the alphas of a batch

AlphaLayout = collections.namedtuple("AlphaLayout", "n count pitch lead tail")


def alpha_layout(n, count, loose):
    """the alphas of a batch: image i's n floats at lead + i * pitch; loose: a pitch of its own above n"""
    return AlphaLayout(n, count, n + 3 if loose else n, ALPHA_SLACK, ALPHA_SLACK)


def alpha_size(al):
    return al.lead + al.count * al.pitch + al.tail


def new_alphas(al, dtype=np.float32):
    return np.full(alpha_size(al), SENTINEL, dtype=dtype)


def unpack_alphas(flat, al):
    """[count, n] copies of the alphas"""
    return np.stack([flat[al.lead + i * al.pitch: al.lead + i * al.pitch + al.n].copy() for i in range(al.count)]) if al.count else np.zeros((0, al.n))


def alphas_outside_untouched(flat, al):
    rest = np.array(flat, copy=True)
    for i in range(al.count):
        rest[al.lead + i * al.pitch: al.lead + i * al.pitch + al.n] = SENTINEL
    return bool(np.all(rest == SENTINEL))


# ---- float64 model of one image (the reference of the GPU test) -----------------------------------------------------------
def start_and_step(form, d, psf, M, N, weights=None, sigma=SIGMA, dtype=np.float64):
    """(u_0, step) of either form from the step functions of _rlaccel_model.py"""
    if form == "plain":
        return rl_step_fn(d, psf, M, N, dtype)
    st, step = rlfree_step_fn(d, psf, M, N, weights, sigma, dtype)
    return st["u"], step


def single_path(form, d, psf, M, N, counts, weights=None, sigma=SIGMA, dtype=np.float64):
    """({n: raw u_n for n in counts}, the alphas of max(counts) iterations) of one image, in one run of `accelerate`"""
    u0, step = start_and_step(form, d, psf, M, N, weights, sigma, dtype)
    keep = dict.fromkeys(counts)
    _, alphas = accelerate(u0, step, max(counts), dtype, keep=keep)
    return keep, alphas


def output_of(u, olay, area, M, N):
    return normalize(u[:olay.rows, :olay.cols], area, M, N)


# ---- float64 batched call with fault models -------------------------------------------------------------------------------
def _alpha(num, den):
    q = num / den if den != 0.0 else 0.0
    return min(max(q, 0.0), ACCEL_MAX) if np.isfinite(q) else 0.0


def group_recursion(u0, steps, iterations, fault=None, held=None):
    """The recursion of `accelerate` on a group, pass by pass as the device runs it: (u_n per image, alphas [n images, iterations]).
    held: {slot: the u_(k-1) plane the slot held when the previous group ended} for the fault 'previous_group_u'; it is updated.
      alpha_of_image0   the extrapolation of every image takes image 0's alpha
      sums_over_group   the inner products run over the whole group: one quotient for all images
      shared_g_plane    the images share one plane for g: every direction pass reads the old g the group's last image left
      previous_group_u  from the second group on, the extrapolation reads the u_(k-1) the slot held for the previous group"""
    n = len(u0)
    u = [np.asarray(x, dtype=np.float64) for x in u0]
    u_prev, g1, g2 = [None] * n, [None] * n, [None] * n
    stale = dict(held) if held is not None and fault == "previous_group_u" else {}
    alphas = np.zeros((n, iterations))
    for k in range(iterations):
        al = [0.0] * n
        if k >= 2:
            old = [g2[n - 1] if fault == "shared_g_plane" else g2[i] for i in range(n)]
            num = [float(np.sum(g1[i] * old[i])) for i in range(n)]
            den = [float(np.sum(old[i] * old[i])) for i in range(n)]
            if fault == "sums_over_group":
                num, den = [sum(num)] * n, [sum(den)] * n
            al = [_alpha(num[i], den[i]) for i in range(n)]
        alphas[:, k] = al
        y = []
        for i in range(n):
            a = al[0] if fault == "alpha_of_image0" else al[i]
            if k >= 2 and a != 0.0:
                y.append(np.maximum(u[i] + a * (u[i] - stale.get(i, u_prev[i])), 0))
            else:
                y.append(u[i])
        nxt = [steps[i](y[i]) for i in range(n)]
        for i in range(n):
            g2[i], g1[i] = g1[i], nxt[i] - y[i]
            u_prev[i], u[i] = u[i], nxt[i]
    if held is not None:
        for i in range(n):
            if u_prev[i] is not None:
                held[i] = u_prev[i]
    return u, alphas


def batched_call(form, flat_in, lay, olay, al, psf, M, N, iterations, area, group, weights=None, sigma=SIGMA, fault=None):
    """The batched accelerated call in float64: (flat output, flat alphas), both SENTINEL outside their windows.  `fault`: one of
    FAULTS -- the four of group_recursion, and
      ignore_alpha_pitch  image i's alphas are stored at i * iterations
      drop_last_group     a last group smaller than `group` is not run"""
    assert form in ("plain", "free") and (fault is None or fault in FAULTS) and al.n == iterations
    rows, cols = lay.rows, lay.cols
    out = bm.new_output(olay, np.float64)
    alphas = new_alphas(al, np.float64)
    held = {}
    i0 = 0
    for n in bm.launches(lay.count, group):
        if fault == "drop_last_group" and n < group and i0 > 0:
            break
        pairs = [start_and_step(form, np.asarray(bm._window(flat_in, (i0 + k) * lay.img_pitch, rows, cols, lay.stride), dtype=np.float64), psf,
                                M, N, weights, sigma) for k in range(n)]
        u, a = group_recursion([p[0] for p in pairs], [p[1] for p in pairs], iterations, fault, held)
        for k in range(n):
            bm._window(out, bm.out_base(olay, i0 + k), olay.rows, olay.cols, olay.out_stride)[...] = output_of(u[k], olay, area, M, N)
            base = al.lead + (i0 + k) * (iterations if fault == "ignore_alpha_pitch" else al.pitch)
            alphas[base: base + iterations] = a[k]
        i0 += n
    return out, alphas


# ---- the judge ------------------------------------------------------------------------------------------------------------
def judge(what, out, olay, alphas, al, ones, one_alphas, refs, ref_alphas, tol, alpha_tol, area):
    """One batch result (flat output, flat alphas) against the one-by-one results (`ones` [count, rows, cols], `one_alphas` [count, n]:
    bit for bit) and the float64 model (`refs`, `ref_alphas`: rb.error() within tol per image, max |alpha - model| within alpha_tol);
    NaN and inf fail; everything outside the output windows and outside the alphas must hold SENTINEL.  Verdict.checks names what
    failed: "bits", "model", "layout", "finite" for the images, "alpha_bits", "alpha_model", "alpha_layout", "alpha_finite"."""
    v = rb.judge(what, out, olay, ones, refs, tol, area)
    bad, checks, worst = list(v.bad), set(v.checks), v.worst
    if not alphas_outside_untouched(alphas, al):
        bad.append("%s: a value outside the alphas was overwritten (or an image's alphas are not where alpha_pitch puts them)" % what)
        checks.add("alpha_layout")
    got = unpack_alphas(alphas, al)
    worst_a = 0.0
    for i in range(al.count):
        if not np.all(np.isfinite(got[i])):
            bad.append("%s: the alphas of image %d hold NaN or inf" % (what, i))
            checks.add("alpha_finite")
        if not np.array_equal(got[i], one_alphas[i]):
            bad.append("%s: image %d: alphas %s differ from the single call's %s" % (what, i, got[i], one_alphas[i]))
            checks.add("alpha_bits")
        e = float(np.max(np.abs(got[i].astype(np.float64) - ref_alphas[i][:al.n]))) if al.n else 0.0
        worst_a = max(worst_a, e) if e == e and worst_a == worst_a else float("nan")
        if not e <= alpha_tol:
            bad.append("%s: image %d: alpha error %.3g > %.3g against the float64 model" % (what, i, e, alpha_tol))
            checks.add("alpha_model")
    return AccelVerdict(worst, worst_a, bad, checks)


AccelVerdict = collections.namedtuple("AccelVerdict", "worst worst_alpha bad checks")


def alphas_apart(ref_alphas, n, gap=1e-3):
    """every two images of the batch differ by at least `gap` in the model's alpha at some 2 <= k < n: without that, image 0's alpha
    on every image, or sums over the group, would go unseen"""
    a = np.asarray(ref_alphas)[:, 2:n]
    return all(float(np.max(np.abs(a[i] - a[j]))) >= gap for i in range(len(a)) for j in range(i + 1, len(a)))


# ---- the case list of test_rlaccel_batch_gpu.py ---------------------------------------------------------------------------
COUNT = 5
GROUPS = (2, 3, 4, 8, 1)             # 5 images: launches 2 2 1, 3 2, 4 1, 5 (count < group), and the loop of the single calls
ITERATIONS = (0, 1, 2, 3, 4, 7)      # both parities of `first`; the first extrapolation is at 3
RA_COLS, RA_ROWS = 1024, 8           # the tile of the acceleration kernels (kRaCols x kRaRows)

# form, plan M x N, window, loose layout (odd strides and pitches: the 16-byte path off), weights (free form), the M x N output
Scene = collections.namedtuple("Scene", "name form M N rows cols loose masked full_out")
SCENES = [Scene("plain 64x2048 win 61x1027 loose", "plain", 64, 2048, 61, 1027, True, False, False),
          Scene("plain 32x64 full tight", "plain", 32, 64, 32, 64, False, False, False),
          Scene("plain 128x256 win 100x200", "plain", 128, 256, 100, 200, False, False, False)]
for _M, _N, _r, _c in ((16, 2048, 11, 1500), (64, 64, 40, 50)):
    for _tag, _masked, _full in (("null weights", False, False), ("masked", True, False), ("out MxN", False, True)):
        SCENES.append(Scene("free %dx%d win %dx%d %s" % (_M, _N, _r, _c, _tag), "free", _M, _N, _r, _c, _full, _masked, _full))
SCENE_IDS = [s.name.replace(" ", "-") for s in SCENES]


def scene_psf(fdr_motion15, sc):
    """plain form: the motion PSF of test_rl_batch_gpu.py (top-left on the full window, centred on a cropped one); free form: the dense
    5 x 5 PSF that test_rlaccel_gpu.py holds to RLA_FREE_TOL (the thin motion PSF is held to the float32 CPU run there)"""
    if sc.form == "free":
        return dense_psf(5, 5)
    motion = bm.fit_psf(fdr_motion15, sc.M, sc.N)
    return motion if (sc.rows, sc.cols) == (sc.M, sc.N) else centred_psf(motion, sc.M, sc.N)


def scene_images(sc):
    """rb.images with a seed per plan (the plan's logarithms plus SEED_STEP).  The seed must give a scene that single precision can resolve at all: on a window of a few
    rows about every second seed puts a blurred estimate of some image next to the ratio's guard FDR_RL_TAU, where a last-bit
    difference in c switches r between d / c and 0, and then the float64 model run in float32 ON THE CPU is itself 1e-4 .. 1e-3 off
    the float64 run after 7 iterations.  test_rlaccel_batch_host.py holds every scene to resolvable(): that float32 CPU run within
    a quarter of the tolerance the GPU is held to, in the estimate and in the alphas."""
    return rb.images(sc.M, sc.N, sc.rows, sc.cols, COUNT, 1000 * bm.log2(sc.M) + bm.log2(sc.N) + SEED_STEP.get((sc.M, sc.N), 3))


# the first seed step from 3 on that gives a resolvable scene with the alphas apart (3 does on every plan but the 11-row window)
SEED_STEP = {(16, 2048): 4}


def resolvable(sc, psf, tol, alpha_tol):
    """(largest error of the float32 CPU run of the model against the float64 run at the largest iteration count over the images of
    the scene, estimate and alphas; whether both lie within a quarter of tol / alpha_tol)"""
    imgs, w, n = scene_images(sc), scene_mask(sc), max(ITERATIONS)
    worst, worst_a = 0.0, 0.0
    for d in imgs:
        k64, a64 = single_path(sc.form, d, psf, sc.M, sc.N, (n,), w)
        k32, a32 = single_path(sc.form, d, psf, sc.M, sc.N, (n,), w, dtype=np.float32)
        worst = max(worst, rb.error(k32[n], k64[n], NORM_NONE))
        worst_a = max(worst_a, float(np.max(np.abs(a32 - a64))))
    return worst, worst_a, worst <= tol / 4 and worst_a <= alpha_tol / 4


def scene_mask(sc):
    return rb.mask(sc.rows, sc.cols, sc.M + sc.N) if sc.masked else None


def scene_layouts(sc):
    lay = (bm.loose_layout if sc.loose else bm.tight_layout)(sc.rows, sc.cols, COUNT)
    return lay, (rb.out_layout(lay, sc.M, sc.N) if sc.full_out else lay)


def sum_window(sc):
    """the window the inner products run over: the data window (plain form), the whole plan (free form)"""
    return (sc.rows, sc.cols) if sc.form == "plain" else (sc.M, sc.N)


def vec_path(sc):
    """whether the 16-byte path of the acceleration kernels can be taken: every plane's stride a multiple of 4 (the plain form's
    estimate lives in the output window with out_stride; the free form's planes are dense M x N)"""
    lay, _ = scene_layouts(sc)
    return sc.form == "free" or (lay.out_stride % 4 == 0 and lay.cols % 4 == 0 and lay.out_pitch % 4 == 0 and lay.lead % 4 == 0)
