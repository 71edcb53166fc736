"""Batched Wiener launches (fdr_wiener_batch_f32_dev + fdr_plan_set_batching): which kernel a group of images runs and how deep
its persistent loops go, restated from the launchers as plain Python; the images, buffer layouts and judge that
test_batch_lengths_gpu.py uses; a float64 batched operator with fault models that test_batch_host.py turns against that judge;
and the case lists of both files, as data.

A group of 2 .. 8 images does not run the kernels one image runs (csrc file : line of what each function below mirrors):

    column pass B' (launch_cols_panel_t, fdr_panel_cols.hip:639-676)
      M = 8 .. 128     persistent radix-8 kernel for one image and for a group; the tile sequence runs across the images
      M = 256, 512     one image: split kernel (:651-657); a group: the persistent radix-8 kernel (:665-671)
      M = 1024, 2048   one image: split kernel; a group: fused16 (:658-664)
      M = 4096, 8192   fused16 for both; a group adds the image dimension
      fused16: 2, 4 or 8 images and a tile count divisible by 8 take a flat grid (img_shift), everything else (tiles, images) (:661-662)
    row passes (launch_rows4_fwd_t, fdr_panel_rows.hip:574-620; launch_rows4_inv_kind, :1243-1262)
      N = 256 .. 2048, M <= 2048, half spectrum: one image split kernels, a group the packed kernels, blockIdx.y = image (:62-64)
      N = 8192         forward: the persistent kernel, its group sequence over groups * images (:592-612)
    full spectrum: pass B' takes the group, the row passes run image by image (panel_group, fdr_api_wiener.hip:200-209)
"""
import collections

import numpy as np

from _mixed_model import wiener_raw
from _spectral import SPATIAL_TOL, max_abs, tone_image

K32 = float(np.float32(0.01))
NORM_CROPPED, NORM_PADDED = 0, 1
AREAS = (NORM_CROPPED, NORM_PADDED)
AREA_NAME = {NORM_CROPPED: "CROPPED", NORM_PADDED: "PADDED"}
FLAG_FULL_SPECTRUM = 32  # include/fdr.h FDR_FLAG_FULL_SPECTRUM
SENTINEL = -7.0          # what every output buffer holds before a call
GARBAGE = 1.0e6          # what the input's pitch gap and stride padding hold: far above any pixel (|tone_image| < 10, times 2^10, plus 1)
SLACK = 32               # floats in front of and behind the output images (a multiple of 4: the images keep their 16-byte alignment)
NUM_CU = 256             # MI355X; the launchers' own default where the device does not say (fdr_panel_cols.hip:667)


# ---- launch geometry -------------------------------------------------------------------------------------------------------
def log2(n):
    l = int(n).bit_length() - 1
    assert n == 1 << l, "%r is no power of two" % (n,)
    return l


def steps_t(logl, logv=3):
    """Steps<LOGL, LOGV>::T, threads per transform (fdr_fft_core.hpp:73-74)"""
    return 1 << (logl - logv if logl >= logv else 0)


def steps_buf(logl):
    """Steps::BUF, float2 elements of one exchange buffer (fdr_fft_core.hpp:85)"""
    L = 1 << logl
    return L + (L >> 3) + 8


PanelGeom = collections.namedtuple("PanelGeom", "T G THREADS PIPE_WG_PER_CU")


def panel_geom(M):
    """PanelGeom<LOGM> of the persistent radix-8 kernel (fdr_panel.hpp:34-39)"""
    T = steps_t(log2(M))
    G = 1 if T >= 512 else (2 if T >= 256 else 4)
    threads = T * G
    return PanelGeom(T, G, threads, 1 if threads >= 512 else 512 // threads)


def is_half(N, full):
    """the half-spectrum path (layout_radix2, fdr_api_plan.hip:163)"""
    return N >= 32 and not full


def npanels(N, full):
    """panels of 4 spectrum columns: N/8 on the half-spectrum path, N/4 otherwise (fdr_api_plan.hip:176)"""
    return N // 8 if is_half(N, full) else N // 4


def cols_tiles(M, N, full=False):
    """tiles of pass B' per image: PanelGeom::G panels each for the radix-8 kernel (fdr_panel_cols.hip:643), one panel each for fused16
    (Panel16Geom::G = 1, :341, :660) and the split kernel (:653)"""
    np_ = npanels(N, full)
    if M >= 1024:
        return np_
    G = panel_geom(M).G
    return (np_ + G - 1) // G


def cols_kernel(M, nimg, N=64, full=False):
    """the kernel of pass B' for a launch of nimg images: "split", "radix8-persistent", "fused16-flat" or "fused16-2d"
    (fdr_panel_cols.hip:651-671; N and full decide the tile count, on which the fused16 grid depends, :661)"""
    logm = log2(M)
    assert 3 <= logm <= 13 and 1 <= nimg <= 8
    if 8 <= logm <= 11 and nimg == 1:
        return "split"
    if logm >= 10:
        flat = npanels(N, full) % 8 == 0 and nimg in (2, 4, 8)
        return "fused16-flat" if flat else "fused16-2d"
    return "radix8-persistent"


def persistent_grid(M, N, nimg, full=False, num_cu=NUM_CU):
    """workgroups of the persistent radix-8 kernel: num_cu * PIPE_WG_PER_CU, at most one per tile (fdr_panel_cols.hip:666-668)"""
    return min(num_cu * panel_geom(M).PIPE_WG_PER_CU, cols_tiles(M, N, full) * nimg)


def _depth(total, grid):
    return total // grid, (total + grid - 1) // grid


def tiles_per_workgroup(M, N, nimg, full=False, num_cu=NUM_CU):
    """(min, max) tiles that one workgroup of pass B' handles: workgroup b of the persistent kernel takes the tiles b, b + grid, ...
    of ntiles * nimg (fdr_panel_cols.hip:256-257, 277-280); the split and fused16 kernels take one"""
    if cols_kernel(M, nimg, N, full) != "radix8-persistent":
        return 1, 1
    return _depth(cols_tiles(M, N, full) * nimg, persistent_grid(M, N, nimg, full, num_cu))


def rows4_use_split(N, M, nimg, half):
    """rows4_use_split (fdr_panel_rows.hip:62-64)"""
    return nimg <= 1 and half and 8 <= log2(N) <= 11 and M % 4 == 0 and 0 < M <= 2048


ROWS_FWD_PERS_MIN_LOG = 13  # kRowsFwdPersMinLog (fdr_panel_rows.hip:315)


def rows_pers_wg_per_cu(N):
    """RowsPersGeom<LOGL, 4>::WG_PER_CU (fdr_panel_rows.hip:320-327)"""
    threads = steps_t(log2(N), 4)
    by_lds = (160 * 1024) // (2 * steps_buf(log2(N)) * 8)
    by_regs = 2 * 256 // threads
    return max(min(by_lds, by_regs), 1)


def rows_launch_images(N, nimg, full=False):
    """images per row-pass launch: the group on the half-spectrum path, one on the full spectrum (fdr_api_wiener.hip:202)"""
    return nimg if is_half(N, full) else 1


def rows_fwd_kernel(M, N, nimg, full=False):
    """the kernel of pass A: "split", "persistent" or "packed" (launch_rows4_fwd_t, fdr_panel_rows.hip:583-618)"""
    n = rows_launch_images(N, nimg, full)
    if rows4_use_split(N, M, n, is_half(N, full)):
        return "split"
    if log2(N) >= ROWS_FWD_PERS_MIN_LOG and M % 4 == 0:
        return "persistent"
    return "packed"


def rows_fwd_groups_per_workgroup(M, N, nimg, num_cu=NUM_CU, full=False):
    """(min, max) 4-row groups that one workgroup of pass A handles: the persistent kernel walks groups * images on
    num_cu * WG_PER_CU workgroups (fdr_panel_rows.hip:595-598, 345-348); the other kernels take one"""
    if rows_fwd_kernel(M, N, nimg, full) != "persistent":
        return 1, 1
    total = ((M + 3) // 4) * rows_launch_images(N, nimg, full)
    return _depth(total, min(num_cu * rows_pers_wg_per_cu(N), total))


def launches(count, group):
    """images per launch of one batch call (batch_enqueue, fdr_api_wiener.hip:333-334)"""
    return [min(group, count - i0) for i0 in range(0, count, group)]


def spectrum_bytes(M, N, full=False):
    """Plan.filter_bytes(): npanels panels of 4 M + 16 float2 (fdr_api_plan.hip:175-177)"""
    return npanels(N, full) * (4 * M + 16) * 8


def ce_chunk(spec_bytes, chunk_mb, n, nstreams):
    """images per C1 + C2 launch pair of a group of n (batch_enqueue, fdr_api_wiener.hip:352-359): n = no split"""
    chunk_bytes = chunk_mb << 20
    if nstreams > 1 and 0 < chunk_bytes and spec_bytes <= chunk_bytes and chunk_bytes // spec_bytes < n:
        return chunk_bytes // spec_bytes
    return n


# ---- inputs, layouts ------------------------------------------------------------------------------------------------------
def fit_psf(psf, M, N):
    """a PSF larger than the plan cut to its central window and renormalised (as _fit of test_fast_spectral_gpu.py)"""
    r, c = psf.shape
    if r <= M and c <= N:
        return psf
    r0, c0 = (r - min(r, M)) // 2, (c - min(c, N)) // 2
    h = psf[r0:r0 + min(r, M), c0:c0 + min(c, N)].astype(np.float64)
    return (h / h.sum()).astype(np.float32)


def batch_images(M, N, rows, cols, count, seed):
    """float32 [count, rows, cols]: image i is tone_image with its own seed, times 2^i, plus 0.1 i.  Every image has its largest and
    its smallest value on pixels of its own and a range of its own, so a min/max partial or a tile taken from a neighbour changes
    the normalised result (test_batch_host.py asserts both).  Where a small window puts an extreme of image i on the pixel of an
    earlier image's, image i takes the next seed."""
    imgs, his, los = [], set(), set()
    for i in range(count):
        s = seed + 7919 * i
        while True:
            img = tone_image(M, N, s, rows=rows, cols=cols)
            hi, lo = int(np.argmax(img)), int(np.argmin(img))
            if hi not in his and lo not in los:
                break
            s += 1
        his.add(hi)
        los.add(lo)
        imgs.append(img * np.float32(2.0 ** i) + np.float32(0.1 * i))
    return np.stack(imgs)


Layout = collections.namedtuple("Layout", "rows cols count stride out_stride img_pitch out_pitch lead tail")


def tight_layout(rows, cols, count):
    return Layout(rows, cols, count, cols, cols, rows * cols, rows * cols, SLACK, SLACK)


def loose_layout(rows, cols, count):
    """a row stride and an image pitch of their own for input and output, none a multiple of 4"""
    stride, out_stride = cols + 7, cols + 13
    return Layout(rows, cols, count, stride, out_stride, rows * stride + 5, rows * out_stride + 3, SLACK + 1, SLACK)


def in_size(lay):
    return lay.count * lay.img_pitch


def out_size(lay):
    return lay.lead + lay.count * lay.out_pitch + lay.tail


def _window(flat, base, rows, cols, stride):
    return np.lib.stride_tricks.as_strided(flat[base:], shape=(rows, cols), strides=(flat.itemsize * stride, flat.itemsize))


def pack_inputs(imgs, lay):
    """the flat input buffer: image i at i * img_pitch, its rows `stride` apart, everything else GARBAGE"""
    flat = np.full(in_size(lay), GARBAGE, dtype=np.asarray(imgs).dtype)
    for i in range(lay.count):
        _window(flat, i * lay.img_pitch, lay.rows, lay.cols, lay.stride)[...] = imgs[i]
    return flat


def new_output(lay, dtype=np.float32):
    return np.full(out_size(lay), SENTINEL, dtype=dtype)


def out_base(lay, i):
    return lay.lead + i * lay.out_pitch


def unpack(out, lay):
    """[count, rows, cols] copies of the output windows"""
    return np.stack([_window(out, out_base(lay, i), lay.rows, lay.cols, lay.out_stride).copy() for i in range(lay.count)])


def outside_untouched(out, lay):
    """everything but the windows still holds SENTINEL: the stride padding, the pitch gap, the slack in front and behind"""
    if lay.out_stride == lay.cols and lay.out_pitch == lay.rows * lay.cols:  # the windows are one block
        return bool(np.all(out[:lay.lead] == SENTINEL) and np.all(out[lay.lead + lay.count * lay.out_pitch:] == SENTINEL))
    rest = np.array(out, copy=True)
    for i in range(lay.count):
        _window(rest, out_base(lay, i), lay.rows, lay.cols, lay.out_stride)[...] = SENTINEL
    return bool(np.all(rest == SENTINEL))


# ---- reference and judge --------------------------------------------------------------------------------------------------
def references(imgs, psf, K, M, N):
    """{area: [count, rows, cols] float64}: wiener_model of every image, both normalisation areas from one raw plane
    (test_batch_host.py pins this against wiener_model itself, ==)"""
    out = {NORM_CROPPED: [], NORM_PADDED: []}
    for img in imgs:
        rows, cols = img.shape
        raw = wiener_raw(img, psf, K, M, N)
        win = raw[:rows, :cols]
        for area, a in ((NORM_CROPPED, win), (NORM_PADDED, raw)):
            lo, hi = a.min(), a.max()
            out[area].append((win - lo) / (hi - lo) if hi > lo else np.zeros_like(win))
    return {a: np.stack(v) for a, v in out.items()}


Verdict = collections.namedtuple("Verdict", "worst bad checks")  # checks: which of "bits", "model", "layout", "finite" failed


def model_errors(imgs, refs):
    """max-abs of every image against its float64 reference"""
    return [max_abs(a, b) for a, b in zip(imgs, refs)]


def judge(what, out, lay, ones, refs, tol=SPATIAL_TOL, ones_err=None):
    """One batch result (the flat output buffer) against the one-by-one results `ones` (bit for bit) and the float64 model `refs`
    (max-abs within tol, per image); NaN and inf fail; everything outside the windows must hold SENTINEL.  ones_err:
    model_errors(ones, refs) where the caller has them -- an image that equals `ones` bit for bit has that error."""
    got = unpack(out, lay)
    bad, checks, worst = [], set(), 0.0
    if not outside_untouched(out, lay):
        bad.append("%s: a value outside the output windows was overwritten" % what)
        checks.add("layout")
    for i in range(lay.count):
        if not np.all(np.isfinite(got[i])):
            bad.append("%s: image %d holds NaN or inf" % (what, i))
            checks.add("finite")
        n = int(np.count_nonzero(~(got[i] == ones[i])))
        if n:
            bad.append("%s: image %d: %d of %d values differ from the image restored alone" % (what, i, n, got[i].size))
            checks.add("bits")
        sp = max_abs(got[i], refs[i]) if n or ones_err is None else ones_err[i]
        worst = max(worst, sp) if sp == sp and worst == worst else float("nan")
        if not sp <= tol:
            bad.append("%s: image %d: max-abs %.3g > %.3g against the float64 model" % (what, i, sp, tol))
            checks.add("model")
    return Verdict(worst, bad, checks)


def log(lst, what, worst, tol, calls):
    print("BATCH\t%s\t%s\tmax-abs=%.3g\ttol=%.3g\tbatch calls=%d" % (lst, what, worst, tol, calls))


# ---- float64 batched operator with fault models (test_batch_host.py) -------------------------------------------------------
FAULTS = ("boundary_reads_image0", "minmax_of_previous", "ignore_img_pitch", "ignore_out_stride", "drop_last_tile")


def batched_operator(flat_in, lay, psf, K, M, N, area, group, grid, full=False, fault=None):
    """The batch call in float64 with the structure of the device's: launches of `group` images (launches()); per launch pass A
    (every image read through img_pitch and stride, padded, transformed), pass B' as tiles of 4 G spectrum columns handed to
    `grid` persistent workgroups (workgroup b: global tiles b, b + grid, ... of ntiles * n, global tile = image * ntiles + tile; the
    Nyquist column of the half spectrum travels in tile 0, where the device packs it), the inverse transform, min/max over the
    area, normalisation, and the store through out_pitch and out_stride into a SENTINEL-filled buffer.  `fault`: one of FAULTS.
      boundary_reads_image0  the tile a workgroup reaches by stepping over an image boundary reads image 0's spectrum
      minmax_of_previous     image k >= 1 of a launch is normalised with the extremes of image k - 1
      ignore_img_pitch       image i is read at i * rows * stride
      ignore_out_stride      output rows are stored cols apart
      drop_last_tile         the last tile of a sequence of two or more is not processed (its columns keep the unfiltered spectrum)"""
    assert fault is None or fault in FAULTS
    rows, cols = lay.rows, lay.cols
    half = is_half(N, full)
    h = np.zeros((M, N))
    h[:psf.shape[0], :psf.shape[1]] = psf
    H = np.fft.rfft2(h) if half else np.fft.fft2(h)
    W = np.conj(H) / (np.abs(H) ** 2 + K)
    width = 4 * panel_geom(M).G
    ncols = N // 2 if half else N
    ntiles = (ncols + width - 1) // width
    assert ntiles == cols_tiles(M, N, full) or M >= 1024

    def columns(tl):
        c = list(range(tl * width, min((tl + 1) * width, ncols)))
        return c + [N // 2] if half and tl == 0 else c

    out = new_output(lay, np.float64)
    i0 = 0
    for n in launches(lay.count, group):
        F = []
        for k in range(n):  # pass A
            base = (i0 + k) * (rows * lay.stride if fault == "ignore_img_pitch" else lay.img_pitch)
            f = np.zeros((M, N))
            f[:rows, :cols] = _window(flat_in, base, rows, cols, lay.stride)
            F.append(np.fft.rfft2(f) if half else np.fft.fft2(f))
        Z = [f.copy() for f in F]
        total, g = ntiles * n, min(grid, ntiles * n)
        for b in range(g):  # pass B'
            seq = list(range(b, total, g))
            prev = None
            for j, t in enumerate(seq):
                img, tl = divmod(t, ntiles)
                src = 0 if fault == "boundary_reads_image0" and prev is not None and prev != img else img
                prev = img
                if fault == "drop_last_tile" and len(seq) > 1 and j == len(seq) - 1:
                    continue
                c = columns(tl)
                Z[img][:, c] = F[src][:, c] * W[:, c]
        mm = []
        for k in range(n):  # passes C + E
            raw = np.fft.irfft2(Z[k], s=(M, N)) if half else np.real(np.fft.ifft2(Z[k]))
            a = raw[:rows, :cols] if area == NORM_CROPPED else raw
            mm.append((a.min(), a.max()))
            lo, hi = mm[k - 1] if fault == "minmax_of_previous" and k >= 1 else mm[k]
            win = (raw[:rows, :cols] - lo) / (hi - lo)
            _window(out, out_base(lay, i0 + k), rows, cols, cols if fault == "ignore_out_stride" else lay.out_stride)[...] = win
        i0 += n
    return out


# ---- the case lists (test_batch_lengths_gpu.py runs them, test_batch_host.py reasons about them) ----------------------------
# (nstreams, group): with COUNT images, launches of 2, 3, 4, 5 and 8 images and tails of 1, 2 and 3
GROUPINGS = [(1, 2), (1, 3), (1, 4), (1, 5), (1, 8), (2, 4)]
COUNT = 11
ONE_SWEEP_M = (8, 512, 4096)  # FDR_OPT_TWO_SWEEP_NORM = 0 as well

# 1. column lengths: (M, N).  N = 64: 8 fused16 tiles, the flat grid at 2, 4 and 8 images; N = 32: 4 tiles, always (tiles, images)
COLUMN_PLANS = [(1 << l, 64) for l in range(3, 14)] + [(1 << l, 32) for l in range(10, 14)]
# 2. row lengths
ROW_PLANS = [(16, 1 << l) for l in range(5, 14)] + [(2048, 256), (2048, 2048)]


def short_window(M, N):
    return M - 1, N - 3


# 3. tile loops: (M, N, flags, group, count, tiles per workgroup (min, max) on 256 CUs)
TILE_CASES = [(512, 8192, 0, 8, 8, (4, 4)),
              (512, 8192, 0, 5, 5, (2, 3)),
              (256, 8192, 0, 8, 8, (2, 2)),
              (128, 8192, FLAG_FULL_SPECTRUM, 8, 8, (2, 2))]
TILE_SECOND = (2, 4, 8)  # every tile case also on (nstreams, group) = (2, 4) with 8 images

# 4. pitch and stride: (M, N, rows, cols, flags, FDR_OPT_TWO_SWEEP_NORM or None)
PITCH_CASES = [(256, 512, 201, 375, 0, None), (1024, 64, 999, 33, 0, None), (8, 8192, 7, 8191, 0, None), (4096, 32, 4001, 29, 0, None),
               (256, 512, 201, 375, FLAG_FULL_SPECTRUM, None), (8, 32, 7, 29, 0, 0)]
PITCH_GROUPINGS = [(1, 3), (2, 4), (1, 8)]
PITCH_COUNT = 9

# 5. chunks of passes C1 + C2: (M, N, FDR_OPT_CE_CHUNK_MB, images per chunk; None = no split).  One spectrum of 128 x 1024 is
# 128 panels of 528 float2 = 528 KiB: one image per MiB.  One of 256 x 1024 is 1040 KiB, 16 KiB (the panels' 16-element skew)
# more than a MiB, and batch_enqueue does not split a group whose single image is above the limit: pairs need 3 MiB there.
CHUNK_CASES = [(128, 1024, 1, 1), (256, 1024, 3, 2), (256, 1024, 1, None)]
CHUNK_GROUPINGS = [(2, 4), (2, 8)]
CHUNK_DEFAULT_MB = 160  # fdr_host.hpp:213
