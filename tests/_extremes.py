"""Planted extremes for the min/max normalisation: pictures whose largest and smallest value sit on chosen pixels, an exact
transform-free reference for delta PSFs, fault models of the counted mask, and the case tables the host and GPU files share.

Every call ends in a min-max normalisation over the counted area: the rows x cols window (NORM_CROPPED) or the M x N plan
(NORM_PADDED).  With a random picture the extreme lies on a random pixel, so a mask that is off by one line passes nearly always.
Here the extremes are put on the lines where the masks end.  For the PSF delta_psf(r0, c0) the restored plane needs no transform:

    Z = roll(pad(img), (-r0, -c0)) / (1 + K)        pad(img): the picture top-left in an M x N plane of zeros

and the output is the window of Z, normalised by min and max of Z over the counted area.  Three deltas put a planted value
anywhere relative to the window: (0, 0) keeps it, (1, 1) sends picture row 0 / column 0 to plane row M-1 / column N-1, and
(M-1, N-1) sends picture row rows-1 / column cols-1 to plane row rows / column cols, just outside the window.
Pinned in test_extremes_host.py (against wiener_model, the CPU oracle and its own fault models) before it judges the GPU
(test_extremes_gpu.py)."""
import functools

import numpy as np

K = float(np.float32(0.01))
HI, LO = 1.0, 0.0625  # the planted values; the base lies in [0.375, 0.625), the padding is 0: three distinct levels below the base
NORM_CROPPED, NORM_PADDED = 0, 1

# Parity mode against delta_reference: 4x the largest max-abs the CPU oracle (the reference of parity mode, which the device
# matches bit for bit) shows against delta_reference over PARITY_CASES, every window, delta, position and area
# (test_extremes_host.py::test_oracle_against_delta_reference prints it).  Measured: 4.22e-5, on the 16384-point columns of
# parity-16384x8-long, whose twiddles come from the serial path's float recurrence; 1.1e-6 (6 x 10, naive DFT) and 2.0e-7 ..
# 6.7e-7 on the other plans.  A missed or extra extreme moves the output by more than 0.05 (the host file proves it).
PARITY_EDGE_TOL = 1.69e-4

FAULTS = ("drop_last_row", "drop_last_col", "drop_first_row", "drop_first_col", "extra_row", "extra_col", "cropped_counts_plan",
          "padded_counts_window", "drop_partial_group", "drop_col_tail", "drop_upper_half", "drop_nyquist_col", "drop_odd_row_tail")


@functools.lru_cache(maxsize=8)
def _base(rows, cols, seed):
    base = (0.375 + 0.25 * np.random.default_rng(seed).random((rows, cols))).astype(np.float32)
    base.setflags(write=False)
    return base


def planted(rows, cols, hi_at, lo_at, seed):
    """float32 rows x cols: 0.375 + 0.25 U[0, 1), HI at hi_at and LO at lo_at.  LO is above 0, so the zeros of the padding are a
    third level: PADDED takes its minimum from the padding, CROPPED must not.  Missing either spike moves the output by > 0.3."""
    img = _base(rows, cols, seed).copy()
    img[hi_at] = HI
    img[lo_at] = LO
    return img


def edge_positions(M, N, rows, cols):
    """The window pixels where a mask or an index formula can end: the four corners, the middle of the last row and of the last
    column, and in rows 0, rows/2, rows-1 the columns 0, cols-1, cols/2 and N/2-1, N/2, N/2+1 clipped to the window (the direct /
    mirrored split of the half spectrum).  Unique, in this order."""
    pos = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (rows - 1, cols // 2), (rows // 2, cols - 1)]
    for r in (0, rows // 2, rows - 1):
        for c in (0, cols - 1, cols // 2, N // 2 - 1, N // 2, N // 2 + 1):
            pos.append((r, min(max(c, 0), cols - 1)))
    return list(dict.fromkeys(pos))


def position_pairs(pos):
    """(hi_at, lo_at) for every entry of `pos`: hi_at walks the list, lo_at is the entry half a list further on"""
    n = len(pos)
    return [(pos[i], pos[(i + n // 2) % n]) for i in range(n)]


def deltas(M, N):
    return [(0, 0), (1 % M, 1 % N), (M - 1, N - 1)]


def _counted(M, N, rows, cols, cropped, fault):
    """(row indices, column indices) of the counted area; `fault` moves this mask only"""
    mr, mc = (rows, cols) if cropped else (M, N)
    if fault == "cropped_counts_plan" and cropped:
        mr, mc = M, N
    if fault == "padded_counts_window" and not cropped:
        mr, mc = rows, cols
    r, c = np.arange(mr), np.arange(mc)
    if fault == "drop_last_row":
        r = r[:-1]
    elif fault == "drop_last_col":
        c = c[:-1]
    elif fault == "drop_first_row":
        r = r[1:]
    elif fault == "drop_first_col":
        c = c[1:]
    elif fault == "extra_row":
        r = np.arange(min(mr + 1, M))
    elif fault == "extra_col":
        c = np.arange(min(mc + 1, N))
    elif fault == "drop_partial_group":  # the rows of a partial 4-row group
        r = r[:4 * (mr // 4)]
    elif fault == "drop_col_tail":       # the columns of a partial 4-column quad
        c = c[:4 * (mc // 4)]
    elif fault == "drop_upper_half":     # the mirrored half of the half spectrum's row pass
        c = c[c < N // 2]
    elif fault == "drop_nyquist_col":
        c = c[c != N // 2]
    elif fault == "drop_odd_row_tail":   # the half-empty last pair of a pass that handles real rows in pairs
        r = r[:mr - mr % 2]
    elif fault not in (None, "cropped_counts_plan", "padded_counts_window"):
        raise ValueError("unknown fault model %r" % (fault,))
    return r, c


def _scale(win, lo, hi):
    """the flat-plane rule of _rl_model.normalize: a flat (or empty) counted area gives all 0"""
    if not hi - lo > 2.2204460492503131e-16:
        return np.zeros_like(win)
    out = np.subtract(win, lo)
    out /= hi - lo
    return out


def delta_plane(img, r0, c0, K, M, N):
    """Z, float64 M x N"""
    rows, cols = np.shape(img)
    P = np.zeros((M, N))
    P[:rows, :cols] = img
    return np.roll(P, (-r0, -c0), axis=(0, 1)) / (1.0 + K)


def delta_reference(img, r0, c0, K, M, N, cropped, fault=None):
    """float64 rows x cols: the output of a Wiener call with the PSF delta_psf(r0, c0) on an M x N plan, normalised over the
    window (cropped) or the plan.  fault: one of FAULTS, for the CPU pins only."""
    rows, cols = np.shape(img)
    Z = delta_plane(img, r0, c0, K, M, N)
    r, c = _counted(M, N, rows, cols, cropped, fault)
    area = Z[np.ix_(r, c)]
    if area.size == 0:
        return np.zeros((rows, cols))
    return _scale(Z[:rows, :cols], float(area.min()), float(area.max()))


def _runs(n, shift, size):
    """(out start, out stop, source start) of the runs of window indices a < n whose source (a + shift) % size lies in the picture"""
    if n - shift > 0:
        yield 0, n - shift, shift
    if size - shift < n:
        yield size - shift, n, 0


def delta_references(img, r0, c0, K, M, N):
    """{NORM_CROPPED: ..., NORM_PADDED: ...} of delta_reference (no fault) without building the plane, for the GPU cases, which ask
    for both: the window of Z copied run by run, and min / max of Z over the plan from the picture's own and the zero of the
    padding (Z holds the values of pad(img), moved).  test_extremes_host.py holds it to the bits of delta_reference."""
    rows, cols = np.shape(img)
    win = np.zeros((rows, cols))
    for a0, a1, s0 in _runs(rows, r0, M):
        for b0, b1, t0 in _runs(cols, c0, N):
            win[a0:a1, b0:b1] = img[s0:s0 + a1 - a0, t0:t0 + b1 - b0]
    win /= 1.0 + K
    lo, hi = float(np.min(img)) / (1.0 + K), float(np.max(img)) / (1.0 + K)
    if rows < M or cols < N:
        lo, hi = min(lo, 0.0), max(hi, 0.0)
    return {NORM_CROPPED: _scale(win, float(win.min()), float(win.max())), NORM_PADDED: _scale(win, lo, hi)}


# ---- the case tables ------------------------------------------------------------------------------------------------------------
# (id, path, M, N, flag names, OPT_TWO_SWEEP_NORM or None, (a, b)): the smallest plans that reach each producer of the min/max.
# The window cropped on both sides is (M - a, N - b); windows() adds the two forms with one side full.  Over the table the row
# counts have rows % 4 in {1, 2, 3, 0} and the column counts cols % 4 in {1, 3, 0}.
FAST_CASES = [
    ("fast-8x32", "two-sweep", 8, 32, (), None, (3, 3)),
    ("fast-16x64", "two-sweep", 16, 64, (), None, (2, 1)),
    ("fast-8x4096", "two-sweep", 8, 4096, (), None, (1, 4)),
    ("fast-8x8192", "two-sweep", 8, 8192, (), None, (3, 1)),
    ("fast-8x256-split", "split", 8, 256, (), None, (3, 3)),
    ("fast-16x2048-split", "split", 16, 2048, (), None, (1, 4)),
    ("fast-4096x256-packed", "packed-at-split-N", 4096, 256, (), None, (3, 3)),   # M > 2048: packed kernels at the split kernels' N
    ("fast-8x32-one-sweep", "one-sweep", 8, 32, (), 0, (2, 4)),
    ("fast-8x16", "one-sweep", 8, 16, (), None, (1, 1)),
    ("fast-8x32-full", "full-spectrum", 8, 32, ("FLAG_FULL_SPECTRUM",), None, (3, 3)),
    ("fast-12x20-mixed", "mixed-radix", 12, 20, ("FLAG_MIXED_RADIX",), None, (1, 3)),
    ("fast-15x20-mixed", "mixed-radix", 15, 20, ("FLAG_MIXED_RADIX",), None, (2, 1)),  # odd M: the last real pair is half empty
    ("fast-4x64-simple", "simple", 4, 64, (), None, (1, 3)),
    ("fast-64x4-simple", "simple", 64, 4, (), None, (3, 1)),
    ("fast-8x8-simple-flag", "simple", 8, 8, ("FLAG_SIMPLE_PATH",), None, (2, 3)),
    ("fast-8192x4-simple", "simple", 8192, 4, (), None, (3, 1)),       # more than 4096 partials: the separate reduce_minmax_kernel
    ("fast-16384x8-long", "simple", 16384, 8, (), None, (1, 3)),       # the long path
]
PARITY_CASES = [
    ("parity-8x8", "parity", 8, 8, (), None, (3, 1)),
    ("parity-16x64", "parity", 16, 64, (), None, (3, 3)),
    ("parity-4x4", "parity", 4, 4, (), None, (1, 1)),
    ("parity-8x8-simple-flag", "parity", 8, 8, ("FLAG_SIMPLE_PATH",), None, (2, 3)),
    ("parity-6x10-any-size", "parity", 6, 10, ("FLAG_ANY_SIZE",), None, (1, 3)),
    ("parity-16384x8-long", "parity", 16384, 8, (), None, (3, 1)),
]


def windows(case):
    """the three forms of a case's window: both sides cropped, rows == M with cols < N, cols == N with rows < M"""
    _id, _path, M, N, _flags, _two, (a, b) = case
    return [(M - a, N - b), (M, N - b), (M - a, N)]


def combos(case):
    """every (rows, cols, (r0, c0), hi_at, lo_at) of a case; each is one device call per norm area"""
    M, N = case[2], case[3]
    for rows, cols in windows(case):
        pairs = position_pairs(edge_positions(M, N, rows, cols))
        for r0, c0 in deltas(M, N):
            for hi_at, lo_at in pairs:
                yield rows, cols, (r0, c0), hi_at, lo_at


def seed_of(rows, cols):
    """one base picture per window size: only the planted values move"""
    return rows * 8191 + cols


def oracle_reference(oracle, img, psf, K, M, N):
    """{NORM_CROPPED: ..., NORM_PADDED: ...} from the CPU oracle on the M x N plan, in one run: the picture padded to the plan, the
    oracle's result (normalised over the plan) cropped, and its raw plane cropped and normalised by the oracle over the window.
    Where the plan is the next power of two of the window the PADDED form is what oracle.serial_channel computes, by the same
    steps (test_extremes_host.py compares the bits)."""
    rows, cols = img.shape
    padded = np.zeros((M, N), dtype=np.float32)
    padded[:rows, :cols] = img
    out, raw = oracle.wiener(padded, psf, K, want_raw=True)
    return {NORM_CROPPED: oracle.normalize_minmax(np.ascontiguousarray(raw[:rows, :cols])), NORM_PADDED: out[:rows, :cols].copy()}


def log(path, what, worst, tol, calls):
    print("EXTREMES\t%s\t%s\tmax=%.3g\ttol=%.3g\tcalls=%d" % (path, what, worst, tol, calls))
