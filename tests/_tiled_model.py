"""Model of sectioned restoration (fdr_restore_tiled_f32*; include/fdr.h): the specification.

Geometry per axis (integers): a picture of `extent` pixels, tile window T, overlap 0 <= O <= T / 2.  extent <= T: one tile of the
picture's extent.  Otherwise n = ceil((extent - O) / (T - O)) tiles of T pixels, tile a at y_a = min(a (T - O), extent - T).
Weights per axis (double, rounded to float32 once): h(s) = 0.5 - 0.5 cos(pi s) below 1, else 1; the raw weight of tile a at its
local position t is rise . fall, rise = h((t + 0.5) / O_a) with O_a the real overlap with tile a - 1 (1 for a = 0 or O_a = 0), fall
the same from the far end against tile a + 1; W_a(y) = w_a(y - y_a) / sum of the covering tiles' raw weights.
Blend (float32, every product and sum rounded on its own, from +0):

    out[y, x] = sum over covering a (outer, ascending), covering b (inner, ascending) of (Wy_a(y) Wx_b(x)) o_ab[y - y_a, x - x_b]

Tile (a, b) is the free-boundary model of its method (_rlfree_model.py / _tvfree_model.py) on its window, on the M x N tile plan,
with the tile's PSF centred (centred_psf of _rl_model.py).  Pinned in test_tiled_host.py before it judges the GPU
(test_tiled_gpu.py); the faults below are what the judge must tell apart from the right model."""
import math

import numpy as np

from _rl_model import NORM_CROPPED, NORM_NONE, centred_psf, normalize, smooth_image  # noqa: F401
from _rlfree_model import RLFREE_TOL, SIGMA, rlfree_model  # noqa: F401
from _tvfree_model import TVF_TOL, tvfree_model  # noqa: F401

RL_FREE, TV_FREE = 0, 1
MAX_COVER = 3
FAULTS = ("hard_seams", "unnormalised", "origin_off_by_one", "psf_not_centred", "last_tile_unshifted")


def axis(extent, T, O):
    """(n, win, step, last): n tiles of `win` pixels, tile a at min(a step, last)"""
    assert extent >= 1 and T >= 1 and 0 <= O <= T // 2
    if extent <= T:
        return 1, extent, 0, 0
    step = T - O
    return -(-(extent - O) // step), T, step, extent - T


def origin(ax, a):
    return min(a * ax[2], ax[3])


def next_pow2(n):
    return 1 << max(n - 1, 0).bit_length()


def layout(rows, cols, prows, pcols, tile, overlap):
    """what fdr_tiled_layout_get returns but work_bytes: tiles_r, tiles_c, win_rows, win_cols, min_M, min_N"""
    ar, ac = axis(rows, tile[0], overlap[0]), axis(cols, tile[1], overlap[1])
    return (ar[0], ac[0], ar[1], ac[1], min(max(next_pow2(min(ar[1] + prows - 1, 8192)), 8), 8192),
            min(max(next_pow2(min(ac[1] + pcols - 1, 8192)), 32), 8192))


def ramp(s):
    return 0.5 - 0.5 * math.cos(math.pi * s) if s < 1.0 else 1.0


def raw_weight(ax, a, t):
    n, win = ax[0], ax[1]
    w = 1.0
    if a > 0:
        o = origin(ax, a - 1) + win - origin(ax, a)
        if o > 0:
            w *= ramp((t + 0.5) / o)
    if a + 1 < n:
        o = origin(ax, a) + win - origin(ax, a + 1)
        if o > 0:
            w *= ramp((win - 1 - t + 0.5) / o)
    return w


def cover_table(ax, extent, fault=None):
    """per position: first covering tile, their count, the normalised float32 weights (extent x 3, 0 beyond the count) and the
    double sum of the raw weights.  fault 'hard_seams': the first covering tile alone, weight 1; 'unnormalised': the raw weights."""
    first = np.zeros(extent, dtype=np.int64)
    count = np.zeros(extent, dtype=np.int64)
    w = np.zeros((extent, MAX_COVER), dtype=np.float32)
    sums = np.zeros(extent)
    for y in range(extent):
        cover = [a for a in range(ax[0]) if origin(ax, a) <= y < origin(ax, a) + ax[1]]
        assert cover and cover == list(range(cover[0], cover[0] + len(cover)))
        raw = [raw_weight(ax, a, y - origin(ax, a)) for a in cover]
        s = 0.0
        for r in raw:
            s += r
        first[y], count[y], sums[y] = cover[0], len(cover), s
        for k, r in enumerate(raw):  # (more than MAX_COVER tiles would raise here)
            w[y, k] = np.float32((1.0 if k == 0 else 0.0) if fault == "hard_seams" else r if fault == "unnormalised" else r / s)
    return first, count, w, sums


def blend(tiles, ar, ac, rows, cols, dtype=np.float32, fault=None):
    """the blend of tiles[(a, b)] (win_rows x win_cols each) in `dtype`: float32 is the device's arithmetic, bit for bit.  Tiles
    are added in the order a outer, b inner, which is the order of every pixel's own sum.  fault 'origin_off_by_one': the staged rows
    read one row off; 'last_tile_unshifted': the last tile of an axis taken as lying at a (T - O)."""
    rf, rc, rw, _ = cover_table(ar, rows, fault)
    cf, cc, cw, _ = cover_table(ac, cols, fault)
    out = np.zeros((rows, cols), dtype=dtype)
    for a in range(ar[0]):
        ya = origin(ar, a)
        ys = np.arange(ya, ya + ar[1])
        wy = rw[ys, a - rf[ys]].astype(dtype)
        ty = np.clip(ys - a * ar[2], 0, ar[1] - 1) if fault == "last_tile_unshifted" else ys - ya
        if fault == "origin_off_by_one":
            ty = np.clip(ty + 1, 0, ar[1] - 1)
        for b in range(ac[0]):
            xb = origin(ac, b)
            xs = np.arange(xb, xb + ac[1])
            wx = cw[xs, b - cf[xs]].astype(dtype)
            tx = np.clip(xs - b * ac[2], 0, ac[1] - 1) if fault == "last_tile_unshifted" else xs - xb
            o = np.asarray(tiles[(a, b)], dtype=dtype)[np.ix_(ty, tx)]
            w = wy[:, None] * wx[None, :]
            out[ya:ya + ar[1], xb:xb + ac[1]] = out[ya:ya + ar[1], xb:xb + ac[1]] + w * o
    return out


def tile_psf(psfs, ac_n, a, b):
    psfs = np.asarray(psfs)
    if psfs.ndim == 2:
        return psfs
    return psfs[0] if psfs.shape[0] == 1 else psfs[a * ac_n + b]


def restore_tile(d, psf, M, N, prm, weights=None, dtype=np.float64, fault=None):
    """one tile window by its method's free-boundary model, the PSF centred in the plan"""
    plane = np.asarray(psf, dtype=np.float32) if fault == "psf_not_centred" else centred_psf(np.asarray(psf, dtype=np.float32), M, N)
    if prm["method"] == RL_FREE:
        return rlfree_model(d, plane, M, N, prm["iterations"], weights, prm.get("sigma", SIGMA), dtype=dtype)
    return tvfree_model(d, plane, M, N, prm["mu"], prm.get("rho", 2.0), prm["iterations"], weights, prm.get("nu", 0.0),
                        prm.get("anisotropic", False), prm.get("nonneg", False), dtype=dtype)


def tiled_tiles(img, psfs, M, N, prm, weights=None, dtype=np.float64, fault=None):
    """every tile's restored window: dict (a, b) -> array, and the two axes"""
    img = np.asarray(img)
    rows, cols = img.shape
    ar, ac = axis(rows, prm["tile"][0], prm["overlap"][0]), axis(cols, prm["tile"][1], prm["overlap"][1])
    assert M >= ar[1] + np.asarray(psfs).shape[-2] - 1 and N >= ac[1] + np.asarray(psfs).shape[-1] - 1
    tiles = {}
    for a in range(ar[0]):
        for b in range(ac[0]):
            y, x = origin(ar, a), origin(ac, b)
            w = None if weights is None else np.asarray(weights)[y:y + ar[1], x:x + ac[1]]
            tiles[(a, b)] = restore_tile(img[y:y + ar[1], x:x + ac[1]], tile_psf(psfs, ac[0], a, b), M, N, prm, w, dtype, fault)
    return tiles, ar, ac


def tiled_model(img, psfs, M, N, prm, weights=None, norm_area=NORM_NONE, dtype=np.float64, fault=None):
    """the output of fdr_restore_tiled_f32 in float64 (the weights are the float32 ones of the tables)"""
    assert fault is None or fault in FAULTS, fault
    tiles, ar, ac = tiled_tiles(img, psfs, M, N, prm, weights, dtype, fault)
    out = blend(tiles, ar, ac, img.shape[0], img.shape[1], np.float64, fault)
    return normalize(out, norm_area, M, N)


# ---- the inputs of test_tiled_gpu.py, which test_tiled_host.py judges the fault models on ----
PLAN = (32, 64)
TILE = (24, 40)
PICTURES = ((24, 40), (20, 33), (50, 100), (61, 131), (100, 300))
OVERLAPS = ((0, 0), (8, 8), (12, 20))


def gpu_picture(rows, cols, seed=11):
    """float32 positive picture with structure at every scale of the small tiles"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    img = 0.35 + 0.25 * np.sin(0.23 * yy + 0.5) * np.cos(0.17 * xx) + 0.15 * np.sin(0.05 * xx * yy / max(rows, 1))
    img += 0.2 * (((yy // 7) + (xx // 9)) % 2) + 0.02 * rng.standard_normal((rows, cols))
    return np.clip(img, 0.02, None).astype(np.float32)


def gpu_psf(prows, pcols, seed=3):
    rng = np.random.default_rng(seed + 100 * prows + pcols)
    k = rng.uniform(0.2, 1.0, (prows, pcols))
    return (k / k.sum()).astype(np.float32)


def gpu_psfs(count, prows, pcols):
    return np.stack([gpu_psf(prows, pcols, seed=3 + k) for k in range(count)])


def gpu_weights(rows, cols, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.random((rows, cols)) > 0.1).astype(np.float32)


def method_params(method, iterations, tile=TILE, overlap=(8, 8)):
    if method == RL_FREE:
        return dict(method=RL_FREE, tile=tile, overlap=overlap, iterations=iterations, sigma=SIGMA)
    return dict(method=TV_FREE, tile=tile, overlap=overlap, iterations=iterations, mu=50.0, rho=1.0, nu=3.0, anisotropic=False, nonneg=False)


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())
