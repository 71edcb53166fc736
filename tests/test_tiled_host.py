"""Sectioned restoration on the host: the layout and the weight tables of tests/_tiled_model.py (properties over many sizes), the C
layout functions of libfdr.so against them, the float32 blend against a direct per-pixel sum, the quality of the float64 model on
the two scenes that motivated the call, and the fault models that the judge of test_tiled_gpu.py must tell apart from the right
one on that test's own inputs.  Prints `TILED` lines with the measured values (pytest -s)."""
import ctypes

import numpy as np
import pytest

import _tiled_model as tm
from _rl_model import centred_psf, psnr
from _rlfree_model import crop_scene, rlfree_model
from _rltv_model import line_psf

AXES = [(extent, T, O) for T in (1, 2, 3, 7, 8, 24, 40, 97, 160) for O in sorted({0, 1, T // 4, T // 2 - 1, T // 2}) if 0 <= O <= T // 2
        for extent in (1, 2, T - 1, T, T + 1, 2 * T - O, 2 * T - O + 1, 3 * T, 61, 131, 211, 384, 997) if extent >= 1]


def test_layout_properties():
    """every pixel covered, by at most three tiles, the normalised weights summing to 1 within 1e-6; one tile size; the last tile
    ends at the edge; real overlaps of at least O"""
    worst = 0.0
    for extent, T, O in AXES:
        ax = tm.axis(extent, T, O)
        n, win, step, last = ax
        org = [tm.origin(ax, a) for a in range(n)]
        assert org[0] == 0 and org[-1] + win == extent and win == min(T, extent), (extent, T, O)
        assert all(b > a for a, b in zip(org, org[1:])), (extent, T, O)
        assert all(a + win - b >= O for a, b in zip(org, org[1:])), (extent, T, O)  # real overlap (no gap either: O >= 0)
        if n > 1:
            assert n == -(-(extent - O) // (T - O)) and org[:-1] == [a * (T - O) for a in range(n - 1)], (extent, T, O)
        first, count, w, sums = tm.cover_table(ax, extent)
        assert count.min() >= 1 and count.max() <= tm.MAX_COVER, (extent, T, O, count.max())
        assert np.all(sums > 0)
        for y in range(extent):
            assert np.all(w[y, count[y]:] == 0) and np.all(w[y, :count[y]] >= 0)
        worst = max(worst, float(np.abs(w.astype(np.float64).sum(axis=1) - 1).max()))
    print("TILED\tlayout\t%d axes, worst |sum W - 1| = %.3g" % (len(AXES), worst))
    assert worst <= 1e-6


def test_three_fold_cover_exists_and_is_the_bound():
    """O = T / 2 with a shifted last tile covers some pixels three times: the bound the blend kernel relies on is reached, not exceeded"""
    ax = tm.axis(61, 24, 12)
    _, count, _, _ = tm.cover_table(ax, 61)
    assert count.max() == 3
    assert tm.cover_table(tm.axis(131, 40, 20), 131)[1].max() == 3


def test_c_layout_against_the_model(fdr):
    """fdr_tiled_layout_get and fdr_tiled_tile_origin (pure host: the library loads without a device) against the model"""
    checked = 0
    for rows, T, O in AXES[::3]:
        for cols, Tc, Oc in ((131, 40, 8), (33, 40, 20), (300, 40, 0)):
            for prows, pcols in ((5, 7), (1, 1)):
                prm = fdr.TiledParams.make(fdr.TILED_RL_FREE, (T, Tc), (O, Oc))
                lay = fdr.tiled_layout(rows, cols, prows, pcols, prm)
                assert tuple(lay[:6]) == tm.layout(rows, cols, prows, pcols, (T, Tc), (O, Oc)), (rows, cols, T, O)
                ar, ac = tm.axis(rows, T, O), tm.axis(cols, Tc, Oc)
                staging = 4 * ar[0] * ac[0] * ar[1] * ac[1]
                assert lay.work_bytes >= staging + 4 * lay.min_M * lay.min_N + 32 * (rows + cols) and lay.work_bytes % 256 == 0
                for a in sorted({0, ar[0] // 2, ar[0] - 1}):
                    for b in sorted({0, ac[0] - 1}):
                        assert fdr.tiled_tile_origin(rows, cols, prm, a, b) == (tm.origin(ar, a), tm.origin(ac, b))
                checked += 1
    assert checked > 100
    big = fdr.tiled_layout(12288, 12288, 15, 15, fdr.TiledParams.make(fdr.TILED_TV_FREE, 1024, 64))
    assert big[:6] == (13, 13, 1024, 1024, 2048, 2048)
    assert fdr.tiled_layout(100000, 9000, 31, 31, fdr.TiledParams.make(fdr.TILED_RL_FREE, 9000, 0))[4:6] == (8192, 8192)  # clamped


def test_c_layout_refusals(fdr):
    L = fdr.lib
    lay = fdr.TiledLayoutC()
    y, x = ctypes.c_int(), ctypes.c_int()
    good = fdr.TiledParams.make(fdr.TILED_RL_FREE, (24, 40), (8, 8))
    assert L.fdr_tiled_layout_get(50, 100, 5, 7, ctypes.byref(good), ctypes.byref(lay)) == 0
    for kw in (dict(tile=(0, 40)), dict(tile=(24, 0)), dict(overlap=(13, 8)), dict(overlap=(8, 21)), dict(overlap=(-1, 8)), dict(overlap=(8, -1))):
        prm = fdr.TiledParams.make(fdr.TILED_RL_FREE, kw.get("tile", (24, 40)), kw.get("overlap", (8, 8)))
        assert L.fdr_tiled_layout_get(50, 100, 5, 7, ctypes.byref(prm), ctypes.byref(lay)) == -1, kw
        assert L.fdr_tiled_tile_origin(50, 100, ctypes.byref(prm), 0, 0, ctypes.byref(y), ctypes.byref(x)) == -1, kw
    for args in ((0, 100, 5, 7), (50, 0, 5, 7), (50, 100, 0, 7), (50, 100, 5, 0)):
        assert L.fdr_tiled_layout_get(*args, ctypes.byref(good), ctypes.byref(lay)) == -1, args
    assert L.fdr_tiled_layout_get(50, 100, 5, 7, None, ctypes.byref(lay)) == -1
    assert L.fdr_tiled_layout_get(50, 100, 5, 7, ctypes.byref(good), None) == -1
    for a, b in ((-1, 0), (3, 0), (0, 3), (0, -1)):
        assert L.fdr_tiled_tile_origin(50, 100, ctypes.byref(good), a, b, ctypes.byref(y), ctypes.byref(x)) == -1, (a, b)
    assert L.fdr_tiled_tile_origin(50, 100, ctypes.byref(good), 2, 2, ctypes.byref(y), ctypes.byref(x)) == 0 and (y.value, x.value) == (26, 60)


def test_blend_is_the_stated_per_pixel_sum():
    """the tile-by-tile float32 blend of the model equals, bit for bit, the per-pixel sum written out as the header states it"""
    rng = np.random.default_rng(2)
    for rows, cols, ov in ((61, 131, (12, 20)), (50, 100, (8, 8)), (20, 33, (0, 0)), (100, 90, (0, 20))):
        ar, ac = tm.axis(rows, tm.TILE[0], ov[0]), tm.axis(cols, tm.TILE[1], ov[1])
        tiles = {(a, b): rng.standard_normal((ar[1], ac[1])).astype(np.float32) for a in range(ar[0]) for b in range(ac[0])}
        got = tm.blend(tiles, ar, ac, rows, cols)
        rf, rc, rw, _ = tm.cover_table(ar, rows)
        cf, cc, cw, _ = tm.cover_table(ac, cols)
        want = np.zeros((rows, cols), dtype=np.float32)
        for y in range(rows):
            for x in range(cols):
                acc = np.float32(0)
                for i in range(rc[y]):
                    a = rf[y] + i
                    for j in range(cc[x]):
                        b = cf[x] + j
                        acc = np.float32(acc + np.float32(np.float32(rw[y, i] * cw[x, j]) * tiles[(a, b)][y - tm.origin(ar, a), x - tm.origin(ac, b)]))
                want[y, x] = acc
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rows, cols, ov)
        ones = tm.blend({k: np.ones_like(v) for k, v in tiles.items()}, ar, ac, rows, cols, np.float64)
        assert np.abs(ones - 1).max() <= 2e-6  # a partition of unity in two dimensions


# ---- quality on the float64 model --------------------------------------------------------------------------------------------------
S, AT, WIN, NOISE, STEPS = 512, (60, 60), 384, 0.002, 30
QT = dict(method=tm.RL_FREE, tile=(160, 160), overlap=(48, 48), iterations=STEPS)
# Measured by this test's own run (float64 model): whole-picture free call 34.121 dB, tiled (160^2 windows on 256^2 plans, overlap
# 48, raised cosine) 34.103 dB: a gap of 0.018 dB, max |tiled - whole| = 0.0108; hard seams (overlap 0) 33.689 dB.  The bound is
# about twice the measured gap.
TILED_GAP_DB = 0.04
# Measured likewise on the scene whose blur length runs from 3 to 17 px across the columns (16 bands, linear partition of unity;
# blurred window 31.74 dB): the central PSF for every tile 28.75 dB, the PSF of each tile's centre 34.64 dB, a gain of 5.89 dB.  Half
# of it is asserted.
PER_TILE_GAIN_DB = 2.9


def _embed(k, size=17):
    p = np.zeros((size, size), dtype=np.float32)
    o = (size - k.shape[0]) // 2
    p[o:o + k.shape[0], o:o + k.shape[1]] = k
    return p


def _odd(length):
    return int(2 * round((length - 1) / 2) + 1)


@pytest.fixture(scope="module")
def scene():
    return crop_scene(S, 5)


def test_quality_tiled_against_whole(scene):
    psf = line_psf(15, 30.0)
    blurred = np.fft.irfft2(np.fft.rfft2(scene) * np.fft.rfft2(centred_psf(psf, S, S).astype(np.float64)), s=scene.shape)
    rng = np.random.default_rng(6)
    truth = scene[AT[0]:AT[0] + WIN, AT[1]:AT[1] + WIN]
    d = (blurred[AT[0]:AT[0] + WIN, AT[1]:AT[1] + WIN] + rng.normal(0, NOISE, truth.shape)).astype(np.float32)
    whole = rlfree_model(d, centred_psf(psf, 512, 512), 512, 512, STEPS)
    tiled = tm.tiled_model(d, psf, 256, 256, QT)
    seams = tm.tiled_model(d, psf, 256, 256, dict(QT, overlap=(0, 0)))
    pw, pt, ps = psnr(whole, truth), psnr(tiled, truth), psnr(seams, truth)
    print("TILED\tquality\tblurred %.2f dB, whole %.3f dB, tiled %.3f dB (gap %.3f dB, max abs %.4f), hard seams %.3f dB"
          % (psnr(d, truth), pw, pt, pw - pt, float(np.abs(tiled - whole).max()), ps))
    assert pw - pt <= TILED_GAP_DB
    assert pt - ps >= 0.2  # the overlap is what closes the gap


def test_quality_psf_per_tile(scene):
    sizes = [_odd(3 + 14 * k / 15) for k in range(16)]
    bands = [_embed(line_psf(s, 30.0)) for s in sizes]
    cent = AT[1] + (np.arange(16) + 0.5) * WIN / 16
    xs = np.arange(S)
    pos = np.clip((xs - cent[0]) / (cent[1] - cent[0]), 0, 15)
    lo = np.minimum(np.floor(pos).astype(int), 14)
    wts = np.zeros((16, S))
    wts[lo, xs] = 1 - (pos - lo)
    wts[lo + 1, xs] += pos - lo
    F = np.fft.rfft2(scene)
    blurred = sum(wts[k][None, :] * np.fft.irfft2(F * np.fft.rfft2(centred_psf(bands[k], S, S).astype(np.float64)), s=scene.shape) for k in range(16))
    rng = np.random.default_rng(7)
    truth = scene[AT[0]:AT[0] + WIN, AT[1]:AT[1] + WIN]
    d = (blurred[AT[0]:AT[0] + WIN, AT[1]:AT[1] + WIN] + rng.normal(0, NOISE, truth.shape)).astype(np.float32)
    one = tm.tiled_model(d, _embed(line_psf(sizes[8], 30.0)), 256, 256, QT)
    ax = tm.axis(WIN, 160, 48)
    psfs = []
    for a in range(ax[0]):
        for b in range(ax[0]):
            xc = AT[1] + tm.origin(ax, b) + 79.5
            psfs.append(_embed(line_psf(_odd(3 + 14 * float(np.clip((xc - cent[0]) / (cent[15] - cent[0]), 0, 1))), 30.0)))
    per = tm.tiled_model(d, np.stack(psfs), 256, 256, QT)
    p1, pp = psnr(one, truth), psnr(per, truth)
    print("TILED\tpsf per tile\tblurred %.2f dB, one central PSF %.2f dB, the PSF of each tile's centre %.2f dB (gain %.2f dB)"
          % (psnr(d, truth), p1, pp, pp - p1))
    assert pp - p1 >= PER_TILE_GAIN_DB


# ---- the judge: fault models on the inputs of test_tiled_gpu.py --------------------------------------------------------------------
# (method, picture, overlap, PSF shape, per-tile PSFs): a picture with a shifted last tile and three-fold coverage, and the large one
JUDGE_CASES = ((tm.RL_FREE, (61, 131), (12, 20), (5, 7), False), (tm.TV_FREE, (61, 131), (12, 20), (5, 7), False),
               (tm.RL_FREE, (50, 100), (8, 8), (5, 7), True), (tm.TV_FREE, (100, 300), (8, 8), (5, 7), False))
# every fault model lies at least this many tolerances of its method from the right model, on every case above, at n = 3
FAULT_MULTIPLE = 5.0


@pytest.mark.parametrize("case", JUDGE_CASES, ids=lambda c: "%s-%dx%d-o%d" % ("rl" if c[0] == tm.RL_FREE else "tv", c[1][0], c[1][1], c[2][0]))
def test_the_judge_tells_the_fault_models_apart(case):
    method, (rows, cols), ov, (pr, pc), per_tile = case
    tol = tm.RLFREE_TOL if method == tm.RL_FREE else tm.TVF_TOL
    img = tm.gpu_picture(rows, cols)
    prm = tm.method_params(method, 3, overlap=ov)
    lay = tm.layout(rows, cols, pr, pc, tm.TILE, ov)
    psfs = tm.gpu_psfs(lay[0] * lay[1], pr, pc) if per_tile else tm.gpu_psf(pr, pc)
    right = tm.tiled_model(img, psfs, *tm.PLAN, prm)
    f32 = tm.tiled_model(img, psfs, *tm.PLAN, prm, dtype=np.float32)
    assert tm.rel_err(f32, right) <= tol  # the arithmetic class of the device passes
    three = max(tm.cover_table(tm.axis(n, t, o), n)[1].max() for n, t, o in zip((rows, cols), tm.TILE, ov)) == 3
    line = []
    for fault in tm.FAULTS:
        e = tm.rel_err(tm.tiled_model(img, psfs, *tm.PLAN, prm, fault=fault), right)
        line.append("%s %.3g" % (fault, e / tol))
        if fault == "unnormalised" and not three:
            # where two tiles overlap the raised cosines are complementary, h(s) + h(1 - s) = 1, whatever the real overlap: the raw
            # weights are the normalised ones and the fault cannot show.  It shows where three tiles meet (the first two cases).
            assert e <= 1e-6, (fault, e)
            continue
        assert e >= FAULT_MULTIPLE * tol, (fault, e, tol)
    print("TILED\tjudge\t%s %dx%d overlap %s: errors in tolerances: %s" % ("RL" if method == tm.RL_FREE else "TV", rows, cols, ov, ", ".join(line)))
