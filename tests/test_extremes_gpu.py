"""Min/max normalisation at the window's edges on the MI355X, on every path that computes or applies it.

Pictures with a planted maximum and minimum (tests/_extremes.py) through delta PSFs, for which the normalised output is known
without a transform: the extremes walk the corners, the last row and column, the partial 4-row group and 4-column quad and the
direct / mirrored split of the half spectrum, and the three deltas move them inside, far outside and just outside the window.
Every call compares the whole output window with delta_reference, for NORM_CROPPED and NORM_PADDED; the host file proves that
each fault model of the counted mask moves some call of this table by more than 0.05.  Each case prints an `EXTREMES` line with
its largest error (pytest -s)."""
import ctypes

import numpy as np
import pytest

import _rl_model
from _extremes import (FAST_CASES, K, NORM_CROPPED, NORM_PADDED, PARITY_CASES, PARITY_EDGE_TOL, combos, delta_references, deltas,
                       edge_positions, log, oracle_reference, planted, position_pairs, seed_of, windows)
from _rlfree_model import RLFREE_TOL
from _spectral import BIN_TOL, SPATIAL_TOL, delta_psf, failures, max_abs
from _tv_model import TV_TOL

pytestmark = pytest.mark.gpu

AREAS = (NORM_CROPPED, NORM_PADDED)
AREA_NAME = {NORM_CROPPED: "CROPPED", NORM_PADDED: "PADDED", 2: "NONE"}
SENTINEL = -7.0
BY_ID = {c[0]: c for c in FAST_CASES + PARITY_CASES}


def _plan(fdr, case, graph=False):
    _id, _path, M, N, flags, two_sweep, _ab = case
    f = 0
    for name in flags:
        f |= getattr(fdr, name)
    p = fdr.Plan(M, N, fdr.MODE_PARITY if _path == "parity" else fdr.MODE_FAST, flags=f)
    if two_sweep is not None:
        p.set_option(fdr.OPT_TWO_SWEEP_NORM, two_sweep)
    if graph:
        p.set_option(fdr.OPT_BATCH_GRAPH, 1)
    return p


def _tol(case):
    return PARITY_EDGE_TOL if case[1] == "parity" else SPATIAL_TOL


def _judge(what, M, N, got, want, tol):
    """(max-abs, failure messages) of one output window: NaN, inf and values outside [0, 1 + tol] fail as well"""
    sp = max_abs(got, want)
    bad = failures(what, M, N, None, None, sp, BIN_TOL, tol)
    if not (float(np.min(got)) >= 0.0 and float(np.max(got)) <= 1.0 + tol):  # (NaN fails both, inf the second)
        bad.append("%s: output not finite or outside [0, 1 + %.3g] (min %r, max %r)" % (what, tol, float(np.min(got)), float(np.max(got))))
    return sp, bad


def _what(case, rows, cols, delta, hi_at, lo_at, area):
    return "%s window %dx%d delta %s hi %s lo %s %s" % (case[0], rows, cols, delta, hi_at, lo_at, AREA_NAME[area])


def _sweep(fdr, case, oracle=None):
    """every window, delta, position and area of a case through Plan.wiener; parity cases also bit for bit against the oracle"""
    M, N, tol = case[2], case[3], _tol(case)
    bad, worst, calls, psf_of = [], 0.0, 0, None
    with _plan(fdr, case) as p:
        for rows, cols, delta, hi_at, lo_at in combos(case):
            if psf_of != delta:
                psf = delta_psf(*delta)
                p.set_psf(psf, K)
                psf_of = delta
            img = planted(rows, cols, hi_at, lo_at, seed_of(rows, cols))
            refs = delta_references(img, delta[0], delta[1], K, M, N)
            orefs = oracle_reference(oracle, img, psf, K, M, N) if oracle is not None else None
            for area in AREAS:
                got = p.wiener(img, area)
                what = _what(case, rows, cols, delta, hi_at, lo_at, area)
                sp, b = _judge(what, M, N, got, refs[area], tol)
                if orefs is not None:
                    n = int(np.count_nonzero(~(got == orefs[area])))
                    if n:
                        b.append("%s: %d of %d values differ from the oracle's bits" % (what, n, got.size))
                bad += b
                worst = max(worst, sp) if sp == sp else sp
                calls += 1
    log(case[1], case[0], worst, tol, calls)
    assert not bad, "%d failures, the first:\n%s" % (len(bad), "\n".join(bad[:12]))


@pytest.mark.parametrize("case", FAST_CASES, ids=[c[0] for c in FAST_CASES])
def test_fast_extremes_at_the_window_edges(fdr, case):
    _sweep(fdr, case)


@pytest.mark.parametrize("case", PARITY_CASES, ids=[c[0] for c in PARITY_CASES])
def test_parity_extremes_at_the_window_edges(fdr, oracle, case):
    _sweep(fdr, case, oracle)


LAYOUT_IDS = ("fast-8x32", "fast-8x256-split", "parity-16x64")


@pytest.mark.parametrize("cid", LAYOUT_IDS)
def test_output_layout_keeps_everything_outside_the_window(fdr, cid):
    """wiener_dev into a buffer prefilled with a sentinel: out_stride of cols, cols + 1 and cols + 4, the output base at an offset
    of 0 and of 1 float, the case's windows and one with cols % 4 == 0 -- the vector and the scalar form of normalize_kernel,
    normalize_panels_kernel and the C2 store.  The window must match its reference, everything else must keep the sentinel."""
    import torch
    case = BY_ID[cid]
    M, N, tol = case[2], case[3], _tol(case)
    wins = windows(case) + [(M - 3, N - 4)]
    bad, worst, calls = [], 0.0, 0
    with _plan(fdr, case) as p:
        for delta in deltas(M, N):
            p.set_psf(delta_psf(*delta), K)
            for rows, cols in wins:
                for hi_at, lo_at in position_pairs(edge_positions(M, N, rows, cols))[::4]:
                    img = planted(rows, cols, hi_at, lo_at, seed_of(rows, cols))
                    refs = delta_references(img, delta[0], delta[1], K, M, N)
                    d_in = torch.from_numpy(img).cuda()
                    for stride in (cols, cols + 1, cols + 4):
                        for off in (0, 1):
                            for area in AREAS:
                                buf = torch.full((off + rows * stride + 5,), SENTINEL, dtype=torch.float32, device="cuda")
                                p.wiener_dev(d_in.data_ptr(), rows, cols, cols, buf.data_ptr() + 4 * off, stride, area)
                                torch.cuda.synchronize()
                                host = buf.cpu().numpy()
                                body = host[off:off + rows * stride].reshape(rows, stride)
                                what = _what(case, rows, cols, delta, hi_at, lo_at, area) + " stride %d offset %d" % (stride, off)
                                sp, b = _judge(what, M, N, body[:, :cols], refs[area], tol)
                                kept = np.all(body[:, cols:] == SENTINEL) and np.all(host[:off] == SENTINEL) and np.all(host[off + rows * stride:] == SENTINEL)
                                if not kept:
                                    b.append("%s: a value outside the window was overwritten" % what)
                                bad += b
                                worst = max(worst, sp) if sp == sp else sp
                                calls += 1
    log("layout", cid, worst, tol, calls)
    assert not bad, "%d failures, the first:\n%s" % (len(bad), "\n".join(bad[:12]))


@pytest.mark.parametrize("cid", ("fast-8x256-split", "fast-8x32", "parity-16x64"))
def test_partials_of_an_earlier_call_do_not_enter_the_next(fdr, cid):
    """One plan, a PADDED call on the full window with values scaled by 100 and a CROPPED call on the small window of a planted
    picture, in both orders: each result must match its own reference (the larger call leaves more partials behind)."""
    case = BY_ID[cid]
    M, N, tol = case[2], case[3], _tol(case)
    rows, cols = windows(case)[0]
    bad, worst, calls = [], 0.0, 0
    with _plan(fdr, case) as p:
        for delta in deltas(M, N):
            p.set_psf(delta_psf(*delta), K)
            full_pairs = position_pairs(edge_positions(M, N, M, N))
            for i, (hi_at, lo_at) in enumerate(position_pairs(edge_positions(M, N, rows, cols))):
                fhi, flo = full_pairs[i % len(full_pairs)]
                big = planted(M, N, fhi, flo, seed_of(M, N)) * np.float32(100.0)
                small = planted(rows, cols, hi_at, lo_at, seed_of(rows, cols))
                want_big = delta_references(big, delta[0], delta[1], K, M, N)[NORM_PADDED]
                want_small = delta_references(small, delta[0], delta[1], K, M, N)[NORM_CROPPED]
                for step in "ABBAB":
                    if step == "A":
                        got, want, what = p.wiener(big, NORM_PADDED), want_big, "full window x100 PADDED"
                    else:
                        got, want, what = p.wiener(small, NORM_CROPPED), want_small, _what(case, rows, cols, delta, hi_at, lo_at, NORM_CROPPED)
                    sp, b = _judge("%s delta %s, step %s of ABBAB: %s" % (cid, delta, step, what), M, N, got, want, tol)
                    bad += b
                    worst = max(worst, sp) if sp == sp else sp
                    calls += 1
    log("stale", cid, worst, tol, calls)
    assert not bad, "%d failures, the first:\n%s" % (len(bad), "\n".join(bad[:12]))


# (nstreams, group, FDR_OPT_BATCH_GRAPH)
BATCHINGS = [(1, 2, False), (1, 3, False), (1, 8, False), (2, 4, False), (1, 8, True)]
BATCH_COUNT = 10  # 2+2+2+2+2, 3+3+3+1, 8+2, 4+4+2


@pytest.mark.parametrize("batching", BATCHINGS, ids=["%dx%d%s" % (a, b, "-graph" if g else "") for a, b, g in BATCHINGS])
@pytest.mark.parametrize("cid", ("fast-8x32", "fast-8x256-split"))
def test_batches_each_image_against_its_own_reference(fdr, cid, batching):
    """wiener_batch_dev: image i is a planted picture scaled by 2^i with its extremes walking the position list, so a partial
    taken from a neighbour's buffer changes the result.  Each image against its own delta_reference, and the batch bit for bit
    against the one-by-one results."""
    import torch
    case = BY_ID[cid]
    M, N, tol = case[2], case[3], _tol(case)
    nstreams, group, graph = batching
    bad, worst, calls = [], 0.0, 0
    s = torch.cuda.current_stream().cuda_stream
    with _plan(fdr, case, graph) as p:
        p.set_batching(nstreams, group)
        for rows, cols in windows(case):
            pairs = position_pairs(edge_positions(M, N, rows, cols))
            d_in = torch.empty((BATCH_COUNT, rows, cols), dtype=torch.float32, device="cuda")
            d_out = torch.empty_like(d_in)
            for delta in deltas(M, N):
                p.set_psf(delta_psf(*delta), K)
                for start in range(0, len(pairs), BATCH_COUNT):
                    use = [pairs[(start + i) % len(pairs)] for i in range(BATCH_COUNT)]
                    imgs = np.stack([planted(rows, cols, hi, lo, seed_of(rows, cols) + i) * np.float32(2.0 ** i)
                                     for i, (hi, lo) in enumerate(use)])
                    refs = [delta_references(imgs[i], delta[0], delta[1], K, M, N) for i in range(BATCH_COUNT)]
                    d_in.copy_(torch.from_numpy(imgs))
                    for area in AREAS:
                        d_out.fill_(SENTINEL)
                        p.wiener_batch_dev(d_in.data_ptr(), rows * cols, BATCH_COUNT, rows, cols, cols, d_out.data_ptr(), rows * cols, cols, area, stream=s)
                        torch.cuda.synchronize()
                        got = d_out.cpu().numpy()
                        one = np.stack([p.wiener(imgs[i], area) for i in range(BATCH_COUNT)])
                        for i, (hi_at, lo_at) in enumerate(use):
                            what = "image %d of %s" % (i, _what(case, rows, cols, delta, hi_at, lo_at, area))
                            sp, b = _judge(what, M, N, got[i], refs[i][area], tol)
                            bad += b
                            worst = max(worst, sp) if sp == sp else sp
                        n = int(np.count_nonzero(~(got == one)))
                        if n:
                            bad.append("%s window %dx%d delta %s %s: %d values of the batch differ from image by image"
                                       % (cid, rows, cols, delta, AREA_NAME[area], n))
                        calls += 1
    log("batch %dx%d%s" % (nstreams, group, " graph" if graph else ""), cid, worst, tol, calls)
    assert not bad, "%d failures, the first:\n%s" % (len(bad), "\n".join(bad[:12]))


@pytest.mark.parametrize("cid", ("fast-8x32", "fast-8x256-split"))
def test_operators_sharing_normalize_window(fdr, cid):
    """richardson_lucy (0 and 2 iterations), tv_deconv (0 iterations) and richardson_lucy_free (1 iteration, no weights) with the
    operator PSF delta(0, 0): the raw result is the planted picture itself, normalised as _rl_model.normalize defines for NONE,
    CROPPED and PADDED (PADDED counts one zero).  The free-boundary call also returns the whole plan, whose zeros are pixels."""
    case = BY_ID[cid]
    M, N = case[2], case[3]
    bad, calls = [], 0
    worst = {"rl": 0.0, "tv": 0.0, "rlfree": 0.0}
    tols = {"rl": _rl_model.DELTA_TOL, "tv": TV_TOL, "rlfree": RLFREE_TOL}

    def judge(kind, what, got, raw, norm):
        want = _rl_model.normalize(raw, norm, M, N)
        e = _rl_model.rel_err(got, want) if norm == _rl_model.NORM_NONE else max_abs(got, want)
        worst[kind] = max(worst[kind], e) if e == e else e
        if not e <= tols[kind]:
            bad.append("%s: error %.3g > %.3g" % (what, e, tols[kind]))
        if norm != _rl_model.NORM_NONE and not (np.all(np.isfinite(got)) and got.min() >= 0.0 and got.max() <= 1.0 + tols[kind]):
            bad.append("%s: output not finite or outside [0, 1]" % what)

    with _plan(fdr, case) as p:
        p.set_operator_psf(np.ones((1, 1), dtype=np.float32))
        for rows, cols in windows(case):
            for hi_at, lo_at in position_pairs(edge_positions(M, N, rows, cols)):
                img = planted(rows, cols, hi_at, lo_at, seed_of(rows, cols))
                raw = img.astype(np.float64)
                plane = np.zeros((M, N))
                plane[:rows, :cols] = raw
                for norm in (_rl_model.NORM_NONE, _rl_model.NORM_CROPPED, _rl_model.NORM_PADDED):
                    what = "%s window %dx%d hi %s lo %s %s" % (cid, rows, cols, hi_at, lo_at, AREA_NAME[norm])
                    for n in (0, 2):
                        judge("rl", "richardson_lucy n=%d %s" % (n, what), p.richardson_lucy(img, n, norm), raw, norm)
                    judge("tv", "tv_deconv n=0 " + what, p.tv_deconv(img, 50.0, iterations=0, norm_area=norm), raw, norm)
                    judge("rlfree", "richardson_lucy_free n=1 " + what, p.richardson_lucy_free(img, 1, norm_area=norm), raw, norm)
                    judge("rlfree", "richardson_lucy_free n=1 full plane " + what, p.richardson_lucy_free(img, 1, norm_area=norm, full_plane=True), plane, norm)
                    calls += 5
    for kind in ("rl", "tv", "rlfree"):
        log("operator " + kind, cid, worst[kind], tols[kind], calls)
    assert not bad, "%d failures, the first:\n%s" % (len(bad), "\n".join(bad[:12]))


# The slab normaliser applies OpenCV's float scale and shift: the scale is rounded to float, then one float multiply and one float
# add on values of at most 1.  Each of the four roundings is at most 2^-24 relative on a magnitude of at most 1.07 (hi / (hi - lo)):
# 2.6e-7 in all; the bound is 4x that.
SLAB_TOL = 1e-6


def test_slab_minmax_and_normalize(fdr):
    """fdr_slab_minmax_dev + fdr_slab_normalize_dev as slab.py calls them, on a tables-only plan: a real rows x ld plane holding
    a planted picture, the counted window equal to the plane, one smaller in each direction, and placed so that a spike lies just
    outside it.  min and max must be the exact float values; the normalised window is compared with numpy."""
    import torch
    lib = fdr.lib
    rows, ld = 13, 301  # two workgroups per row, the second partly filled
    bad, worst, calls = [], 0.0, 0
    with fdr.Plan(16, 512, fdr.MODE_PARITY, flags=fdr.FLAG_TABLES_ONLY) as p:
        for mm_rows, mm_cols in ((rows, ld), (rows - 1, ld), (rows, ld - 1), (rows - 1, ld - 1), (5, 257), (4, 256)):
            inside = position_pairs(edge_positions(rows, ld, mm_rows, mm_cols))
            outside = [((min(mm_rows, rows - 1), mm_cols - 1), (mm_rows - 1, min(mm_cols, ld - 1))),   # hi just below, lo just right of it
                       ((mm_rows - 1, min(mm_cols, ld - 1)), (min(mm_rows, rows - 1), 0))]
            for hi_at, lo_at in inside + [o for o in outside if o[0] != o[1]]:
                img = planted(rows, ld, hi_at, lo_at, seed_of(rows, ld))
                d_raw = torch.from_numpy(img).cuda()
                d_mm = torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device="cuda")
                d_out = torch.full((mm_rows, mm_cols + 3), SENTINEL, dtype=torch.float32, device="cuda")
                st = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))
                fdr._check(lib.fdr_slab_minmax_dev(p._h, ctypes.c_void_p(d_raw.data_ptr()), rows, ld, mm_rows, mm_cols, ctypes.c_void_p(d_mm.data_ptr()), st))
                fdr._check(lib.fdr_slab_normalize_dev(ctypes.c_void_p(d_raw.data_ptr()), ld, ctypes.c_void_p(d_mm.data_ptr()),
                                                      ctypes.c_void_p(d_out.data_ptr()), mm_rows, mm_cols, mm_cols + 3, st))
                torch.cuda.synchronize()
                win = img[:mm_rows, :mm_cols]
                mm, out = d_mm.cpu().numpy(), d_out.cpu().numpy()
                what = "slab %dx%d window %dx%d hi %s lo %s" % (rows, ld, mm_rows, mm_cols, hi_at, lo_at)
                if not (mm[0] == win.min() and mm[1] == win.max()):
                    bad.append("%s: min/max (%r, %r), numpy (%r, %r)" % (what, float(mm[0]), float(mm[1]), float(win.min()), float(win.max())))
                w64 = win.astype(np.float64)
                sp = max_abs(out[:, :mm_cols], (w64 - w64.min()) / (w64.max() - w64.min()))
                if not sp <= SLAB_TOL:
                    bad.append("%s: max-abs %.3g > %.3g against numpy" % (what, sp, SLAB_TOL))
                if not np.all(out[:, mm_cols:] == SENTINEL):
                    bad.append("%s: a value outside the window was overwritten" % what)
                worst = max(worst, sp) if sp == sp else sp
                calls += 1
    log("slab", "13x301", worst, SLAB_TOL, calls)
    assert not bad, "%d failures, the first:\n%s" % (len(bad), "\n".join(bad[:12]))
