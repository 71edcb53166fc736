"""The tables of tests/_edge_windows.py, pinned on the CPU before test_edge_windows_gpu.py judges the device with them: for every
(family, plan, window, PSF) the float64 model runs and is finite, the Richardson-Lucy inputs are well conditioned (c = blur(u) of
the family's basic iteration stays at least 1e-2 max c wherever the weighted datum is positive: _c_ratio says what that covers), the
float32 run of the model lies below a quarter of the family's threshold (printed: the floor), and window and PSF faults of one line
move the model by at least 100 thresholds (test_sensitivity says on which cases, and where that is less than the issue asked).  Each
(family, plan) prints an `EDGE` line (pytest -s)."""
import numpy as np
import pytest

from _edge_windows import (FAMILIES, FAMILY, FAULTS, PLANS, cases, core_windows, fault_model, frames_of, picture, stop_decision, psfs, second_psf, tolerance, weights,
                           windows)
from _frames_model import frames_state
from _rl_model import NORM_NONE, TAU, blur_model, op_spectrum, rel_err
from _rlfree_model import SIGMA, SIGMA_MARGIN, fullblur, rlfree_state
from _rlstop_model import DECISION_MARGIN, decision_margin

C_FLOOR = 1e-2  # c >= C_FLOOR max c: a condition on the inputs
PAIRS = [(f.name, M, N) for f in FAMILIES for M, N in PLANS]
IDS = ["%s-%dx%d" % p for p in PAIRS]


def test_tables():
    for M, N in PLANS:
        ws = windows(M, N)
        assert len(ws) == len(set(ws)) and all(1 <= r <= M and 1 <= c <= N for r, c in ws), (M, N)
        assert set(core_windows(M, N)) <= set(ws)
        assert len(ws) == (5 if max(M, N) >= 4096 else 16)
        for centred in (False, True):
            ps = psfs(M, N, centred)
            assert sorted(p.shape[0] for _, p, main in ps if not main) == [1, 2, 4] + ([M - 1] if M * N <= 64 * 256 else [])
            for name, p, _ in ps:
                assert p.dtype == np.float32 and float(p.min()) >= 0 and abs(float(p.sum(dtype=np.float64)) - 1) < 1e-6, name
                assert p[0, 0] > 0, name  # weight at (0, 0): c = blur(u) does not vanish along the first rows of a cropped window
        for rows, cols in ws:
            img = picture(rows, cols)
            assert img.shape == (rows, cols) and np.array_equal(img, picture(rows, cols, grow=1)[:rows, :cols])
            assert int((img < 0).sum()) == (1 if rows * cols > 1 else 0) and float(np.abs(img).min()) >= 0.2 and float(img.max()) <= 1
            hole = weights("hole", rows, cols)
            assert int((hole == 0).sum()) == 1 and float(weights("frac", rows, cols).min()) >= 0.25


def _c_ratio(fam, img, psf, M, N, w, n):
    """the smallest c / max c over the window and over the iterations 0 .. n-1 of the family's basic iteration (plain RL, or
    free-boundary RL on the whole plan; both frames' PSFs for the frames), and for the free forms the distance of the coverage
    from its threshold.  The minimum runs over the pixels whose weighted datum is positive: where m d+ = 0 the ratio r = m d+ / c
    is 0 whatever c is, and under a one-row PSF on a one-column window nothing but the pixel itself reaches its c, so the one
    negative pixel (u = d+ = 0 there) has c = 0 by construction.  The restriction holds for every case, not only that one.
    The c is that of the BASIC iteration with the family's PSF and weights -- plain RL for every periodic family (accelerated,
    RL-TV, stop rules, plain blind), free-boundary RL for every free one -- not the c of the family's own extrapolated,
    TV-weighted or PSF-refining iterates: three steps of those stay within a few per cent of the basic ones, and the floor
    is a condition on the inputs (picture, PSF, weights), which they share."""
    worst, margin = np.inf, np.inf
    rows, cols = img.shape
    plist = [psf, second_psf(psf)] if fam.frames == 2 and fam.name.endswith("frames") else [psf]
    for k in range(n):
        if fam.free:
            if len(plist) == 2:
                st = frames_state(frames_of(img), plist, M, N, k, w)
                margin = min(margin, float(np.min(np.abs(st["alpha"] - 2 * SIGMA))) / 2)
            else:
                st = rlfree_state(img, psf, M, N, k, w)
                margin = min(margin, float(np.min(np.abs(st["alpha"] - SIGMA))))
            cs = [fullblur(st["u"], op_spectrum(q, M, N))[:rows, :cols] for q in plist]
        else:
            u = np.asarray(FAMILY["rl"].model(img, psf, M, N, k, None, np.float64))
            cs = [blur_model(u, psf, M, N)]
        live = (img > 0) if w is None else ((img > 0) & (w > 0))
        for c in cs:
            assert float(c.max()) > 1e3 * TAU
            worst = min(worst, float(c[live].min()) / float(c.max()))
    return worst, margin


@pytest.mark.parametrize("name,M,N", PAIRS, ids=IDS)
def test_models_run_and_inputs_are_well_conditioned(name, M, N):
    fam = FAMILY[name]
    floor, floor_at, cmin, cmin_at, amin, psf_floor = 0.0, None, np.inf, None, np.inf, 0.0
    for rows, cols, pname, psf, main in cases(fam, M, N):
        img = picture(rows, cols)
        nmax = fam.iters[-1]
        for kind in (fam.kinds() if main else ("none",)):  # the weights go with the main PSF (test_edge_windows_gpu.py)
            if kind == "hole" and rows * cols == 1:
                continue
            w = weights(kind, rows, cols)
            for n in ((fam.iters[0], nmax) if kind == "none" else (nmax,)):  # the run to nmax passes through every count below it
                want = np.asarray(fam.model(img, psf, M, N, n, w, np.float64), dtype=np.float64)
                assert np.all(np.isfinite(want)), (rows, cols, pname, kind, n)
            low = np.asarray(fam.model(img, psf, M, N, nmax, w, np.float32), dtype=np.float64)
            e = fam.error(low, want, NORM_NONE)
            if e > floor:
                floor, floor_at = e, "%dx%d %s w=%s" % (rows, cols, pname, kind)
            if fam.psf_model is not None:  # blind RL: the refined PSF's float32 replay stays in the class the device bound assumes
                pe = rel_err(fam.psf_model(img, psf, M, N, nmax, w, np.float32), fam.psf_model(img, psf, M, N, nmax, w, np.float64))
                psf_floor = max(psf_floor, pe)
                assert pe <= 1e-5, (rows, cols, pname, kind, pe)
            if name == "rl_auto_res":  # no statistic at its target: a rounding flip of the decision would void the case
                assert decision_margin(stop_decision(img, psf, M, N, nmax)) >= DECISION_MARGIN, (rows, cols, pname)
            if fam.rl:
                c, a = _c_ratio(fam, img, psf, M, N, w, nmax)
                amin = min(amin, a)
                if c < cmin:
                    cmin, cmin_at = c, "%dx%d %s w=%s" % (rows, cols, pname, kind)
    print("EDGE\thost\t%s\t%dx%d\tfloat32 floor=%.3g at %s\tmin c / max c=%.3g at %s\tcoverage margin=%.3g\tPSF float32 floor=%.3g" % (name, M, N, floor, floor_at, cmin, cmin_at, amin, psf_floor))
    if fam.rl:
        assert cmin >= C_FLOOR, (cmin, cmin_at)
        assert amin >= SIGMA_MARGIN, amin  # no coverage within SIGMA_MARGIN of the threshold: a rounding flip would void the case
    if fam.tol is not None:
        assert floor <= fam.tol / 4, (floor, floor_at)  # else the case needs a bound of its own (CASE_TOL)


@pytest.mark.parametrize("name,M,N", PAIRS, ids=IDS)
def test_sensitivity(name, M, N):
    """A window one line short or long (fault_model) and a PSF one row short against the true model, in thresholds of the family.

    Asserted: on every (family, plan) each of the five faults moves at least one case by 100 thresholds, and every case is moved
    that far by at least one fault, unless it is a core window.  This is LESS than 'each fault moves each case': under a PSF that
    starts at (0, 0) the line a `*_long` fault reads lies beyond the window and reaches the window only around the plan's edge
    (a forward blur sees `row_long` on 11 of 31 cases of 8 x 32 and 3 of 16 of 4096 x 32; the iterations see it on nearly all,
    their adjoint brings the line back), a one-row window has no second PSF row in reach, and a one-pixel window has no line to
    lose.  Dropping every case that misses one fault would empty the table of exactly the small windows the files are about, so
    such cases stay, and the `seen / could` counts printed per fault say how many cases would catch each fault (could: the
    cases where the fault exists at all).  The cases no fault moves are one-pixel windows only; they stay for the masks, tails
    and sums they degenerate, which the model comparison itself judges."""
    fam = FAMILY[name]
    seen_by, could, blind = {}, {}, []
    for rows, cols, pname, psf, main in cases(fam, M, N):
        img = picture(rows, cols)
        n = fam.iters[-1]
        want = np.asarray(fam.model(img, psf, M, N, n, None, np.float64), dtype=np.float64)
        tol = tolerance(fam, M, N, rows, cols, pname)
        if tol is None:
            tol = fam.err32_tol(fam.error(np.asarray(fam.model(img, psf, M, N, n, None, np.float32), dtype=np.float64), want, NORM_NONE))
        if want.shape[-2:] == (M, N):
            want = want[..., :rows, :cols]
        sees = 0
        for fault in FAULTS:
            got = fault_model(fam, fault, rows, cols, psf, M, N, n, "none")
            if got is None:
                continue
            could[fault] = could.get(fault, 0) + 1
            if fam.error(got, want, NORM_NONE) >= 100 * tol:
                sees += 1
                seen_by[fault] = seen_by.get(fault, 0) + 1
        if not sees:
            blind.append((rows, cols, pname))
    print("EDGE\tsensitivity\t%s\t%dx%d\t%s\tmoved by no fault: %s" % (name, M, N, "\t".join("%s seen by %d of %d" % (f, seen_by.get(f, 0), could.get(f, 0))
                                                                                            for f in FAULTS), blind))
    assert all(seen_by.get(f, 0) > 0 for f in FAULTS), seen_by
    assert all((r, c) in core_windows(M, N) for r, c, _ in blind), blind
