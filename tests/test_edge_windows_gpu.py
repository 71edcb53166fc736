"""Every windowed call on the MI355X at the smallest windows, against its float64 model: the tables of tests/_edge_windows.py (pinned
in test_edge_windows_host.py).  One test per (family, plan): every window of the plan under the dense PSF for 0, 1 and 3 iterations
and every norm_area, with no, fractional and holed weights where the call takes some; the core windows under PSFs of 1, 2, 4 and
M - 1 rows; each case on a 16-byte aligned base with strides that are multiples of 4 and again one float off it with odd strides;
the _dev form behind NaN guard bands and then the host form, which must have its bytes.  Thresholds and error measures are those of
the families' own model files.  Then what needs no model: exact data (the PSF {1}, zero pictures, zero weights, one pixel), the
group calls against their single calls, and what a small call leaves behind in a plan.  Each case prints an `EDGE` line (pytest -s)."""
import numpy as np
import pytest

from _edge_windows import (BATCH, FAMILIES, FAMILY, ONE, PLANS, cases, core_windows, defined, frames_of, picture, psfs, run_dev, stage,
                           second_psf, stop_decision, tolerance, weights)
from _rl_model import DELTA_TOL, NORM_CROPPED, NORM_NONE, NORM_PADDED, rel_err
from _rlstop_model import stop_ok

pytestmark = pytest.mark.gpu

PAIRS = [(f.name, M, N) for f in FAMILIES for M, N in PLANS]
IDS = ["%s-%dx%d" % p for p in PAIRS]


def flat_plane(fam, rows, cols, area):
    """Smooth padding continues a one-pixel window as a constant plane, and FDR_NORM_PADDED then normalises a restored plane that is
    constant up to rounding: (x - lo) / (hi - lo) of rounding noise, in the model as on the device (which gave 0.06 .. 0.63 where
    the exact answer is 0).  include/fdr.h (FDR_OPT_PAD_MODE) names the case as not defined; a constant full-plane picture does the
    same on any path.  test_zero_picture_and_one_pixel holds what is left: a finite value in [0, 1], nothing outside the window."""
    return fam.name.endswith("_smooth") and rows * cols == 1 and area == NORM_PADDED


def _imgs(fam, img):
    return frames_of(img) if fam.frames == 2 else img


@pytest.mark.parametrize("name,M,N", PAIRS, ids=IDS)
def test_against_model(fdr, name, M, N):
    """every case of the family on the plan: _dev form, aligned and odd, against the float64 model; then the host form, bit for bit.
    One `EDGE case` line per (window, PSF) with its largest error, one `EDGE model` line for the whole (family, plan)."""
    fam = FAMILY[name]
    bad, worst, worst_at, calls, worst_trace, stops, worst_psf = [], 0.0, None, 0, 0.0, 0, 0.0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        last = None
        for rows, cols, pname, psf, main in cases(fam, M, N):
            if pname != last:
                fam.setup(p, psf)
                last = pname
            img = picture(rows, cols)
            case_worst, case_tol = 0.0, 0.0
            for kind in (fam.kinds() if main else ("none",)):
                if kind == "hole" and rows * cols == 1:
                    continue  # the hole is the whole window: test_zero_weights
                w = weights(kind, rows, cols)
                full = main and kind == "none"
                for n in fam.iters:
                    raw = fam.model(img, psf, M, N, n, w, np.float64)
                    tol = tolerance(fam, M, N, rows, cols, pname)
                    if tol is None:  # blind RL: from the float32 replay of the same case
                        tol = fam.err32_tol(fam.error(np.asarray(fam.model(img, psf, M, N, n, w, np.float32), dtype=np.float64), np.asarray(raw), NORM_NONE))
                    for area in (fam.areas if full else dict.fromkeys((fam.areas[0], fam.areas[-1]))):
                        if flat_plane(fam, rows, cols, area):
                            continue
                        want = fam.finish(raw, area, M, N, rows, cols)
                        what = "%dx%d win %dx%d %s w=%s n=%s norm=%d" % (M, N, rows, cols, pname, kind, n, area)
                        got = {}
                        for mis in (False, True):
                            got[mis], a = run_dev(fam, p, _imgs(fam, img), w, psf, n, area, mis)
                            calls += 1
                            e = fam.error(got[mis], want, area)
                            if fam.trace is not None and n and area == fam.areas[0]:
                                te = fam.trace[2](a.trace_out, fam.trace[1](img, psf, M, N, n, w))
                                worst_trace = max(worst_trace, te) if te == te else te
                                if not te <= fam.trace[3]:
                                    bad.append("%s %s: trace error %.3g > %.3g" % (what, "odd" if mis else "aligned", te, fam.trace[3]))
                            if fam.psf_model is not None and area == fam.areas[0]:  # blind RL: the refined PSF against the model's
                                want_p = np.asarray(fam.psf_model(img, psf, M, N, n, w, np.float64), dtype=np.float64)
                                tol_p = fam.err32_tol(rel_err(fam.psf_model(img, psf, M, N, n, w, np.float32), want_p))
                                ep = rel_err(a.psf_out, want_p)
                                worst_psf = ep if not ep <= worst_psf else worst_psf
                                if not ep <= tol_p:
                                    bad.append("%s %s: PSF error %.3g > %.3g" % (what, "odd" if mis else "aligned", ep, tol_p))
                            if name == "rl_auto_res" and area == fam.areas[0]:
                                m, r = stop_decision(img, psf, M, N, n), a.returned
                                stops += m["stopped"]
                                if not stop_ok(r.iterations_done, r.stopped, m):
                                    bad.append("%s: stopped after %d (%d), the model after %d (%d)" % (what, r.iterations_done, r.stopped, m["iterations_done"], m["stopped"]))
                            case_worst, case_tol = (e if not e <= case_worst else case_worst), max(case_tol, tol)
                            if not e <= worst:
                                worst, worst_at = e, what + (" odd" if mis else " aligned")
                            if not e <= tol:
                                bad.append("%s %s: error %.3g > %.3g" % (what, "odd" if mis else "aligned", e, tol))
                        if fam.host is not None and not bad:
                            host = fam.host(p, img, n, area, w, psf)
                            calls += 1
                            assert np.array_equal(host, got[False]), "%s: the host form and the _dev form differ" % what
            print("EDGE\tcase\t%s\t%dx%d\twin %dx%d\t%s\terr=%.3g\tthreshold=%.3g" % (name, M, N, rows, cols, pname, case_worst, case_tol))
    print("EDGE\tmodel\t%s\t%dx%d\tworst=%.3g\tat %s\tthreshold=%s\tcalls=%d\ttrace=%.3g\tstops=%d\tpsf=%.3g" % (name, M, N, worst, worst_at, fam.tol, calls, worst_trace, stops, worst_psf))
    assert not bad, "\n".join(bad[:40])


def _exact_windows(M, N):
    return [(1, 1), (1, 2), (2, 1), (3, 3), (4, 4), (1, N), (M, 1), (M - 1, N - 1)]


@pytest.mark.parametrize("M,N", PLANS, ids=["%dx%d" % q for q in PLANS])
def test_unit_psf_is_exact(fdr, M, N):
    """PSF {1}: a blur returns the window, Richardson-Lucy max(d, 0) -- the accelerated form too, whose g = u_(k+1) - y_k is 0 from the
    second step on, so that its alpha is 0 / 0 -- all to DELTA_TOL"""
    worst = 0.0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(ONE)
        for rows, cols in (_exact_windows(M, N) if M * N <= 1 << 14 else core_windows(M, N)):
            img = picture(rows, cols)
            for name, want in (("blur_fwd", img), ("blur_adj", img), ("rl", np.maximum(img, 0)), ("rl_accel", np.maximum(img, 0))):
                fam = FAMILY[name]
                for mis in (False, True):
                    got, _ = run_dev(fam, p, img, None, ONE, fam.iters[-1], NORM_NONE, mis)
                    assert np.all(np.isfinite(got)), (name, rows, cols)
                    e = rel_err(got, want)
                    worst = max(worst, e)
                    assert e <= DELTA_TOL, (name, rows, cols, mis, e)
    print("EDGE\tunit psf\t%dx%d\tworst=%.3g\tthreshold=%.3g" % (M, N, worst, DELTA_TOL))


@pytest.mark.parametrize("name", [f.name for f in FAMILIES])
def test_zero_picture_and_one_pixel(fdr, name):
    """an all-zero window comes back all zero (where the model's answer is: Poisson TV with a background moves off zero, and is held
    to the model); a one-pixel window comes back as exactly 0.0f under FDR_NORM_CROPPED (it is flat) and
    as the model's value under FDR_NORM_PADDED, which counts the zeros of the padding beside it"""
    fam = FAMILY[name]
    for M, N in (PLANS[0], PLANS[1], PLANS[3]):
        _, psf, _ = psfs(M, N, fam.centred)[0]
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            fam.setup(p, psf)
            n = fam.iters[-1]
            for rows, cols in core_windows(M, N):
                if not defined(fam, rows, cols, psf):
                    continue
                zero = np.zeros((rows, cols), dtype=np.float32)
                raw = fam.model(zero, psf, M, N, n, None, np.float64)
                for area in fam.areas:
                    if np.asarray(raw).any() and area != NORM_NONE:
                        continue  # Poisson TV: a constant, not zero; its normalisation is that of a flat plane (flat_plane)
                    for mis in (False, True):
                        got, _ = run_dev(fam, p, _imgs(fam, zero), None, psf, n, area, mis)
                        want = np.asarray(fam.finish(raw, area, M, N, rows, cols), dtype=np.float64)
                        if not want.any():
                            assert np.array_equal(got, np.zeros_like(got)), (name, M, N, rows, cols, area, mis, got.ravel()[:4])
                        else:
                            assert fam.error(got, want, area) <= fam.tol, (name, M, N, rows, cols, area, mis)
            img = picture(1, 1)
            for area in fam.areas:
                if area == NORM_NONE or not defined(fam, 1, 1, psf):
                    continue
                if flat_plane(fam, 1, 1, area):
                    for mis in (False, True):
                        got, _ = run_dev(fam, p, img, None, psf, n, area, mis)
                        assert np.all(np.isfinite(got)) and 0.0 <= float(got.min()) and float(got.max()) <= 1.0, (name, M, N, got)
                    continue
                raw = fam.model(img, psf, M, N, n, None, np.float64)
                want = np.asarray(fam.finish(raw, area, M, N, 1, 1), dtype=np.float64)
                for mis in (False, True):
                    got, _ = run_dev(fam, p, _imgs(fam, img), None, psf, n, area, mis)
                    if area == NORM_CROPPED:
                        assert got.tobytes() == np.zeros_like(got).tobytes(), (name, M, N, area, got)
                    else:
                        assert np.all(np.abs(got - want) <= (fam.tol or 1e-5)), (name, M, N, area, got, want)


@pytest.mark.parametrize("name", [f.name for f in FAMILIES if f.weighted])
def test_zero_weights(fdr, name):
    """all-zero weights: the model's result (zeros for the Richardson-Lucy forms: nothing is seen, sw = 0) and nothing non-finite"""
    fam = FAMILY[name]
    for M, N in PLANS[:2]:
        _, psf, _ = psfs(M, N, fam.centred)[0]
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            fam.setup(p, psf)
            for rows, cols in core_windows(M, N) + [(4, 4)]:
                if not defined(fam, rows, cols, psf):
                    continue
                img, w = picture(rows, cols), np.zeros((rows, cols), dtype=np.float32)
                n = fam.iters[-1]
                want = np.asarray(fam.model(img, psf, M, N, n, w, np.float64), dtype=np.float64)
                assert np.all(np.isfinite(want))
                for mis in (False, True):
                    got, _ = run_dev(fam, p, _imgs(fam, img), w, psf, n, NORM_NONE, mis)
                    assert np.all(np.isfinite(got)), (name, M, N, rows, cols, mis)
                    if not want.any():
                        assert np.array_equal(got, np.zeros_like(got)), (name, M, N, rows, cols, mis)
                    else:
                        tol = fam.tol if fam.tol is not None else 1e-5
                        assert fam.error(got, want, NORM_NONE) <= tol, (name, M, N, rows, cols, mis, fam.error(got, want, NORM_NONE))


@pytest.mark.parametrize("name", sorted(BATCH))
def test_groups_have_the_bytes_of_single_calls(fdr, name):
    """count = 3 under set_batching(1, 2) (a group of two, then one): every image equals the bytes of its single call; image 1
    lies at a pitch that breaks image 0's 16-byte alignment"""
    fam = FAMILY[name]
    for M, N in (PLANS[0], PLANS[1], PLANS[4]):
        _, psf, _ = psfs(M, N, fam.centred)[0]
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            p.set_batching(1, 2)
            fam.setup(p, psf)
            for rows, cols in core_windows(M, N)[:4]:
                imgs = np.stack([picture(rows, cols, seed) for seed in (0, 1, 2)])
                w = weights("frac", rows, cols) if fam.weighted else None
                n = fam.iters[-1]
                for area in dict.fromkeys((fam.areas[0], fam.areas[-1])):
                    singles = np.stack([run_dev(fam, p, imgs[k], w, psf, n, area, False)[0] for k in range(3)])
                    for mis in (False, True):
                        got, _ = run_dev(fam, p, imgs, w, psf, n, area, mis, call=BATCH[name], out_count=3, odd_pitch=True)
                        assert got.tobytes() == singles.tobytes(), (name, M, N, rows, cols, area, mis, float(np.nanmax(np.abs(got - singles))))


def test_frames_have_the_bytes_of_single_calls(fdr):
    """fdr_blur_frames_f32_dev, three frames under set_batching(1, 2): window k has the bytes of fdr_blur_f32_dev under PSF k"""
    fam = FAMILY["blur_frames_fwd"]
    for M, N in (PLANS[0], PLANS[1], PLANS[4]):
        _, psf, _ = psfs(M, N, False)[0]
        plist = [psf, second_psf(psf), np.ascontiguousarray(psf[::-1, ::-1])]
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            p.set_batching(1, 2)
            p.set_frame_psfs(plist)
            for rows, cols in core_windows(M, N)[:4]:
                img = picture(rows, cols)
                singles = []
                for q in plist:
                    p.set_operator_psf(q)
                    singles.append(run_dev(FAMILY["blur_fwd"], p, img, None, q, None, NORM_NONE, False)[0])
                for mis in (False, True):
                    got, _ = run_dev(fam, p, img, None, psf, None, NORM_NONE, mis, out_count=3, odd_pitch=True,
                                     call=lambda p, a: p.blur_frames_dev(a.img, 0, a.rows, a.cols, a.stride, a.out, a.opitch, a.ostride, 3, False))
                    assert got.tobytes() == np.stack(singles).tobytes(), (M, N, rows, cols, mis)


@pytest.mark.parametrize("name", [f.name for f in FAMILIES])
def test_nothing_left_behind(fdr, name):
    """a full-plane call with a picture 100 times brighter, then a small-window call, then the full-plane call again: the second has
    the bytes of the same call on a fresh plan and the third those of the first, whatever the workspaces beyond the window still
    hold of the bright picture"""
    fam = FAMILY[name]
    M, N = PLANS[1]
    _, psf, _ = psfs(M, N, fam.centred)[0]
    bright = (100.0 * picture(M, N)).astype(np.float32)
    n = fam.iters[-1]
    w_full = weights("frac", M, N) if fam.weighted else None

    def call(p, img, w, area):
        fam.setup(p, psf)
        return run_dev(fam, p, _imgs(fam, img), w, psf, n, area, False)[0]

    for rows, cols in ((1, 1), (3, 3), (1, N), (M, 1), (5, N // 2 - 1)):
        if not defined(fam, rows, cols, psf):
            continue
        img = picture(rows, cols)
        w = weights("frac", rows, cols) if fam.weighted else None
        for area in dict.fromkeys((fam.areas[0], fam.areas[-1])):
            with fdr.Plan(M, N, fdr.MODE_FAST) as fresh:
                want = call(fresh, img, w, area)
            with fdr.Plan(M, N, fdr.MODE_FAST) as p:
                first = call(p, bright, w_full, area)
                second = call(p, img, w, area)
                third = call(p, bright, w_full, area)
            assert second.tobytes() == want.tobytes(), (name, rows, cols, area, float(np.nanmax(np.abs(second - want))))
            assert third.tobytes() == first.tobytes(), (name, rows, cols, area)


def test_blind_free_refuses_windows_below_the_psf(fdr):
    """The free-boundary blind form has no defined answer on a window smaller than its PSF (_edge_windows.defined says why): both
    forms refuse it with FDR_ERR_ARG and a message naming the minimum, launch nothing and write nothing; a window of the PSF's
    size is taken"""
    import torch
    fam = FAMILY["blind_free_hold0"]
    for M, N in PLANS[:2]:
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            p.profile(True)
            refused = 0
            for pname, psf, _ in psfs(M, N, False):
                fam.setup(p, psf)
                for rows, cols in core_windows(M, N) + [(psf.shape[0] - 1, N), (M, psf.shape[1] - 1)]:
                    if rows < 1 or cols < 1 or defined(fam, rows, cols, psf):
                        continue
                    img = picture(rows, cols)
                    for mis in (False, True):
                        a, bufs = stage(fam, img, None, psf, 3, NORM_NONE, mis)
                        with pytest.raises(fdr.FdrError) as e:
                            fam.dev(p, a)
                        assert e.value.code == -1 and "prows x pcols" in str(e.value), (pname, rows, cols, str(e.value))
                        torch.cuda.synchronize()
                        assert bufs["psf"].unchanged() and bufs["img"].unchanged() and bufs["out"].unchanged()
                    with pytest.raises(fdr.FdrError) as e:
                        fam.host(p, img, 3, NORM_NONE, None, psf)
                    assert e.value.code == -1 and "prows x pcols" in str(e.value)
                    refused += 1
            assert refused >= 8
            assert [n for n, _, c in p.pass_times() if c] == [], "a refused call launched something"
            p.profile(False)
            psf = psfs(M, N, False)[0][1]  # 5 x 5: a 5 x 5 window is the minimum
            img = picture(5, 5)
            got, a = run_dev(fam, p, img, None, psf, 3, NORM_NONE, False)
            want_p = np.asarray(fam.psf_model(img, psf, M, N, 3, None, np.float64), dtype=np.float64)
            ep, ep32 = rel_err(a.psf_out, want_p), rel_err(fam.psf_model(img, psf, M, N, 3, None, np.float32), want_p)
            print("EDGE\tblind minimum\t%dx%d win 5x5\tPSF err=%.3g\tfloat32 model=%.3g" % (M, N, ep, ep32))
            assert ep <= fam.err32_tol(ep32), (M, N, ep, ep32)
            want = np.asarray(fam.model(img, psf, M, N, 3, None, np.float64))
            err32 = fam.error(np.asarray(fam.model(img, psf, M, N, 3, None, np.float32), dtype=np.float64), want, NORM_NONE)
            e = fam.error(got, want, NORM_NONE)
            print("EDGE\tblind minimum\t%dx%d win 5x5\terr=%.3g\tfloat32 model=%.3g" % (M, N, e, err32))
            assert e <= fam.err32_tol(err32), (M, N, e, err32)
