"""Richardson-Lucy that stops from the data (fdr_richardson_lucy_auto_f32*) on the MI355X against the float64 model of
tests/_rlstop_model.py and against the existing calls of the four forms: (a) the trace and the output bits at n = 3 on every row
length and both inverse row kernels, full and ragged windows; (b) the stop, both rules; (c) a rule that never fires and one that
fires at once; (d) the refusals; the _dev form.  Each case prints an `RLS` line with its measured values (pytest -s)."""
import ctypes

import numpy as np
import pytest

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, dense_psf
from _rlfree_model import SIGMA, SIGMA_MARGIN, rlfree_state, sigma_margin
from _rlstop_model import (DECISION_MARGIN, STOP_CONFIGS, STOP_KL, STOP_N, STOP_NONE, STOP_PLAN, STOP_RESIDUAL, STOP_TAU, STOP_WINDOW, TRACE_TOL,
                           decision_margin, guard_case, run_model, stop_model, stop_ok, stop_scene, trace_ok)

pytestmark = pytest.mark.gpu

PACKED = [(8, 32), (16, 64), (8, 128), (8, 4096), (8, 8192)]   # fft_rows4_inv_packed_kernel, one plan per row length
SPLIT = [(64, 256), (32, 512), (32, 1024), (16, 2048)]         # fft_rows4_inv_split_kernel
PACKED_AT_SPLIT_LENGTH = [(4096, 256)]                         # M > 2048: the packed kernel at a length the split kernel serves
SHAPES = PACKED + SPLIT + PACKED_AT_SPLIT_LENGTH
FORMS = [(False, False), (False, True), (True, False), (True, True)]  # (free_boundary, accelerate)


def _ragged(M, N):
    """rows not a multiple of 4, cols odd"""
    return M - 3, (N - N // 5) | 1


def _picture(rows, cols, seed):
    """positive noise on a pedestal with a corner of negative pixels (RL starts from d+)"""
    d = (0.3 + 0.5 * np.random.default_rng(seed).random((rows, cols))).astype(np.float32)
    d[: max(1, rows // 8), : max(1, cols // 8)] -= np.float32(0.6)
    return d


def _existing(p, img, n, free, acc, weights=None, area=NORM_NONE):
    """the call of the same form that takes its count from the caller"""
    if free:
        return p.richardson_lucy_free(img, n, weights, SIGMA, area, accelerate=acc)
    return p.richardson_lucy(img, n, area, accelerate=acc)


def _weights(kind, rows, cols):
    if kind == "none":
        return None
    r = np.random.default_rng(8).random((rows, cols))
    return (r >= 0.2).astype(np.float32) if kind == "mask" else (0.25 + 0.75 * r).astype(np.float32)


@pytest.mark.parametrize("window", ["full", "ragged"])
@pytest.mark.parametrize("M,N", SHAPES)
def test_a_trace_and_bits_at_three_steps(fdr, M, N, window):
    """(a) rule NONE, n = 3, the four forms (the free-boundary ones with no weights, a 0/1 mask and fractional weights): the output is
    the existing call's, bit for bit; the trace is the model's to TRACE_TOL per entry and bit-equal between two calls"""
    rows, cols = (M, N) if window == "full" else _ragged(M, N)
    img = _picture(rows, cols, M + N)
    psf = centred_psf(dense_psf(5, 5), M, N)
    cases = [(False, False, "none"), (False, True, "none"), (True, False, "none"), (True, False, "mask"), (True, True, "frac")]
    bad, worst = [], 0.0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        for free, acc, wkind in cases:
            w = _weights(wkind, rows, cols)
            what = "%dx%d win %dx%d free=%d accel=%d weights=%s" % (M, N, rows, cols, free, acc, wkind)
            if free:
                assert sigma_margin(rlfree_state(img, psf, M, N, 0, w)["alpha"], SIGMA) >= SIGMA_MARGIN, what
            want = run_model(img, psf, M, N, 3, free, acc, w)
            got, res, trace = p.richardson_lucy_auto(img, 3, fdr.RL_STOP_NONE, free_boundary=free, accelerate=acc, weights=w)
            again = p.richardson_lucy_auto(img, 3, fdr.RL_STOP_NONE, free_boundary=free, accelerate=acc, weights=w)
            ref = _existing(p, img, 3, free, acc, w)
            e, ok = trace_ok(trace, want["trace"])
            worst = max(worst, e)
            print("RLS\ttrace\t%s\terr=%.3g\tres=%s\tkl=%s" % (what, e, trace[:, 0], trace[:, 1]))
            if (res.iterations_done, res.stopped) != (3, 0) or trace.shape != (3, 2):
                bad.append("%s: result %s" % (what, res))
            if not np.array_equal(got, ref):
                bad.append("%s: the output is not the existing call's" % what)
            if not ok:
                bad.append("%s: trace error %.3g > %.3g" % (what, e, TRACE_TOL))
            if not (np.array_equal(trace, again[2]) and np.array_equal(got, again[0])):
                bad.append("%s: two calls differ" % what)
    print("RLS\tworst\t%dx%d %s\terr=%.3g" % (M, N, window, worst))
    assert not bad, "\n".join(bad)


def test_a_guard_of_the_kl_sum(fdr):
    """(a) where c <= FDR_RL_TAU and d+ > 0 the KL term is c - d+ alone (guard_case of the model)"""
    M, N, d, psf = guard_case()
    want = run_model(d, psf, M, N, 3)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        got, res, trace = p.richardson_lucy_auto(d, 3, fdr.RL_STOP_NONE)
        assert np.array_equal(got, p.richardson_lucy(d, 3))
    e, ok = trace_ok(trace, want["trace"])
    print("RLS\ttrace\tguard case\terr=%.3g\tres=%s\tkl=%s" % (e, trace[:, 0], trace[:, 1]))
    assert ok, e


@pytest.fixture(scope="module")
def stop_runs(oracle):
    """the model's runs of check (b), shared by its cases: (noise, free, accel) -> (window, run)"""
    psf = oracle.motion_blur_kernel(9, 30.0)
    M, N = STOP_PLAN
    runs, cps = {}, {}
    for noise in ("gauss", "poisson"):
        cp, d = stop_scene(psf, noise)
        cps[noise] = cp
        for free, acc in FORMS:
            win = np.ascontiguousarray(d[: STOP_WINDOW[0], : STOP_WINDOW[1]]) if free else d
            runs[(noise, free, acc)] = (win, run_model(win, cp, M, N, STOP_N, free, acc))
    return cps, runs


@pytest.mark.parametrize("config", sorted(STOP_CONFIGS))
def test_b_the_stop(fdr, stop_runs, config):
    """(b) both rules (the residual one with sigma given and estimated), check_every 1 and 4, the four forms: the count and the flag
    are the model's, the output is the existing call's with that count, bit for bit.  Before the device runs, the model's
    stat_k / target must keep DECISION_MARGIN from 1 up to the stop."""
    noise, rule, kw = STOP_CONFIGS[config]
    cps, runs = stop_runs
    M, N = STOP_PLAN
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(cps[noise])
        for free, acc in FORMS:
            win, run = runs[(noise, free, acc)]
            tau = STOP_TAU[(config, free, acc)]
            for every, area in ((1, NORM_NONE), (4, NORM_CROPPED if acc else NORM_PADDED)):
                m = stop_model(run, rule, tau=tau, check_every=every, **kw)
                assert decision_margin(m) >= DECISION_MARGIN and m["stopped"] == 1, (config, free, acc)
                got, res, trace = p.richardson_lucy_auto(win, STOP_N, rule, tau=tau, check_every=every, free_boundary=free, accelerate=acc,
                                                         norm_area=area, **kw)
                what = "%s free=%d accel=%d every=%d norm=%d" % (config, free, acc, every, area)
                e, ok = trace_ok(trace, run["trace"])
                print("RLS\tstop\t%s\tdone=%d (model %d)\tstopped=%d\tsigma=%.6g (model %.6g)\tstatistic=%.6g\ttarget=%.6g\ttrace err=%.3g" %
                      (what, res.iterations_done, m["iterations_done"], res.stopped, res.sigma, m["sigma"], res.statistic, res.target, e))
                if not stop_ok(res.iterations_done, res.stopped, m):
                    bad.append("%s: stopped %d at %d, the model %d at %d" % (what, res.stopped, res.iterations_done, m["stopped"],
                                                                              m["iterations_done"]))
                    continue
                if not np.array_equal(got, _existing(p, win, res.iterations_done, free, acc, None, area)):
                    bad.append("%s: the output is not the existing call's at %d steps" % (what, res.iterations_done))
                if not ok or len(trace) != res.iterations_done:
                    bad.append("%s: trace error %.3g > %.3g or %d entries" % (what, e, TRACE_TOL, len(trace)))
                if not (abs(res.target / m["target"] - 1) <= 1e-6 and abs(res.statistic / m["statistic"] - 1) <= 10 * TRACE_TOL
                        and res.statistic <= res.target):
                    bad.append("%s: target %.9g (model %.9g), statistic %.9g (model %.9g)" % (what, res.target, m["target"], res.statistic,
                                                                                            m["statistic"]))
    assert not bad, "\n".join(bad)


def test_c_never_and_at_once(fdr, stop_runs):
    """(c) a tiny tau never fires: stopped = 0 and the n-step bits; a huge one fires at k = 0: iterations_done = check_every"""
    cps, runs = stop_runs
    M, N = STOP_PLAN
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(cps["gauss"])
        for free, acc in FORMS:
            win, _ = runs[("gauss", free, acc)]
            for rule, kw in ((fdr.RL_STOP_RESIDUAL, dict(sigma=0.005)), (fdr.RL_STOP_KL, dict(gain=2000.0))):
                what = "free=%d accel=%d rule=%d" % (free, acc, rule)
                got, res, trace = p.richardson_lucy_auto(win, 6, rule, tau=1e-6, check_every=4, free_boundary=free, accelerate=acc, **kw)
                if (res.iterations_done, res.stopped, len(trace)) != (6, 0, 6) or not np.array_equal(got, _existing(p, win, 6, free, acc)):
                    bad.append("%s never: %s" % (what, res))
                if not res.statistic > res.target:
                    bad.append("%s never: statistic %g <= target %g" % (what, res.statistic, res.target))
                for every in (1, 3):
                    got, res, trace = p.richardson_lucy_auto(win, 8, rule, tau=1e6, check_every=every, free_boundary=free, accelerate=acc, **kw)
                    if (res.iterations_done, res.stopped, len(trace)) != (every, 1, every) or \
                            not np.array_equal(got, _existing(p, win, every, free, acc)):
                        bad.append("%s at once, every %d: %s" % (what, every, res))
            got, res, trace = p.richardson_lucy_auto(win, 0, fdr.RL_STOP_RESIDUAL, sigma=0.005, free_boundary=free, accelerate=acc)
            if (res.iterations_done, res.stopped, len(trace)) != (0, 0, 0) or not np.array_equal(got, _existing(p, win, 0, free, acc)):
                bad.append("free=%d accel=%d n = 0: %s" % (free, acc, res))
    assert not bad, "\n".join(bad)


def test_dev_form(fdr, stop_runs):
    """the _dev form on strided device windows with the caller's trace: the bits and the trace of the host form, nothing stored
    outside the windows or past 2 iterations_done doubles; with a rule and without the caller's trace the same count"""
    import torch
    cps, runs = stop_runs
    M, N = STOP_PLAN
    n = 9
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(cps["gauss"])
        for free, acc in FORMS:
            win, _ = runs[("gauss", free, acc)]
            rows, cols = win.shape
            stride, ws, out_stride = cols + 5, cols + 2, cols + 3
            src = np.zeros((rows, stride), dtype=np.float32)
            src[:, :cols] = win
            d_in = torch.from_numpy(src).cuda()
            w = _weights("frac", rows, cols) if free else None
            d_w = None
            if free:
                wp = np.full((rows, ws), 7.0, dtype=np.float32)  # the padding must not be read
                wp[:, :cols] = w
                d_w = torch.from_numpy(wp).cuda()
            for rule, kw in ((fdr.RL_STOP_NONE, {}), (fdr.RL_STOP_RESIDUAL, dict(sigma=0.005, tau=1.3, check_every=2))):
                host = p.richardson_lucy_auto(win, n, rule, free_boundary=free, accelerate=acc, weights=w, norm_area=NORM_CROPPED, **kw)
                for with_trace in (True, False):
                    d_out = torch.full((rows + 1, out_stride), float("nan"), dtype=torch.float32, device="cuda")
                    d_tr = torch.full((2 * n + 2,), float("nan"), dtype=torch.float64, device="cuda")
                    res = p.richardson_lucy_auto_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), out_stride, n, rule,
                                                     free_boundary=free, accelerate=acc, d_weights=d_w.data_ptr() if free else None, wstride=ws,
                                                     norm_area=NORM_CROPPED, d_trace=d_tr.data_ptr() if with_trace else None, **kw)
                    torch.cuda.synchronize()
                    out, tr = d_out.cpu().numpy(), d_tr.cpu().numpy()
                    what = "free=%d accel=%d rule=%d trace=%d" % (free, acc, rule, with_trace)
                    assert np.all(np.isnan(out[:rows, cols:])) and np.all(np.isnan(out[rows:, :])), what
                    assert res.iterations_done == host[1].iterations_done and res.stopped == host[1].stopped, (what, res, host[1])
                    assert np.array_equal(out[:rows, :cols], host[0]), what
                    done = res.iterations_done
                    if with_trace:
                        assert np.array_equal(tr[: 2 * done].reshape(done, 2), host[2]) and np.all(np.isnan(tr[2 * done:])), what
                    else:
                        assert np.all(np.isnan(tr)), what
                    if rule != fdr.RL_STOP_NONE:
                        assert res.stopped == 1 and 0 < done < n and done % 2 == 0, (what, res)


def test_d_refusals(fdr):
    """(d) every refusal of the auto call returns FDR_ERR_ARG before any device work and leaves the plan working"""
    import torch
    L = fdr.lib
    M = N = 64
    img = _picture(M, N, 1)
    out = np.empty((M, N), dtype=np.float32)
    w = np.ones((M, N), dtype=np.float32)
    res = fdr.RlAutoResultC()
    psf = centred_psf(dense_psf(5, 5), M, N)

    def prm(n=2, free=0, acc=0, rule=0, sigma=0.01, gain=100.0, tau=1.0, every=1, area=2, cov=1e-2, orows=0, ocols=0):
        return ctypes.byref(fdr.RlAutoParams(n, free, acc, rule, sigma, gain, tau, every, area, cov, orows, ocols))

    def call(p, pr, rows=16, cols=16, wp=None, ip=None, op=None, rp=True):
        return L.fdr_richardson_lucy_auto_f32(p._h, img.ctypes.data if ip is None else ip, rows, cols, N, wp, N, out.ctypes.data if op is None else op,
                                              N, pr, ctypes.byref(res) if rp else None, None)

    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        assert call(p, prm()) == -4 and b"operator PSF" in L.fdr_last_error()  # the underlying form's refusal
        p.set_operator_psf(psf)
        before = p.richardson_lucy_auto(img, 4, fdr.RL_STOP_RESIDUAL, sigma=0.01, accelerate=True)
        assert call(p, None) == -1 and call(p, prm(), rp=False) == -1 and call(p, prm(), ip=0) == -1
        for rule in (3, -1, 7):
            assert call(p, prm(rule=rule)) == -1 and b"unknown rule" in L.fdr_last_error(), rule
        for gain in (0.0, -1.0, float("nan"), float("inf")):
            assert call(p, prm(rule=2, gain=gain)) == -1 and b"gain" in L.fdr_last_error(), gain
        for bad in (-1.0, float("nan"), float("inf")):
            assert call(p, prm(rule=1, sigma=bad)) == -1 and b"sigma and tau" in L.fdr_last_error(), bad
            assert call(p, prm(rule=1, tau=bad)) == -1 and b"sigma and tau" in L.fdr_last_error(), bad
        assert call(p, prm(every=-1)) == -1 and b"check_every" in L.fdr_last_error()
        assert call(p, prm(), wp=w.ctypes.data) == -1 and b"no weights" in L.fdr_last_error()
        assert call(p, prm(orows=17, ocols=16)) == -1 and call(p, prm(orows=16, ocols=15)) == -1
        assert call(p, prm(rule=1, sigma=0.0), rows=2, cols=16) == -1 and b"noise estimate" in L.fdr_last_error()
        # what the underlying forms refuse
        assert call(p, prm(n=-1)) == -1 and call(p, prm(area=3)) == -1 and call(p, prm(), rows=65) == -1
        assert call(p, prm(), op=img.ctypes.data) == -1 and b"overlaps" in L.fdr_last_error()
        assert call(p, prm(free=1, cov=0.0, orows=16, ocols=16)) == -1 and call(p, prm(free=1, orows=15, ocols=16)) == -1
        assert call(p, prm(free=1, orows=16, ocols=16), wp=w.ctypes.data, op=w.ctypes.data) == -1 and b"overlaps the weights" in L.fdr_last_error()
        # the _dev form: a trace range that overlaps a window
        vp = ctypes.c_void_p
        d = torch.from_numpy(img).cuda()
        o = torch.zeros((M, N), dtype=torch.float32, device="cuda")
        dw = torch.ones((M, N), dtype=torch.float32, device="cuda")
        t = torch.zeros(64, dtype=torch.float64, device="cuda")

        def dev(pr, tp, wp=None):
            return L.fdr_richardson_lucy_auto_f32_dev(p._h, vp(d.data_ptr()), 16, 16, N, wp, N, vp(o.data_ptr()), N, pr, ctypes.byref(res), vp(tp), None)

        assert dev(prm(n=4), d.data_ptr() + 8) == -1 and b"trace overlaps the input" in L.fdr_last_error()
        assert dev(prm(n=4), o.data_ptr() + 4 * (15 * N + 15) - 4) == -1 and b"trace overlaps the output" in L.fdr_last_error()
        assert dev(prm(n=4), o.data_ptr() - 8 * 8 + 4) == -1 and b"trace overlaps the output" in L.fdr_last_error()  # its last double
        assert dev(prm(n=4, free=1, orows=16, ocols=16), dw.data_ptr(), vp(dw.data_ptr())) == -1 and b"trace overlaps the weights" in L.fdr_last_error()
        assert dev(prm(n=4), t.data_ptr()) == 0
        torch.cuda.synchronize()
        after = p.richardson_lucy_auto(img, 4, fdr.RL_STOP_RESIDUAL, sigma=0.01, accelerate=True)
        assert np.array_equal(before[0], after[0]) and before[1] == after[1] and np.array_equal(before[2], after[2])


def test_cli_rl_auto(fdr, tmp_path):
    """tools/cli/gpu --rl auto: the printed count is that of richardson_lucy_auto on the mean of B, G and R with the same arguments, and
    the planes (--raw-out) are those of --rl k: three richardson_lucy(..., NORM_PADDED) calls with that count; the options of
    --rl auto without it, and a kl rule without its gain, are refused"""
    import os
    import re
    import subprocess
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(root, "tools", "cli", "gpu")
    png = os.path.join(root, "tests", "golden", "car_blurred.png")
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    psf = fdr.motionBlurKernel(40, 45.0)
    out_png, out_raw = str(tmp_path / "rls.png"), str(tmp_path / "rls.f32")
    r = subprocess.run([gpu, png, "40", "45", "--rl", "auto", "--rl-max", "12", "--rl-check", "2", "--sigma", "0.02", "--accel", "--out", out_png,
                        "--raw-out", out_raw], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^rl: iterations (\d+) of 12 rule residual sigma (\S+) statistic (\S+) target (\S+) stopped ([01])$", r.stdout, re.M)
    assert m, r.stdout
    k = int(m.group(1))
    assert "Deblurring 3 channels took(gpu[richardson-lucy %d accelerated]): " % k in r.stdout, r.stdout
    planes = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
    gray = ((rgb[:, :, 2] + rgb[:, :, 1]) + rgb[:, :, 0]) / np.float32(3.0)  # (B + G + R) / 3 in float32, as the tool forms it
    size = fdr._rl_plan_size(h, w)
    with fdr.Plan(size[0], size[1], fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        _, res, _ = p.richardson_lucy_auto(gray, 12, fdr.RL_STOP_RESIDUAL, sigma=0.02, check_every=2, accelerate=True, norm_area=fdr.NORM_PADDED)
        print("RLS\tcli\t%s\tlibrary %s" % (m.group(0), res))
        assert (res.iterations_done, res.stopped) == (k, int(m.group(5)))
        assert float(m.group(3)) == pytest.approx(res.statistic, rel=1e-8) and float(m.group(4)) == pytest.approx(res.target, rel=1e-8)
        for i, c in enumerate((2, 1, 0)):  # B, G, R
            want = p.richardson_lucy(np.ascontiguousarray(rgb[:, :, c]), k, fdr.NORM_PADDED, accelerate=True)
            assert np.array_equal(planes[i], want), (i, float(np.abs(planes[i] - want).max()))
    for args in (["--rl", "5", "--rl-max", "9"], ["--rl-stop", "kl", "--gain", "100"], ["--rl", "auto", "--rl-stop", "kl"],
                 ["--rl", "auto", "--rl-stop", "gcv"], ["--rl", "auto", "--gain", "3"], ["--rl", "auto", "--rl-check", "-1"]):
        r = subprocess.run([gpu, png, "40", "45"] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "Usage" in r.stdout, (args, r.returncode, r.stdout[-300:])
