"""Choosing the regularisation weight (fdr_noise_sigma_f32*, fdr_reg_curve_f32*, fdr_choose_reg_f32*) on the MI355X, against the
float64 model of tests/_reg_model.py: the residual / trace curve candidate by candidate on tone and random pictures for every
column length of the power pass, strided and tiny windows, Parseval, the noise estimate, the search by both methods on both
weights, the range's ends, the all-zero window, the restoration quality of the chosen weight, the refusals, determinism and
isolation from the other calls.  Each case prints a `REG` line with its measured values (pytest -s)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _pad_model
import _reg_model as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

KS = [c[0] for c in rm.CANDIDATES]
GS = [c[1] for c in rm.CANDIDATES]


def _model_curves(psf, M, N):
    """q and q^2 of every candidate on the full spectrum, once per (plan, PSF): (trace[], lambda P: rho[])"""
    h2, l2, w = rm.operator_terms(psf, M, N)
    qs = [rm.q_of(h2, l2, K, g) for K, g in rm.CANDIDATES]
    tr = np.array([float(q.sum()) for q in qs])
    q2 = [q * q for q in qs]
    return tr, lambda P: np.array([float(np.sum(P * x)) for x in q2])


def _check_curve(what, rho, tr, rho_m, tr_m, sum_d2):
    er, et = rm.curve_errors(rho, tr, rho_m, tr_m, sum_d2)
    assert np.all(np.isfinite(rho)) and np.all(np.isfinite(tr)), what
    return er, et


@pytest.mark.parametrize("M,N", rm.CURVE_PLANS)
def test_curve_per_bin(fdr, oracle, M, N):
    worst = (0.0, 0.0, "", "")
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for pname, psf in rm.curve_psfs(oracle, M, N):
            p.set_operator_psf(psf)
            tr_m, rho_of = _model_curves(psf, M, N)
            for name, d in rm.curve_pictures(M, N):
                rho, tr = p.reg_curve(d, KS, GS)
                P = rm.power(d, M, N)
                sum_d2 = float(np.sum(d.astype(np.float64) ** 2))
                er, et = _check_curve((pname, name), rho, tr, rho_of(P), tr_m, sum_d2)
                assert rho[0] == 0.0 and tr[0] == 0.0, "the pair (0, 0) leaves nothing"
                if er > worst[0]:
                    worst = (er, worst[1], "%s / %s" % (pname, name), worst[3])
                if et > worst[1]:
                    worst = (worst[0], et, worst[2], "%s / %s" % (pname, name))
    print("REG\tcurve\t%dx%d\trho=%.3g (%s)\ttrace=%.3g (%s)" % (M, N, worst[0], worst[2], worst[1], worst[3]))
    assert worst[0] <= rm.CURVE_TOL and worst[1] <= rm.CURVE_TOL, worst


@pytest.mark.parametrize("M,N", rm.WINDOW_PLANS)
def test_curve_windows(fdr, oracle, M, N):
    import torch
    worst = 0.0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        for pname, psf in rm.curve_psfs(oracle, M, N):
            p.set_operator_psf(psf)
            tr_m, rho_of = _model_curves(psf, M, N)
            for rows, cols, stride in ((M - 3, N - 5, N + 7), (3, 3, N + 7), (3, 3, 3)):
                buf = rm.random_picture(M, N, rows, cols, stride)
                d = buf[:, :cols]
                d_buf = torch.from_numpy(buf).cuda()
                rho, tr = p.reg_curve_dev(d_buf.data_ptr(), rows, cols, stride, KS, GS)
                host = p.reg_curve(np.ascontiguousarray(d), KS, GS)
                assert np.array_equal(rho, host[0]) and np.array_equal(tr, host[1]), "the strided _dev form and the host form differ"
                sum_d2 = float(np.sum(d.astype(np.float64) ** 2))
                er, et = _check_curve((pname, rows, cols), rho, tr, rho_of(rm.power(d, M, N)), tr_m, sum_d2)
                worst = max(worst, er, et)
    print("REG\twindow\t%dx%d\tmax=%.3g" % (M, N, worst))
    assert worst <= rm.CURVE_TOL


@pytest.mark.parametrize("M,N", rm.CURVE_PLANS)
def test_parseval(fdr, oracle, M, N):
    """q = 1 at K = 1e30: rho is the picture's energy, trace the number of bins"""
    d = rm.random_picture(M, N)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf(rm.curve_psfs(oracle, M, N)[0][1])
        rho, tr = p.reg_curve(d, [rm.PARSEVAL_K], [0.0])
    sum_d2 = float(np.sum(d.astype(np.float64) ** 2))
    er, et = abs(rho[0] - sum_d2) / sum_d2, abs(tr[0] - M * N) / (M * N)
    print("REG\tparseval\t%dx%d\trho=%.3g\ttrace=%.3g" % (M, N, er, et))
    assert er <= rm.CURVE_TOL and et <= rm.CURVE_TOL


@pytest.mark.parametrize("rows,cols,stride", rm.NOISE_WINDOWS)
def test_noise_against_model(fdr, rows, cols, stride):
    import torch
    buf = rm.random_picture(rows, cols, rows, cols, stride) * np.float32(255)
    d = np.ascontiguousarray(buf[:, :cols])
    want = rm.noise_sigma(d)
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        d_buf = torch.from_numpy(buf).cuda()
        got_dev = p.noise_sigma_dev(d_buf.data_ptr(), rows, cols, stride)
        got = p.noise_sigma(d)
    err = abs(got - want) / want
    print("REG\tnoise\t%dx%d stride %d\tsigma=%.6g\terr=%.3g" % (rows, cols, stride, got, err))
    assert got == got_dev, "the strided _dev form and the host form differ"
    assert err <= rm.NOISE_TOL


def test_noise_refusals(fdr):
    d = np.ones((8, 8), dtype=np.float32)
    s = ctypes.c_double()
    for rows, cols, stride in ((2, 8, 8), (8, 2, 8), (0, 0, 0), (8, 8, 7)):
        assert fdr.lib.fdr_noise_sigma_f32(0, d.ctypes.data_as(ctypes.c_void_p), rows, cols, stride, ctypes.byref(s)) == -1
    assert fdr.lib.fdr_noise_sigma_f32(0, None, 8, 8, 8, ctypes.byref(s)) == -1
    assert fdr.lib.fdr_noise_sigma_f32(0, d.ctypes.data_as(ctypes.c_void_p), 8, 8, 8, None) == -1
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        assert p.noise_sigma(d) == 0.0  # a flat picture


CHOICE_CASES = [(s, l, m, q) for s in rm.CHOICE_SCENES for l in rm.CHOICE_NOISE for m in (rm.REG_DISCREPANCY, rm.REG_GCV)
                for q in (rm.REG_PARAM_K, rm.REG_PARAM_GAMMA)]
_NAMES = {rm.REG_DISCREPANCY: "discrepancy", rm.REG_GCV: "gcv", "p0": "K", "p1": "gamma"}


@pytest.fixture(scope="module")
def choice_plan(fdr):
    n = rm.CHOICE_SIZE
    with fdr.Plan(n, n, fdr.MODE_FAST) as p:
        p.set_operator_psf(rm.choice_psf())
        yield p


@pytest.fixture(scope="module")
def device_choices(choice_plan):
    """every choice of CHOICE_CASES, made once: the agreement test and the quality test share them"""
    out = {}
    for scene, level, method, param in CHOICE_CASES:
        _, b = rm.choice_case(scene, level)
        out[(scene, level, method, param)] = choice_plan.choose_regularisation(b, method=method, param=param)
    return out


@pytest.mark.parametrize("scene,level,method,param", CHOICE_CASES)
def test_choice_against_model(device_choices, scene, level, method, param):
    n = rm.CHOICE_SIZE
    _, b = rm.choice_case(scene, level)
    state = rm.choice_state(scene, level)
    got = device_choices[(scene, level, method, param)]
    want = rm.choose(b, rm.choice_psf(), n, n, method=method, param=param, state=state)
    what = "%s %g %s %s" % (scene, level, _NAMES[method], _NAMES["p%d" % param])
    assert (got.flags, got.evaluations) == (want.flags, want.evaluations), what
    assert all(math.isfinite(x) for x in got[:5]), what
    if method == rm.REG_DISCREPANCY:
        err = abs(math.log(got.value / want.value))
        print("REG\tchoice\t%s\tvalue=%.6g model=%.6g\tlog err=%.3g\tsigma=%.6g model=%.6g" % (what, got.value, want.value, err, got.sigma,
                                                                                            want.sigma))
        assert abs(got.sigma - want.sigma) <= rm.NOISE_TOL * want.sigma, what
        assert err <= rm.VALUE_LOG_TOL, what
    else:
        rho, tr = rm.curve_from(state[0], state[1], *[[x] for x in rm.pair_of(param, got.value)])
        excess = rm.gcv(rho[0], tr[0], n, n) / want.gcv - 1.0
        print("REG\tchoice\t%s\tvalue=%.6g model=%.6g\tgcv excess=%.3g" % (what, got.value, want.value, excess))
        assert got.sigma == 0.0, what
        assert excess <= rm.GCV_EXCESS_TOL, what
    # what is reported beside the value is the curve at the candidate nearest to it
    assert abs(got.gcv - n * n * got.residual / got.trace ** 2) <= 1e-12 * got.gcv, what


@pytest.mark.parametrize("scene,level,method,param", CHOICE_CASES)
def test_quality_of_choice(fdr, device_choices, scene, level, method, param):
    """restoring through fdr_set_psf_cls + fdr_wiener_f32 with the device's choice, against the best weight of an 81-point grid"""
    n = rm.CHOICE_SIZE
    truth, b = rm.choice_case(scene, level)
    c = device_choices[(scene, level, method, param)]
    K, gamma = rm.pair_of(param, c.value)
    with fdr.Plan(n, n, fdr.MODE_FAST) as p:
        p.set_psf(rm.choice_psf(), K=K, gamma=gamma)
        x = p.wiener(b, norm_area=fdr.NORM_PADDED)
    # fdr_wiener_f32 returns the min-max normalised plane: undo it with the model's extremes (an affine map, exact to rounding)
    raw = rm.restore(b, K, gamma)
    x = x.astype(np.float64) * (raw.max() - raw.min()) + raw.min()
    got, blurred = _pad_model.psnr(x, truth), _pad_model.psnr(b, truth)
    best, at = rm.best_psnr(scene, level, param)
    what = "%s %g %s %s" % (scene, level, _NAMES[method], _NAMES["p%d" % param])
    print("REG\tquality\t%s\tvalue=%.4g\tpsnr=%.2f\tbest=%.2f at %.3g\tblurred=%.2f" % (what, c.value, got, best, at, blurred))
    margin = rm.QUALITY_MARGIN.get((method, param))
    if margin is None:
        return  # GCV with K: reported, not judged
    assert got >= best - margin, what
    if rm.beats_blurred_required(method, param, scene, level):
        assert got > blurred, what


def test_choice_on_a_window(choice_plan):
    """a window smaller than the plan: the target counts the window's pixels, not the plan's"""
    n = rm.CHOICE_SIZE
    _, b = rm.choice_case(*rm.WINDOW_CHOICE[:2])
    w = np.ascontiguousarray(b[:rm.WINDOW_CHOICE[2], :rm.WINDOW_CHOICE[3]])
    state = rm.power(w, n, n), rm.operator_terms(rm.choice_psf(), n, n)
    for param in (rm.REG_PARAM_K, rm.REG_PARAM_GAMMA):
        got = choice_plan.choose_regularisation(w, method=rm.REG_DISCREPANCY, param=param)
        want = rm.choose(w, rm.choice_psf(), n, n, method=rm.REG_DISCREPANCY, param=param, state=state)
        err = abs(math.log(got.value / want.value))
        print("REG\tchoice\twindow %dx%d param %d\tvalue=%.6g model=%.6g\tlog err=%.3g" % (w.shape + (param, got.value, want.value, err)))
        assert (got.flags, got.evaluations) == (want.flags, want.evaluations)
        assert err <= rm.VALUE_LOG_TOL


def test_choice_hits_the_ends(choice_plan):
    _, b = rm.choice_case("blocks", 0.01)
    low = choice_plan.choose_regularisation(b, method=rm.REG_DISCREPANCY, param=rm.REG_PARAM_GAMMA, fixed=1.0, sigma=1e-6)
    assert (low.flags, low.value, low.evaluations) == (rm.REG_AT_LOW, 1e-8, 32), low
    high = choice_plan.choose_regularisation(b, method=rm.REG_DISCREPANCY, param=rm.REG_PARAM_K, sigma=1e3)
    assert (high.flags, high.value, high.evaluations) == (rm.REG_AT_HIGH, 1e2, 32), high
    assert high.sigma == 1e3 and abs(low.sigma - 1e-6) < 1e-12


def test_all_zero_window(choice_plan):
    z = np.zeros((100, 200), dtype=np.float32)
    for param in (rm.REG_PARAM_K, rm.REG_PARAM_GAMMA):
        d = choice_plan.choose_regularisation(z, method=rm.REG_DISCREPANCY, param=param)
        g = choice_plan.choose_regularisation(z, method=rm.REG_GCV, param=param)
        assert (d.value, d.flags, d.residual, d.sigma) == (1e2, rm.REG_AT_HIGH, 0.0, 0.0), d
        assert (g.value, g.flags, g.residual, g.gcv) == (1e-8, rm.REG_AT_LOW, 0.0, 0.0), g
        assert not any(math.isnan(x) for x in d[:5] + g[:5])
        want = rm.choose(z, rm.choice_psf(), rm.CHOICE_SIZE, rm.CHOICE_SIZE, method=rm.REG_GCV, param=param)
        assert (g.flags, g.evaluations) == (want.flags, want.evaluations)
    rho, tr = choice_plan.reg_curve(z, KS, GS)
    assert not np.any(rho) and np.all(np.isfinite(tr))


def test_arguments_and_grid(choice_plan):
    """non-default ranges, grids and rounds against the model"""
    n = rm.CHOICE_SIZE
    _, b = rm.choice_case("pad scene", 0.01)
    state = rm.choice_state("pad scene", 0.01)
    for kw in (dict(n_grid=4, refine=0), dict(n_grid=64, refine=8, lo=1e-6, hi=10.0), dict(n_grid=17, refine=1, tau=1.5, fixed=float(np.float32(1e-3))),
               dict(n_grid=5, refine=3, sigma=float(np.float32(0.02)))):
        for method in (rm.REG_DISCREPANCY, rm.REG_GCV):
            got = choice_plan.choose_regularisation(b, method=method, **kw)
            want = rm.choose(b, rm.choice_psf(), n, n, method=method, state=state, **kw)
            assert (got.flags, got.evaluations) == (want.flags, want.evaluations), (kw, method)
            if method == rm.REG_DISCREPANCY:
                assert abs(math.log(got.value / want.value)) <= rm.VALUE_LOG_TOL, (kw, got, want)
            else:
                rho, tr = rm.curve_from(state[0], state[1], [0.0], [got.value]) if "fixed" not in kw else rm.curve_from(
                    state[0], state[1], [kw["fixed"]], [got.value])
                assert rm.gcv(rho[0], tr[0], n, n) / want.gcv - 1.0 <= rm.GCV_EXCESS_TOL, (kw, got, want)


def test_refusals_leave_the_plan_usable(fdr, choice_plan, oracle):
    p = choice_plan
    _, b = rm.choice_case("blocks", 0.01)
    before = p.choose_regularisation(b)
    nan, inf = float("nan"), float("inf")
    bad = [dict(method=2), dict(method=-1), dict(param=2), dict(param=-1), dict(fixed=-1.0), dict(fixed=nan), dict(fixed=inf),
           dict(sigma=-1.0), dict(sigma=nan), dict(tau=-0.5), dict(tau=inf), dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0), dict(lo=-1.0, hi=1.0),
           dict(lo=0.0, hi=1.0), dict(lo=1e-3, hi=inf), dict(lo=nan, hi=1.0), dict(n_grid=3), dict(n_grid=65), dict(n_grid=-1),
           dict(refine=9), dict(refine=-2)]
    for kw in bad:
        with pytest.raises(fdr.FdrError) as e:
            p.choose_regularisation(b, **kw)
        assert e.value.code == -1, kw
    vp = ctypes.c_void_p
    img = b.ctypes.data_as(vp)
    prm, out = fdr.RegParams(1, 1, 0.0, 0.0, 0.0, 0.0, 0.0, 0, -1), fdr.RegChoiceC()
    n = rm.CHOICE_SIZE
    lib = fdr.lib
    assert lib.fdr_choose_reg_f32(p._h, None, n, n, n, ctypes.byref(prm), ctypes.byref(out)) == -1
    assert lib.fdr_choose_reg_f32(p._h, img, n, n, n, None, ctypes.byref(out)) == -1
    assert lib.fdr_choose_reg_f32(p._h, img, n, n, n, ctypes.byref(prm), None) == -1
    assert lib.fdr_choose_reg_f32(None, img, n, n, n, ctypes.byref(prm), ctypes.byref(out)) == -1
    for rows, cols, stride in ((n + 1, n, n), (n, n + 1, n + 1), (n, n, n - 1), (0, n, n)):
        assert lib.fdr_choose_reg_f32(p._h, img, rows, cols, stride, ctypes.byref(prm), ctypes.byref(out)) == -1
    prm_d = fdr.RegParams(0, 1, 0.0, 0.0, 0.0, 0.0, 0.0, 0, -1)  # the discrepancy principle estimates the noise: 3 x 3 at least
    assert lib.fdr_choose_reg_f32(p._h, img, 2, n, n, ctypes.byref(prm_d), ctypes.byref(out)) == -1
    assert lib.fdr_choose_reg_f32(p._h, img, 2, n, n, ctypes.byref(prm), ctypes.byref(out)) == 0  # GCV needs no noise estimate
    k1, r1 = (ctypes.c_double * 1)(0.1), (ctypes.c_double * 1)()
    for Ks, gs, cnt in (([-1.0], [0.0], 1), ([0.0], [nan], 1), ([inf], [0.0], 1), ([0.0], [0.0], 0), ([0.0], [0.0], 4097)):
        Ka, ga = (ctypes.c_double * 1)(*Ks), (ctypes.c_double * 1)(*gs)
        assert lib.fdr_reg_curve_f32(p._h, img, n, n, n, Ka, ga, cnt, r1, r1) == -1
    assert lib.fdr_reg_curve_f32(p._h, img, n, n, n, None, k1, 1, r1, r1) == -1
    assert lib.fdr_reg_curve_f32(p._h, img, n, n, n, k1, k1, 1, None, r1) == -1
    # plans the operator does not run on: FDR_ERR_ARG; tables-only plans and plans without an operator PSF: FDR_ERR_STATE
    small = np.ones((8, 16), dtype=np.float32)
    for M, N, mode, flags in ((64, 64, fdr.MODE_PARITY, 0), (64, 64, fdr.MODE_FAST, fdr.FLAG_SIMPLE_PATH), (64, 64, fdr.MODE_FAST, fdr.FLAG_FULL_SPECTRUM),
                              (64, 16, fdr.MODE_FAST, 0), (60, 64, fdr.MODE_FAST, fdr.FLAG_MIXED_RADIX)):
        with fdr.Plan(M, N, mode, flags=flags) as q:
            for call in (lambda: q.choose_regularisation(small), lambda: q.reg_curve(small, [0.1], [0.0])):
                with pytest.raises(fdr.FdrError) as e:
                    call()
                assert e.value.code == -1, (M, N, mode, flags)
    with fdr.Plan(64, 64, fdr.MODE_FAST) as q:
        with pytest.raises(fdr.FdrError) as e:
            q.choose_regularisation(small)
        assert e.value.code == -4
        q.set_operator_psf(oracle.motion_blur_kernel(15, 30.0))
        assert q.choose_regularisation(small).evaluations == 96
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as q:
        with pytest.raises(fdr.FdrError) as e:
            q.reg_curve(small, [0.1], [0.0])
        assert e.value.code == -4
    assert p.choose_regularisation(b) == before, "a refusal changed the plan"


def test_repeat_is_bit_identical_and_other_state_untouched(fdr, oracle):
    n = rm.CHOICE_SIZE
    _, b = rm.choice_case("pad scene", 0.01)
    psf = oracle.motion_blur_kernel(15, 30.0)
    with fdr.Plan(n, n, fdr.MODE_FAST) as p:
        p.set_psf(psf, K=0.01, gamma=0.02)
        p.set_operator_psf(psf)
        before = (p.wiener(b), p.blur(b), p.richardson_lucy(b, 3))
        first = [p.choose_regularisation(b, method=m, param=q) for m in (0, 1) for q in (0, 1)]
        curve = p.reg_curve(b, KS, GS)
        sigma = p.noise_sigma(b)
        after = (p.wiener(b), p.blur(b), p.richardson_lucy(b, 3))
        for x, y in zip(before, after):
            assert x.tobytes() == y.tobytes(), "a choice changed the result of another call"
        again = [p.choose_regularisation(b, method=m, param=q) for m in (0, 1) for q in (0, 1)]
        curve2 = p.reg_curve(b, KS, GS)
        assert first == again and sigma == p.noise_sigma(b)
        assert curve[0].tobytes() == curve2[0].tobytes() and curve[1].tobytes() == curve2[1].tobytes()
    with fdr.Plan(n, n, fdr.MODE_FAST) as p:  # a fresh plan, no CLS filter before it: the Laplacian table is built by the call itself
        p.set_operator_psf(psf)
        assert [p.choose_regularisation(b, method=m, param=q) for m in (0, 1) for q in (0, 1)] == first


def test_module_level_call(fdr):
    n = rm.CHOICE_SIZE
    _, b = rm.choice_case("blocks", 0.01)
    psf = rm.choice_psf()
    with fdr.Plan(n, n, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        want = p.choose_regularisation(b[:400, :300])
    got = fdr.chooseRegularisation(b[:400, :300], psf)
    assert got == want
    rgb = np.stack([b, b * np.float32(0.5), b * np.float32(0.25)], axis=2)
    mean = rgb.mean(axis=2, dtype=np.float32)
    with fdr.Plan(n, n, fdr.MODE_FAST) as p:
        p.set_operator_psf(psf)
        assert fdr.chooseRegularisation(rgb, psf, method=fdr.REG_DISCREPANCY, param=fdr.REG_PARAM_K) == p.choose_regularisation(
            mean, method=fdr.REG_DISCREPANCY, param=fdr.REG_PARAM_K)


_REG_LINE = r"^regularisation: K (\S+) gamma (\S+) sigma (\S+) method (\S+) flags (\d+)$"


@pytest.mark.parametrize("option,method", [("--cls", "gcv"), ("--k", "discrepancy")])
def test_cli_round_trip(fdr, tmp_path, option, method):
    """tools/cli/gpu <img> L A --cls auto / --k auto: one `regularisation:` line, then exactly the run with the printed numbers"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")
    png = os.path.join(GOLDEN_DIR, "car_blurred.png")
    a_png, b_png = str(tmp_path / "auto.png"), str(tmp_path / "given.png")
    r = subprocess.run([gpu, png, "40", "45", option, "auto", "--out", a_png], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(_REG_LINE, r.stdout, re.M)
    assert m, r.stdout
    K, gamma, sigma, meth, flags = m.groups()
    print("REG\tcli\t%s auto\tK=%s gamma=%s sigma=%s method=%s flags=%s" % (option, K, gamma, sigma, meth, flags))
    assert meth == method and flags == "0", r.stdout
    searched, other = (gamma, K) if option == "--cls" else (K, gamma)
    assert 1e-8 < float(searched) < 1e2 and float(other) == 0.0
    r2 = subprocess.run([gpu, png, "40", "45", "--cls", gamma, "--k", K, "--out", b_png], capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert "regularisation:" not in r2.stdout
    assert open(a_png, "rb").read() == open(b_png, "rb").read(), "auto wrote another picture than the printed K and gamma"
    # the line's numbers are those of the library call on the same mean picture
    from PIL import Image
    img = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32)[:, :, ::-1] / np.float32(255)
    mean = (img[:, :, 0] + img[:, :, 1] + img[:, :, 2]) / np.float32(3)
    c = fdr.chooseRegularisation(mean, fdr.motionBlurKernel(40, 45.0), method=fdr.REG_GCV if method == "gcv" else fdr.REG_DISCREPANCY,
                                 param=fdr.REG_PARAM_GAMMA if option == "--cls" else fdr.REG_PARAM_K)
    assert np.float32(float(searched)) == np.float32(c.value), (searched, c)


def test_cli_usage(tmp_path):
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")
    png = os.path.join(GOLDEN_DIR, "car_blurred.png")
    for extra in (["--cls", "auto", "--k", "auto"], ["--reg", "gcv"], ["--sigma", "0.01"], ["--k", "auto", "--reg", "lcurve"], ["--k", "-1"]):
        r = subprocess.run([gpu, png, "40", "45"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "Usage" in r.stdout, extra
