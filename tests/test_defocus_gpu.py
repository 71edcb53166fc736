"""The defocus estimate (fdr_psf_disk*, fdr_estimate_defocus_f32*, fdr_estimate_blur_f32*) on the MI355X, against the float64 model of
tests/_defocus_model.py: the disk PSF bit for bit, the angular-median profile on small, strided, large and mixed-radix plans and at
every kind of angle count, the pick and the recovered radius, the combined call against the two single calls, a restoration end to
end, determinism, allocations, isolation from the other calls' state and the refusals.  Each case prints a `DEFOCUS` line with its
measured values (pytest -s)."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import _cls_model
import _defocus_model as dm
import _motion_model as mm
import _reg_model as rm
from _spectral import tone_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def _golden(name):
    return mm.load_golden(os.path.join(GOLDEN_DIR, name)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _defocused(rows, cols, R, seed):
    return dm.defocused_scene(rows, cols, R, seed).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _model_cepstrum(key, M, N):
    return mm.cepstrum_model(_PICTURES[key]().astype(np.float64), M, N)


_PICTURES = {
    "tone16": lambda: tone_image(32, 32, 5, 16, 16) * np.float32(255),
    "tone37": lambda: tone_image(64, 128, 9, 37, 101) * np.float32(255),
    "disk5": lambda: _defocused(512, 512, 5, 31),
    "cat": lambda: _golden("cat_blurred.png"),
    "const": lambda: np.full((100, 120), 7.0, dtype=np.float32),
}


def _step_for(n):
    """an angle step with ceil(180 / step) = n exactly"""
    step = 180.0 / n
    while math.ceil(180.0 / step) > n:
        step = math.nextafter(step, math.inf)
    assert math.ceil(180.0 / step) == n
    return step


DISK_CASES = [(1, 0.5), (3, 0.5), (3, 1.5), (5, 2.0), (8, 3.3), (9, 4.0), (9, 4.5), (31, 13.0), (256, 127.5), (256, 0.75)]


def test_psf_disk_bit_for_bit(fdr):
    import torch
    side = torch.cuda.Stream()
    for size, R in DISK_CASES:
        want = dm.disk(size, R)
        buf = torch.full((size * size + 7,), float("nan"), dtype=torch.float32, device="cuda")
        assert fdr.lib.fdr_psf_disk_dev(0, size, R, ctypes.c_void_p(buf.data_ptr()), None) == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[:size * size].reshape(size, size), want), (size, R)
        assert np.all(np.isnan(got[size * size:])), "wrote past the PSF"
        # on a side stream, into an offset pointer
        buf2 = torch.full((size * size + 7,), float("nan"), dtype=torch.float32, device="cuda")
        assert fdr.lib.fdr_psf_disk_dev(0, size, R, ctypes.c_void_p(buf2.data_ptr() + 12), ctypes.c_void_p(side.cuda_stream)) == 0
        side.synchronize()
        got2 = buf2.cpu().numpy()
        assert np.array_equal(got2[3:3 + size * size].reshape(size, size), want) and np.all(np.isnan(got2[:3])), (size, R)
        assert np.array_equal(fdr.psf_disk(size, R), want), "the host form differs"
        print("DEFOCUS\tdisk\tsize %d R=%.2f\tcentre=%.6g sum=%.8f" % (size, R, want[size // 2, size // 2], want.astype(np.float64).sum()))


def test_psf_disk_refusals_and_setters(fdr):
    import torch
    L = fdr.lib
    buf = torch.zeros(256 * 256, dtype=torch.float32, device="cuda")
    hbuf = np.zeros(256 * 256, dtype=np.float32)
    ptr = ctypes.c_void_p(buf.data_ptr())
    for size, R in ((0, 0.5), (-3, 0.5), (257, 1.0), (3, 0.0), (3, -1.0), (3, math.nextafter(1.5, 2.0)), (8, math.nextafter(3.5, 4.0)),
                    (256, math.nextafter(127.5, 128.0)), (1, math.nextafter(0.5, 1.0)), (3, float("nan")), (3, float("inf"))):
        assert L.fdr_psf_disk_dev(0, size, R, ptr, None) == -1, (size, R)
        assert L.fdr_psf_disk(size, R, hbuf.ctypes.data) == -1, (size, R)
    assert L.fdr_psf_disk_dev(0, 3, 0.5, None, None) == -1
    torch.cuda.synchronize()
    assert not torch.any(buf).item(), "a refused call wrote"
    img = tone_image(128, 128, 3)
    with fdr.Plan(128, 128, fdr.MODE_FAST) as p:
        # each setter is its _dev counterpart on the generated disk
        for R in (0.75, 4.5, 6.0):
            d = torch.from_numpy(dm.disk(dm.disk_size(R), R)).cuda()
            n = dm.disk_size(R)
            p.set_psf_disk(R, 0.01)
            a = p.wiener(img)
            p.set_psf_dev(d.data_ptr(), n, n, n, 0.01)
            assert np.array_equal(a, p.wiener(img)), R
            p.set_psf_disk(R, 0.001, gamma=0.02)
            a = p.wiener(img)
            p.set_psf_dev(d.data_ptr(), n, n, n, 0.001, gamma=0.02)
            assert np.array_equal(a, p.wiener(img)), R
            p.set_operator_psf_disk(R)
            a = p.blur(img)
            p.set_operator_psf_dev(d.data_ptr(), n, n, n)
            assert np.array_equal(a, p.blur(img)), R
        before = p.wiener(img)
        for R in (0.0, -1.0, 127.5, float("nan"), float("inf"), 64.0):  # 64: the 129 x 129 disk is larger than the plan
            assert L.fdr_set_psf_disk(p._h, R, 0.01, None) == -1, R
            assert L.fdr_set_psf_disk_cls(p._h, R, 0.01, 0.1, None) == -1, R
            assert L.fdr_set_operator_psf_disk(p._h, R, None) == -1, R
        assert L.fdr_set_psf_disk_cls(p._h, 3.0, 0.01, -1.0, None) == -1  # what fdr_set_psf_cls_dev refuses
        assert L.fdr_set_psf_disk(None, 3.0, 0.01, None) == -1
        assert np.array_equal(p.wiener(img), before), "a refused setter changed the filter"
    with fdr.Plan(64, 64, fdr.MODE_PARITY) as q:
        assert L.fdr_set_operator_psf_disk(q._h, 3.0, None) == -1  # no operator on a parity plan
        q.set_psf_disk(3.0, 0.01)  # the Wiener filter of either mode


def _check_profile(est, T, want_T, lo, what):
    dev = float(np.abs(T.astype(np.float64) - want_T).max())
    print("DEFOCUS\tprofile\t%s\tmax |T - model| = %.3g\td=%d conf=%.2f" % (what, dev, est.diameter, est.confidence))
    assert dev <= dm.DEFOCUS_PROFILE_TOL, what
    # the pick from the returned profile, in double, as the model computes it
    d, ring, radius, score, conf = dm.pick(T, lo)
    assert (est.diameter, est.ring, est.radius, est.score) == (d, ring, radius, np.float32(score)), what
    assert abs(est.confidence - conf) <= 1e-5 * max(1.0, abs(conf)), what
    return dev


# (picture, M, N, flags, stride of the _dev form or 0 for the host form)
PROFILE_PLANS = [("tone16", 32, 32, 0, 0), ("tone37", 64, 128, 0, 103), ("disk5", 512, 512, 0, 0), ("cat", 1024, 2048, 0, 0),
                 ("cat", 800, 1920, 2048, 0)]


@pytest.mark.parametrize("key,M,N,flags,stride", PROFILE_PLANS)
def test_profile_against_model(fdr, key, M, N, flags, stride):
    import torch
    img = _PICTURES[key]()
    rows, cols = img.shape
    lo, hi, step, na, nd = dm.defaults(rows, cols)
    want = dm.profile(mm.score_table(_model_cepstrum(key, M, N), lo, hi, step))
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        if stride:
            src = np.full((rows, stride), np.nan, dtype=np.float32)
            src[:, :cols] = img
            d_in = torch.from_numpy(src).cuda()
            d_T = torch.full((nd + 3,), float("nan"), dtype=torch.float32, device="cuda")
            est = p.estimate_defocus_dev(d_in.data_ptr(), rows, cols, stride, d_profile=d_T.data_ptr())
            T = d_T.cpu().numpy()
            assert np.all(np.isnan(T[nd:])), "wrote past the profile"
            T = T[:nd]
            host = p.estimate_defocus(img, return_profile=True)
            assert host[0] == est and np.array_equal(host[1], T), "the strided _dev form and the host form differ"
        else:
            est, T = p.estimate_defocus(img, return_profile=True)
    assert (est.n_angles, est.n_diameters) == (na, nd) and T.shape == (nd,)
    _check_profile(est, T, want, lo, "%s %dx%d win %dx%d" % (key, M, N, rows, cols))


def test_profile_angle_counts_and_ranges(fdr):
    """odd, even, power-of-two and one-over angle counts (the sort pads to the next power of two), and 1, 2 and 98 diameters.  One
    angle would need a step of 180 degrees, which the motion estimate's rule for the step, (0, 90], refuses here too."""
    img = _PICTURES["disk5"]()
    c = _model_cepstrum("disk5", 512, 512)
    est0 = fdr.DefocusEstimateC()
    with fdr.Plan(512, 512, fdr.MODE_FAST) as p:
        for n in (2, 3, 5, 64, 65, 360, 361, 4096):
            step = _step_for(n)
            est, T = p.estimate_defocus(img, 3, 40, step, return_profile=True)
            assert est.n_angles == n
            _check_profile(est, T, dm.profile(mm.score_table(c, 3, 40, step)), 3, "disk5 %d angles" % n)
        for lo, hi in ((9, 9), (9, 10), (3, 100)):
            est, T = p.estimate_defocus(img, lo, hi, 0.5, return_profile=True)
            assert est.n_diameters == hi - lo + 1 == T.size
            _check_profile(est, T, dm.profile(mm.score_table(c, lo, hi, 0.5)), lo, "disk5 diameters %d..%d" % (lo, hi))
        good = p.estimate_defocus(img, return_profile=True)
        # 4097 angles are refused, before any launch, and the plan answers as before
        assert fdr.lib.fdr_estimate_defocus_f32(p._h, img.ctypes.data, 512, 512, 512, 0, 0, _step_for(4097), ctypes.byref(est0), None) == -1
        assert "4096" in fdr.lib.fdr_last_error().decode()
        assert fdr.lib.fdr_estimate_defocus_f32(p._h, img.ctypes.data, 512, 512, 512, 0, 0, 180.0, ctypes.byref(est0), None) == -1
        again = p.estimate_defocus(img, return_profile=True)
        assert again[0] == good[0] and np.array_equal(again[1], good[1])


def test_ties_and_the_zero_window(fdr):
    img = _PICTURES["const"]()
    with fdr.Plan(128, 128, fdr.MODE_FAST) as p:
        lo, hi, step, na, nd = dm.defaults(*img.shape)
        est, T = p.estimate_defocus(img, return_profile=True)
        assert np.all(np.isfinite(T)) and all(math.isfinite(v) for v in est[:5])
        # Nearly every bin of a windowed constant is 0 but for rounding, so log |G| there, and with it the cepstrum, is what the
        # float32 transform's rounding makes of it (1.7e-5 from the float64 cepstrum, measured): the model's profile is taken
        # from the device's own cepstrum here, which judges the gather, the sort and the median alone
        _check_profile(est, T, dm.profile(mm.score_table(p.cepstrum(img).astype(np.float64), lo, hi, step)), lo, "constant 128x128")
        _, S = p.estimate_motion(img, scores=True)
        s = np.sort(S, axis=0)
        assert np.array_equal(T, np.float32(0.5) * (s[(na - 1) // 2] + s[na // 2]))
        # two angles: the mean of the motion estimate's two table entries, bit for bit
        e1, T1 = p.estimate_defocus(img, 3, 20, 90.0, return_profile=True)
        _, S = p.estimate_motion(img, 3, 20, 90.0, scores=True)
        assert np.array_equal(T1, (0.5 * (S[0] + S[1])).astype(np.float32))
        z = np.zeros((100, 120), dtype=np.float32)
        e, Tz = p.estimate_defocus(z, return_profile=True)
        assert e == fdr.DefocusEstimate(0, 0.0, 0.0, 0.0, 0.0, 360, nd) and Tz.shape == (nd,) and not np.any(Tz)
        b = p.estimate_blur(z)
        assert b.kind == fdr.BLUR_NONE and b.defocus == e and b.motion == p.estimate_motion(z)
        # the zero result does not stick
        est2, T2 = p.estimate_defocus(img, return_profile=True)
        assert est2 == est and np.array_equal(T2, T)


def test_median_is_the_sorted_middle(fdr):
    """the profile from the motion estimate's own table (same plane, same gather): numpy.median of its float32 columns, within one
    rounding of 0.5 (a + b)"""
    img = _PICTURES["disk5"]()
    with fdr.Plan(512, 512, fdr.MODE_FAST) as p:
        for n in (5, 64, 360):
            step = _step_for(n)
            _, S = p.estimate_motion(img, 3, 40, step, scores=True)
            _, T = p.estimate_defocus(img, 3, 40, step, return_profile=True)
            s = np.sort(S, axis=0)
            assert np.array_equal(T, np.float32(0.5) * (s[(n - 1) // 2] + s[n // 2])), n


def test_picks_and_recovery(fdr):
    rows, cols, seed = dm.REC_SCENES[0]
    M, N = dm.plan_size(rows, cols)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_MIXED_RADIX) as p:
        for R in dm.REC_RADII:
            img = _defocused(rows, cols, R, seed)
            want = dm.estimate(img.astype(np.float64), M, N)
            got = p.estimate_defocus(img)
            print("DEFOCUS\trecover\t%dx%d R=%.1f\tgpu %.4f (d=%d conf=%.1f)\tmodel %.4f (d=%d conf=%.1f)" %
                  (rows, cols, R, got.radius, got.diameter, got.confidence, want.radius, want.diameter, want.confidence))
            assert got.diameter == want.diameter, R
            assert abs(got.radius - want.radius) <= 1e-3, R
            assert abs(got.radius - R) <= dm.DEFOCUS_RADIUS_TOL, R
            assert got.confidence >= dm.CONF_DEFOCUS_MIN, R
    e = fdr.estimateDefocusBlur(np.repeat(_defocused(rows, cols, 5, seed)[:, :, None], 3, axis=2))
    assert abs(e.radius - 5) <= dm.DEFOCUS_RADIUS_TOL, e


def test_combined_call(fdr):
    import torch
    car = _golden("car_blurred.png")
    L, a = mm.SYNTH_PAIRS[2]
    cases = [("defocus", _defocused(512, 512, 5, 31), fdr.BLUR_DEFOCUS), ("sharp", mm.scene(*dm.SHARP_SCENES[1]).astype(np.float32), fdr.BLUR_NONE),
             ("motion", mm.blurred_scene(512, 512, L, a, fdr.motionBlurKernel(L, a), seed=1002).astype(np.float32), fdr.BLUR_MOTION),
             ("car", car, fdr.BLUR_MOTION)]
    for what, img, kind in cases:
        M, N = dm.plan_size(*img.shape)
        with fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_MIXED_RADIX) as p:
            mo, de = p.estimate_motion(img), p.estimate_defocus(img)
            b = p.estimate_blur(img)
            print("DEFOCUS\tkind\t%s\tkind=%d motion conf=%.1f ring conf=%.1f radius=%.2f" % (what, b.kind, mo.confidence, de.confidence, de.radius))
            assert b.motion == mo and b.defocus == de, "the combined call differs from the single calls: " + what
            assert b.kind == kind == fdr.lib.fdr_blur_kind(mo.confidence, de.confidence), what
            d_img = torch.from_numpy(img).cuda()
            assert p.estimate_blur_dev(d_img.data_ptr(), img.shape[0], img.shape[1], img.shape[1]) == b, what
            # search arguments of their own, each as its single call takes them
            b2 = p.estimate_blur(img, 5, 60, 1.0, 4, 30, 0.25)
            assert b2.motion == p.estimate_motion(img, 5, 60, 1.0) and b2.defocus == p.estimate_defocus(img, 4, 30, 0.25), what
            assert p.estimate_motion(img) == mo and p.estimate_defocus(img) == de
    from PIL import Image
    rgb = np.asarray(Image.open(os.path.join(GOLDEN_DIR, "car_blurred.png")).convert("RGB"), dtype=np.float32)
    assert fdr.estimateBlur(rgb).kind == fdr.BLUR_MOTION


def test_end_to_end_restoration(fdr):
    """A 512^2 scene defocused circularly with the disk of radius 6 (noise sigma 1): estimate, CLS filter of the estimated disk with
    gamma by GCV, Wiener call.  Float64 model of the same chain on this scene: blurred 23.73 dB, restored 26.25 dB (radius 5.928,
    gamma 1.75e-3); the device must gain at least half of that.  Measured on an MI355X: 26.25 dB (radius 5.928, gamma 1.75e-3)."""
    n, R = 512, 6.0
    truth = mm.scene(n, n, 61)
    k = dm.disk(dm.disk_size(R), R).astype(np.float64)
    h = np.zeros((n, n))
    h[:k.shape[0], :k.shape[1]] = k
    h = np.roll(h, (-(k.shape[0] // 2), -(k.shape[1] // 2)), axis=(0, 1))  # centred at the origin: the blur does not shift
    blurred = np.fft.irfft2(np.fft.rfft2(truth) * np.fft.rfft2(h), s=(n, n)) + np.random.default_rng(62).normal(0.0, 1.0, (n, n))
    b32 = blurred.astype(np.float32)

    def restore_model(radius, gamma):
        psf = dm.disk(dm.disk_size(radius), radius)
        return np.roll(_cls_model.cls_raw(b32, psf, 0.0, gamma, n, n), (psf.shape[0] // 2, psf.shape[1] // 2), axis=(0, 1))

    r_m = dm.estimate(b32.astype(np.float64), n, n).radius
    g_m = rm.choose(b32, dm.disk(dm.disk_size(r_m), r_m), n, n).value
    psnr_blurred, psnr_model = dm.psnr(blurred, truth), dm.psnr(restore_model(r_m, g_m), truth)
    with fdr.Plan(n, n, fdr.MODE_FAST) as p:
        est = p.estimate_defocus(b32)
        p.set_operator_psf_disk(est.radius)
        gamma = p.choose_regularisation(b32).value
        p.set_psf_disk(est.radius, 0.0, gamma=gamma)
        x = p.wiener(b32, norm_area=fdr.NORM_PADDED).astype(np.float64)
    # fdr_wiener_f32 returns the min-max normalised plane: undo it with the extremes of the float64 restoration with the device's
    # radius and gamma (an affine map, exact to rounding), and the shift by the disk's centre
    raw = restore_model(est.radius, gamma)
    c = dm.disk_size(est.radius) // 2
    x = np.roll(x, (c, c), axis=(0, 1)) * (raw.max() - raw.min()) + raw.min()
    psnr_gpu = dm.psnr(x, truth)
    print("DEFOCUS\tend to end\tblurred %.2f dB\tmodel %.2f dB (radius %.3f gamma %.3g)\tgpu %.2f dB (radius %.3f gamma %.3g)" %
          (psnr_blurred, psnr_model, r_m, g_m, psnr_gpu, est.radius, gamma))
    assert psnr_model > psnr_blurred
    assert psnr_gpu - psnr_blurred >= 0.5 * (psnr_model - psnr_blurred)


def test_determinism_and_allocations(fdr):
    import torch
    img = _PICTURES["cat"]()
    d_img = torch.from_numpy(img).cuda()
    for M, N, flags in ((1024, 2048, 0), (800, 1920, fdr.FLAG_MIXED_RADIX)):
        with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
            e1, T1 = p.estimate_defocus(img, return_profile=True)
            b1 = p.estimate_blur(img)
            p.estimate_defocus(img, 3, 100, _step_for(4096))  # the largest trig table
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            for _ in range(3):
                e2, T2 = p.estimate_defocus(img, return_profile=True)
                assert e2 == e1 and np.array_equal(T2, T1), "two estimates differ"
                assert p.estimate_blur(img) == b1
                assert p.estimate_defocus_dev(d_img.data_ptr(), img.shape[0], img.shape[1], img.shape[1]) == e1
                p.estimate_defocus(img, 3, 100, _step_for(4096))
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free0, "a later call allocated device memory"


def test_isolation(fdr):
    from _rl_model import NORM_NONE
    M, N = 512, 1024
    img = tone_image(M, N, 21, 400, 900)
    car = _golden("car_blurred.png")
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_psf_motion(15, 30.0, 0.01)
        p.set_operator_psf_motion(50, 123.4)
        before = (p.wiener(img), p.richardson_lucy(img, 5, NORM_NONE), p.blur(img), p.estimate_motion(car, scores=True))
        p.estimate_defocus(car, return_profile=True)
        p.estimate_blur(car)
        p.estimate_defocus(car, 5, 50, 1.0)
        after = (p.wiener(img), p.richardson_lucy(img, 5, NORM_NONE), p.blur(img), p.estimate_motion(car, scores=True))
        for what, a, b in zip(("Wiener", "RL", "blur"), before, after):
            assert np.array_equal(a, b), what + " output changed after a defocus estimate"
        assert before[3][0] == after[3][0] and np.array_equal(before[3][1], after[3][1]), "the motion estimate changed after a defocus estimate"


def test_refusals(fdr):
    import torch
    L = fdr.lib
    img = tone_image(64, 64, 3)
    est, mo, kind = fdr.DefocusEstimateC(), fdr.MotionEstimateC(), ctypes.c_int(0)

    def calls(p, rows, cols, stride, lo=0, hi=0, step=0.0, null_est=False):
        """(host rc, _dev rc, combined host rc, combined _dev rc) on valid buffers, so that a refusal that did not happen could do no harm"""
        e = None if null_est else ctypes.byref(est)
        n = max(rows, 1) * max(stride, 1) + 64
        hbuf = np.zeros(n, dtype=np.float32)
        dbuf = torch.zeros(n, dtype=torch.float32, device="cuda")
        dp = ctypes.c_void_p(dbuf.data_ptr())
        rc = (L.fdr_estimate_defocus_f32(p._h, hbuf.ctypes.data, rows, cols, stride, lo, hi, step, e, None),
              L.fdr_estimate_defocus_f32_dev(p._h, dp, rows, cols, stride, lo, hi, step, e, None, None),
              L.fdr_estimate_blur_f32(p._h, hbuf.ctypes.data, rows, cols, stride, 0, 0, 0.0, lo, hi, step, ctypes.byref(mo), e, ctypes.byref(kind)),
              L.fdr_estimate_blur_f32_dev(p._h, dp, rows, cols, stride, 0, 0, 0.0, lo, hi, step, ctypes.byref(mo), e, ctypes.byref(kind), None))
        torch.cuda.synchronize()
        return rc

    psf = fdr.motionBlurKernel(15, 30.0)
    for M, N, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (360, 640, fdr.MODE_FAST, fdr.FLAG_ANY_SIZE, "any size fast"),
                                    (16, 64, fdr.MODE_FAST, 0, "M < 32"), (64, 16384, fdr.MODE_FAST, 0, "N > 8192")):
        with fdr.Plan(M, N, mode, flags=flags) as p:
            p.set_psf(psf, 0.01)
            im = tone_image(M, N, 2, min(M, 64), min(N, 64))
            before = p.wiener(im)
            assert calls(p, min(M, 64), min(N, 64), min(N, 64)) == (-1,) * 4, what
            assert np.array_equal(p.wiener(im), before), what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert calls(p, 64, 64, 64) == (-4,) * 4
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        good = p.estimate_defocus(img, return_profile=True)
        bad_args = [dict(rows=15, cols=64, stride=64), dict(rows=64, cols=15, stride=64), dict(rows=65, cols=64, stride=64),
                    dict(rows=64, cols=65, stride=65), dict(rows=64, cols=64, stride=63), dict(rows=-1, cols=64, stride=64),
                    dict(rows=64, cols=64, stride=64, lo=-1), dict(rows=64, cols=64, stride=64, hi=-1),
                    dict(rows=64, cols=64, stride=64, lo=1), dict(rows=64, cols=64, stride=64, lo=10, hi=9),
                    dict(rows=64, cols=64, stride=64, lo=17), dict(rows=64, cols=64, stride=64, hi=31),
                    dict(rows=64, cols=64, stride=64, step=-0.5), dict(rows=64, cols=64, stride=64, step=90.0001),
                    dict(rows=64, cols=64, stride=64, step=float("nan")), dict(rows=64, cols=64, stride=64, step=float("inf")),
                    dict(rows=64, cols=64, stride=64, null_est=True), dict(rows=64, cols=64, stride=64, step=_step_for(4097)),
                    dict(rows=64, cols=64, stride=64, lo=2, hi=30, step=5e-5)]
        for kw in bad_args:
            assert calls(p, **kw) == (-1,) * 4, kw
        assert calls(p, rows=64, cols=64, stride=64, lo=1) == (-1,) * 4 and "min_diameter < 2" in L.fdr_last_error().decode()
        assert L.fdr_estimate_defocus_f32(p._h, None, 64, 64, 64, 0, 0, 0.0, ctypes.byref(est), None) == -1
        assert L.fdr_estimate_blur_f32(p._h, img.ctypes.data, 64, 64, 64, 0, 0, 0.0, 0, 0, 0.0, None, ctypes.byref(est), ctypes.byref(kind)) == -1
        assert L.fdr_estimate_blur_f32(p._h, img.ctypes.data, 64, 64, 64, 0, 0, 0.0, 0, 0, 0.0, ctypes.byref(mo), ctypes.byref(est), None) == -1
        assert L.fdr_estimate_blur_f32(p._h, img.ctypes.data, 64, 64, 64, 1, 0, 0.0, 0, 0, 0.0, ctypes.byref(mo), ctypes.byref(est),
                                       ctypes.byref(kind)) == -1  # the motion search's own refusal
        # the limits themselves are accepted, and the plan still gives the same answer
        assert p.estimate_defocus(img, 2, 30, 90.0).n_angles == 2
        assert p.estimate_defocus(img, 3, 16, _step_for(4096)).n_angles == 4096
        again = p.estimate_defocus(img, return_profile=True)
        assert again[0] == good[0] and np.array_equal(again[1], good[1])


def test_cli_defocus(fdr, tmp_path):
    """tools/cli/gpu <img> defocus auto: one `estimate:` line, then exactly the run of <img> defocus R -- the same PNG bytes; `auto auto
    --any-blur` names the kind and runs the matching form; `defocus` beside `blind` and a sharp picture end the run with a message"""
    import re
    import subprocess
    from PIL import Image
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")

    def run(*args):
        return subprocess.run([gpu] + [str(a) for a in args], capture_output=True, text=True, timeout=600)

    def png(name, img):
        path = str(tmp_path / name)
        Image.fromarray(np.repeat(np.clip(img, 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)).save(path)
        return path

    blurred, sharp = png("defocused.png", _defocused(512, 512, 5, 31)), png("sharp.png", mm.scene(*dm.SHARP_SCENES[1]))
    a_png, b_png, c_png = str(tmp_path / "auto.png"), str(tmp_path / "given.png"), str(tmp_path / "any.png")
    r = run(blurred, "defocus", "auto", "--out", a_png)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^estimate: defocus radius (\S+) diameter (\d+) confidence (\S+)$", r.stdout, re.M)
    assert m, r.stdout
    R, D, C = m.group(1), int(m.group(2)), float(m.group(3))
    print("DEFOCUS\tcli\tR=%s D=%d conf=%.2f" % (R, D, C))
    assert abs(float(R) - 5) <= dm.DEFOCUS_RADIUS_TOL and C >= dm.CONF_DEFOCUS_MIN and "low confidence" not in r.stderr
    r2 = run(blurred, "defocus", R, "--out", b_png)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert open(a_png, "rb").read() == open(b_png, "rb").read(), "defocus auto wrote another picture than the printed radius"
    r3 = run(blurred, "auto", "auto", "--any-blur", "--out", c_png)
    assert r3.returncode == 0 and re.search(r"^estimate: kind defocus radius %s diameter %d " % (re.escape(R), D), r3.stdout, re.M), r3.stdout
    assert open(c_png, "rb").read() == open(a_png, "rb").read()
    # the car: a motion blur, the run of `auto auto`
    car = os.path.join(GOLDEN_DIR, "car_blurred.png")
    d_png, e_png = str(tmp_path / "car_any.png"), str(tmp_path / "car_auto.png")
    r4, r5 = run(car, "auto", "auto", "--any-blur", "--out", d_png), run(car, "auto", "auto", "--out", e_png)
    assert r4.returncode == 0 and r5.returncode == 0, r4.stdout + r4.stderr + r5.stderr
    m4, m5 = re.search(r"^estimate: kind motion (length .*)$", r4.stdout, re.M), re.search(r"^estimate: (length .*)$", r5.stdout, re.M)
    assert m4 and m5 and m4.group(1) == m5.group(1), r4.stdout
    assert open(d_png, "rb").read() == open(e_png, "rb").read(), "--any-blur on a motion blur wrote another picture than auto auto"
    r6 = run(sharp, "auto", "auto", "--any-blur")
    assert r6.returncode != 0 and re.search(r"^estimate: kind none ", r6.stdout, re.M) and "neither" in r6.stdout, r6.stdout
    for args in ((blurred, "defocus", "5", "blind"), (blurred, "blind", "9", "--rl", "5", "defocus"), (blurred, "defocus", "blind")):
        r7 = run(*args)
        assert r7.returncode != 0 and "cannot be combined" in r7.stdout, args
    assert run(blurred, "defocus", "0").returncode != 0 and run(blurred, "defocus", "128").returncode != 0
    assert run(blurred, "5", "30", "--any-blur").returncode != 0
