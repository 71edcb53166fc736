"""CPU checks of the defocus estimate's float64 model (tests/_defocus_model.py) before it judges the GPU (test_defocus_gpu.py): the
disk generator against counts made by hand, the refit of the two calibration constants, recovery of radii outside the fit, the
separation of disk blurs from motion blurs and sharp scenes, the blur kind, wrong implementations that each have to be caught, a
float32 restatement inside its recorded bound, and the declared surface.  Each case prints a `DEFOCUS` line (pytest -s).

One analysis per picture (cepstrum, score table, profiles, motion pick) is made once and shared by the tests."""
import functools
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _defocus_model as dm
import _motion_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def _analyse(img):
    rows, cols = img.shape
    M, N = dm.plan_size(rows, cols)
    lo, hi, step, _, _ = dm.defaults(rows, cols)
    S = mm.score_table(mm.cepstrum_model(img, M, N), lo, hi, step)
    T = dm.profile(S)
    return dict(T=T, T_mean=dm.profile_mean(S), T_upper=dm.profile_upper_middle(S), est=dm.Estimate(*dm.pick(T, lo), *S.shape),
                motion_conf=mm.pick(S, lo, step)[3], lo=lo)


@functools.lru_cache(maxsize=None)
def _disk_case(rows, cols, seed, R):
    return _analyse(dm.defocused_scene(rows, cols, R, seed))


@functools.lru_cache(maxsize=None)
def _sharp_case(rows, cols, seed):
    return _analyse(mm.scene(rows, cols, seed))


_MOTION = {}


def _motion_cases(oracle):
    if not _MOTION:
        for rows, cols in mm.SYNTH_SIZES:
            for k, (L, a) in enumerate(mm.SYNTH_PAIRS):
                _MOTION[(rows, cols, L, a)] = _analyse(mm.blurred_scene(rows, cols, L, a, oracle.motion_blur_kernel(L, a), seed=1000 + k))
    return _MOTION


@functools.lru_cache(maxsize=None)
def _golden_case(name):
    return _analyse(mm.load_golden(os.path.join(GOLDEN_DIR, name)))


def _all_disk_cases():
    return [(r, c, s, R) for r, c, s in dm.CAL_SCENES for R in dm.CAL_RADII] + [(r, c, s, R) for r, c, s in dm.REC_SCENES for R in dm.REC_RADII]


def test_disk_generator():
    """Counts by hand for S = 16 (units of 1 / 32 px; the sub-samples of a pixel lie at the odd offsets -15 .. 15 about its centre,
    which is 32 units from its neighbour's).  Radius 0.5, q = 256: in the centre pixel the odd pairs (a, b) with a^2 + b^2 <= 256
    number 8 + 8 + 8 + 7 + 7 + 6 + 5 + 3 = 52 per quadrant, 208 in all; the nearest sub-sample of an edge neighbour lies 17 units
    out (289 > 256), so the neighbours and corners hold none: the disk of radius 0.5 lies inside the centre pixel's own square.
    Radius 0.75, q = 576: the centre pixel is full (225 + 225 <= 576); an edge neighbour holds, at X = 17, 19, 21, 23, the 16, 14,
    12 and 6 sub-samples with Y^2 <= 287, 215, 135, 47, and none from X = 25 (625) on: 48; a corner none (289 + 289 > 576)."""
    n = dm.disk_counts(3, 0.5)
    assert n.tolist() == [[0, 0, 0], [0, 208, 0], [0, 0, 0]]
    assert dm.disk(3, 0.5)[1, 1] == 1.0
    n = dm.disk_counts(3, 0.75)
    assert n.tolist() == [[0, 48, 0], [48, 256, 48], [0, 48, 0]]
    assert dm.disk(3, 0.75)[0, 1] == np.float32(48.0 / 448.0)
    for size, R in ((5, 2.0), (11, 4.5), (27, 13.0), (31, 13.0), (9, 3.3)):
        d = dm.disk(size, R)
        assert d.dtype == np.float32 and abs(float(d.astype(np.float64).sum()) - 1.0) <= 1e-6
        assert np.array_equal(d, d.T) and np.array_equal(d, d[::-1]) and np.array_equal(d, d[:, ::-1]), (size, R)
    for R in (2.0, 4.5, 13.0):
        n = dm.disk_counts(dm.disk_size(R), R)
        area = n.sum() / 256.0
        print("DEFOCUS\tdisk\tR=%.1f area=%.4f pi R^2=%.4f hard=%d" % (R, area, math.pi * R * R, dm.disk_hard(dm.disk_size(R), R).sum()))
        assert abs(area - math.pi * R * R) <= 0.01 * math.pi * R * R
        d = dm.disk(dm.disk_size(R), R)
        assert len(set(d[n == 256].tolist())) == 1 and (n == 256).sum() > 0
    # an even size: the centre is size // 2, as fdr_psf_gaussian's
    n = dm.disk_counts(8, 3.3)
    assert n[4, 4] == 256 and n[4, 7] == n[4, 1] and n[4, 0] == 0
    # fault: a disk without sub-samples misses the area at R = 2 (13 pixels against 12.57)
    hard = dm.disk_hard(5, 2.0).sum()
    assert abs(hard - math.pi * 4.0) > 0.01 * math.pi * 4.0


def test_refit_of_the_constants():
    A, B, rings = dm.calibrate(ring_of=lambda r, c, s, R: _disk_case(r, c, s, R)["est"].ring)
    worst = max(abs(dm.DEFOCUS_A * d + dm.DEFOCUS_B - k[3]) for k, d in rings.items())
    print("DEFOCUS\tfit\tA=%.6f B=%.6f (file %.5f %.5f)\tworst fit error %.3f px over %d cases" % (A, B, dm.DEFOCUS_A, dm.DEFOCUS_B, worst, len(rings)))
    assert abs(A - dm.DEFOCUS_A) <= 1e-3 and abs(B - dm.DEFOCUS_B) <= 2e-2
    hdr = open(os.path.join(ROOT, "include", "fdr.h")).read()
    assert float(re.search(r"#define FDR_DEFOCUS_A (\S+)", hdr).group(1)) == dm.DEFOCUS_A
    assert float(re.search(r"#define FDR_DEFOCUS_B \((\S+)\)", hdr).group(1)) == dm.DEFOCUS_B
    assert float(re.search(r"#define FDR_MOTION_CONF_MIN (\S+)", hdr).group(1)) == dm.MOTION_CONF_MIN
    assert float(re.search(r"#define FDR_DEFOCUS_CONF_MIN (\S+)", hdr).group(1)) == dm.DEFOCUS_CONF_MIN
    for k, name in enumerate(("NONE", "MOTION", "DEFOCUS")):
        assert int(re.search(r"#define FDR_BLUR_%s (\d+)" % name, hdr).group(1)) == k == getattr(dm, "BLUR_" + name)


def test_recovery_outside_the_fit():
    errs, half = [], []
    for rows, cols, seed in dm.REC_SCENES:
        for R in dm.REC_RADII:
            e = _disk_case(rows, cols, seed, R)["est"]
            errs.append(abs(e.radius - R))
            half.append(abs(e.ring / 2.0 - R))
            print("DEFOCUS\trecover\t%dx%d R=%.1f\tgot %.3f (d=%d ring=%.3f conf=%.1f) err=%.3f\tring/2 err=%.3f" %
                  (rows, cols, R, e.radius, e.diameter, e.ring, e.confidence, errs[-1], half[-1]))
    assert dm.DEFOCUS_RADIUS_TOL <= 0.3
    assert max(errs) <= 0.15, "the model alone misses by more than 0.15 px"
    assert 2.0 * max(errs) <= dm.DEFOCUS_RADIUS_TOL, "DEFOCUS_RADIUS_TOL is below twice the model's largest error"
    assert max(errs) <= dm.DEFOCUS_RADIUS_TOL
    # fault: d / 2 as the radius misses the tolerance
    assert max(half) > dm.DEFOCUS_RADIUS_TOL


def test_separation_and_kind(oracle):
    disk_conf = {k: _disk_case(*k)["est"].confidence for k in _all_disk_cases()}
    print("DEFOCUS\tconf\tdisk cases %.1f .. %.1f" % (min(disk_conf.values()), max(disk_conf.values())))
    assert min(disk_conf.values()) >= dm.CONF_DEFOCUS_MIN, min(disk_conf, key=disk_conf.get)
    for k in _all_disk_cases():
        if k[3] >= 3:
            c = _disk_case(*k)
            assert dm.classify(c["motion_conf"], c["est"].confidence) == dm.BLUR_DEFOCUS, (k, c["motion_conf"], c["est"])
    mean_conf = []
    for k, c in _motion_cases(oracle).items():
        conf_mean = dm.pick(c["T_mean"], c["lo"])[4]
        mean_conf.append(conf_mean)
        print("DEFOCUS\tmotion\t%dx%d L=%d a=%.1f\tring conf=%.2f (mean profile %.2f) motion conf=%.1f" % (*k, c["est"].confidence, conf_mean,
                                                                                                       c["motion_conf"]))
        assert c["est"].confidence <= dm.CONF_OTHER_MAX, k
        assert dm.classify(c["motion_conf"], c["est"].confidence) == dm.BLUR_MOTION, k
    # fault: the mean over the directions fires on motion blur
    assert max(mean_conf) > dm.DEFOCUS_CONF_MIN > dm.CONF_OTHER_MAX
    for k in dm.SHARP_SCENES:
        c = _sharp_case(*k)
        print("DEFOCUS\tsharp\t%dx%d\tring conf=%.2f motion conf=%.1f" % (k[0], k[1], c["est"].confidence, c["motion_conf"]))
        assert c["est"].confidence <= dm.CONF_OTHER_MAX, k
        assert dm.classify(c["motion_conf"], c["est"].confidence) == dm.BLUR_NONE, k
    for name, _, _ in mm.GOLDEN:
        c = _golden_case(name)
        print("DEFOCUS\tgolden\t%s\tring conf=%.2f at d=%d motion conf=%.1f" % (name, c["est"].confidence, c["est"].diameter, c["motion_conf"]))
        assert dm.classify(c["motion_conf"], c["est"].confidence) == dm.BLUR_MOTION, name
    # the car is the case the normalised comparison exists for: a clear ring beside a clearer motion peak
    car = _golden_case("car_blurred.png")
    assert car["est"].confidence >= dm.DEFOCUS_CONF_MIN and car["est"].diameter == 10


def test_classify():
    assert dm.classify(9.9, 5.9) == dm.BLUR_NONE
    assert dm.classify(10.0, 0.0) == dm.BLUR_MOTION and dm.classify(0.0, 6.0) == dm.BLUR_DEFOCUS
    assert dm.classify(20.0, 12.0) == dm.BLUR_MOTION  # a tie of the normalised confidences goes to motion
    assert dm.classify(20.0, 12.1) == dm.BLUR_DEFOCUS and dm.classify(43.2, 18.5) == dm.BLUR_MOTION


def test_median_and_pick():
    S = np.array([[3.0, 1.0, 5.0], [1.0, 2.0, 5.0], [4.0, 9.0, 5.0], [2.0, 0.0, 5.0]])
    assert dm.profile(S).tolist() == [2.5, 1.5, 5.0]
    assert dm.profile(S[:3]).tolist() == [3.0, 2.0, 5.0]
    assert dm.profile_upper_middle(S).tolist() == [3.0, 2.0, 5.0]  # the fault, at an even count
    # parabola through (-1, 3), (0, 1), (1, 2): the minimum lies at +1/6
    d, ring, radius, score, conf = dm.pick([5.0, 3.0, 1.0, 2.0, 5.0, 5.0, 5.0], 3)
    assert d == 5 and abs(ring - (5 + 1.0 / 6.0)) < 1e-12 and score == 1.0 and radius == dm.DEFOCUS_A * ring + dm.DEFOCUS_B
    assert dm.pick([1.0, 3.0, 2.0], 3)[:2] == (3, 3.0) and dm.pick([3.0, 2.0, 1.0], 3)[:2] == (5, 5.0)  # either end: d* itself
    assert dm.pick([2.0, 1.0, 1.0, 2.0], 3)[0] == 4  # exact ties: the lowest index
    assert dm.pick([1.0, 1.0, 1.0], 3)[1:] == (3.0, dm.DEFOCUS_A * 3.0 + dm.DEFOCUS_B, 1.0, 0.0)  # MAD 0, denominator 0
    assert dm.pick([5.0, 1.0, 1.0 + 1e-9, 5.0], 3)[1] <= 4.5  # the offset is clamped
    # fault: the upper-middle element at the even default count moves the profile of a disk case far outside the device tolerance
    c = _disk_case(512, 512, 31, 5)
    assert float(np.abs(c["T_upper"] - c["T"]).max()) > 10 * dm.DEFOCUS_PROFILE_TOL


def test_defaults_and_edges():
    assert dm.defaults(782, 1920) == (3, 100, 0.5, 360, 98)
    e, T = dm.estimate(np.zeros((40, 50)), 64, 64, with_profile=True)
    assert e == dm.Estimate(0, 0.0, 0.0, 0.0, 0.0, 360, 8) and T.shape == (8,) and not np.any(T)
    e = dm.estimate(np.full((40, 50), 3.0), 64, 64)
    assert all(math.isfinite(v) for v in e[:5])
    with pytest.raises(ValueError):
        dm.estimate(np.ones((40, 50)), 64, 64, angle_step=180.0 / 4097)
    assert dm.estimate(np.ones((40, 50)), 64, 64, angle_step=180.0 / 4096).n_angles == 4096
    assert dm.disk_size(4.5) == 11 and dm.disk_size(6) == 13 and dm.disk_radius_max(256) == 127.5 and dm.disk_radius_max(1) == 0.5


def test_single_precision_profile():
    worst = 0.0
    for rows, cols, seed in dm.REC_SCENES:
        M, N = dm.plan_size(rows, cols)
        lo, hi, step, _, _ = dm.defaults(rows, cols)
        for R in dm.REC_RADII:
            T32 = dm.profile_f32(dm.cepstrum_f32(dm.defocused_scene(rows, cols, R, seed), M, N), lo, hi, step)
            T = _disk_case(rows, cols, seed, R)["T"]
            assert T32.dtype == np.float32
            dev = float(np.abs(T32.astype(np.float64) - T).max())
            worst = max(worst, dev)
            assert dm.pick(T32, lo)[0] == dm.pick(T, lo)[0] and abs(dm.pick(T32, lo)[2] - dm.pick(T, lo)[2]) <= 1e-3
    print("DEFOCUS\tf32\tmax |T32 - T| = %.3g (bound %.3g, device tolerance %.3g)" % (worst, dm.PROFILE_F32_BOUND, dm.DEFOCUS_PROFILE_TOL))
    assert worst <= dm.PROFILE_F32_BOUND <= dm.DEFOCUS_PROFILE_TOL


NAMES = ("fdr_estimate_defocus_f32", "fdr_estimate_defocus_f32_dev", "fdr_estimate_blur_f32", "fdr_estimate_blur_f32_dev", "fdr_set_psf_disk",
         "fdr_set_psf_disk_cls", "fdr_set_operator_psf_disk")


def test_symbols_and_surface(fdr):
    hdr = open(os.path.join(ROOT, "include", "fdr.h")).read()
    assert re.search(r"typedef struct fdr_defocus_estimate \{[^}]*int diameter;[^}]*double ring;[^}]*double radius;[^}]*float score;"
                     r"[^}]*float confidence;[^}]*int n_angles;[^}]*int n_diameters;[^}]*\} fdr_defocus_estimate;", hdr)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name in NAMES:
        assert re.search(r"\bint %s\(fdr_plan\* plan," % name, hdr), name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    for name in ("fdr_psf_disk", "fdr_psf_disk_dev", "fdr_blur_kind"):
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    assert [f[0] for f in fdr.DefocusEstimateC._fields_] == ["diameter", "ring", "radius", "score", "confidence", "n_angles", "n_diameters"]
    assert fdr.DefocusEstimate._fields == dm.Estimate._fields
    assert fdr.BlurEstimate._fields == ("kind", "motion", "defocus")
    assert (fdr.BLUR_NONE, fdr.BLUR_MOTION, fdr.BLUR_DEFOCUS) == (dm.BLUR_NONE, dm.BLUR_MOTION, dm.BLUR_DEFOCUS)
    sig = inspect.signature(fdr.Plan.estimate_defocus)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [
        ("img", inspect.Parameter.empty), ("min_diameter", 0), ("max_diameter", 0), ("angle_step", 0.0), ("return_profile", False)]
    sig = inspect.signature(fdr.Plan.set_psf_disk)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:4] == [("radius", inspect.Parameter.empty), ("K", 0.01), ("gamma", 0.0)]
    for meth in ("estimate_defocus_dev", "estimate_blur", "estimate_blur_dev", "set_operator_psf_disk"):
        assert callable(getattr(fdr.Plan, meth)), meth
    for f in (fdr.psf_disk, fdr.estimateDefocusBlur, fdr.estimateBlur):
        assert callable(f)
    # the blur kind needs no device: the library's rule is the model's
    for m, f in ((9.9, 5.9), (10.0, 0.0), (0.0, 6.0), (20.0, 12.0), (20.0, 12.1), (43.2, 18.5), (0.0, 0.0)):
        assert fdr.lib.fdr_blur_kind(m, f) == dm.classify(m, f), (m, f)
    # refusals of the generator come before any device work
    buf = np.zeros(256 * 256, dtype=np.float32)
    for size, radius in ((0, 0.5), (257, 1.0), (3, 0.0), (3, -1.0), (3, 1.5000001), (8, 3.5000001), (1, 0.6), (3, float("nan")), (3, float("inf"))):
        assert fdr.lib.fdr_psf_disk(size, radius, buf.ctypes.data) == -1, (size, radius)
        assert fdr.lib.fdr_psf_disk_dev(0, size, radius, buf.ctypes.data, None) == -1, (size, radius)
    assert fdr.lib.fdr_psf_disk(3, 0.5, None) == -1
