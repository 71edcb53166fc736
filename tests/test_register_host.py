"""The frame registration on the CPU: the float64 model of tests/_register_model.py pinned -- its accuracy table,
the end-to-end quality through the multi-frame Richardson-Lucy model, the bilinear PSF shift, injected faults, the margins the device
cases rest on -- then the public surface, the refusals that need no device, the workspace block and the command line.  No GPU needed."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _register_model as rm
from _frames_model import QUALITY_EPS, QUALITY_LAMBDA, QUALITY_N, frames_model
from _rl_model import psnr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the committed model measures (float64, fixed seeds): the largest and the mean distance |estimate - shift| in pixels over the four
# PSF pairs and five shifts, per noise level; each is asserted at 1.5x, which only has to cover another platform's libm and FFT
MEASURED_WORST = {0.0: 0.318, 0.01: 0.284}
MEASURED_MEAN = {0.0: 0.142, 0.01: 0.155}


def _need(fdr):
    assert hasattr(fdr.lib, "fdr_register_frames_f32") and hasattr(fdr.lib, "fdr_psf_shift_f32"), "the library has no frame registration"


@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_accuracy_table_of_the_model(noise):
    """the 200^2 crop of the 512^2 rectangle scene on a 256^2 plan, frame 1 through another PSF and moved: the estimate with the PSFs is
    right to a fraction of a pixel, plain phase correlation misses by whole pixels"""
    errs, plain = [], {}
    for pair in rm.PSF_PAIRS:
        for s in rm.SHIFTS:
            frames, psfs = rm.pair_frames(pair, s, noise)
            e = rm.register_model(frames, psfs, rm.PLAN, rm.PLAN)[1]
            q = rm.register_model(frames, None, rm.PLAN, rm.PLAN)[1]
            errs.append(float(np.hypot(e["dy"] - s[0], e["dx"] - s[1])))
            plain[(pair, s)] = float(np.hypot(q["dy"] - s[0], q["dx"] - s[1]))
            print("ACCURACY noise %g %s %s: (%.3f, %.3f) error %.3f px confidence %.1f; plain %.2f px"
                  % (noise, pair, s, e["dy"], e["dx"], errs[-1], e["confidence"], plain[(pair, s)]))
            assert e["confidence"] > 30
    print("ACCURACY noise %g: worst %.3f mean %.3f px" % (noise, max(errs), np.mean(errs)))
    assert max(errs) <= 1.5 * MEASURED_WORST[noise] and np.mean(errs) <= 1.5 * MEASURED_MEAN[noise]
    for (pair, s), err in plain.items():
        if pair in rm.LINE_PAIRS:
            assert err > 2.0, (pair, s, err)  # without this the PSF term shows nothing


@pytest.fixture(scope="module")
def quality():
    """the PSNRs of the quality case: shifts ignored, frame 0 alone, the true shifts, the estimated shifts"""
    c = rm.quality_case()
    est = rm.register_model(c["ds"], c["psfs"], c["M"], c["N"])

    def run(frames, shifts):
        planes = rm.plan_psfs([c["psfs"][k] for k in frames], [shifts[k] for k in frames], c["M"], c["N"])
        return psnr(frames_model([c["ds"][k] for k in frames], list(planes), c["M"], c["N"], QUALITY_N, lam=QUALITY_LAMBDA, eps=QUALITY_EPS), c["truth"])

    zero = [(0.0, 0.0)] * 3
    return dict(est=est, ignored=run((0, 1, 2), zero), single=max(run((k,), [(e["dy"], e["dx"]) for e in est]) for k in range(3)),
                true=run((0, 1, 2), rm.QUALITY_SHIFTS), registered=run((0, 1, 2), [(e["dy"], e["dx"]) for e in est]))


def test_quality_end_to_end(quality):
    """section 37's three frames with frames 1 and 2 moved: registered, the joint restoration beats the best single frame, stays within
    1 dB of the restoration with the true shifts and lies more than 10 dB above the one that ignores them"""
    q = quality
    print("QUALITY registered %.2f best single %.2f true shifts %.2f ignored %.2f dB" % (q["registered"], q["single"], q["true"], q["ignored"]))
    for e, s in zip(q["est"], rm.QUALITY_SHIFTS):
        assert np.hypot(e["dy"] - s[0], e["dx"] - s[1]) < 0.5
    assert q["registered"] > q["single"]
    assert q["registered"] > q["true"] - 1.0
    assert q["registered"] > q["ignored"] + 10.0


# ---- psf_shift --------------------------------------------------------------------------------------------------------------------------
def test_psf_shift_model():
    rng = np.random.default_rng(0)
    p = rng.uniform(0, 1, (7, 9))
    pad_r, pad_c = 4, 5
    yy, xx = np.mgrid[0:7 + 2 * pad_r, 0:9 + 2 * pad_c]

    def com(a):
        return np.array([np.sum(yy * a), np.sum(xx * a)]) / a.sum()

    base = rm.psf_shift_model([p], [(0, 0)], pad_r, pad_c)[0]
    assert np.array_equal(base[pad_r:pad_r + 7, pad_c:pad_c + 9], p) and np.count_nonzero(base) == p.size
    for s in ((1.3, -2.6), (0.5, 0.5), (-4, 3.999), (2.25, -5), (3, 4), (-0.001, 0.001)):
        q = rm.psf_shift_model([p], [s], pad_r, pad_c)[0]
        assert abs(q.sum() / p.sum() - 1) < 1e-12 and q.min() >= 0      # the sum kept, the weights non-negative
        assert np.allclose(com(q) - com(base), s, atol=1e-12), s            # the centre of mass moves by the shift
    for s in ((2, -3), (-4, 4), (3, 0)):                                   # whole shifts: np.roll placement, exactly
        assert np.array_equal(rm.psf_shift_model([p], [s], pad_r, pad_c)[0], np.roll(base, s, axis=(0, 1))), s
    # a shift outside [-pad, pad - 1] is clamped, a NaN is taken as 0
    for s, c in (((9.5, 0.25), (pad_r - 1, 0.25)), ((-7, 5), (-pad_r, pad_c - 1)), ((3.5, 1e30), (3.5, pad_c - 1)), ((-np.inf, np.inf), (-pad_r, pad_c - 1)),
                 ((np.nan, 1.5), (0.0, 1.5)), ((1.5, np.nan), (1.5, 0.0))):
        assert np.array_equal(rm.psf_shift_model([p], [s], pad_r, pad_c)[0], rm.psf_shift_model([p], [c], pad_r, pad_c)[0]), s
    # the float32 restatement: within float32 round-off of the float64 model, and a different thing (it rounds)
    q32 = rm.psf_shift_model([p.astype(np.float32)], [(1.3, -2.6)], pad_r, pad_c, dtype=np.float32)[0]
    q64 = rm.psf_shift_model([p.astype(np.float32)], [(1.3, -2.6)], pad_r, pad_c)[0]
    assert q32.dtype == np.float32 and np.max(np.abs(q32 - q64)) < 4e-7 and np.max(np.abs(q32 - q64)) > 0
    # several PSFs, each by its own shift
    two = rm.psf_shift_model([p, 2 * p], [(1, 1), (-1.5, 0)], pad_r, pad_c)
    assert np.array_equal(two[0], rm.psf_shift_model([p], [(1, 1)], pad_r, pad_c)[0]) and np.array_equal(two[1], rm.psf_shift_model([2 * p], [(-1.5, 0)], pad_r, pad_c)[0])


def test_shifted_psfs_shift_the_frame():
    """the convention: d_k(r) = (p_k * x)(r - s_k) is the blur of x by PSF k moved by s_k -- whole shifts exactly"""
    rng = np.random.default_rng(1)
    x = rng.uniform(0, 1, (32, 48))
    p = rng.uniform(0, 1, (5, 5))
    for s in ((3, -2), (-4, 5)):
        moved = rm.scene_blur(x, p, s, pad=6)
        assert np.allclose(moved, np.roll(rm.scene_blur(x, p, (0, 0), pad=6), s, axis=(0, 1)), atol=1e-12)
        est = rm.register_model([rm.scene_blur(x, p, (0, 0), pad=6), moved], [p, p], 32, 48, max_shift=(7, 7))[1]
        # (the Hann window stays where it is while the picture moves: the peak is whole, the parabola not exactly 0)
        assert (est["iy"], est["ix"]) == s and abs(est["dy"] - s[0]) < 0.1 and abs(est["dx"] - s[1]) < 0.1 and est["confidence"] > 10


# ---- faults -----------------------------------------------------------------------------------------------------------------------------
SHORT = rm.GPU_CASES[1]  # 32 x 32, window 20 x 27, with PSFs


@pytest.mark.parametrize("fault", [f for f in rm.FAULTS if f != "tie_high"])
def test_plane_faults_are_visible(fault):
    """each wrong version of the correlation plane lies more than 100 PLANE_TOL from the right one on the short case"""
    frames, psfs = rm.gpu_case(SHORT)
    for k in (1, 2):
        good = rm.correlation_plane(frames[0], frames[k], psfs[0], psfs[k], 32, 32)
        bad = rm.correlation_plane(frames[0], frames[k], psfs[0], psfs[k], 32, 32, fault=fault)
        dev = float(np.max(np.abs(good - bad)))
        print("FAULT %s frame %d: %.3e (PLANE_TOL %.1e)" % (fault, k, dev, rm.PLANE_TOL))
        assert dev > 100 * rm.PLANE_TOL, (fault, k, dev)


def test_fault_conj_wrong_flips_the_shift_and_swap_h_moves_it():
    frames, psfs = rm.pair_frames("lines-30-90", (3.3, -5.7), 0.0)
    good = rm.register_model(frames, psfs, rm.PLAN, rm.PLAN)[1]
    flipped = rm.register_model(frames, psfs, rm.PLAN, rm.PLAN, fault="conj_wrong")[1]
    assert abs(flipped["dy"] + good["dy"]) < 1e-9 and abs(flipped["dx"] + good["dx"]) < 1e-9 and abs(good["dy"]) > 3
    e = rm.register_model(frames, psfs, rm.PLAN, rm.PLAN, fault="no_psf")[1]
    assert np.hypot(e["dy"] - good["dy"], e["dx"] - good["dx"]) > 2.0
    # (H_a conj(H_b) of two centred symmetric lines is real: swapping them shows only with PSFs that are not symmetric)
    frames, psfs = rm.short_case(64, 64, 48, 48, 2, [(0, 0), (3, -2)], 5, psf_size=9)
    psfs[1] = np.roll(psfs[1] * np.linspace(0.1, 1.9, 9)[:, None], 2, axis=1).astype(np.float32)
    good = rm.register_model(frames, psfs, 64, 64)[1]
    e = rm.register_model(frames, psfs, 64, 64, fault="swap_h")[1]
    assert np.hypot(e["dy"] - good["dy"], e["dx"] - good["dx"]) > 1.0


def test_fault_tie_high_and_the_pick():
    """two exactly equal maxima: the lowest flat index of the search window wins, (dy, dx) row-major from (-R_r, -R_c); the parabola's
    neighbours are periodic and may lie outside the window; a flat neighbourhood gives offset 0"""
    r = np.zeros((16, 20))
    r[14, 3] = r[2, 17] = 1.0      # (dy, dx) = (-2, 3) and (2, -3)
    a, b = rm.pick(r, 4, 5), rm.pick(r, 4, 5, fault="tie_high")
    assert (a["iy"], a["ix"]) == (-2, 3) and (b["iy"], b["ix"]) == (2, -3)
    r[14, 3] = 0.0
    r[2, 3] = 1.0                  # same row: the lower column wins
    assert (rm.pick(r, 4, 5)["iy"], rm.pick(r, 4, 5)["ix"]) == (2, -3)
    r = np.zeros((16, 20))
    r[4, 5], r[5, 5], r[4, 6] = 1.0, 0.5, 0.25   # the peak at the corner (R_r, R_c) of the window: its neighbours lie outside it
    e = rm.pick(r, 4, 5)
    assert (e["iy"], e["ix"]) == (4, 5) and e["dy"] == 4 + rm.parabola(0.0, 1.0, 0.5) and e["dx"] == 5 + rm.parabola(0.0, 1.0, 0.25)
    assert rm.parabola(1.0, 1.0, 1.0) == 0.0 and rm.parabola(0.0, 1.0, 1.0) == 0.5 and rm.parabola(1.0, 1.0, 0.0) == -0.5
    assert abs(rm.parabola(0.2, 1.0, 0.6) - 0.5 * (0.2 - 0.6) / (0.2 - 2.0 + 0.6)) < 1e-15
    e = rm.pick(r, 2, 2)           # the maximum of the plane lies outside the range: the best inside it
    assert abs(e["iy"]) <= 2 and abs(e["ix"]) <= 2


def test_zero_frames_and_the_reference():
    frames, psfs = rm.gpu_case(rm.GPU_CASES[0])
    frames[2] = np.zeros_like(frames[2])
    est = rm.register_model(frames, psfs, 32, 32)
    assert (est[0]["dy"], est[0]["dx"], est[0]["peak"], est[0]["confidence"]) == (0.0, 0.0, 1.0, 0.0)
    assert (est[2]["dy"], est[2]["dx"], est[2]["peak"], est[2]["confidence"]) == (0.0, 0.0, 0.0, 0.0) and est[1]["peak"] > 0
    border = np.zeros_like(frames[1])
    border[0, :] = border[:, 0] = 1.0  # only where the Hann window is 0: all zero under the window
    assert rm.register_model([frames[0], border], psfs[:2], 32, 32)[1]["peak"] == 0.0


@pytest.mark.parametrize("case", rm.GPU_CASES, ids=rm.GPU_IDS)
def test_the_device_cases_have_a_decided_peak(case):
    """what test_register_gpu.py rests on: the model's peak of every frame stands PEAK_MARGIN x PLANE_TOL above everything else in the
    search window (its neighbours included), and both parabola denominators are far from 0, so shift_bound is small"""
    frames, psfs = rm.gpu_case(case)
    est = rm.register_model(frames, psfs, case[1], case[2], reference=case[6], max_shift=case[7])
    for k, e in enumerate(est):
        if k == case[6]:
            continue
        assert e["peak"] - e["second"] >= rm.PEAK_MARGIN * rm.PLANE_TOL, (k, e["peak"] - e["second"])
        assert min(abs(d) for d in e["denom"]) > 1000 * rm.PLANE_TOL and rm.shift_bound(min(e["denom"], key=abs)) < 1e-3, (k, e["denom"])


def test_the_device_cases_cover_what_they_claim():
    ids = dict(zip(rm.GPU_IDS, rm.GPU_CASES))
    assert any(c[1] == c[3] and c[2] == c[4] for c in rm.GPU_CASES), "no case with window = plan"
    assert any(c[5] and c[1] % 2 and c[2] % 2 for c in rm.GPU_CASES) and any(c[5] and c[1] % 2 and c[2] % 2 == 0 for c in rm.GPU_CASES)
    assert any(c[2] > 1024 for c in rm.GPU_CASES), "no case with two column workgroups of the pair pass"
    assert any(len(c[9]) == 1 for c in rm.GPU_CASES) and any(len(c[9]) == 8 and c[6] != 0 for c in rm.GPU_CASES)
    assert any(not c[8] for c in rm.GPU_CASES), "no plain case"
    # exactly at +- max_shift, found there by the model; and a shift beyond the range
    frames, psfs = rm.gpu_case(ids["32x32-win20x27"])
    est = rm.register_model(frames, psfs, 32, 32, max_shift=(5, 6))
    assert (est[2]["iy"], est[2]["ix"]) == (-5, 6)
    frames, psfs = rm.gpu_case(ids["256-win200-K8"])
    est = rm.register_model(frames, psfs, 256, 256, reference=3)
    assert (est[6]["iy"], est[6]["ix"]) == (50, -50) and abs(est[1]["dy"] - 0.5) < 0.2


# ---- the public surface -----------------------------------------------------------------------------------------------------------------
FUNCS = {"fdr_register_frames_f32": 13, "fdr_register_frames_f32_dev": 14, "fdr_psf_shift_f32": 11, "fdr_psf_shift_f32_dev": 11}  # commas
STRUCTS = {
    "fdr_frame_shift": ("FrameShiftC", (("double", "dy"), ("double", "dx"), ("float", "peak"), ("float", "confidence")), 24, [0, 8, 16, 20]),
    "fdr_register_params": ("RegisterParams", (("int", "reference"), ("int", "max_shift_rows"), ("int", "max_shift_cols"), ("float", "eps_rel"),
                                               ("void*", "stream")), 24, [0, 4, 8, 12, 16]),
    "fdr_psf_shift_params": ("PsfShiftParams", (("int", "pad_rows"), ("int", "pad_cols"), ("void*", "stream")), 16, [0, 4, 8]),
}


def test_symbols_and_surface(fdr):
    _need(fdr)
    header = open(os.path.join(ROOT, "include", "fdr.h")).read()
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "void*": ctypes.c_void_p}
    for name, (pyname, want, size, offsets) in STRUCTS.items():
        m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), header, re.S)
        assert m, "%s is not in the header" % name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        fields = tuple((t.replace(" ", ""), n.strip()) for t, names in re.findall(r"\b(int|float|double|void\s*\*)\s*([^;]+);", body) for n in names.split(","))
        assert fields == want, (name, fields)
        P = getattr(fdr, pyname)
        assert [f[0] for f in P._fields_] == [n for _, n in want] and [f[1] for f in P._fields_] == [ctype[t] for t, _ in want], name
        assert ctypes.sizeof(P) == size and [getattr(P, n).offset for _, n in want] == offsets, name
    assert re.search(r"#define\s+FDR_REGISTER_EPS_REL\s+1e-3f\b", header) and fdr.REGISTER_EPS_REL == rm.EPS_REL == 1e-3
    assert re.search(r"#define\s+FDR_MAX_FRAMES\s+8\b", header) and fdr.MAX_FRAMES == rm.MAX_FRAMES
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", fdr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split()}
    for name, commas in FUNCS.items():
        d = re.search(r"\bint\s+%s\s*\(([^;{]*)\)\s*;" % name, code)
        assert d, name
        assert "stream" not in d.group(1), "the stream travels in the struct"
        assert d.group(1).count(",") == commas, name
        assert name in exported and name in fdr.EXPORTED_SYMBOLS, name
    assert "THE STREAM TRAVELS IN THE STRUCT" in header[header.index("registering the frames of a burst"):header.index("typedef struct fdr_frame_shift")]
    assert fdr.FrameShift._fields == ("dy", "dx", "peak", "confidence")
    sig = inspect.signature(fdr.Plan.register_frames).parameters
    assert list(sig) == ["self", "frames", "psfs", "reference", "max_shift", "eps_rel"] and sig["psfs"].default is None
    sig = inspect.signature(fdr.Plan.register_frames_dev).parameters
    assert list(sig)[:8] == ["self", "d_imgs", "img_pitch", "count", "rows", "cols", "stride", "d_shifts"] and sig["stream"].default is None
    assert list(inspect.signature(fdr.registerFrames).parameters)[:2] == ["imgs", "psfs"] and inspect.signature(fdr.registerFrames).parameters["psfs"].default is None
    assert "stream" in inspect.signature(fdr.psf_shift_dev).parameters and callable(fdr.psf_shift)
    for f in (fdr.richardsonLucyFrames_myfft, fdr.richardsonLucyFrames_RGB, fdr.tvDeblurFrames_myfft, fdr.tvDeblurFrames_RGB):
        assert inspect.signature(f).parameters["register"].default is False, f.__name__
    mk = open(os.path.join(os.path.dirname(fdr.LIB_PATH), "Makefile")).read()
    assert "csrc/fdr_register.hip" in mk and "csrc/fdr_api_register.hip" in mk
    hpp = open(os.path.join(ROOT, "include", "fft", "fft.hpp")).read()
    assert re.search(r"\bregisterFrames\s*\(", hpp) and "RegisterOptions& register_frames" in hpp


def test_refusals_without_a_device(fdr):
    """null pointers, and everything fdr_psf_shift_f32* refuses, come before a device is touched"""
    _need(fdr)
    L = fdr.lib
    img = np.ones((2, 16, 32), dtype=np.float32)
    sh = (fdr.FrameShiftC * 8)()
    rp = fdr.RegisterParams(0, 0, 0, 0.0, None)
    for h, i, q, o in ((None, img.ctypes.data, ctypes.byref(rp), sh), (1, None, ctypes.byref(rp), sh), (1, img.ctypes.data, None, sh),
                       (1, img.ctypes.data, ctypes.byref(rp), None)):
        assert L.fdr_register_frames_f32(h, i, 512, 2, 16, 32, 32, None, 0, 0, 0, 0, q, o) == -1
        assert b"fdr_register_frames_f32: null argument" in L.fdr_last_error()
        assert L.fdr_register_frames_f32_dev(h, i, 512, 2, 16, 32, 32, None, 0, 0, 0, 0, q, o, None) == -1
        assert b"fdr_register_frames_f32_dev: null argument" in L.fdr_last_error()
    psf = np.ones((2, 5, 8), dtype=np.float32)
    out = np.zeros((2, 11, 16), dtype=np.float32)

    def shift(fn, pp=psf.ctypes.data, ppitch=40, count=2, pr=5, pc=7, ps=8, shp=ctypes.addressof(sh), pad=(3, 4), op=out.ctypes.data, opitch=176, ostride=16,
              prm=True):
        sp = fdr.PsfShiftParams(pad[0], pad[1], None)
        return getattr(L, fn)(0, pp, ppitch, count, pr, pc, ps, shp, ctypes.byref(sp) if prm else None, op, opitch, ostride)

    for fn in ("fdr_psf_shift_f32", "fdr_psf_shift_f32_dev"):
        for kw in (dict(pp=None), dict(shp=None), dict(op=None), dict(prm=False)):
            assert shift(fn, **kw) == -1 and (fn + ": null argument").encode() in L.fdr_last_error(), (fn, kw)
        for kw, msg in ((dict(count=0), b"count must be 1 .. FDR_MAX_FRAMES"), (dict(count=9), b"count must be"), (dict(pr=0), b"PSFs must be 1 .. 8192"),
                        (dict(pc=8193, ps=8193), b"PSFs must be 1 .. 8192"), (dict(ps=6), b"pstride >= pcols"), (dict(pad=(0, 4)), b"pad_rows and pad_cols"),
                        (dict(pad=(3, 8193)), b"pad_rows and pad_cols"), (dict(ostride=14), b"out_stride is below"), (dict(ppitch=38), b"psf_pitch is below"),
                        (dict(opitch=174), b"out_pitch is below"), (dict(op=psf.ctypes.data + 64), b"overlaps the PSFs or the shifts"),
                        (dict(op=ctypes.addressof(sh)), b"overlaps the PSFs or the shifts")):
            assert shift(fn, **kw) == -1 and msg in L.fdr_last_error(), (fn, kw, L.fdr_last_error())
    assert shift("fdr_psf_shift_f32_dev", shp=ctypes.addressof(sh) + 4) == -1 and b"d_shifts must be 8-byte aligned" in L.fdr_last_error()
    with pytest.raises(ValueError):
        fdr.psf_shift([psf[0]], [(0, 0), (1, 1)], 2)


# ---- the workspace block ------------------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("M,N", [(32, 32), (32, 2048), (45, 75), (1024, 1024), (8192, 4096)])
def test_workspace_block(M, N):
    """the new block through workspace_check's new argument: the PSF pair plane, the cross-power partials with their sum and the gate, four
    doubles per workgroup of the peak pass, 24 bytes per frame of results -- the sizes from the kernels' grids, written out again here"""
    d = os.path.join(ROOT, "tools", "cli")
    subprocess.check_call(["make", "-C", d, "-s", "workspace_check"])
    rc_, rp_ = (M // 2 + 1) * ceil_div(N, 256), M * ceil_div(N, 1024)
    arg = "register:M=%d,N=%d,rc=%d,rp=%d,frames=8" % (M, N, rc_, rp_)
    r = subprocess.run([os.path.join(d, "workspace_check"), arg], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "workspace check ok: 1 cases" in r.stdout, (r.stdout[-500:], r.stderr[-1000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    assert lines[0] == ["case", arg]
    plane, part, peak, res = 8 * M * N, 8 * (rc_ + 2), 32 * rp_, 24 * 8
    assert lines[1] == ["workspace", "register", "bytes", str(plane + part + peak + res), "count", "1"]
    want = [("psf", 0, plane), ("part", plane, part), ("peak", plane + part, peak), ("result", plane + part + peak, res)]
    got = [(l[1], int(l[3]), int(l[5]), int(l[7])) for l in lines[2:6]]
    assert [g[:3] for g in got] == want and all(g[3] == 8 and g[1] % 8 == 0 for g in got), got
    # the pair pass lends the peak partials for its two sums per workgroup: they fit
    assert 2 * rp_ <= 4 * rp_
    bad = subprocess.run([os.path.join(d, "workspace_check"), "register:M=32,N=32"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "5 numbers" in bad.stderr


# ---- the command line -----------------------------------------------------------------------------------------------------------------------
def test_cli_register_usage_and_refusals():
    """tools/cli/gpu: --register without --frame, --max-shift without --register or below 1, and --register beside anything the frames leg
    refuses print a usage text and fail before a picture is read (the paths do not exist); the accepted form gets as far as the picture"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "cli"), "-s", "gpu"])
    gpu = os.path.join(ROOT, "tools", "cli", "gpu")
    frame = ["--frame", "none2.png", "15", "30"]
    ok = ["--rl", "5", "--free-boundary"]
    for args in (["--register"], ok + ["--register"], ok + frame + ["--max-shift", "8"], ok + frame + ["--register", "--max-shift", "0"],
                 ok + frame + ["--register", "--max-shift", "-3"]):
        r = subprocess.run([gpu, "none.png", "15", "30"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" in r.stdout and "--register" in r.stdout and "Cannot read" not in r.stdout, (args, r.stdout[-300:])
    for args in (ok + ["--accel"] + frame + ["--register"], ["--tv", "5", "--free-boundary"] + frame + ["--register"], ok + frame + ["--register", "--verify"]):
        r = subprocess.run([gpu, "none.png", "15", "30"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" in r.stdout and "Cannot read" not in r.stdout, (args, r.stdout[-300:])
    for args in (ok + frame + ["--register"], ok + frame + ["--register", "--max-shift", "12", "--rl-tv", "0.01", "--out", "o.png"]):
        r = subprocess.run([gpu, "none.png", "15", "30"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Cannot read image" in r.stdout, (args, r.stdout[-300:])
    src = open(os.path.join(ROOT, "tools", "cli", "gpu.cpp")).read()
    assert '"shift: frame "' in src and '" confidence "' in src
