"""CPU pins of tests/_rlaccel_batch_model.py, the judge of test_rlaccel_batch_gpu.py: the float64 batched accelerated call equals
`accelerate` image by image for every group size; the judge flags each fault model of a batched accelerated call; on every scene of
the GPU case list the model's alphas of any two images lie at least 1e-3 apart (or two of the faults would go unseen); the case list
covers what the GPU test claims; and the header, the binding and the wrappers declare the new entry points."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import _batch_model as bm
import _rl_batch_model as rb
import _rlaccel_batch_model as ab
from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, centred_psf, dense_psf
from _rlaccel_model import RLA_ALPHA_TOL, RLA_FREE_TOL, RLA_TOL
from _rlfree_model import SIGMA, SIGMA_MARGIN, rlfree_state, sigma_margin
from conftest import ROOT

M, N, ROWS, COLS, COUNT, ITER = 16, 32, 15, 29, 5, 5
PSF = centred_psf(dense_psf(3, 5), M, N)
TOL = {"plain": RLA_TOL, "free": RLA_FREE_TOL}


@pytest.fixture(autouse=True)
def _needs_the_feature(fdr):
    """the judge and the case list serve the accelerated batch: without its entry points nothing here passes"""
    assert "fdr_richardson_lucy_batch_accel_f32_dev" in fdr.EXPORTED_SYMBOLS, "the library has no batched accelerated Richardson-Lucy"


def _case(loose, form, n=ITER):
    lay = (bm.loose_layout if loose else bm.tight_layout)(ROWS, COLS, COUNT)
    imgs = rb.images(M, N, ROWS, COLS, COUNT, 7)
    w = rb.mask(ROWS, COLS, 3) if form == "free" else None
    return lay, ab.alpha_layout(n, COUNT, loose), imgs, bm.pack_inputs(imgs.astype(np.float64), lay), w


_REFS = {}


def _refs(form, n, area):
    """per image (output, alphas) of the single-image model: one run of `accelerate` per image and form, shared by the tests"""
    if form not in _REFS:
        lay, _, imgs, _, w = _case(False, form)
        _REFS[form] = [ab.single_path(form, d, PSF, M, N, range(ITER + 1), w) for d in imgs]
    lay = bm.tight_layout(ROWS, COLS, COUNT)
    return (np.stack([ab.output_of(keep[n], lay, area, M, N) for keep, _ in _REFS[form]]), np.stack([a[:n] for _, a in _REFS[form]]))


@pytest.mark.parametrize("loose", (False, True))
@pytest.mark.parametrize("form", ("plain", "free"))
def test_fault_free_call_is_the_single_image_model(loose, form):
    for n in (0, 2, 3, ITER):
        lay, al, imgs, flat, w = _case(loose, form, n)
        for area in ab.AREAS:
            refs, ref_a = _refs(form, n, area)
            for group in (1, 2, 3, 5, 8):
                out, alphas = ab.batched_call(form, flat, lay, lay, al, PSF, M, N, n, area, group, weights=w)
                v = ab.judge("group %d" % group, out, lay, alphas, al, refs, ref_a, refs, ref_a, 1e-13, 1e-13, area)
                assert not [b for b in v.bad if "differ from" not in b], v.bad[:3]  # (bits: equal up to the order of float64 sums)
                assert v.worst <= 1e-13 and v.worst_alpha <= 1e-13


def _flagged(form, fault, group, area=NORM_NONE, loose=True, n=ITER):
    lay, al, imgs, flat, w = _case(loose, form, n)
    refs, ref_a = _refs(form, n, area)
    out, alphas = ab.batched_call(form, flat, lay, lay, al, PSF, M, N, n, area, group, weights=w, fault=fault)
    return ab.judge(fault, out, lay, alphas, al, refs, ref_a, refs, ref_a, TOL[form], RLA_ALPHA_TOL, area)


def test_the_pin_images_have_alphas_apart():
    for form in ("plain", "free"):
        assert ab.alphas_apart(_refs(form, ITER, NORM_NONE)[1], ITER), form


@pytest.mark.parametrize("form", ("plain", "free"))
def test_judge_flags_image_0s_alpha_on_every_image(form):
    v = _flagged(form, "alpha_of_image0", 2)
    assert "model" in v.checks and "bits" in v.checks
    assert not any("image 0:" in b or "image 2:" in b or "image 4:" in b for b in v.bad) and any("image 1:" in b for b in v.bad)
    assert not _flagged(form, "alpha_of_image0", 2, n=2).bad  # no extrapolation before the third step: the GPU test iterates further


@pytest.mark.parametrize("form", ("plain", "free"))
def test_judge_flags_sums_over_the_group(form):
    v = _flagged(form, "sums_over_group", 3)
    assert {"alpha_bits", "alpha_model"} <= v.checks and "bits" in v.checks
    assert any("image 0:" in b for b in v.bad) and any("image 4:" in b for b in v.bad)
    assert not _flagged(form, "sums_over_group", 1).bad  # groups of one have nothing to mix


@pytest.mark.parametrize("form", ("plain", "free"))
def test_judge_flags_a_shared_g_plane(form):
    v = _flagged(form, "shared_g_plane", 2)
    assert {"alpha_bits", "alpha_model"} <= v.checks
    # the last image of every group reads its own g
    assert any("image 0:" in b for b in v.bad) and not any("image 1:" in b or "image 3:" in b or "image 4:" in b for b in v.bad)


@pytest.mark.parametrize("form", ("plain", "free"))
def test_judge_flags_the_previous_groups_u(form):
    v = _flagged(form, "previous_group_u", 2)
    assert {"bits", "model"} <= v.checks
    assert not any("image 0:" in b or "image 1:" in b for b in v.bad) and any("image 2:" in b for b in v.bad)  # the first group is right


def test_judge_flags_an_ignored_alpha_pitch():
    v = _flagged("plain", "ignore_alpha_pitch", 3)
    assert "alpha_layout" in v.checks and "alpha_bits" in v.checks and not {"bits", "model", "layout"} & v.checks
    assert not _flagged("plain", "ignore_alpha_pitch", 3, loose=False).bad  # a pitch of `iterations` cannot tell: the GPU test runs loose ones


def test_judge_flags_a_dropped_tail():
    for area in ab.AREAS:
        v = _flagged("plain", "drop_last_group", 2, area=area)  # 5 images: 2, 2, 1
        assert {"bits", "alpha_bits"} <= v.checks and any("image 4:" in b for b in v.bad) and not any("image 3:" in b for b in v.bad)
    assert not _flagged("plain", "drop_last_group", 5).bad  # no tail, no fault


def test_judge_flags_nan_and_stray_stores():
    lay, al, imgs, flat, w = _case(True, "plain", 3)
    refs, ref_a = _refs("plain", 3, NORM_NONE)
    out, alphas = ab.batched_call("plain", flat, lay, lay, al, PSF, M, N, 3, NORM_NONE, 2)
    alphas[al.lead + al.pitch + 2] = np.nan
    assert "alpha_finite" in ab.judge("nan", out, lay, alphas, al, refs, ref_a, refs, ref_a, RLA_TOL, RLA_ALPHA_TOL, NORM_NONE).checks
    out, alphas = ab.batched_call("plain", flat, lay, lay, al, PSF, M, N, 3, NORM_NONE, 2)
    alphas[al.lead + 3] = 0.0  # the pitch gap behind image 0's alphas
    assert ab.judge("stray", out, lay, alphas, al, refs, ref_a, refs, ref_a, RLA_TOL, RLA_ALPHA_TOL, NORM_NONE).checks == {"alpha_layout"}
    out[bm.out_base(lay, 0) + lay.cols] = 0.0  # the stride padding of row 0
    assert "layout" in ab.judge("stray", out, lay, alphas, al, refs, ref_a, refs, ref_a, RLA_TOL, RLA_ALPHA_TOL, NORM_NONE).checks


# ---- the GPU case list ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", ab.SCENES, ids=ab.SCENE_IDS)
def test_alphas_of_every_scene_lie_apart(oracle, sc):
    """every case of the GPU list that extrapolates (3, 4 and 7 iterations): any two images differ by >= 1e-3 in a model alpha it
    computes; no free-form scene has a coverage at the threshold sigma; and single precision can resolve the scene (the model's own
    float32 run on the CPU stays within a quarter of the GPU's tolerances)"""
    psf = ab.scene_psf(oracle.motion_blur_kernel(15, 30.0), sc)  # (the device's motionBlurKernel(15, 30.0), bit for bit)
    imgs, w = ab.scene_images(sc), ab.scene_mask(sc)
    ref_a = [ab.single_path(sc.form, d, psf, sc.M, sc.N, (max(ab.ITERATIONS),), w)[1] for d in imgs]
    for n in ab.ITERATIONS:
        if n >= 3:
            assert ab.alphas_apart(ref_a, n), (sc.name, n, np.asarray(ref_a)[:, 2:n])
    if sc.form == "free":
        assert sigma_margin(rlfree_state(imgs[0], psf, sc.M, sc.N, 0, weights=w)["alpha"], SIGMA) >= SIGMA_MARGIN
    e, ea, ok = ab.resolvable(sc, psf, TOL[sc.form], RLA_ALPHA_TOL)
    assert ok, "%s: the model run in float32 on the CPU is %.3g (alphas %.3g) off the float64 run: single precision cannot resolve the scene" % (sc.name, e, ea)


def test_case_list_covers_what_the_gpu_test_claims():
    by_name = {s.name: s for s in ab.SCENES}
    # plain form, sums over the window: two column tiles with a 3-column tail, rows no multiple of 8, the scalar path
    s = by_name["plain 64x2048 win 61x1027 loose"]
    r, c = ab.sum_window(s)
    assert (c + ab.RA_COLS - 1) // ab.RA_COLS == 2 and c % ab.RA_COLS == 3 and c % 4 == 3 and r % ab.RA_ROWS != 0 and not ab.vec_path(s)
    # one tile, full window, the 16-byte path
    s = by_name["plain 32x64 full tight"]
    assert ab.sum_window(s) == (s.M, s.N) and s.N <= ab.RA_COLS and ab.vec_path(s)
    # one image takes the split row kernels, a group the packed ones
    s = by_name["plain 128x256 win 100x200"]
    assert bm.rows4_use_split(s.N, s.M, 1, True) and not bm.rows4_use_split(s.N, s.M, 2, True)
    # free form, sums over the whole plan: both plans with NULL weights, a mask with zeros, the M x N output
    for plan, win in (((16, 2048), (11, 1500)), ((64, 64), (40, 50))):
        kinds = {(x.masked, x.full_out) for x in ab.SCENES if x.form == "free" and (x.M, x.N) == plan and (x.rows, x.cols) == win}
        assert kinds == {(False, False), (True, False), (False, True)}, plan
    assert ab.sum_window(by_name["free 16x2048 win 11x1500 null weights"]) == (16, 2048)  # 2 x 2 tiles
    assert len(ab.SCENES) == 9 and all(np.any(ab.scene_mask(x) == 0) for x in ab.SCENES if x.masked)
    # 5 images in groups of 2, 3, 4, 8 and 1: tails, count < group, the loop of the single calls
    assert ab.COUNT == 5 and set(ab.GROUPS) == {1, 2, 3, 4, 8}
    launches = {g: bm.launches(ab.COUNT, g) for g in ab.GROUPS}
    assert launches == {2: [2, 2, 1], 3: [3, 2], 4: [4, 1], 8: [5], 1: [1] * 5}
    # iterations: nothing, the plain steps, the first extrapolation, both parities of `first` beyond it
    assert set(ab.ITERATIONS) == {0, 1, 2, 3, 4, 7} and {n & 1 for n in ab.ITERATIONS if n >= 3} == {0, 1}
    assert set(ab.AREAS) == {NORM_NONE, NORM_CROPPED, NORM_PADDED}
    # loose layouts exist in both forms (the alphas' pitch gaps, the output's stride padding and pitch gaps)
    assert {x.form for x in ab.SCENES if x.loose} == {"plain", "free"}
    assert ab.alpha_layout(7, 5, True).pitch > 7 and ab.alpha_layout(7, 5, False).pitch == 7


# ---- the surface ----------------------------------------------------------------------------------------------------------
def _header_args(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fdr.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_binding_declares_the_batched_accelerated_entry_points(fdr):
    """fails without the feature: the header, the signatures table, Plan and the RGB functions all gain the accelerated batch"""
    for name in ("fdr_richardson_lucy_batch_accel_f32_dev", "fdr_richardson_lucy_batch_accel_f32"):
        assert name in fdr.EXPORTED_SYMBOLS, name
        restype, argtypes = fdr._SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == _header_args(name), name
    assert _header_args("fdr_richardson_lucy_batch_accel_f32") + 1 == _header_args("fdr_richardson_lucy_batch_accel_f32_dev") == 16
    assert _header_args("fdr_richardson_lucy_batch_f32_dev") == 14 and ctypes.sizeof(fdr.RlBatchParams) == 24  # unchanged
    for fn, names in ((fdr.Plan.richardson_lucy_batch_dev, ("accelerate", "d_alphas", "alpha_pitch")),
                      (fdr.Plan.richardson_lucy_batch, ("accelerate", "return_alphas")),
                      (fdr.richardsonLucy_RGB, ("accelerate",)), (fdr.richardsonLucyFree_RGB, ("accelerate",))):
        prm = inspect.signature(fn).parameters
        for n in names:
            assert n in prm and prm[n].default in (False, None), (fn.__name__, n)


def test_refusals_need_no_device(fdr):
    """a null plan and a null params pointer are refused before anything else"""
    L = fdr.lib
    assert L.fdr_richardson_lucy_batch_accel_f32_dev(None, None, 0, 1, 8, 32, 32, None, 0, None, 0, 32, None, None, 0, None) == -1
    assert L.fdr_richardson_lucy_batch_accel_f32(None, None, 0, 1, 8, 32, 32, None, 0, None, 0, 32, None, None, 0) == -1
    assert b"null" in L.fdr_last_error()
