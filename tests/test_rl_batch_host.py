"""CPU pins of tests/_rl_batch_model.py, the judge of test_rl_batch_gpu.py: the float64 batched call equals the single-image models
image by image, on tight and loose layouts, for every group size; the judge flags each fault model of a batched Richardson-Lucy; the
case lists reach what they claim; and the Python binding declares the three new entry points as the header does."""
import os
import re

import numpy as np
import pytest

import _batch_model as bm
import _rl_batch_model as rb
from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, RL_TOL, centred_psf, dense_psf
from _rlfree_model import RLFREE_TOL
from conftest import ROOT

M, N, ROWS, COLS, COUNT = 16, 32, 15, 29, 5
PSF = centred_psf(dense_psf(3, 5), M, N)


def _case(loose, form, full_out=False):
    lay = (bm.loose_layout if loose else bm.tight_layout)(ROWS, COLS, COUNT)
    olay = rb.out_layout(lay, M, N) if full_out else lay
    imgs = rb.images(M, N, ROWS, COLS, COUNT, 7)
    w = rb.mask(ROWS, COLS, 3) if form == "free" else None
    return lay, olay, imgs, bm.pack_inputs(imgs.astype(np.float64), lay), w


@pytest.mark.parametrize("loose", (False, True))
@pytest.mark.parametrize("form,full_out", (("plain", False), ("free", False), ("free", True)))
def test_fault_free_call_is_the_single_image_model(loose, form, full_out):
    lay, olay, imgs, flat, w = _case(loose, form, full_out)
    for area in rb.AREAS:
        for n in (0, 2):
            refs = rb.references(form, imgs, PSF, M, N, n, area, w, out_shape=(olay.rows, olay.cols))
            for group in (1, 2, 3, 5, 8):
                out = rb.batched_call(form, flat, lay, olay, PSF, M, N, n, area, group, weights=w)
                v = rb.judge("group %d" % group, out, olay, refs, refs, 0.0, area)
                assert not v.bad, v.bad[:3]


def _flagged(form, fault, group, area=NORM_NONE, loose=True, n=2, tol=None):
    lay, olay, imgs, flat, w = _case(loose, form)
    refs = rb.references(form, imgs, PSF, M, N, n, area, w)
    out = rb.batched_call(form, flat, lay, olay, PSF, M, N, n, area, group, weights=w, fault=fault)
    return rb.judge(fault, out, olay, refs, refs, RL_TOL if form == "plain" else RLFREE_TOL if tol is None else tol, area)


@pytest.mark.parametrize("form", ("plain", "free"))
def test_judge_flags_a_ratio_on_image_0s_datum(form):
    v = _flagged(form, "ratio_reads_image0", 2)
    assert {"bits", "model"} <= v.checks
    # image 0 of every group is right, the others are not
    assert not any("image 0:" in b or "image 2:" in b or "image 4:" in b for b in v.bad) and any("image 1:" in b for b in v.bad)


@pytest.mark.parametrize("form", ("plain", "free"))
def test_judge_flags_an_update_on_the_previous_groups_estimate(form):
    v = _flagged(form, "update_reads_previous_group", 2)
    assert {"bits", "model"} <= v.checks
    assert not any("image 0:" in b or "image 1:" in b for b in v.bad) and any("image 2:" in b for b in v.bad)  # the first group is right


def test_judge_flags_an_ignored_out_pitch():
    v = _flagged("plain", "ignore_out_pitch", 3)
    assert "layout" in v.checks and "bits" in v.checks
    assert not _flagged("plain", "ignore_out_pitch", 3, loose=False).bad  # a tight layout cannot tell: the GPU test runs loose ones


def test_judge_flags_wgt_on_image_0_only():
    v = _flagged("free", "wgt_image0_only", 3)
    assert {"bits", "model"} <= v.checks
    assert not any("image 0:" in b or "image 3:" in b for b in v.bad) and any("image 1:" in b for b in v.bad)
    assert not _flagged("free", "wgt_image0_only", 3, n=0).bad  # the start has no update: the GPU test iterates


def test_judge_flags_a_dropped_tail():
    for area in rb.AREAS:
        v = _flagged("plain", "drop_last_group", 2, area=area)  # 5 images: 2, 2, 1
        assert "bits" in v.checks and any("image 4:" in b for b in v.bad) and not any("image 3:" in b for b in v.bad)
    assert not _flagged("plain", "drop_last_group", 5).bad  # no tail, no fault


def test_judge_flags_nan_and_stray_stores():
    lay, olay, imgs, flat, w = _case(True, "plain")
    refs = rb.references("plain", imgs, PSF, M, N, 1, NORM_NONE)
    out = rb.batched_call("plain", flat, lay, olay, PSF, M, N, 1, NORM_NONE, 2)
    out[bm.out_base(olay, 1) + 3] = np.nan
    assert "finite" in rb.judge("nan", out, olay, refs, refs, RL_TOL, NORM_NONE).checks
    out = rb.batched_call("plain", flat, lay, olay, PSF, M, N, 1, NORM_NONE, 2)
    out[bm.out_base(olay, 0) + olay.cols] = 0.0  # the stride padding of row 0
    assert rb.judge("stray", out, olay, refs, refs, RL_TOL, NORM_NONE).checks == {"layout"}


def test_case_lists_reach_what_they_claim():
    # groups and tails: launches of 2, 3, 4, 5, 8 and tails of 1, 2, 3
    sizes = {n for g in rb.GROUPS for n in bm.launches(rb.COUNT, g)}
    assert {2, 3, 4, 5, 8} <= sizes and {bm.launches(rb.COUNT, g)[-1] for g in rb.GROUPS} >= {1, 2, 3}
    # column lengths: every pass-B' kernel kind that bm.cols_kernel names, with the launches of the length sweep
    kinds = {bm.cols_kernel(Mc, n, Nc) for Mc, Nc in rb.COLUMN_PLANS for g in rb.LENGTH_GROUPS for n in bm.launches(rb.LENGTH_COUNT, g)}
    assert kinds == {"split", "radix8-persistent", "fused16-flat", "fused16-2d"}
    # row lengths: every LOGL 5 .. 13, the 2048-row plans where one image takes the split kernel and a group may not
    assert {bm.log2(Nr) for _, Nr in rb.ROW_PLANS} == set(range(5, 14))
    assert bm.rows4_use_split(256, 2048, 1, True) and not bm.rows4_use_split(256, 2048, 2, True)
    for Mr, Nr in rb.ROW_PLANS:
        count, groups = (rb.BIG_COUNT, rb.BIG_GROUPS) if Mr * Nr >= rb.BIG_PIXELS else (rb.LENGTH_COUNT, rb.LENGTH_GROUPS)
        ns = {n for g in groups for n in bm.launches(count, g)}
        assert 1 in ns and max(ns) >= 3  # the single-image kernels and a group, in one case
    assert {c.form for c in rb.LENGTH_CASES} == set(rb.FORMS)


def _header_args(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fdr.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_binding_declares_the_batched_entry_points(fdr):
    """fails without the feature: the header, the signatures table and Plan all gain the batched calls"""
    import ctypes
    for name in ("fdr_blur_batch_f32_dev", "fdr_richardson_lucy_batch_f32_dev", "fdr_richardson_lucy_batch_f32"):
        assert name in fdr.EXPORTED_SYMBOLS, name
        restype, argtypes = fdr._SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == _header_args(name), name
    assert _header_args("fdr_richardson_lucy_batch_f32") + 1 == _header_args("fdr_richardson_lucy_batch_f32_dev") == 14
    assert _header_args("fdr_blur_batch_f32_dev") == 12
    assert [f[0] for f in fdr.RlBatchParams._fields_] == ["iterations", "norm_area", "free_boundary", "sigma", "out_rows", "out_cols"]
    assert ctypes.sizeof(fdr.RlBatchParams) == 24
    for method in ("blur_batch_dev", "richardson_lucy_batch_dev", "richardson_lucy_batch"):
        assert callable(getattr(fdr.Plan, method, None)), method
    assert callable(fdr.richardsonLucy_RGB) and callable(fdr.richardsonLucyFree_RGB)


def test_refusals_need_no_device(fdr):
    """a null plan and a null params pointer are refused before anything else"""
    L = fdr.lib
    assert L.fdr_blur_batch_f32_dev(None, None, 0, 1, 8, 32, 32, None, 0, 32, 0, None) == -1
    assert L.fdr_richardson_lucy_batch_f32_dev(None, None, 0, 1, 8, 32, 32, None, 0, None, 0, 32, None, None) == -1
    assert L.fdr_richardson_lucy_batch_f32(None, None, 0, 1, 8, 32, 32, None, 0, None, 0, 32, None) == -1
    assert b"null" in L.fdr_last_error()
