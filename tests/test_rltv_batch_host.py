"""CPU pins of tests/_rltv_batch_model.py, the specification of Richardson-Lucy with the TV prior in groups
(fdr_richardson_lucy_tv_batch_f32*, fdr_rl_tv_factor_group_f32_dev): the judge flags each fault model of such a call and of the
coupled factor; the model agrees with _rltv_model.py (uncoupled, and coupled on one channel) and with _rl_batch_model.py (lambda = 0);
the coupled form restores the colour quality scene no worse than the channel-wise one, by the gains the model file records; and the
binding declares the new surface as the header does."""
import ctypes
import os
import re

import numpy as np
import pytest

import _batch_model as bm
import _rl_batch_model as rb
import _rltv_batch_model as tb
from _rl_model import NORM_NONE, centred_psf, dense_psf
from _rltv_model import RLTV_FREE_TOL, RLTV_TOL, rltv_free_model, rltv_model, tv_factor
from conftest import ROOT

M, N, ROWS, COLS, COUNT = 16, 32, 15, 29, 5
PSF = centred_psf(dense_psf(3, 5), M, N)
LAM, EPS = 0.05, 1e-3


def _case(loose, form, full_out=False):
    lay = (bm.loose_layout if loose else bm.tight_layout)(ROWS, COLS, COUNT)
    olay = rb.out_layout(lay, M, N) if full_out else lay
    imgs = rb.images(M, N, ROWS, COLS, COUNT, 7)
    w = rb.mask(ROWS, COLS, 3) if form == "free" else None
    return lay, olay, imgs, bm.pack_inputs(imgs.astype(np.float64), lay), w


def _tol(form):
    return RLTV_TOL if form == "plain" else RLTV_FREE_TOL


# ---- (ii) the model is consistent with the existing ones ------------------------------------------------------------------
@pytest.mark.parametrize("loose", (False, True))
@pytest.mark.parametrize("form,full_out", (("plain", False), ("free", False), ("free", True)))
def test_uncoupled_call_is_the_single_image_model(loose, form, full_out):
    lay, olay, imgs, flat, w = _case(loose, form, full_out)
    for area in rb.AREAS:
        for n in (0, 2):
            if form == "plain":
                refs = np.stack([rltv_model(d, PSF, M, N, n, LAM, EPS, area) for d in imgs])
            else:
                refs = np.stack([rltv_free_model(d, PSF, M, N, n, LAM, EPS, w, out_shape=(olay.rows, olay.cols), norm_area=area) for d in imgs])
            assert np.array_equal(refs, tb.references(form, imgs, PSF, M, N, n, LAM, EPS, area, w, out_shape=(olay.rows, olay.cols)))
            for group in (1, 2, 3, 5, 8):
                out = tb.batched_call(form, flat, lay, olay, PSF, M, N, n, LAM, EPS, area, group, weights=w)
                v = tb.judge("group %d" % group, out, olay, refs, refs, 0.0, area)
                assert not v.bad, v.bad[:3]


@pytest.mark.parametrize("form", ("plain", "free"))
def test_lambda_zero_is_the_batch_without_the_prior(form):
    lay, olay, imgs, flat, w = _case(True, form)
    for area in rb.AREAS:
        for group in (1, 2, 5):
            want = rb.batched_call(form, flat, lay, olay, PSF, M, N, 2, area, group, weights=w)
            for coupled in (False, True):
                got = tb.batched_call(form, flat, lay, olay, PSF, M, N, 2, 0.0, EPS, area, group, weights=w, coupled=coupled)
                assert np.array_equal(got, want), (form, area, group, coupled)


def test_coupled_factor_on_one_channel_is_the_single_factor():
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (3, 5), (65, 127)):
        u = rng.random(shape).astype(np.float32)
        w = rng.random(shape).astype(np.float32)
        for dtype in (np.float64, np.float32):
            for wv in (None, w):
                one = tb.tv_factor_coupled([u], 0.1, 1e-3, wv, dtype)[0]
                assert np.array_equal(one, tv_factor(u, 0.1, 1e-3, w=wv, dtype=dtype)), (shape, dtype)
    # and a coupled group of one image is the single-image model, in both forms
    lay, olay, imgs, flat, w = _case(False, "free")
    assert np.array_equal(tb.rltv_coupled_model(imgs[:1], PSF, M, N, 3, LAM, EPS)[0], rltv_model(imgs[0], PSF, M, N, 3, LAM, EPS))
    assert np.array_equal(tb.rltv_free_coupled_model(imgs[:1], PSF, M, N, 3, LAM, EPS, w)[0], rltv_free_model(imgs[0], PSF, M, N, 3, LAM, EPS, w))


def test_coupled_factor_properties():
    """the joint norm: flat channels give w exactly, a zero of w stays zero, g stays within its bound at the largest lambda, and a
    channel that is flat still feels the edges of the others"""
    rng = np.random.default_rng(9)
    us = rng.random((3, 70, 90)).astype(np.float32)
    w = rng.random((70, 90)).astype(np.float32)
    w[rng.random((70, 90)) < 0.2] = 0
    f = tb.tv_factor_coupled(us, 0.125, 1e-6, w)
    assert all(np.all(x[w == 0] == 0) for x in f)
    g = tb.tv_g_coupled(us, 0.125, 1e-6)
    assert min(float(x.min()) for x in g) >= 1 - 0.125 * (2 + np.sqrt(2)) - 1e-12
    flat = np.stack([np.full((70, 90), v, dtype=np.float32) for v in (0.2, 0.5, 0.9)])
    assert all(np.array_equal(x, w.astype(np.float64)) for x in tb.tv_factor_coupled(flat, 0.1, 1e-3, w))
    mixed = np.stack([us[0], flat[1]])
    assert np.array_equal(tb.tv_factor_coupled(mixed, 0.1, 1e-3)[1], np.ones((70, 90)))  # grad u_1 = 0: p_1 = 0 under any norm
    assert np.array_equal(tb.tv_factor_coupled(mixed, 0.1, 1e-3)[0], tv_factor(us[0], 0.1, 1e-3))  # u_0's norm is its own plus nothing ...
    both = np.stack([us[0], us[1]])
    assert not np.array_equal(tb.tv_factor_coupled(both, 0.1, 1e-3)[0], tv_factor(us[0], 0.1, 1e-3))  # ... and here it is not


# ---- (i) the judge flags each fault model ---------------------------------------------------------------------------------
def _flagged(form, fault, group, area=NORM_NONE, loose=True, n=2, coupled=False, count=COUNT):
    lay, olay, imgs, flat, w = _case(loose, form)
    if count != COUNT:
        lay = (bm.loose_layout if loose else bm.tight_layout)(ROWS, COLS, count)
        olay, imgs = lay, imgs[:count]
        flat = bm.pack_inputs(imgs.astype(np.float64), lay)
    refs = tb.references(form, imgs, PSF, M, N, n, LAM, EPS, area, w, coupled=coupled)
    out = tb.batched_call(form, flat, lay, olay, PSF, M, N, n, LAM, EPS, area, group, weights=w, coupled=coupled, fault=fault)
    return tb.judge(fault, out, olay, refs, refs, _tol(form), area)


@pytest.mark.parametrize("form", ("plain", "free"))
def test_judge_flags_image_0s_factor_for_every_image(form):
    """the one-plane second source of the weighted update, which the per-image pitch replaces"""
    v = _flagged(form, "factor_image0", 2)
    assert {"bits", "model"} <= v.checks
    assert not any("image 0:" in b or "image 2:" in b or "image 4:" in b for b in v.bad) and any("image 1:" in b for b in v.bad)
    assert not _flagged(form, "factor_image0", 1).bad  # groups of one cannot tell: the GPU test runs larger ones


@pytest.mark.parametrize("form", ("plain", "free"))
def test_judge_flags_the_previous_groups_factor(form):
    v = _flagged(form, "factor_previous_group", 2)
    assert {"bits", "model"} <= v.checks
    assert not any("image 0:" in b or "image 1:" in b for b in v.bad) and any("image 2:" in b for b in v.bad)  # the first group is right


@pytest.mark.parametrize("form", ("plain", "free"))
def test_judge_flags_a_factor_from_the_new_u(form):
    v = _flagged(form, "factor_new_u", 3)
    assert {"bits", "model"} <= v.checks and any("image 0:" in b for b in v.bad)
    assert not _flagged(form, "factor_new_u", 3, n=0).bad  # the start has no factor: the GPU test iterates


@pytest.mark.parametrize("form", ("plain", "free"))
@pytest.mark.parametrize("fault", ("channelwise_norm", "first_channel_norm", "sum_no_root"))
def test_judge_flags_a_wrong_joint_norm(form, fault):
    v = _flagged(form, fault, 3, coupled=True, count=3)
    assert {"bits", "model"} <= v.checks, (fault, v.bad[:2])
    assert len([b for b in v.bad if "float64 model" in b]) >= 2  # (no channel is right: channel 0's own norm is not the joint one either)


def test_judge_flags_a_halo_under_the_channels_own_norm():
    """only pixels on the first row or column of a 64 x 64 tile take p from the halo: the factor judged on a picture of several tiles"""
    rng = np.random.default_rng(2)
    us = rng.random((3, 65, 127)).astype(np.float32)
    want = tb.tv_factor_coupled(us, 0.1, 1e-3)
    got = tb.tv_factor_coupled(us, 0.1, 1e-3, fault="halo_own_norm")
    for c in range(3):
        diff = np.abs(got[c] - want[c])
        assert float(diff.max()) > 100 * 9e-7  # far above RLTV_FACTOR_TOL
        inner = np.ones((65, 127), dtype=bool)
        inner[64, :] = False
        inner[:, 64] = False
        assert float(diff[inner].max()) == 0.0  # ... and only there: shapes within one tile cannot tell
    small = rng.random((3, 64, 64)).astype(np.float32)
    assert all(np.array_equal(a, b) for a, b in zip(tb.tv_factor_coupled(small, 0.1, 1e-3), tb.tv_factor_coupled(small, 0.1, 1e-3, fault="halo_own_norm")))


def test_judge_flags_an_ignored_out_pitch():
    v = _flagged("plain", "ignore_out_pitch", 3)
    assert "layout" in v.checks and "bits" in v.checks
    assert not _flagged("plain", "ignore_out_pitch", 3, loose=False).bad  # a tight layout cannot tell: the GPU test runs loose ones


def test_judge_flags_a_dropped_tail():
    for form in ("plain", "free"):
        v = _flagged(form, "drop_last_group", 2)  # 5 images: 2, 2, 1
        assert "bits" in v.checks and any("image 4:" in b for b in v.bad) and not any("image 3:" in b for b in v.bad)
    assert not _flagged("plain", "drop_last_group", 5).bad  # no tail, no fault


# ---- (iii) quality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("photons", sorted({k[0] for k in tb.QUALITY_MEASURED}))
def test_coupling_restores_no_worse(photons):
    """each form at its best lambda of the grid, at the iteration counts the model file records: the coupled form is not below the
    channel-wise one, gains at least half the recorded gain, and reproduces the recorded figures to 0.01 dB"""
    case = tb.colour_quality_case(photons)
    ns = sorted(n for p, n in tb.QUALITY_MEASURED if p == photons)
    best = {(c, n): (-np.inf, None) for c in (False, True) for n in ns}
    for coupled in (False, True):
        for lam in tb.QUALITY_GRID[photons]:
            got = tb.colour_quality_run(case, ns, lam, coupled)
            for n in ns:
                if got[n] > best[(coupled, n)][0]:
                    best[(coupled, n)] = (got[n], lam)
    for n in ns:
        (cw, lam_cw), (cp, lam_cp) = best[(False, n)], best[(True, n)]
        rec_cw, rec_cp = tb.QUALITY_MEASURED[(photons, n)]
        print("RLTVB\tquality\tphotons=%g n=%d\tchannel-wise %.3f dB (lambda %g)\tcoupled %.3f dB (lambda %g)\tgain %.3f dB" % (photons, n, cw, lam_cw, cp, lam_cp, cp - cw))
        assert abs(cw - rec_cw) <= 0.01 and abs(cp - rec_cp) <= 0.01, (photons, n, cw, cp)
        assert cp >= cw, (photons, n, cw, cp)
        assert cp - cw >= 0.5 * (rec_cp - rec_cw), (photons, n, cw, cp)
        assert lam_cp >= lam_cw  # the joint norm is larger: the optimum moves to a larger lambda
        # every optimum lies inside the grid, so it is an optimum and not the grid's edge
        assert tb.QUALITY_GRID[photons][0] < lam_cw and lam_cp < tb.QUALITY_GRID[photons][-1]


# ---- (iv) symbols, struct layout, constants and signatures ------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fdr.h")).read(), flags=re.S)


def _header_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_symbols_and_surface(fdr):
    """fails without the feature: the header, the signatures table, Plan and the module all gain the batched calls"""
    names = ("fdr_richardson_lucy_tv_batch_f32", "fdr_richardson_lucy_tv_batch_f32_dev", "fdr_rl_tv_factor_group_f32_dev")
    for name in names:
        assert name in fdr.EXPORTED_SYMBOLS, name
        restype, argtypes = fdr._SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(_header_args(name)), name
        assert callable(getattr(fdr.lib, name))
    assert len(_header_args(names[0])) + 1 == len(_header_args(names[1])) == 14
    # the arguments are those of the batch without the prior, with the new params struct
    for a, b in zip(_header_args("fdr_richardson_lucy_batch_f32_dev"), _header_args(names[1])):
        assert a == b or (a, b) == ("const fdr_rl_batch_params* params", "const fdr_rl_tv_batch_params* params"), (a, b)
    assert len(_header_args(names[2])) == 15
    for k, (argtypes, sizes) in enumerate(((fdr._SIGNATURES[names[0]][1], (2, 10)), (fdr._SIGNATURES[names[1]][1], (2, 10)), (fdr._SIGNATURES[names[2]][1], (2, 12)))):
        for i, t in enumerate(argtypes):
            assert (t is ctypes.c_size_t) == (i in sizes), (names[k], i)
    # the struct: fdr_rl_tv_params (pinned at 32 bytes, unchanged) plus `couple`
    body = re.search(r"typedef struct fdr_rl_tv_batch_params \{(.*?)\} fdr_rl_tv_batch_params;", _header(), re.S).group(1)
    fields = re.findall(r"\b(int|float)\s+(\w+)\s*;", body)
    assert [f[1] for f in fields] == [f[0] for f in fdr.RlTvBatchParams._fields_] == [f[0] for f in fdr.RlTvParams._fields_] + ["couple"]
    assert [ctypes.c_int if t == "int" else ctypes.c_float for t, _ in fields] == [f[1] for f in fdr.RlTvBatchParams._fields_]
    assert ctypes.sizeof(fdr.RlTvBatchParams) == 36 and ctypes.sizeof(fdr.RlTvParams) == 32
    assert fdr.RlTvBatchParams.couple.offset == 32
    assert (fdr.TV_COUPLE_NONE, fdr.TV_COUPLE_CHANNELS) == (0, 1) and "#define FDR_VERSION 300" in open(os.path.join(ROOT, "include", "fdr.h")).read()
    for method in ("richardson_lucy_tv_batch", "richardson_lucy_tv_batch_dev", "rl_tv_factor_group_dev"):
        assert callable(getattr(fdr.Plan, method, None)), method
    import inspect
    sig = inspect.signature(fdr.richardsonLucyTV_RGB)
    assert list(sig.parameters)[:8] == ["channels", "psf", "iterations", "lam", "eps", "free_boundary", "weights", "coupled"]
    assert sig.parameters["coupled"].default is False and sig.parameters["eps"].default == 0.0
    # the drop-in C++ surface and the CLI flag
    hpp = open(os.path.join(ROOT, "include", "fft", "fft.hpp")).read()
    assert len(re.findall(r"inline void richardsonLucyTV_RGB\([^{;]*bool coupled = false\) \{", hpp)) == 2  # both overloads, trailing
    assert "fdr_richardson_lucy_tv_batch_f32(" in hpp
    assert '"--rl-tv-color"' in open(os.path.join(ROOT, "tools", "cli", "gpu.cpp")).read()


# ---- (v) refusals that need no device -----------------------------------------------------------------------------------------
def test_refusals_need_no_device(fdr):
    """null pointers, a count outside its range, strides, the prior's numbers and `couple` are refused before any device work"""
    L = fdr.lib
    prm = fdr.RlTvBatchParams(1, 0, 0.01, 1e-3, 0, 0.01, 0, 0, 0)
    assert L.fdr_richardson_lucy_tv_batch_f32_dev(None, None, 0, 1, 8, 32, 32, None, 0, None, 0, 32, ctypes.byref(prm), None) == -1
    assert b"null" in L.fdr_last_error()
    assert L.fdr_richardson_lucy_tv_batch_f32(None, None, 0, 1, 8, 32, 32, None, 0, None, 0, 32, None) == -1
    u = np.zeros((3, 8, 32), dtype=np.float32)
    o = np.zeros((3, 8, 32), dtype=np.float32)

    def factor(up=u.ctypes.data, op=o.ctypes.data, count=3, rows=8, cols=32, stride=32, lam=0.01, eps=1e-3, couple=0, upitch=256, opitch=256, ostride=32, w=None):
        return L.fdr_rl_tv_factor_group_f32_dev(0, up, upitch, count, rows, cols, stride, w, lam, eps, couple, op, opitch, ostride, None)

    assert factor(up=None) == -1 and factor(op=None) == -1
    for count in (0, -1, 9):
        assert factor(count=count) == -1 and b"count" in L.fdr_last_error(), count
    assert factor(rows=0) == -1 and factor(cols=0) == -1 and factor(stride=31) == -1 and factor(ostride=31) == -1
    for lam in (-0.01, 0.1251, float("nan")):
        assert factor(lam=lam) == -1 and b"lambda" in L.fdr_last_error(), lam
    for eps in (-1e-3, float("nan"), float("inf")):
        assert factor(eps=eps) == -1 and b"eps" in L.fdr_last_error(), eps
    for couple in (-1, 2):
        assert factor(couple=couple) == -1 and b"couple" in L.fdr_last_error(), couple
    assert factor(opitch=255) == -1 and b"overlap each other" in L.fdr_last_error()
    assert factor(op=u.ctypes.data + 4 * 2 * 256) == -1 and b"overlap an input" in L.fdr_last_error()  # plane 0 of the output is plane 2 of the input
    assert factor(w=o.ctypes.data + 4 * 256) == -1 and b"overlap an input" in L.fdr_last_error()      # the weights are plane 1 of the output
