"""The host side of FDR_FLAG_MIXED_RADIX plans, checked without a GPU: tools/cli/mixed_plan_check (csrc/fdr_mixed_plan.hpp behind
its own main) checks every length's stage list, magic division, twiddle indices and thread count and every (M, N) pair's
panel width and row batch; its --dump is interpreted here in float64 exactly as mx_stage of csrc/fdr_mixed.hip does it
(_mixed_model.stage_model) and compared with np.fft.fft at all 167 lengths.  The checks are pinned by faults injected into a
copy of the dump, the per-line metric of the GPU sweep by one wrong line in an otherwise exact plane, and the GPU sweep's
shape list by what it must reach: every length in both roles and all 15 (logP, B) layouts."""
import copy
import subprocess

import numpy as np
import pytest

import _mixed_model as mm

# stage_model runs in float64 with the float32 tables of the dump: every twiddle is a product of two entries each within
# 2^-24 of the exact value, one twiddle per stage and element, at most 8 stages (3^8 = 6561): 8 * 2 * 2^-24 = 9.5e-7 bounds the
# relative L2 error (measured: 7.8e-8 at L = 2048)
MODEL_TOL = 1e-6


def _x(L):
    rng = np.random.default_rng(L)
    return rng.standard_normal(L) + 1j * rng.standard_normal(L)


def violations(e):
    """What mixed_plan_check checks per length, on one parsed dump entry, and the float64 interpretation against np.fft.fft:
    a list of messages (empty: the entry is sound)."""
    L, bad = e["L"], []
    if e["nt"] % 64 or not 64 <= e["nt"] <= 1024:
        bad.append("nt")
    if len(e["lo"]) != 64 or len(e["hi"]) != (L + 63) // 64 or len(e["stages"]) != e["nst"]:
        bad.append("table sizes")
    ns = 1
    for i, (R, s_ns, magic, step) in enumerate(e["stages"]):
        if R not in (2, 3, 4, 5):
            return bad + ["stage %d: radix" % i]
        if s_ns != ns:
            bad.append("stage %d: ns %d, earlier radices multiply to %d" % (i, s_ns, ns))
        if L % (s_ns * R) or step != L // (s_ns * R):
            bad.append("stage %d: twiddle step" % i)
        j = np.arange(L // R, dtype=np.int64)
        if (magic == 0) != (s_ns == 1) or (magic and not np.array_equal((j * magic) >> 32, j // s_ns)):
            bad.append("stage %d: magic division" % i)
        if (R - 1) * (s_ns - 1) * step >= L:
            bad.append("stage %d: twiddle index reaches %d" % (i, (R - 1) * (s_ns - 1) * step))
        if e["nt"] * -(-16 // R) < L // R:
            bad.append("stage %d: more butterflies than nt threads hold" % i)
        ns *= R
    if ns != L:
        bad.append("radices multiply to %d" % ns)
    x = _x(L)
    try:
        got = mm.stage_model(e, x)
    except IndexError as err:
        return bad + ["model: %s" % err]
    want = np.fft.fft(x)
    err = np.linalg.norm(got - want) / np.linalg.norm(want) if np.all(np.isfinite(got)) else float("nan")
    if not err <= MODEL_TOL:
        bad.append("model: relative error %.3g against np.fft.fft" % err)
    return bad


@pytest.fixture(scope="module")
def dump():
    return mm.plan_dump(())[0]


def test_mixed_plan_check_passes():
    r = subprocess.run([mm.plan_check_exe()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mixed plan ok: 167 lengths, 27693 pairs, 15 (logP, B) layouts" in r.stdout, (r.returncode, r.stdout[-800:], r.stderr[-800:])
    r = subprocess.run([mm.plan_check_exe(), "--dump", "64x64"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, "a power-of-two pair is no mixed plan"


def test_every_dumped_length_transforms_as_numpy(dump):
    assert sorted(dump) == mm.smooth_lengths() and len(dump) == 167
    bad = ["L=%d: %s" % (L, "; ".join(v)) for L in sorted(dump) for v in [violations(dump[L])] if v]
    assert not bad, "\n".join(bad)
    # the radix order the kernels were tuned with: 4s, then 2, 3s, 5s
    for L, e in dump.items():
        order = [s[0] for s in e["stages"]]
        assert order == sorted(order, key=(4, 2, 3, 5).index) and order.count(2) <= 1, (L, order)


def _faults(e):
    """(name, faulted copy) of one entry with at least three stages, a 3 before a 5, two distinct used hi entries, and a radix
    4 or 2 stage (there nt >= L / 16 is tight: the smallest multiple of 64 has no wave to spare)"""
    out = []
    f = copy.deepcopy(e)
    R, ns, magic, step = f["stages"][1]
    f["stages"][1] = (R, ns, magic, step + 1)
    out.append(("twiddle step off by one", f))
    f = copy.deepcopy(e)
    R, ns, magic, step = f["stages"][1]
    f["stages"][1] = (R, ns, magic - 1, step)
    out.append(("magic one below", f))
    f = copy.deepcopy(e)
    f["hi"][[1, 2]] = f["hi"][[2, 1]]
    out.append(("hi entries 1 and 2 swapped", f))
    f = copy.deepcopy(e)
    i3 = max(i for i, s in enumerate(f["stages"]) if s[0] == 3)
    a, b = f["stages"][i3], f["stages"][i3 + 1]
    assert a[0] == 3 and b[0] == 5
    f["stages"][i3], f["stages"][i3 + 1] = (5,) + a[1:], (3,) + b[1:]
    out.append(("radix 5 before 3 with ns unchanged", f))
    f = copy.deepcopy(e)
    f["nt"] -= 64
    out.append(("one wave fewer than nt", f))
    return out


@pytest.mark.parametrize("L", [360, 2700, 4320, 6750, 8100])
def test_injected_faults_fail_the_checks(dump, L):
    assert not violations(dump[L])
    for name, f in _faults(dump[L]):
        assert violations(f), (L, name)


def test_faults_show_in_the_transform_alone(dump):
    """The float64 interpretation by itself (no structural check) rejects each table fault: it is the model the GPU sweep's
    reference stands for."""
    e = dump[2700]
    x, want = _x(2700), np.fft.fft(_x(2700))
    for name, f in _faults(e)[:4]:
        try:
            got = mm.stage_model(f, x)
            err = np.linalg.norm(got - want) / np.linalg.norm(want) if np.all(np.isfinite(got)) else float("nan")
        except IndexError:
            err = float("nan")
        assert not err <= 1e-5, (name, err)  # even the whole-plane bound of the GPU tests


def test_per_line_metric_sees_one_wrong_line():
    """One row, or one column, off by 1e-4 of its own norm in an otherwise exact 1000 x 1500 plane: the whole-plane relative
    norm (3e-6) passes the 1e-5 the GPU tests had; the per-line metric fails it."""
    rng = np.random.default_rng(1)
    want = rng.standard_normal((1000, 1500)) + 1j * rng.standard_normal((1000, 1500))
    line, peak, _ = mm.line_errors(want.astype(np.complex64), want)
    assert line <= 1e-7 and peak <= 1e-6  # complex64 rounding alone
    assert mm.LINE_TOL <= 1e-5 and mm.PEAK_TOL <= 1e-5
    for axis, idx in ((0, 337), (1, 1499)):
        got = want.copy()
        sl = (idx, slice(None)) if axis == 0 else (slice(None), idx)
        noise = rng.standard_normal(want[sl].shape) + 1j * rng.standard_normal(want[sl].shape)
        got[sl] += 1e-4 * noise * np.linalg.norm(want[sl]) / np.linalg.norm(noise)
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-5
        line, peak, where = mm.line_errors(got, want)
        assert not line <= mm.LINE_TOL and where == ("row 337" if axis == 0 else "column 1499"), (line, where)
    got = want.copy()
    got[5, 7] = np.nan
    assert not mm.line_errors(got, want)[0] <= mm.LINE_TOL
    got = want.copy()
    got[5, 7] += 1e-3  # one element: 1e-3 / sqrt(2) of rms
    assert not mm.line_errors(got, want)[1] <= mm.PEAK_TOL


def test_sweep_reaches_every_length_and_layout():
    cases = mm.sweep_cases()
    S = set(mm.smooth_lengths())
    assert len(S) == 167 and len(mm.sweep_plans()) == 668
    assert {c["L"] for c in cases if c["role"] == "row"} == S
    assert {c["L"] for c in cases if c["role"] == "col"} == S
    assert {(c["logP"], c["B"]) for c in cases} == {(lp, B) for lp in (0, 1, 2) for B in (1, 2, 4, 8, 16)}
    # each column length on every panel width its limits allow
    for L in S:
        want = {2, 1, 0} if L <= 2496 else {1, 0} if L <= 4992 else {0}
        assert {c["logP"] for c in cases if c["role"] == "col" and c["L"] == L} == want, L
    assert not any(mm.smooth(c["M"]) is False or (c["M"] & (c["M"] - 1) == 0 and c["N"] & (c["N"] - 1) == 0) for c in cases)
    assert sorted(L for b in mm.bands() for L in b) == sorted(S) and all(mm.bands())


def test_window_and_cls_plans_reach_every_batch_and_panel_width():
    _, lay = mm.plan_dump(tuple(mm.WINDOW_PLANS + mm.CLS_PLANS))
    assert {lay[p][1] for p in mm.WINDOW_PLANS} == {1, 2, 4, 8, 16}
    assert {lay[p][0] for p in mm.WINDOW_PLANS} == {0, 1, 2}
    assert [lay[p][0] for p in mm.CLS_PLANS] == [0, 0, 1, 1, 2, 2, 1, 0]
    assert {M % 2 for M, _ in mm.CLS_PLANS} == {0, 1}
