"""Registering the frames of a burst on the MI355X (fdr_register_frames_f32*, fdr_psf_shift_f32*) against the
float64 model of tests/_register_model.py, which tests/test_register_host.py pins on the CPU first.

Per case of GPU_CASES (the smallest shapes at which the kernels can still go wrong): the correlation plane r of every frame within
PLANE_TOL of the model's (max-abs; each figure is printed before it is asserted), the whole-pixel peak exactly the model's (the host
test holds the model's peak PEAK_MARGIN x PLANE_TOL above everything else), dy and dx within shift_bound of the model's, peak within
PLANE_TOL, the host form with the bits of the _dev form.  Then psf_shift against its float32 model bit for bit, repeatability,
isolation, allocation, refusals and the register=True chain of the convenience calls."""
import ctypes

import numpy as np
import pytest

import _register_model as rm
from _frames_model import FRAMES_TOL, frames_model
from _rl_model import rel_err

pytestmark = pytest.mark.gpu

SHIFT_DTYPE = np.dtype([("dy", "<f8"), ("dx", "<f8"), ("peak", "<f4"), ("confidence", "<f4")])


def _need(fdr):
    assert hasattr(fdr.lib, "fdr_register_frames_f32_dev") and hasattr(fdr.lib, "fdr_psf_shift_f32_dev"), "the library has no frame registration"


def _pitched(planes, stride, pitch, fill=np.nan):
    """the planes in one float32 array, plane k at k * pitch with row stride `stride`; the gaps hold NaN: a kernel that reads one shows it"""
    h = np.full(len(planes) * pitch, fill, dtype=np.float32)
    for k, a in enumerate(planes):
        for r in range(a.shape[0]):
            h[k * pitch + r * stride:k * pitch + r * stride + a.shape[1]] = a[r]
    return h


def _plan(fdr, case):
    return fdr.Plan(case[1], case[2], fdr.MODE_FAST, flags=fdr.FLAG_MIXED_RADIX if case[5] else 0)


def _device_call(fdr, p, case, frames, psfs, corr=True):
    """the _dev form on pitched device arrays: (K results as a structured array, K x M x N planes or None)"""
    import torch
    _, M, N, rows, cols, _, ref, max_shift, _, shifts, _ = case
    K = len(frames)
    stride, pitch = cols + 3, (rows + 1) * (cols + 3) + 5
    d_in = torch.from_numpy(_pitched(frames, stride, pitch)).cuda()
    d_psf, pr, pc, pstride, ppitch = None, 0, 0, 0, 0
    if psfs is not None:
        pr, pc = psfs[0].shape
        pstride, ppitch = pc + 2, pr * (pc + 2) + 3
        d_psf = torch.from_numpy(_pitched(psfs, pstride, ppitch)).cuda()
    d_sh = torch.full((K * 24,), 0xA5, dtype=torch.uint8, device="cuda")
    d_corr = torch.full((K, M, N), float("nan"), dtype=torch.float32, device="cuda") if corr else None
    p.register_frames_dev(d_in.data_ptr(), pitch, K, rows, cols, stride, d_sh.data_ptr(), d_psfs=d_psf.data_ptr() if psfs is not None else None,
                          psf_pitch=ppitch, prows=pr, pcols=pc, pstride=pstride, reference=ref, max_shift=max_shift,
                          d_corr=d_corr.data_ptr() if corr else None)
    torch.cuda.synchronize()
    return d_sh.cpu().numpy().view(SHIFT_DTYPE).copy(), (d_corr.cpu().numpy() if corr else None)


@pytest.fixture(scope="module")
def models():
    """per case: frames, psfs, the model's results and planes -- computed once"""
    out = {}
    for case in rm.GPU_CASES:
        frames, psfs = rm.gpu_case(case)
        est, planes = rm.register_model(frames, psfs, case[1], case[2], reference=case[6], max_shift=case[7], planes=True)
        out[case[0]] = (frames, psfs, est, planes)
    return out


@pytest.mark.parametrize("case", rm.GPU_CASES, ids=rm.GPU_IDS)
def test_against_model(fdr, models, case):
    _need(fdr)
    name, M, N = case[:3]
    ref = case[6]
    frames, psfs, est, planes = models[name]
    with _plan(fdr, case) as p:
        got, corr = _device_call(fdr, p, case, frames, psfs)
        host = p.register_frames(frames, psfs, ref, case[7])
    worst = 0.0
    for k in range(len(frames)):
        dev = float(np.max(np.abs(corr[k].astype(np.float64) - planes[k])))
        worst = max(worst, dev)
        print("REGISTER %s frame %d: plane max-abs %.3e (tol %.1e), peak %.6f, got (%.6f, %.6f) model (%.6f, %.6f)"
              % (name, k, dev, rm.PLANE_TOL, got[k]["peak"], got[k]["dy"], got[k]["dx"], est[k]["dy"], est[k]["dx"]))
    print("REGISTER %s: worst plane deviation %.3e" % (name, worst))
    for k in range(len(frames)):
        g, e = got[k], est[k]
        assert np.all(np.isfinite(corr[k])), "frame %d: the plane is not finite (a gap of the pitched input was read)" % k
        assert np.max(np.abs(corr[k].astype(np.float64) - planes[k])) <= rm.PLANE_TOL, "frame %d: correlation plane" % k
        if k == ref:
            assert (g["dy"], g["dx"], g["peak"], g["confidence"]) == (0.0, 0.0, 1.0, 0.0) and not np.any(corr[k])
            continue
        # the whole-pixel peak: dy = i* + off with |off| <= 0.5, so it is read back from the plane the device wrote
        Rr, Rc = case[7] if isinstance(case[7], tuple) else (case[7] or rm.default_range(case[3], case[4]),) * 2
        dev_pick = rm.pick(corr[k].astype(np.float64), Rr, Rc)
        assert (dev_pick["iy"], dev_pick["ix"]) == (e["iy"], e["ix"]), "frame %d: whole-pixel peak" % k
        assert abs(g["peak"] - e["peak"]) <= rm.PLANE_TOL
        assert abs(g["dy"] - e["dy"]) <= rm.shift_bound(e["denom"][0]) and abs(g["dx"] - e["dx"]) <= rm.shift_bound(e["denom"][1]), \
            "frame %d: (%r, %r) against the model's (%r, %r)" % (k, g["dy"], g["dx"], e["dy"], e["dx"])
        # the device's own pick from its own plane, in double: the same numbers
        assert abs(g["dy"] - dev_pick["dy"]) <= 1e-12 and abs(g["dx"] - dev_pick["dx"]) <= 1e-12 and g["peak"] == np.float32(dev_pick["peak"])
        assert abs(g["confidence"] - dev_pick["confidence"]) <= 1e-4 * abs(dev_pick["confidence"])
    # the host form: the bits of the _dev form
    for k, h in enumerate(host):
        assert (h.dy, h.dx, np.float32(h.peak), np.float32(h.confidence)) == (got[k]["dy"], got[k]["dx"], got[k]["peak"], got[k]["confidence"]), k


def test_zero_frames_give_zeros(fdr):
    _need(fdr)
    case = rm.GPU_CASES[0]
    frames, psfs = rm.gpu_case(case)
    with _plan(fdr, case) as p:
        frames[2] = np.zeros_like(frames[2])
        got = p.register_frames(frames, psfs)
        assert tuple(got[2]) == (0.0, 0.0, 0.0, 0.0) and got[1].peak > 0
        frames[0] = np.zeros_like(frames[0])  # an all-zero reference: every other frame gets zeros
        got = p.register_frames(frames, psfs)
        assert tuple(got[0]) == (0.0, 0.0, 1.0, 0.0) and all(tuple(g) == (0.0, 0.0, 0.0, 0.0) for g in got[1:])


def test_a_wider_search_range_around_the_same_peak_changes_nothing(fdr):
    """the argmax runs over the search window alone (the sums over the whole plane): where the peak of a wide range lies inside a
    narrow one, both give the same result.  (An exact tie cannot be made through two float transforms; the tie-break is held by the
    model's tie_high fault in the host test and by the kernel's comparison, which orders candidates by (value, window index).)"""
    _need(fdr)
    case = rm.GPU_CASES[0]
    frames, psfs = rm.gpu_case(case)
    with _plan(fdr, case) as p:
        a = p.register_frames(frames, psfs, 0, (4, 4))
        b = p.register_frames(frames, psfs, 0, (9, 7))
    e = rm.register_model(frames, psfs, 32, 32, max_shift=(9, 7))
    inside = [k for k in (1, 2, 3) if abs(e[k]["iy"]) <= 4 and abs(e[k]["ix"]) <= 4]
    assert inside, "the case has no peak inside the narrow range"
    for k in inside:
        assert (a[k].dy, a[k].dx, a[k].peak) == (b[k].dy, b[k].dx, b[k].peak), k


@pytest.mark.parametrize("case", [rm.GPU_CASES[1], rm.GPU_CASES[5]], ids=[rm.GPU_IDS[1], rm.GPU_IDS[5]])
def test_two_calls_give_the_same_bytes(fdr, models, case):
    _need(fdr)
    frames, psfs = models[case[0]][:2]
    with _plan(fdr, case) as p:
        a, ca = _device_call(fdr, p, case, frames, psfs)
        b, cb = _device_call(fdr, p, case, frames, psfs)
        assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
        c, _ = _device_call(fdr, p, case, frames, psfs, corr=False)  # without the debug output: the same results
        assert a.tobytes() == c.tobytes()
    with _plan(fdr, case) as q:  # and on a fresh plan
        d, _ = _device_call(fdr, q, case, frames, psfs, corr=False)
        assert a.tobytes() == d.tobytes()


# ---- psf_shift ----------------------------------------------------------------------------------------------------------------------------
def _shift_dev(fdr, psfs, shifts_bytes, pad_r, pad_c, d_shifts=None):
    """fdr_psf_shift_f32_dev on pitched arrays: the K output planes (the gaps of the output must keep their sentinel)"""
    import torch
    K = len(psfs)
    pr, pc = psfs[0].shape
    pstride, ppitch = pc + 1, pr * (pc + 1) + 7
    orows, ocols = pr + 2 * pad_r, pc + 2 * pad_c
    ostride, opitch = ocols + 3, orows * (ocols + 3) + 5
    d_psf = torch.from_numpy(_pitched(psfs, pstride, ppitch)).cuda()
    if d_shifts is None:
        d_shifts = torch.from_numpy(np.frombuffer(shifts_bytes, dtype=np.uint8).copy()).cuda()
    d_out = torch.full((K * opitch,), -7.0, dtype=torch.float32, device="cuda")
    fdr.psf_shift_dev(d_psf.data_ptr(), ppitch, K, pr, pc, pstride, d_shifts.data_ptr(), pad_r, pad_c, d_out.data_ptr(), opitch, ostride)
    torch.cuda.synchronize()
    flat = d_out.cpu().numpy()
    out = np.stack([flat[k * opitch:k * opitch + orows * ostride].reshape(orows, ostride)[:, :ocols] for k in range(K)])
    mask = np.ones(flat.shape, dtype=bool)
    for k in range(K):
        for r in range(orows):
            mask[k * opitch + r * ostride:k * opitch + r * ostride + ocols] = False
    assert np.all(flat[mask] == -7.0), "psf_shift wrote outside its output windows"
    return out


def _shift_bytes(shifts):
    a = np.zeros(len(shifts), dtype=SHIFT_DTYPE)
    for k, s in enumerate(shifts):
        a[k]["dy"], a[k]["dx"] = s
    return a.tobytes()


@pytest.mark.parametrize("pr,pc,pad_r,pad_c", [(5, 5, 3, 4), (1, 1, 1, 1), (15, 9, 52, 52), (7, 300, 2, 6)])
def test_psf_shift_is_the_float32_model_bit_for_bit(fdr, pr, pc, pad_r, pad_c):
    _need(fdr)
    rng = np.random.default_rng(pr * 1000 + pc)
    shifts = [(0.0, 0.0), (1.0, -2.0), (0.5, 0.5), (-0.25, 2.75), (-pad_r, pad_c - 1), (pad_r - 1, -pad_c), (1e9, -1e9), (float("nan"), 0.3)]
    shifts = [(max(min(a, 1e9), -1e9), b) for a, b in shifts]
    psfs = [rng.uniform(0.0, 1.0, (pr, pc)).astype(np.float32) for _ in shifts]
    want = rm.psf_shift_model(psfs, shifts, pad_r, pad_c, dtype=np.float32)
    got = _shift_dev(fdr, psfs, _shift_bytes(shifts), pad_r, pad_c)
    assert got.tobytes() == want.tobytes()
    host = fdr.psf_shift(psfs, shifts, pad_r, pad_c)
    assert host.tobytes() == want.tobytes()
    # out of range and NaN: the clamped shift's planes, and every sum kept to float32 round-off
    assert np.array_equal(got[6], rm.psf_shift_model(psfs[6:7], [(pad_r - 1, -pad_c)], pad_r, pad_c, dtype=np.float32)[0])
    assert np.array_equal(got[7], rm.psf_shift_model(psfs[7:8], [(0.0, 0.3)], pad_r, pad_c, dtype=np.float32)[0])
    for k in range(len(shifts)):
        assert abs(float(got[k].sum(dtype=np.float64)) / float(psfs[k].sum(dtype=np.float64)) - 1) < 1e-6 and got[k].min() >= 0


def test_psf_shift_reads_the_estimate_from_device_memory(fdr, models):
    """the chain estimate -> psf_shift on the device, no host in between: the float32 model fed with the estimate's own results"""
    _need(fdr)
    import torch
    case = rm.GPU_CASES[0]
    frames, psfs = models[case[0]][:2]
    K, (rows, cols) = len(frames), frames[0].shape
    d_in = torch.from_numpy(np.stack(frames)).cuda()
    d_psf = torch.from_numpy(np.stack(psfs)).cuda()
    d_sh = torch.zeros(K * 24, dtype=torch.uint8, device="cuda")
    with _plan(fdr, case) as p:
        p.register_frames_dev(d_in.data_ptr(), rows * cols, K, rows, cols, cols, d_sh.data_ptr(), d_psfs=d_psf.data_ptr(), psf_pitch=25, prows=5,
                              pcols=5, pstride=5)
        got = _shift_dev(fdr, psfs, None, 6, 6, d_shifts=d_sh)
    est = d_sh.cpu().numpy().view(SHIFT_DTYPE)
    want = rm.psf_shift_model(psfs, [(e["dy"], e["dx"]) for e in est], 6, 6, dtype=np.float32)
    assert got.tobytes() == want.tobytes()
    assert any(e["dy"] != np.round(e["dy"]) for e in est), "the case has no sub-pixel estimate"


# ---- the plan around the calls -------------------------------------------------------------------------------------------------------------
def test_isolation(fdr):
    """the Wiener filter, the operator tables, the frame tables and the cepstrum / motion estimate give the same bits before and after
    registrations, which in turn keep theirs"""
    _need(fdr)
    from _spectral import tone_image
    M, N, rows, cols = 64, 64, 48, 40
    img = tone_image(M, N, 21, rows, cols)
    case = ("iso", M, N, rows, cols, False, 0, 0, True, [(0, 0), (2, -3), (-4.5, 1)], 12)
    frames, psfs = rm.gpu_case(case)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_psf_motion(7, 30.0, 0.01)
        p.set_operator_psf_motion(9, 100.0)
        p.set_frame_psfs(psfs)

        def others():
            return [p.wiener(img), p.blur(img), p.richardson_lucy_frames(frames, 3), p.cepstrum(img), np.asarray(p.estimate_motion(img, max_length=10))]

        before = others()
        a = p.register_frames(frames, psfs)
        after = others()
        for k, (x, y) in enumerate(zip(before, after)):
            assert np.array_equal(x, y), "result %d changed after a registration" % k
        assert p.register_frames(frames, psfs) == a and p.register_frames(frames, None) != a
        assert p.frame_count() == 3


def test_later_calls_allocate_nothing(fdr, models):
    _need(fdr)
    import torch
    case = rm.GPU_CASES[3]
    frames, psfs = models[case[0]][:2]
    with _plan(fdr, case) as p:
        _device_call(fdr, p, case, frames, psfs)  # the first call makes the blocks (and this helper's tensors warm torch's allocator)
        K, (rows, cols) = len(frames), frames[0].shape
        d_in = torch.from_numpy(np.stack(frames)).cuda()
        d_psf = torch.from_numpy(np.stack(psfs)).cuda()
        d_sh = torch.zeros(K * 24, dtype=torch.uint8, device="cuda")
        d_corr = torch.zeros((K, case[1], case[2]), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for with_psfs, corr in ((True, True), (False, False), (True, False), (False, True)):
            p.register_frames_dev(d_in.data_ptr(), rows * cols, K, rows, cols, cols, d_sh.data_ptr(), d_psfs=d_psf.data_ptr() if with_psfs else None,
                                  psf_pitch=25, prows=5, pcols=5, pstride=5, d_corr=d_corr.data_ptr() if corr else None)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0, "a later call allocated device memory"


def _prm(fdr, ref=0, mr=0, mc=0, eps=0.0):
    return fdr.RegisterParams(ref, mr, mc, eps, None)


def test_refusals(fdr):
    """every refusal, host and _dev form alike, before any pass, and a plan that still works afterwards"""
    _need(fdr)
    L = fdr.lib
    imgs = np.random.default_rng(0).uniform(0, 1, (2, 64, 64)).astype(np.float32)
    psf = np.ones((2, 5, 5), dtype=np.float32) / 25
    out = (fdr.FrameShiftC * 8)()

    def call(p, pitch=4096, count=2, rows=32, cols=32, stride=64, pp=psf.ctypes.data, ppitch=25, pr=5, pc=5, ps=5, prm=None, dev=False, sh=None):
        f = L.fdr_register_frames_f32_dev if dev else L.fdr_register_frames_f32
        args = [p._h, imgs.ctypes.data, pitch, count, rows, cols, stride, pp, ppitch, pr, pc, ps, ctypes.byref(_prm(fdr) if prm is None else prm),
                ctypes.cast(out, ctypes.c_void_p) if sh is None else sh]
        return f(*args, None) if dev else f(*args)

    def both(p, **kw):
        """the code both forms give (every refusal comes before a pointer is followed, so the _dev form may see host pointers here)"""
        a, b = call(p, **kw), call(p, dev=True, **kw)
        assert a == b, (a, b, kw)
        return a

    for M, N, mode, flags, what in ((64, 64, fdr.MODE_PARITY, 0, "parity"), (64, 16, fdr.MODE_FAST, 0, "N < 32"),
                                    (360, 640, fdr.MODE_FAST, fdr.FLAG_ANY_SIZE, "any size fast")):
        with fdr.Plan(M, N, mode, flags=flags) as p:
            assert both(p, rows=16, cols=16) == -1 and b"needs a FDR_MODE_FAST plan" in L.fdr_last_error(), what
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert both(p) == -4
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        p.profile(True)
        for kw, msg in ((dict(rows=15), b"at least 16 x 16"), (dict(cols=15), b"at least 16 x 16"), (dict(rows=65), b"fit the plan"),
                        (dict(cols=65, stride=65), b"fit the plan"), (dict(stride=31), b"strides >= cols"), (dict(count=0), b"count must be"),
                        (dict(count=9), b"count must be"), (dict(pitch=31 * 64 + 31), b"img_pitch"), (dict(prm=_prm(fdr, ref=2)), b"reference"),
                        (dict(prm=_prm(fdr, ref=-1)), b"reference"), (dict(prm=_prm(fdr, mr=-1)), b"negative max_shift"),
                        (dict(prm=_prm(fdr, mr=32)), b"max_shift_rows"), (dict(prm=_prm(fdr, mc=32)), b"max_shift_cols"),
                        (dict(prm=_prm(fdr, eps=-1e-3)), b"eps_rel"), (dict(prm=_prm(fdr, eps=float("nan"))), b"eps_rel"),
                        (dict(prm=_prm(fdr, eps=float("inf"))), b"eps_rel"), (dict(pr=0), b"PSFs must be"), (dict(pr=65), b"PSFs must be"),
                        (dict(pc=65, ps=65), b"PSFs must be"), (dict(ps=4), b"PSFs must be"), (dict(ppitch=24), b"psf_pitch")):
            assert both(p, **kw) == -1 and msg in L.fdr_last_error(), (kw, L.fdr_last_error())
        assert call(p, dev=True, sh=ctypes.c_void_p(ctypes.addressof(out) + 4)) == -1 and b"8-byte aligned" in L.fdr_last_error()
        assert sum(c for _, _, c in p.pass_times()) == 0, "a refused call launched a pass"
        assert call(p) == 0 and call(p, pp=None) == 0 and call(p, prm=_prm(fdr, mr=31, mc=31)) == 0  # the plan still works
        assert call(p, count=1, pitch=0, ppitch=0) == 0 and (out[0].dy, out[0].dx, out[0].peak, out[0].confidence) == (0.0, 0.0, 1.0, 0.0)
        names = {n for n, _, c in p.pass_times() if c}
        assert {"register window", "register transforms", "register cross-power", "register peak"} <= names, names


# ---- the chain in the convenience calls ----------------------------------------------------------------------------------------------------
E2E_N = 10  # a reduced iteration count: the chain is judged against the model chain, not for its quality


def test_register_true_is_the_model_chain_and_false_the_old_call(fdr):
    """richardsonLucyFrames_myfft and tvDeblurFrames_myfft with register=True on the quality case: the estimate, the shifted PSFs and the
    restoration lie within FRAMES_TOL-class distance of the model chain (register_model -> psf_shift_model -> the frames model on the same
    plan); register=False is bit for bit the call on the plan it documents"""
    _need(fdr)
    from _tvframes_model import TVFR_TOL, tvframes_model
    c = rm.quality_case()
    ds, psfs = c["ds"], c["psfs"]
    rows, cols = ds[0].shape
    pad = rm.QUALITY_PAD
    M, N = fdr._frames_plan_size(rows, cols, np.stack(psfs), pad)
    assert (M, N) == (512, 512)
    est = rm.register_model(ds, psfs, M, N)
    shifts = [(e["dy"], e["dx"]) for e in est]
    planes = list(np.roll(np.pad(rm.psf_shift_model(psfs, shifts, pad, pad), ((0, 0), (0, M - 15 - 2 * pad), (0, N - 15 - 2 * pad))), (-pad, -pad), (1, 2)))
    got = fdr.richardsonLucyFrames_myfft(ds, psfs, E2E_N, tv_lambda=0.01, tv_eps=1e-3, register=True)
    want = frames_model(ds, planes, M, N, E2E_N, lam=0.01, eps=1e-3)
    err = rel_err(got, want)
    print("REGISTER e2e RL: rel err %.3e (FRAMES_TOL %.1e)" % (err, FRAMES_TOL))
    assert err <= FRAMES_TOL
    unreg = frames_model(ds, list(np.pad(np.stack(psfs), ((0, 0), (0, M - 15), (0, N - 15)))), M, N, E2E_N, lam=0.01, eps=1e-3)
    assert rel_err(got, unreg) > 100 * FRAMES_TOL, "the registration changed nothing"
    got = fdr.tvDeblurFrames_myfft(ds, psfs, 60.0, E2E_N, register=True)
    want = tvframes_model(ds, planes, M, N, 60.0, iterations=E2E_N)
    err = rel_err(got, want)
    print("REGISTER e2e TV: rel err %.3e (FRAMES_TOL %.1e; TVFR_TOL %.1e)" % (err, FRAMES_TOL, TVFR_TOL))
    assert err <= FRAMES_TOL
    # register=False: the old call, bit for bit
    with fdr.Plan(256, 256, fdr.MODE_FAST) as p:
        assert fdr._frames_plan_size(rows, cols, np.stack(psfs)) == (256, 256)
        p.set_frame_psfs(np.stack(psfs))
        p.set_batching(1, 3)
        assert np.array_equal(p.richardson_lucy_frames(ds, 3), fdr.richardsonLucyFrames_myfft(ds, psfs, 3))
        assert np.array_equal(p.richardson_lucy_frames(ds, 3), fdr.richardsonLucyFrames_myfft(ds, psfs, 3, register=False))
        assert np.array_equal(p.tv_deconv_frames(ds, 60.0, 3), fdr.tvDeblurFrames_myfft(ds, psfs, 60.0, 3, register=False))


def test_registerFrames_and_the_rgb_calls(fdr):
    """registerFrames on its documented plan is Plan.register_frames; the _RGB calls register once on the mean of the channels"""
    _need(fdr)
    case = rm.GPU_CASES[5]
    frames, psfs = rm.gpu_case(case)
    M, N = fdr._motion_plan_size(40, 61)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_MIXED_RADIX) as p:
        assert fdr.registerFrames(frames, psfs) == p.register_frames(frames, psfs)
        assert fdr.registerFrames([np.dstack([f, f]) for f in frames], psfs, reference=1) == p.register_frames(frames, psfs, 1)
    rgb = [[f, 0.5 * f] for f in frames]
    one = fdr.richardsonLucyFrames_myfft([0.75 * f for f in frames], psfs, 2, register=True, max_shift=6)
    got = fdr.richardsonLucyFrames_RGB(rgb, psfs, 2, register=True, max_shift=6)
    assert len(got) == 2 and got[0].shape == frames[0].shape
    # the shifts come from the mean of the channels (0.75 f), then each channel is the plain call with those PSFs
    assert np.allclose(got[0], one / 0.75, rtol=1e-4, atol=1e-5)
