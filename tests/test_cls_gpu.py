"""The constrained least-squares (CLS) filter (fdr_set_psf_cls*) on the MI355X: every fast-path filter site bin by bin against
the float64 model of tests/_cls_model.py, gamma = 0 against the Wiener calls, the three entry points against each other, batches,
batch-graph replays and filter transport against one-by-one calls, the refusals, and the CLI.

Full-plane tone images restored with NORM_PADDED, judged by _spectral.failures() on bin_error / max-abs at BIN_TOL /
SPATIAL_TOL (NaN and inf fail).  The case list (_cls_model.cases) is the one the CPU fault pins of test_cls_host.py run on.
Each case prints a `CLS` line with its measured values (pytest -s)."""
import ctypes
import os

import numpy as np
import pytest

from _cls_model import SHAPES, cases, cls_raw
from _spectral import BIN_TOL, SPATIAL_TOL, bin_error, failures, max_abs, normalize, tone_image, wiener_raw

pytestmark = pytest.mark.gpu


def _f32(x):
    return float(np.float32(x))


@pytest.mark.parametrize("M,N,flag", SHAPES)
def test_cls_bins_against_float64(fdr, oracle, M, N, flag):
    flags = getattr(fdr, flag) if flag else 0
    img = tone_image(M, N, M * 7919 + N)
    bad = []
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        for name, psf, K, gamma in cases(oracle, M, N):
            K32, g32 = _f32(K), _f32(gamma)
            p.set_psf(psf, K32, gamma=g32)
            got = p.wiener(img, fdr.NORM_PADDED)
            raw = cls_raw(img, psf, K32, g32, M, N)
            e, where = bin_error(got, raw)
            sp = max_abs(got, normalize(raw))
            what = "%dx%d %s %s K=%g gamma=%g" % (M, N, flag or "", name, K, gamma)
            with np.errstate(divide="ignore", invalid="ignore"):  # K = 0: the Wiener model may be singular (differs anyway)
                e_w, _ = bin_error(normalize(raw), wiener_raw(img, psf, K32, M, N))
            print("CLS\t%s\tbin=%.3g\tat=%s\tspatial=%.3g\tvs_wiener=%.3g" % (what, e, where, sp, e_w))
            bad += failures(what, M, N, e, where, sp, BIN_TOL, SPATIAL_TOL)
            if e_w <= 10 * BIN_TOL:
                bad.append("%s: the CLS model differs from the Wiener model by only %.3g" % (what, e_w))
    assert not bad, "\n".join(bad)


def _filter_bytes(fdr, p):
    import torch
    n = p.filter_bytes()
    d = torch.empty(n, dtype=torch.uint8, device="cuda")
    p.export_filter_dev(d.data_ptr(), n)
    torch.cuda.synchronize()
    return d.cpu().numpy()


ZERO_SHAPES = [(256, 256, 0), (64, 1024, "FLAG_FULL_SPECTRUM"), (512, 512, "FLAG_SIMPLE_PATH"), (75, 64, "FLAG_MIXED_RADIX")]


@pytest.mark.parametrize("M,N,flag", ZERO_SHAPES)
def test_gamma_zero_is_the_wiener_call(fdr, oracle, M, N, flag):
    """Each CLS entry point with gamma = 0 leaves the filter bytes and outputs of its fdr_set_psf* counterpart."""
    import torch
    L, f = fdr.lib, ctypes.c_float
    flags = getattr(fdr, flag) if flag else 0
    img = tone_image(M, N, 5)
    psf = fdr.motionBlurKernel(15, 30.0)
    d_psf = torch.from_numpy(psf).cuda()
    K = _f32(0.01)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        calls = {
            "host": (lambda: p.set_psf(psf, K),
                     lambda: L.fdr_set_psf_cls(p._h, psf.ctypes.data, 15, 15, 15, f(K), f(0.0))),
            "dev": (lambda: p.set_psf_dev(d_psf.data_ptr(), 15, 15, 15, K),
                    lambda: L.fdr_set_psf_cls_dev(p._h, ctypes.c_void_p(d_psf.data_ptr()), 15, 15, 15, f(K), f(0.0), None)),
            "motion": (lambda: p.set_psf_motion(15, 30.0, K),
                       lambda: L.fdr_set_psf_motion_cls(p._h, 15, 30.0, f(K), f(0.0), None)),
        }
        for what, (wiener, cls0) in calls.items():
            wiener()
            torch.cuda.synchronize()
            fw, ow = _filter_bytes(fdr, p), p.wiener(img)
            assert cls0() == 0, fdr.lib.fdr_last_error()
            torch.cuda.synchronize()
            fc, oc = _filter_bytes(fdr, p), p.wiener(img)
            assert np.array_equal(fw, fc), what
            assert np.array_equal(ow, oc), what


@pytest.mark.parametrize("M,N,flag", [(256, 512, 0), (64, 1024, "FLAG_FULL_SPECTRUM"), (4, 64, 0), (75, 64, "FLAG_MIXED_RADIX")])
def test_entry_points_agree(fdr, M, N, flag):
    """The host, device and motion CLS calls give identical filter bytes for the same PSF."""
    import torch
    flags = getattr(fdr, flag) if flag else 0
    size = min(15, M, N)
    psf = fdr.motionBlurKernel(size, 30.0)
    d_psf = torch.from_numpy(psf).cuda()
    K, g = _f32(0.01), _f32(0.05)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=flags) as p:
        p.set_psf(psf, K, gamma=g)
        a = _filter_bytes(fdr, p)
        p.set_psf_dev(d_psf.data_ptr(), size, size, size, K, gamma=g)
        b = _filter_bytes(fdr, p)
        p.set_psf_motion(size, 30.0, K, gamma=g)
        c = _filter_bytes(fdr, p)
        p.set_psf(psf, K)
        w = _filter_bytes(fdr, p)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert not np.array_equal(a, w)


def _one_by_one(p, d_in, d_out, count, M, N):
    import torch
    for i in range(count):
        p.wiener_dev(d_in[i].data_ptr(), M, N, N, d_out[i].data_ptr(), N, 1)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("M,N,flags", [(256, 256, 0), (128, 512, 0), (45, 75, "FLAG_MIXED_RADIX")])
def test_batches_graph_replay_and_transport(fdr, M, N, flags):
    import torch
    fl = getattr(fdr, flags) if flags else 0
    count = 8
    imgs = np.stack([tone_image(M, N, 100 + i) for i in range(count)])
    d_in = torch.from_numpy(imgs).cuda()
    K, g = _f32(0.01), _f32(0.05)
    psf = fdr.motionBlurKernel(15, 30.0)
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=fl) as p:
        p.set_psf(psf, K, gamma=g)
        want = _one_by_one(p, d_in, torch.empty_like(d_in), count, M, N)
        for ns, grp in ((1, 1), (2, 1), (2, 4), (4, 2)):
            p.set_batching(ns, grp)
            d_out = torch.full_like(d_in, -1.0)
            p.wiener_batch_dev(d_in.data_ptr(), M * N, count, M, N, N, d_out.data_ptr(), M * N, N, 1)
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), want), (ns, grp)
        # a captured batch graph, replayed after the filter is switched from Wiener to CLS (same call, same K)
        p.set_batching(2, 2)
        p.set_option(fdr.OPT_BATCH_GRAPH, 1)
        p.set_psf(psf, K)
        d_out = torch.full_like(d_in, -1.0)
        p.wiener_batch_dev(d_in.data_ptr(), M * N, count, M, N, N, d_out.data_ptr(), M * N, N, 1)
        torch.cuda.synchronize()
        wiener_out = d_out.cpu().numpy()
        p.set_psf(psf, K, gamma=g)
        p.wiener_batch_dev(d_in.data_ptr(), M * N, count, M, N, N, d_out.data_ptr(), M * N, N, 1)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want)
        assert not np.array_equal(wiener_out, want)
        p.set_option(fdr.OPT_BATCH_GRAPH, 0)
        # a CLS filter exported from this plan and imported into another
        n = p.filter_bytes()
        blk = torch.empty(n, dtype=torch.uint8, device="cuda")
        p.export_filter_dev(blk.data_ptr(), n)
        torch.cuda.synchronize()
    with fdr.Plan(M, N, fdr.MODE_FAST, flags=fl) as q:
        q.import_filter_dev(blk.data_ptr(), n, K)
        got = _one_by_one(q, d_in, torch.empty_like(d_in), count, M, N)
    assert np.array_equal(got, want)


def test_refusals(fdr):
    L, f = fdr.lib, ctypes.c_float
    img = tone_image(64, 64, 3)
    psf = fdr.motionBlurKernel(15, 30.0)
    for M, N, mode, flags in ((64, 64, fdr.MODE_PARITY, 0), (45, 75, fdr.MODE_FAST, fdr.FLAG_ANY_SIZE),
                              (45, 75, fdr.MODE_PARITY, fdr.FLAG_ANY_SIZE)):
        im = img[:M, :N] if M <= 64 and N <= 64 else tone_image(M, N, 4)
        with fdr.Plan(M, N, mode, flags=flags) as p:
            p.set_psf(psf, 0.01)
            before = p.wiener(im)
            assert L.fdr_set_psf_cls(p._h, psf.ctypes.data, 15, 15, 15, f(0.01), f(0.5)) == -1
            assert b"FDR_MODE_FAST" in L.fdr_last_error()
            assert L.fdr_set_psf_motion_cls(p._h, 15, 30.0, f(0.01), f(0.5), None) == -1
            assert np.array_equal(p.wiener(im), before), (M, N, mode, flags)
            assert L.fdr_set_psf_cls(p._h, psf.ctypes.data, 15, 15, 15, f(0.01), f(0.0)) == 0  # gamma = 0: the Wiener call
            assert np.array_equal(p.wiener(im), before)
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        for bad in (-0.5, float("nan"), float("inf")):
            assert L.fdr_set_psf_cls(p._h, psf.ctypes.data, 15, 15, 15, f(0.01), f(bad)) == -1
            assert L.fdr_set_psf_motion_cls(p._h, 15, 30.0, f(0.01), f(bad), None) == -1
        with pytest.raises(fdr.FdrError):
            p.set_psf(psf, 0.01, gamma=-1.0)
    with fdr.Plan(64, 64, fdr.MODE_FAST, flags=fdr.FLAG_TABLES_ONLY) as p:
        assert L.fdr_set_psf_cls(p._h, psf.ctypes.data, 15, 15, 15, f(0.01), f(0.5)) == -4
        assert L.fdr_set_psf_motion_cls(p._h, 15, 30.0, f(0.01), f(0.5), None) == -4
        assert L.fdr_set_psf_cls_dev(p._h, ctypes.c_void_p(16), 15, 15, 15, f(0.01), f(0.5), None) == -4


def test_cli_cls_planes_equal_python(fdr, tmp_path):
    """tools/cli/gpu --cls gamma --raw-out: the restored planes equal wienerDeblur_RGB_optimized(..., cls_gamma=gamma); with
    --mode parity it exits non-zero with the library's message."""
    import subprocess
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", "cli"), "-s", "gpu"])
    png = os.path.join(root, "tests", "golden", "cat_blurred.png")
    rgb = np.asarray(Image.open(png).convert("RGB"), dtype=np.float32) / 255.0
    h, w = rgb.shape[:2]
    out_raw = str(tmp_path / "cls.f32")
    gpu = os.path.join(root, "tools", "cli", "gpu")
    r = subprocess.run([gpu, png, "50", "30", "--cls", "0.05", "--raw-out", out_raw], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    planes = np.fromfile(out_raw, dtype=np.float32).reshape(3, h, w)
    chans = [np.ascontiguousarray(rgb[:, :, c]) for c in (2, 1, 0)]  # B, G, R
    fdr.wienerDeblur_RGB_optimized(chans, fdr.motionBlurKernel(50, 30.0), 0.01, mode=fdr.MODE_FAST, cls_gamma=0.05)
    for k in range(3):
        assert np.array_equal(planes[k], chans[k]), (k, float(np.abs(planes[k] - chans[k]).max()))
    wien = [np.ascontiguousarray(rgb[:, :, c]) for c in (2, 1, 0)]
    fdr.wienerDeblur_RGB_optimized(wien, fdr.motionBlurKernel(50, 30.0), 0.01, mode=fdr.MODE_FAST)
    assert not np.array_equal(planes[0], wien[0])
    r = subprocess.run([gpu, png, "50", "30", "--cls", "0.05", "--mode", "parity"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "FDR_MODE_FAST" in r.stdout + r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-500:])
