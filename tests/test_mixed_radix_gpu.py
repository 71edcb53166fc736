"""FDR_FLAG_MIXED_RADIX on the MI355X: fast-mode plans of size 2^a 3^b 5^c transformed by the mixed-radix kernels of
fdr_mixed.hip.  Checked against numpy (2-D transform), the naive-DFT CPU oracle (small operator sizes) and the float64
model of the optimal-size operator (tests/_mixed_model.py, user sizes), with the fast-mode tolerance of
test_gpu_parity.py; batches, filter export / import and plan state are compared bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from _mixed_model import LINE_TOL, PEAK_TOL, line_errors, optimal_size, wiener_model

pytestmark = pytest.mark.gpu

TOL = 1e-4
MIXED_PASSES = ("A mixed rows: pad+FFT (real pairs)", "B mixed cols: FFT*W*IFFT", "C mixed rows: IFFT+real+minmax",
                "E mixed normalize+crop")


def _errs(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()), float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _img(rows, cols, seed):
    return np.random.default_rng(seed).random((rows, cols), dtype=np.float32)


def _plan(fdr, M, N):
    return fdr.Plan(M, N, fdr.MODE_FAST, 0, flags=fdr.FLAG_MIXED_RADIX)


@pytest.mark.parametrize("shape", [(6, 10), (9, 25), (15, 27), (100, 36), (360, 270), (1000, 1500), (2187, 48), (3125, 40),
                                   (8100, 30), (30, 8000), (1024, 1000), (1000, 1024), (4320, 4320)])
def test_fft2d_against_numpy(fdr, shape):
    M, N = shape
    rng = np.random.default_rng(M * 7 + N)
    x = (rng.standard_normal((M, N)) + 1j * rng.standard_normal((M, N))).astype(np.complex64)
    with _plan(fdr, M, N) as p:
        fwd = p.fft2d(x)
        inv = p.fft2d(x, inverse=True)
        back = p.fft2d(fwd, inverse=True) / (M * N)
    x128 = x.astype(np.complex128)
    want = np.fft.fft2(x128)
    assert np.linalg.norm(fwd - want) / np.linalg.norm(want) <= 1e-5
    want_i = np.fft.ifft2(x128) * (M * N)
    assert np.linalg.norm(inv - want_i) / np.linalg.norm(want_i) <= 1e-5
    assert np.linalg.norm(back - x128) / np.linalg.norm(x128) <= 1e-5
    # ... and line by line: every single row and column of the forward and inverse transforms, and the largest error of the
    # plane (the thresholds of test_mixed_lengths_gpu.py)
    for name, got, ref in (("forward", fwd, want), ("inverse", inv, want_i)):
        line, peak, where = line_errors(got, ref)
        assert line <= LINE_TOL and peak <= PEAK_TOL, (name, line, where, peak)


@pytest.mark.parametrize("shape", [(30, 50), (45, 100), (97, 33), (6, 10), (200, 300), (250, 180)])
def test_operator_against_oracle(fdr, oracle, shape):
    rows, cols = shape
    img = _img(rows, cols, rows + cols)
    psf = oracle.motion_blur_kernel(5, 30.0)
    want = oracle.wiener(img, psf, 0.01)
    got = fdr.wienerDeblur_myfft_unpadded(img, psf, 0.01, mode=fdr.MODE_FAST, mixed_radix=True)
    mx, rel = _errs(got, want)
    assert mx <= TOL and rel <= TOL, (mx, rel)


def test_operator_constant_image(fdr, oracle):
    # 41 x 97 pads to 45 x 100: the zero border gives the restored plane its structure (an unpadded constant image would
    # restore to a constant, whose min-max normalisation only magnifies rounding)
    img = np.full((41, 97), 0.5, dtype=np.float32)
    psf = oracle.motion_blur_kernel(5, 30.0)
    want = oracle.wiener(img, psf, 0.01)
    got = fdr.wienerDeblur_myfft_unpadded(img, psf, 0.01, mode=fdr.MODE_FAST, mixed_radix=True)
    assert np.abs(got.astype(np.float64) - want).max() <= TOL


@pytest.mark.parametrize("size,angle", [(3, 0.0), (9, 45.0), (15, 30.0), (21, 120.0)])
def test_operator_motion_psfs(fdr, oracle, size, angle):
    img = _img(97, 120, size)
    psf = oracle.motion_blur_kernel(size, angle)
    want = oracle.wiener(img, psf, 0.01)
    with _plan(fdr, optimal_size(97), optimal_size(120)) as p:
        p.set_psf_motion(size, angle, 0.01)
        got = p.wiener(img, fdr.NORM_CROPPED)
    mx, rel = _errs(got, want)
    assert mx <= TOL and rel <= TOL, (mx, rel)


def test_operator_large_random_psf(fdr, oracle):
    img = _img(50, 70, 3)
    psf = np.random.default_rng(4).random((30, 40), dtype=np.float32) + 0.01  # larger than half the 50 x 72 plan
    want = oracle.wiener(img, psf, 0.01)
    got = fdr.wienerDeblur_myfft_unpadded(img, psf, 0.01, mode=fdr.MODE_FAST, mixed_radix=True)
    mx, rel = _errs(got, want)
    assert mx <= TOL and rel <= TOL, (mx, rel)


@pytest.mark.parametrize("shape", [(1000, 1500), (1080, 1920), (3000, 5000), (4100, 4100), (8000, 600), (600, 8100)])
def test_operator_against_model(fdr, oracle, shape):
    rows, cols = shape
    M, N = optimal_size(rows), optimal_size(cols)
    img = _img(rows, cols, rows ^ cols)
    psf = oracle.motion_blur_kernel(15, 30.0)
    with _plan(fdr, M, N) as p:
        p.set_psf(psf, 0.01)
        for norm in (fdr.NORM_CROPPED, fdr.NORM_PADDED):
            got = p.wiener(img, norm)
            want = wiener_model(img, psf, 0.01, M, N, norm_cropped=norm == fdr.NORM_CROPPED)
            mx, rel = _errs(got, want)
            assert mx <= TOL and rel <= TOL, (norm, mx, rel)


def test_operator_strides(fdr, oracle):
    import torch
    rows, cols, stride, ostride = 300, 250, 263, 271
    M, N = optimal_size(rows), optimal_size(cols)
    img = _img(rows, cols, 11)
    psf = oracle.motion_blur_kernel(9, 60.0)
    big = np.zeros((rows, stride), dtype=np.float32)
    big[:, :cols] = img
    d_in = torch.from_numpy(big).cuda()
    d_out = torch.full((rows, ostride), -7.0, dtype=torch.float32, device="cuda")
    with _plan(fdr, M, N) as p:
        p.set_psf(psf, 0.01)
        p.wiener_dev(d_in.data_ptr(), rows, cols, stride, d_out.data_ptr(), ostride, fdr.NORM_PADDED)
        torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[:, cols:] == -7.0)
    want = wiener_model(img, psf, 0.01, M, N, norm_cropped=False)
    mx, rel = _errs(out[:, :cols], want)
    assert mx <= TOL and rel <= TOL, (mx, rel)


def _one_by_one(p, imgs, norm):
    return np.stack([p.wiener(im, norm) for im in imgs])


def test_batches_bit_identical(fdr, oracle):
    import torch
    count, rows, cols = 5, 200, 300
    M, N = optimal_size(rows), optimal_size(cols)
    imgs = np.stack([_img(rows, cols, 100 + i) for i in range(count)])
    psf = oracle.motion_blur_kernel(15, 30.0)
    with _plan(fdr, M, N) as p:
        p.set_psf(psf, 0.01)
        ref = _one_by_one(p, imgs, fdr.NORM_PADDED)
        p.set_concurrency(2)
        d_in = torch.from_numpy(imgs).cuda()
        d_out = torch.zeros_like(d_in)
        s = torch.cuda.current_stream().cuda_stream
        p.wiener_batch_dev(d_in.data_ptr(), rows * cols, count, rows, cols, cols, d_out.data_ptr(), rows * cols, cols,
                           fdr.NORM_PADDED, stream=s)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), ref)
        assert np.array_equal(p.wiener_batch(imgs, norm_area=fdr.NORM_PADDED), ref)
        p.set_batching(2, 2)  # documented: images alternate one by one, same bits
        d_out.zero_()
        p.wiener_batch_dev(d_in.data_ptr(), rows * cols, count, rows, cols, cols, d_out.data_ptr(), rows * cols, cols,
                           fdr.NORM_PADDED, stream=s)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), ref)
    imgs6 = np.stack([_img(rows, cols, 200 + i) for i in range(6)])
    with _plan(fdr, M, N) as p:
        p.set_psf(psf, 0.01)
        ref6 = _one_by_one(p, imgs6, fdr.NORM_PADDED)
    st, outs = fdr.batch_run([0, 0], M, N, 6, rows=rows, cols=cols, mode=fdr.MODE_FAST, flags=fdr.FLAG_MIXED_RADIX, psf=psf,
                             imgs=imgs6)
    assert np.array_equal(np.asarray(outs), ref6)


def test_plan_state(fdr, oracle):
    import torch
    rows, cols = 240, 350
    M, N = optimal_size(rows), optimal_size(cols)
    img = _img(rows, cols, 21)
    psf = oracle.motion_blur_kernel(15, 30.0)
    with _plan(fdr, M, N) as p, _plan(fdr, M, N) as q, _plan(fdr, M, N) as fresh:
        dims = (ctypes.c_int(), ctypes.c_int(), ctypes.c_int())
        assert fdr.lib.fdr_plan_dims(p._h, *[ctypes.byref(d) for d in dims]) == 0
        assert [d.value for d in dims] == [M, N, fdr.MODE_FAST]
        p.set_psf(psf, 0.05)
        first = p.wiener(img)
        assert np.array_equal(p.wiener(img), first)  # same input twice: same bits
        # filter export into a second plan
        nb = p.filter_bytes()
        assert nb == q.filter_bytes()
        buf = torch.empty(nb, dtype=torch.uint8, device="cuda")
        p.export_filter_dev(buf.data_ptr(), nb)
        torch.cuda.synchronize()
        q.import_filter_dev(buf.data_ptr(), nb, 0.05)
        torch.cuda.synchronize()
        assert np.array_equal(q.wiener(img), first)
        # set_psf twice with different K == a fresh plan
        p.set_psf(psf, 0.01)
        fresh.set_psf(psf, 0.01)
        assert np.array_equal(p.wiener(img), fresh.wiener(img))
        # per-pass names and phases
        p.profile(True)
        d_in = torch.from_numpy(img).cuda()
        d_out = torch.zeros_like(d_in)
        p.wiener_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), cols)
        names = [n for n, _, _ in p.pass_times()]
        assert all(n in names for n in MIXED_PASSES), names
        assert not any("simple" in n for n in names), names
        p.profile(False)
        assert p.phase_times()["compute"] > 0


CPP = r'''
#include "utils.hpp"
#include "fft/fft.hpp"
#include <cstdio>
int main(int argc, char** argv) {
    const int rows = 120, cols = 175;
    Mat img(rows, cols, CV_32FC1), psf(9, 9, CV_32FC1);
    FILE* f = std::fopen(argv[1], "rb");
    for (int r = 0; r < rows; ++r) if (std::fread(img.ptr<float>(r), sizeof(float), cols, f) != (size_t)cols) return 3;
    for (int r = 0; r < 9; ++r) if (std::fread(psf.ptr<float>(r), sizeof(float), 9, f) != 9) return 3;
    std::fclose(f);
    fft_gpu::Options o;
    o.mode = FDR_MODE_FAST;
    o.mixed_radix = true;
    Mat out = fft_gpu::wienerDeblur_myfft(img, psf, 0.01f, o);
    f = std::fopen(argv[2], "wb");
    for (int r = 0; r < rows; ++r) std::fwrite(out.ptr<float>(r), sizeof(float), cols, f);
    std::fclose(f);
    return 0;
}
'''


def test_cpp_shim_mixed_radix(fdr, oracle, tmp_path):
    src = tmp_path / "mixed_shim.cpp"
    src.write_text(CPP)
    exe = tmp_path / "mixed_shim"
    libdir = os.path.dirname(fdr.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfdr", "-Wl,-rpath," + libdir, "-lpthread"])
    img = _img(120, 175, 5)
    psf = oracle.motion_blur_kernel(9, 30.0)
    inp = tmp_path / "in.raw"
    with open(inp, "wb") as f:
        f.write(img.tobytes())
        f.write(psf.tobytes())
    out = tmp_path / "out.raw"
    subprocess.check_call([str(exe), str(inp), str(out)], timeout=120)
    got = np.fromfile(out, dtype=np.float32).reshape(120, 175)
    want = fdr.wienerDeblur_myfft_unpadded(img, psf, 0.01, mode=fdr.MODE_FAST, mixed_radix=True)
    assert np.array_equal(got, want)
