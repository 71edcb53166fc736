#!/usr/bin/env python3
"""Cost of choosing the regularisation weight on one GPU: prints one JSON line.

For each plan (1024^2, 4096^2, 8192^2; full-plane image): the device time of fdr_choose_reg_f32_dev with the default search (GCV on
gamma, 32 candidates per round, 2 refinements: pass A, the power pass and three sweeps of two launches; hipEvents around each
call, median of `reps` after warm-up), of the discrepancy principle (the same plus the noise sum), of one fdr_reg_curve_f32_dev call
with 16 pairs (one sweep) and of fdr_noise_sigma_f32_dev, next to fdr_wiener_f32_dev on the same plan and image.  The calls are
synchronous (they read their sums back after every round), so their times include those copies.  The algorithmic bytes of the default
choice (about 50 per padded pixel) give the rate it implies.

usage: tools/reg_bench.py [--reps 20] [--sizes 1024,4096,8192]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BYTES_PER_PIXEL = 50  # pass A 4 + 4, the power pass 4 + 2, six sweep launches of 6 each


def timed(torch, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)  # us
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1024,4096,8192")
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"metric": "choose_regularisation_us", "reps": args.reps, "bytes_per_padded_pixel": BYTES_PER_PIXEL, "sizes": {}}
    K16, g16 = [0.0] * 16, [10.0 ** (k / 2 - 6) for k in range(16)]
    for n in (int(s) for s in args.sizes.split(",")):
        d_in = torch.rand((n, n), device="cuda", dtype=torch.float32)
        d_out = torch.empty_like(d_in)
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_psf_motion(15, 30.0, 0.01, stream=stream)
            p.set_operator_psf_motion(15, 30.0, stream=stream)
            t_g = timed(torch, lambda: p.choose_regularisation_dev(d_in.data_ptr(), n, n, n, stream=stream), args.reps)
            t_d = timed(torch, lambda: p.choose_regularisation_dev(d_in.data_ptr(), n, n, n, method=fdr.REG_DISCREPANCY, stream=stream), args.reps)
            t_c = timed(torch, lambda: p.reg_curve_dev(d_in.data_ptr(), n, n, n, K16, g16, stream=stream), args.reps)
            t_n = timed(torch, lambda: p.noise_sigma_dev(d_in.data_ptr(), n, n, n, stream=stream), args.reps)
            t_w = timed(torch, lambda: p.wiener_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, fdr.NORM_PADDED, stream=stream), args.reps)
        nbytes = BYTES_PER_PIXEL * n * n
        out["sizes"]["%dx%d" % (n, n)] = {"choose_gcv_us": round(t_g, 1), "choose_discrepancy_us": round(t_d, 1), "curve16_us": round(t_c, 1),
                                          "noise_us": round(t_n, 1), "wiener_us": round(t_w, 1), "choose_over_wiener": round(t_g / t_w, 2),
                                          "choose_bytes": nbytes, "choose_implied_TBps": round(nbytes / (t_g * 1e-6) / 1e12, 3)}
        del d_in, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
