#!/usr/bin/env python3
"""Motion-blur estimate cost on one GPU: prints one JSON line.

For each plan (1024^2, 4096^2, 8192^2; full-plane image): the device time of fdr_estimate_motion_f32_dev with the default search
(0.5 deg x lengths 3 .. 100, 360 x 98 table; hipEvents around each call, median of `reps` after warm-up) and of
fdr_cepstrum_f32_dev alone, next to fdr_wiener_f32_dev on the same plan and image.  The estimate is synchronous (it reads its table
back), so its time includes that copy and the host's median / MAD.  The algorithmic bytes of the estimate (about 92 per padded
pixel) give the rate it implies; fdr_cepstrum_f32_dev adds the real-part pass (12 more).

usage: tools/motion_bench.py [--reps 20] [--sizes 1024,4096,8192]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BYTES_PER_PIXEL = 92  # pad 12, forward 32, log 16, inverse 32 (the gather reads a few hundred thousand bins)


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
    out = {"metric": "motion_estimate_us", "reps": args.reps, "bytes_per_padded_pixel": BYTES_PER_PIXEL, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        d_in = torch.rand((n, n), device="cuda", dtype=torch.float32)
        d_out = torch.empty_like(d_in)
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_psf_motion(15, 30.0, 0.01, stream=stream)
            t_e = timed(torch, lambda: p.estimate_motion_dev(d_in.data_ptr(), n, n, n, 3, 100, 0.5, stream=stream), args.reps)
            t_c = timed(torch, lambda: p.cepstrum_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), stream=stream), args.reps)
            t_w = timed(torch, lambda: p.wiener_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, fdr.NORM_PADDED, stream=stream), args.reps)
        nbytes = BYTES_PER_PIXEL * n * n
        out["sizes"]["%dx%d" % (n, n)] = {"estimate_us": round(t_e, 1), "cepstrum_us": round(t_c, 1), "wiener_us": round(t_w, 1),
                                          "estimate_over_wiener": round(t_e / t_w, 2), "estimate_bytes": nbytes,
                                          "estimate_implied_TBps": round(nbytes / (t_e * 1e-6) / 1e12, 3)}
        del d_in, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
