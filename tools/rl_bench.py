#!/usr/bin/env python3
"""Richardson-Lucy iteration cost on one GPU: prints one JSON line.

For each plan (1024^2, 4096^2, 8192^2; full-plane image, motion 15/30 PSF): the device time of fdr_richardson_lucy_f32_dev with
`iters` iterations minus the time with 0 (hipEvents around each call, median of `reps` after warm-up) divided by `iters` is one
iteration; the algorithmic bytes of an iteration (64 per padded pixel) give the rate it implies.
fdr_wiener_f32_dev on the same plan and image is timed the same way for comparison, and so is a free-boundary iteration
(fdr_richardson_lucy_free_f32_dev, full-plane window, no weights; 68 bytes per pixel) with its ratio to the
plain iteration of the same run.  --passes adds the per-pass device times of one free-boundary call (fdr_plan_pass_times).

usage: tools/rl_bench.py [--iters 10] [--reps 20] [--sizes 1024,4096,8192] [--passes]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BYTES_PER_PIXEL = 64  # A 2 x 8, B' 2 x 12, ratio 12, update 12
FREE_BYTES_PER_PIXEL = 68  # the update reads wgt as well


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--passes", action="store_true")
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"metric": "richardson_lucy_us_per_iteration", "iters": args.iters, "reps": args.reps, "bytes_per_padded_pixel": BYTES_PER_PIXEL,
           "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        d_in = torch.rand((n, n), device="cuda", dtype=torch.float32)
        d_out = torch.empty_like(d_in)
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)
            p.set_psf_motion(15, 30.0, 0.01, stream=stream)

            def rl(k):
                return lambda: p.richardson_lucy_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, fdr.NORM_NONE, stream=stream)
            t_k = timed(torch, rl(args.iters), args.reps)
            t_0 = timed(torch, rl(0), args.reps)
            t_w = timed(torch, lambda: p.wiener_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, fdr.NORM_PADDED, stream=stream), args.reps)

            def free(k):
                return lambda: p.richardson_lucy_free_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, norm_area=fdr.NORM_NONE,
                                                          stream=stream)
            f_k = timed(torch, free(args.iters), args.reps)
            f_0 = timed(torch, free(0), args.reps)
            passes = None
            if args.passes:
                p.profile(True)
                free(args.iters)()
                torch.cuda.synchronize()
                passes = {name: {"mean_us": round(ms * 1e3, 2), "launches": cnt} for name, ms, cnt in p.pass_times() if cnt}
                p.profile(False)
        it = (t_k - t_0) / args.iters
        fit = (f_k - f_0) / args.iters
        nbytes = BYTES_PER_PIXEL * n * n
        out["sizes"]["%dx%d" % (n, n)] = {"us_per_iteration": round(it, 2), "us_call_%d_iterations" % args.iters: round(t_k, 1),
                                          "us_call_0_iterations": round(t_0, 1), "bytes_per_iteration": nbytes,
                                          "implied_TBps": round(nbytes / (it * 1e-6) / 1e12, 3), "wiener_us": round(t_w, 1),
                                          "iteration_over_wiener": round(it / t_w, 2),
                                          "free_us_per_iteration": round(fit, 2), "free_us_call_0_iterations": round(f_0, 1),
                                          "free_implied_TBps": round(FREE_BYTES_PER_PIXEL * n * n / (fit * 1e-6) / 1e12, 3),
                                          "free_over_plain": round(fit / it, 3)}
        if passes is not None:
            out["sizes"]["%dx%d" % (n, n)]["free_passes"] = passes
        del d_in, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
