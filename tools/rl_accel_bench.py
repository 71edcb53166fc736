#!/usr/bin/env python3
"""Accelerated Richardson-Lucy iteration cost on one GPU: prints one JSON line.

For each plan (1024^2, 4096^2, 8192^2; full-plane image, motion 15/30 PSF) and both forms (plain and free-boundary): the device
time of the _dev call with `iters` iterations minus the time with 0 (hipEvents around each call, median of `reps` after warm-up)
divided by `iters` is one iteration, plain and accelerated in the same run (the method of tools/rl_bench.py).
A call of n >= 3 accelerated iterations runs n - 2 extrapolations and n - 1 directions, so the per-iteration figure at the default
10 carries 0.8 and 0.9 of them.  The per-pass device times of one accelerated call (fdr_plan_pass_times) give the rate of the new
kernels: the direction moves 16 bytes per pixel of the estimate, the extrapolation 12.

usage: tools/rl_accel_bench.py [--iters 10] [--reps 20] [--sizes 1024,4096,8192]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIRECTION_BYTES, EXTRAPOLATE_BYTES = 16, 12  # per pixel of the estimate: u1, y, g in and g out; u1, u0 in and y out
PASS_BYTES = {"RLA direction + alpha": DIRECTION_BYTES, "RLA extrapolate": EXTRAPOLATE_BYTES}


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
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"metric": "richardson_lucy_accel_us_per_iteration", "iters": args.iters, "reps": args.reps, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        d_in = torch.rand((n, n), device="cuda", dtype=torch.float32)
        d_out = torch.empty_like(d_in)
        res = {}
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)

            def plain(k, acc):
                return lambda: p.richardson_lucy_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, fdr.NORM_NONE, stream=stream,
                                                     accelerate=acc)

            def free(k, acc):
                return lambda: p.richardson_lucy_free_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, norm_area=fdr.NORM_NONE,
                                                          stream=stream, accelerate=acc)
            for form, call in (("plain", plain), ("free", free)):
                t0 = timed(torch, call(0, False), args.reps)
                it = (timed(torch, call(args.iters, False), args.reps) - t0) / args.iters
                a0 = timed(torch, call(0, True), args.reps)
                ait = (timed(torch, call(args.iters, True), args.reps) - a0) / args.iters
                p.profile(True)
                call(args.iters, True)()
                torch.cuda.synchronize()
                passes = {}
                for name, ms, cnt in p.pass_times():
                    if cnt and name in PASS_BYTES:
                        passes[name] = {"mean_us": round(ms * 1e3, 2), "launches": cnt,
                                        "TBps": round(PASS_BYTES[name] * n * n / (ms * 1e-3) / 1e12, 3)}
                p.profile(False)
                res[form] = {"us_per_iteration": round(it, 2), "accel_us_per_iteration": round(ait, 2), "accel_over_plain": round(ait / it, 3),
                             "us_call_0_iterations": round(t0, 1), "accel_us_call_0_iterations": round(a0, 1), "passes": passes}
        out["sizes"]["%dx%d" % (n, n)] = res
        del d_in, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
