#!/usr/bin/env python3
"""What the fit trace and the stopping rules of fdr_richardson_lucy_auto_f32_dev cost on one GPU: prints one JSON line.

For each plan (512^2, 4096^2; full-plane image, motion 15/30 PSF) and each of the four forms: the device time of the _dev call with
`iters` iterations minus the time with 0 (hipEvents around each call, median of `reps` after warm-up; the method of
tools/rl_accel_bench.py) divided by `iters` is one iteration -- of the existing call and of the auto call with FDR_RL_STOP_NONE and
the caller's trace, in the same run, with the quartiles of the per-call times so that the ratio can be read against the spread.
With a rule the call waits for the device every check_every steps: a tau so small that the rule never fires gives the wall time
of `iters` iterations at check_every 1 and 8, and (that - the wall time with FDR_RL_STOP_NONE) / checks is one host check.

usage: tools/rl_stop_bench.py [--iters 16] [--reps 20] [--sizes 512,4096]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, reps, warm=3):
    """(median, first quartile, third quartile) of the device time of fn in us"""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    q = statistics.quantiles(ts, n=4)
    return statistics.median(ts), q[0], q[2]


def wall(torch, fn, reps, warm=3):
    """median wall time of fn plus a synchronisation, in us"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e6)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="512,4096")
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"metric": "richardson_lucy_auto_us_per_iteration", "iters": args.iters, "reps": args.reps, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        d_in = torch.rand((n, n), device="cuda", dtype=torch.float32) + 0.1
        d_out = torch.empty_like(d_in)
        d_tr = torch.zeros(2 * args.iters, device="cuda", dtype=torch.float64)
        res = {}
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)
            for free in (False, True):
                for acc in (False, True):
                    def existing(k):
                        if free:
                            return lambda: p.richardson_lucy_free_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, norm_area=fdr.NORM_NONE,
                                                                      stream=stream, accelerate=acc)
                        return lambda: p.richardson_lucy_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, fdr.NORM_NONE, stream=stream,
                                                             accelerate=acc)

                    def auto(k, rule=fdr.RL_STOP_NONE, every=0):
                        return lambda: p.richardson_lucy_auto_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, rule, sigma=1.0, tau=1e-30,
                                                                  check_every=every, free_boundary=free, accelerate=acc, d_trace=d_tr.data_ptr(),
                                                                  stream=stream)
                    e0 = timed(torch, existing(0), args.reps)[0]
                    e = timed(torch, existing(args.iters), args.reps)
                    a0 = timed(torch, auto(0), args.reps)[0]
                    a = timed(torch, auto(args.iters), args.reps)
                    it, ait = (e[0] - e0) / args.iters, (a[0] - a0) / args.iters
                    w_none = wall(torch, auto(args.iters), args.reps)
                    checks = {}
                    for every in (1, 8):
                        w = wall(torch, auto(args.iters, fdr.RL_STOP_RESIDUAL, every), args.reps)
                        n_checks = -(-args.iters // every)
                        checks["check_every_%d" % every] = {"wall_us": round(w, 1), "checks": n_checks, "us_per_check": round((w - w_none) / n_checks, 2)}
                    res["%s%s" % ("free" if free else "plain", "_accel" if acc else "")] = {
                        "us_per_iteration": round(it, 2), "auto_us_per_iteration": round(ait, 2), "auto_over_existing": round(ait / it, 4),
                        "call_us_quartiles": [round(e[1], 1), round(e[0], 1), round(e[2], 1)],
                        "auto_call_us_quartiles": [round(a[1], 1), round(a[0], 1), round(a[2], 1)],
                        "spread_of_call": round((e[2] - e[1]) / e[0], 4), "wall_us_rule_none": round(w_none, 1), "rule": checks}
        out["sizes"]["%dx%d" % (n, n)] = res
        del d_in, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
