#!/usr/bin/env python3
"""Blind Richardson-Lucy step cost on one GPU: prints one JSON line.

For each plan (1024^2, 4096^2, 8192^2; full-plane image, 9 x 9 Gaussian start PSF) and each form (plain, free-boundary): the device
time of fdr_richardson_lucy_blind_f32_dev with `iters` iterations minus the time with 0 (hipEvents around each call, median of
`reps` after warm-up) divided by `iters` is one blind step; beside it the step of the non-blind call of the same form
(fdr_richardson_lucy_f32_dev / fdr_richardson_lucy_free_f32_dev), timed the same way in the same run, and their ratio.  The
algorithmic bytes of a step give the rate it implies.  --passes adds the per-pass device times of one blind
call of each form (fdr_plan_pass_times).

usage: tools/blind_bench.py [--iters 10] [--reps 20] [--sizes 1024,4096,8192] [--passes]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# per padded pixel: the RL step, + the image's table 8, pass A of r 8, B' 12, the PSF crop 4, the tables of the new PSF 8;
# free form: + the same three passes for W 24, the coverage of the new PSF (A 8, B' 12, C 8) and its reciprocal 8
BYTES = {"plain": 64 + 40, "free": 68 + 40 + 24 + 36}
RL_BYTES = {"plain": 64, "free": 68}


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
    out = {"metric": "blind_richardson_lucy_us_per_step", "iters": args.iters, "reps": args.reps, "bytes_per_padded_pixel": BYTES, "sizes": {}}
    start = torch.from_numpy(fdr.psf_gaussian(9)).cuda()
    for n in (int(s) for s in args.sizes.split(",")):
        d_in = torch.rand((n, n), device="cuda", dtype=torch.float32) + 0.05
        d_out = torch.empty_like(d_in)
        d_psf = start.clone()
        res = {}
        for form in ("plain", "free"):  # a plan each: a plan's pass timer remembers 16 names
            free = form == "free"
            with fdr.Plan(n, n, fdr.MODE_FAST) as p:

                def blind(k):
                    def run():
                        d_psf.copy_(start)  # 81 floats: every call starts from the same PSF
                        p.richardson_lucy_blind_dev(d_in.data_ptr(), n, n, n, d_psf.data_ptr(), 9, 9, 9, d_out.data_ptr(), n, k, free_boundary=free,
                                                    stream=stream)
                    return run

                def rl(k):
                    if free:
                        return lambda: p.richardson_lucy_free_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, norm_area=fdr.NORM_NONE, stream=stream)
                    return lambda: p.richardson_lucy_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, fdr.NORM_NONE, stream=stream)
                b_k, b_0 = timed(torch, blind(args.iters), args.reps), timed(torch, blind(0), args.reps)
                r_k, r_0 = timed(torch, rl(args.iters), args.reps), timed(torch, rl(0), args.reps)
                step, rl_step = (b_k - b_0) / args.iters, (r_k - r_0) / args.iters
                res[form] = {"blind_us_per_step": round(step, 2), "rl_us_per_step": round(rl_step, 2), "blind_over_rl": round(step / rl_step, 3),
                             "blind_us_call_0": round(b_0, 1), "blind_implied_TBps": round(BYTES[form] * n * n / (step * 1e-6) / 1e12, 3),
                             "rl_implied_TBps": round(RL_BYTES[form] * n * n / (rl_step * 1e-6) / 1e12, 3)}
                if args.passes:
                    p.pass_times()
                    p.profile(True)
                    blind(args.iters)()
                    torch.cuda.synchronize()
                    res[form]["passes"] = {name: {"mean_us": round(ms * 1e3, 2), "launches": cnt} for name, ms, cnt in p.pass_times() if cnt}
                    p.profile(False)
        out["sizes"]["%dx%d" % (n, n)] = res
        del d_in, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
