#!/usr/bin/env python3
"""Defocus and combined blur estimate cost on one GPU, beside the motion estimate: prints one JSON line.

For each plan (1024^2, 4096^2, 8192^2; full-plane image) the device time of fdr_estimate_defocus_f32_dev, fdr_estimate_motion_f32_dev
and fdr_estimate_blur_f32_dev with the default searches (0.5 deg x 3 .. 100: a 360 x 98 table, a 98-entry profile), each the median of
`reps` calls after warm-up, hipEvents around each call.  The three calls alternate inside one loop, so a change of the machine's load
falls on all of them.  All three are synchronous (they read their result back), so a time includes that copy and the host's pick.
What DESIGN.md section 28 expects: the defocus estimate at most 1.10x and the combined one at most 1.25x the motion estimate.
--passes adds the per-pass device times of one call of each kind (fdr_plan_pass_times).

usage: tools/defocus_bench.py [--reps 20] [--sizes 1024,4096,8192] [--passes]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_alternating(torch, fns, reps, warm=3):
    """median device time in us of each of fns, called in turn `reps` times after `warm` rounds"""
    for _ in range(warm):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    return [statistics.median(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--passes", action="store_true")
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"metric": "blur_estimates_us", "reps": args.reps, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        d_in = torch.rand((n, n), device="cuda", dtype=torch.float32)
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            calls = [lambda: p.estimate_defocus_dev(d_in.data_ptr(), n, n, n, 3, 100, 0.5, stream=stream),
                     lambda: p.estimate_motion_dev(d_in.data_ptr(), n, n, n, 3, 100, 0.5, stream=stream),
                     lambda: p.estimate_blur_dev(d_in.data_ptr(), n, n, n, 3, 100, 0.5, 3, 100, 0.5, stream=stream)]
            t_d, t_m, t_b = timed_alternating(torch, calls, args.reps)
            res = {"defocus_us": round(t_d, 1), "motion_us": round(t_m, 1), "blur_us": round(t_b, 1), "defocus_over_motion": round(t_d / t_m, 3),
                   "blur_over_motion": round(t_b / t_m, 3)}
            if args.passes:
                for name, call in zip(("defocus", "motion", "blur"), calls):
                    p.pass_times()
                    p.profile(True)
                    call()
                    res[name + "_passes"] = {nm: {"mean_us": round(ms * 1e3, 2), "launches": cnt} for nm, ms, cnt in p.pass_times() if cnt}
                    p.profile(False)
        out["sizes"]["%dx%d" % (n, n)] = res
        del d_in
    print(json.dumps(out))


if __name__ == "__main__":
    main()
