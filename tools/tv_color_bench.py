#!/usr/bin/env python3
"""Colour / batched total-variation deconvolution against the one-by-one calls on one GPU (after tools/rl_batch_bench.py).

For each size (256^2 .. 4096^2; full-plane images, motion 15/30 PSF) and `count` channels (3): the device time of a call with `iters`
iterations minus the time with 0 (hipEvents around each call, median of `reps` after warm-up), divided by `iters` and by the count,
is the time of one iteration of one image.  "one_by_one" is the loop of `count` fdr_tv_deconv_f32_dev calls, "single" one such
call, "group" one fdr_tv_deconv_batch_f32_dev call with group = count and FDR_TV_COUPLE_NONE, "coupled" the same call with
FDR_TV_COUPLE_CHANNELS (the last two only where the package has them: --root names the tree whose package and library are measured,
so a build of the parent commit gives the baseline of the single-image call in the same session).  The ratios group / one_by_one and
coupled / group follow.  One profiled call of each batched kind gives the time of its spatial launch.  Prints one JSON line.

usage: tools/tv_color_bench.py [--root DIR] [--iters 10] [--reps 20] [--sizes 256,1024,2048,4096] [--count 3]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd"
SPATIAL = {"group": "TV spatial: shrink+dual+div", "coupled": "TV spatial: joint shrink+dual+div"}


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
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="256,1024,2048,4096")
    ap.add_argument("--count", type=int, default=3)
    ap.add_argument("--mu", type=float, default=500.0)
    ap.add_argument("--rho", type=float, default=2.0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    fdr = importlib.import_module(PKG)
    stream = torch.cuda.current_stream().cuda_stream
    has_batch = hasattr(fdr.Plan, "tv_deconv_batch_dev")
    count = args.count
    out = {"metric": "tv_admm_us_per_image_iteration", "root": os.path.abspath(args.root), "iters": args.iters, "reps": args.reps, "count": count,
           "mu": args.mu, "rho": args.rho, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        d_in = torch.rand((count, n, n), device="cuda", dtype=torch.float32)
        d_out = torch.empty_like(d_in)
        px = n * n
        res = {}
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)

            def loop(k, cnt):
                def fn():
                    for i in range(cnt):
                        p.tv_deconv_dev(d_in.data_ptr() + 4 * i * px, n, n, n, d_out.data_ptr() + 4 * i * px, n, args.mu, args.rho, k, stream=stream)
                return fn

            def batch(k, coupled):
                return lambda: p.tv_deconv_batch_dev(d_in.data_ptr(), px, count, n, n, n, d_out.data_ptr(), px, n, args.mu, args.rho, k,
                                                     coupled=coupled, stream=stream)

            def per_image(make_k, make_0, cnt):
                return (timed(torch, make_k, args.reps) - timed(torch, make_0, args.reps)) / args.iters / cnt

            p.set_batching(1, 1)
            res["single"] = round(per_image(loop(args.iters, 1), loop(0, 1), 1), 2)
            res["one_by_one"] = round(per_image(loop(args.iters, count), loop(0, count), count), 2)
            if has_batch:
                p.set_batching(1, count)
                for kind, coupled in (("group", False), ("coupled", True)):
                    res[kind] = round(per_image(batch(args.iters, coupled), batch(0, coupled), count), 2)
                    p.profile(True)
                    for _ in range(3):
                        batch(args.iters, coupled)()
                    torch.cuda.synchronize()
                    passes = {name: ms * 1e3 for name, ms, _ in p.pass_times()}  # (mean per launch)
                    p.profile(False)
                    res[kind + "_spatial_us_per_launch"] = round(passes.get(SPATIAL[kind], float("nan")), 2)
                res["group_over_one_by_one"] = round(res["group"] / res["one_by_one"], 4)
                res["coupled_over_group"] = round(res["coupled"] / res["group"], 4)
        out["sizes"]["%dx%d" % (n, n)] = res
        del d_in, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
