#!/usr/bin/env python3
"""Free-boundary and noise-constrained TV deconvolution in groups against the loop of single calls on one GPU (after
tools/tv_color_bench.py).

For each size (256^2 .. 4096^2; motion 15/30 PSF; the window is the plan less the PSF's reach, n - 14 square, so its rows have no
16-byte alignment) and each group size (3 and 4 images): the device time of a call with `iters` iterations minus the time with 0
(hipEvents around each call, median of `reps` after warm-up), divided by `iters` and by the number of images, is the time of one
iteration of one image.  Modes: "free" (fdr_tv_deconv_free_batch_f32_dev, uncoupled), "auto" (fdr_tv_deconv_auto_batch_f32_dev with
sigma given, uncoupled) and "free_coupled" (FDR_TV_COUPLE_CHANNELS).  Each is compared with "one_by_one", the loop of single
fdr_tv_deconv_free_f32_dev / fdr_tv_deconv_auto_f32_dev calls on the library of --parent: a tree with a build of the parent
commit, whose package is loaded under another name into this process, so that both libraries run on one GPU in one session.  The
kinds alternate `rounds` times (parent loop, group, parent loop, ...); the figure of a kind is the median over its rounds, and the
spread of the parent's rounds (max / min) says what a ratio near 1 is worth.  "single" / "group_of_one": one single call of the
parent against one single call of this tree, the same way.  Without --parent the loop runs on this tree's own single calls;
--parent naming a copy of this tree is the control: what it shows between "single" and "group_of_one" belongs to the measurement
(two plans in one process), not to a library.  Prints one JSON line.

usage: tools/tv_free_batch_bench.py [--parent DIR] [--iters 10] [--reps 10] [--rounds 3] [--sizes 256,1024,2048,4096] [--groups 3,4]"""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd"


def timed(torch, fn, reps, warm=2):
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


def load_parent(root):
    """the package of another tree under the name fdr_parent: its own __init__.py and its own libfdr.so"""
    init = os.path.join(os.path.abspath(root), PKG, "__init__.py")
    spec = importlib.util.spec_from_file_location("fdr_parent", init, submodule_search_locations=[os.path.dirname(init)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["fdr_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="256,1024,2048,4096")
    ap.add_argument("--groups", default="3,4")
    ap.add_argument("--mu", type=float, default=500.0)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--rho", type=float, default=2.0)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    fdr = importlib.import_module(PKG)
    old = load_parent(args.parent) if args.parent else fdr
    stream = torch.cuda.current_stream().cuda_stream
    groups = [int(g) for g in args.groups.split(",")]
    gmax = max(groups)
    out = {"metric": "tv_crop_admm_us_per_image_iteration", "parent": os.path.abspath(args.parent) if args.parent else None, "iters": args.iters,
           "reps": args.reps, "rounds": args.rounds, "mu": args.mu, "sigma": args.sigma, "rho": args.rho, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        m = n - 14
        px = m * m
        d_in = torch.rand((gmax, m, m), device="cuda", dtype=torch.float32)
        d_out = torch.empty_like(d_in)
        res = {"window": "%dx%d" % (m, m)}
        with fdr.Plan(n, n, fdr.MODE_FAST) as p, old.Plan(n, n, old.MODE_FAST) as q:
            p.set_operator_psf_motion(15, 30.0, stream=stream)
            q.set_operator_psf_motion(15, 30.0, stream=stream)

            def loop(plan, auto, k, cnt):
                def fn():
                    for i in range(cnt):
                        src, dst = d_in.data_ptr() + 4 * i * px, d_out.data_ptr() + 4 * i * px
                        if auto:
                            plan.tv_deconv_auto_dev(src, m, m, m, dst, m, args.sigma, args.rho, k, stream=stream)
                        else:
                            plan.tv_deconv_free_dev(src, m, m, m, dst, m, args.mu, args.rho, k, stream=stream)
                return fn

            def batch(auto, k, cnt, coupled):
                if auto:
                    return lambda: p.tv_deconv_auto_batch_dev(d_in.data_ptr(), px, cnt, m, m, m, d_out.data_ptr(), px, m, args.sigma, args.rho, k,
                                                              coupled=coupled, stream=stream)
                return lambda: p.tv_deconv_free_batch_dev(d_in.data_ptr(), px, cnt, m, m, m, d_out.data_ptr(), px, m, args.mu, args.rho, k,
                                                          coupled=coupled, stream=stream)

            def per_image(make, cnt):
                return (timed(torch, make(args.iters), args.reps) - timed(torch, make(0), args.reps)) / args.iters / cnt

            def compare(kinds, cnt):
                """{kind: median over the rounds}, the kinds alternating, and the spread of the first kind's rounds"""
                seen = {k: [] for k, _ in kinds}
                for _ in range(args.rounds):
                    for k, make in kinds:
                        seen[k].append(per_image(make, cnt))
                first = seen[kinds[0][0]]
                return {k: round(statistics.median(v), 2) for k, v in seen.items()}, round(max(first) / min(first), 3)

            for auto, tag in ((False, "free"), (True, "auto")):
                p.set_batching(1, 1)
                r, spread = compare([("single", lambda k: loop(q, auto, k, 1)), ("group_of_one", lambda k: loop(p, auto, k, 1))], 1)
                res[tag + "_single"] = dict(r, parent_spread=spread, group_of_one_over_single=round(r["group_of_one"] / r["single"], 4))
            for g in groups:
                p.set_batching(1, g)
                for auto, coupled, tag in ((False, False, "free"), (True, False, "auto"), (False, True, "free_coupled")):
                    r, spread = compare([("one_by_one", lambda k: loop(q, auto, k, g)), ("group", lambda k: batch(auto, k, g, coupled))], g)
                    res["%s_group%d" % (tag, g)] = dict(r, parent_spread=spread, group_over_one_by_one=round(r["group"] / r["one_by_one"], 4))
        out["sizes"]["%dx%d" % (n, n)] = res
        del d_in, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
