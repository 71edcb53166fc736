#!/usr/bin/env python3
"""Batched Richardson-Lucy with the TV prior against the one-by-one calls on one GPU (after tools/rl_accel_batch_bench.py).

measure: for each size (256^2 .. 4096^2; full-plane images, motion 15/30 PSF, lambda 0.01), form (plain, free-boundary without
weights) and count (3, 4): the device time of a call with `iters` iterations minus the time with 0 (hipEvents around each call,
median of `reps` after warm-up), divided by `iters` and by the count, is the time of one iteration of one image.  "one_by_one" is
the loop of `count` single-image fdr_richardson_lucy_tv_f32_dev calls, "single" one such call, "batched" one
fdr_richardson_lucy_tv_batch_f32_dev call with group = count and "coupled" the same with FDR_TV_COUPLE_CHANNELS (both only where the
package has them).  --root names the tree whose package and library are measured: the baseline is a build of the parent commit.
Prints one JSON line.

report: the new tree's JSON and the baseline's (repeated: spread = (max - min) / median of its runs is the run-to-run noise) ->
medians, spread and ratios, and the two conditions: up to 2048^2 the batched per-image iteration lies below the baseline's LOWEST
one-by-one run, and the new single-image iteration lies within the baseline's spread of its median; the cost of the coupled launch
over the uncoupled group is stated.  Prints one JSON document (profiles/rl_tv_batch_bench.json).

usage: tools/rl_tv_batch_bench.py measure [--root DIR] [--iters 10] [--reps 20] [--sizes 256,512,1024,2048,4096] [--counts 3,4]
       tools/rl_tv_batch_bench.py report NEW.json BASE1.json [BASE2.json ...]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd"
FORMS = ("plain", "free")
LAMBDA = 0.01
CONDITION_UP_TO = 2048  # the batched time has to beat the loop up to this size; larger sizes are reported


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


def measure(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    fdr = importlib.import_module(PKG)
    stream = torch.cuda.current_stream().cuda_stream
    has_batch = hasattr(fdr.Plan, "richardson_lucy_tv_batch_dev")
    counts = [int(c) for c in args.counts.split(",")]
    out = {"metric": "richardson_lucy_tv_us_per_image_iteration", "root": os.path.abspath(args.root), "iters": args.iters, "reps": args.reps, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        cmax = max(counts)
        d_in = torch.rand((cmax, n, n), device="cuda", dtype=torch.float32)
        d_out = torch.empty_like(d_in)
        px = n * n
        res = {}
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)

            def loop(form, k, count, couple):
                def fn():
                    for i in range(count):
                        p.richardson_lucy_tv_dev(d_in.data_ptr() + 4 * i * px, n, n, n, d_out.data_ptr() + 4 * i * px, n, k, LAMBDA,
                                                 free_boundary=form == "free", stream=stream)
                return fn

            def batch(form, k, count, couple):
                return lambda: p.richardson_lucy_tv_batch_dev(d_in.data_ptr(), px, count, n, n, n, d_out.data_ptr(), px, n, k, LAMBDA,
                                                              free_boundary=form == "free", couple=couple, stream=stream)

            def per_image(make, form, count, couple=0):
                return (timed(torch, make(form, args.iters, count, couple), args.reps) - timed(torch, make(form, 0, count, couple), args.reps)) / args.iters / count

            for form in FORMS:
                p.set_batching(1, 1)
                res["%s_single" % form] = round(per_image(loop, form, 1), 2)
                for count in counts:
                    p.set_batching(1, 1)
                    res["%s_one_by_one_%d" % (form, count)] = round(per_image(loop, form, count), 2)
                    if has_batch:
                        p.set_batching(1, count)
                        res["%s_batched_%d" % (form, count)] = round(per_image(batch, form, count), 2)
                        res["%s_coupled_%d" % (form, count)] = round(per_image(batch, form, count, fdr.TV_COUPLE_CHANNELS), 2)
        out["sizes"]["%dx%d" % (n, n)] = res
        del d_in, d_out
    print(json.dumps(out))


def report(args):
    new = json.load(open(args.files[0]))
    bases = [json.load(open(f)) for f in args.files[1:]]
    doc = {"metric": "richardson_lucy_tv_us_per_image_iteration", "iters": new["iters"], "reps": new["reps"], "baseline_runs": len(bases),
           "baseline": "one-by-one fdr_richardson_lucy_tv_f32_dev calls on a build of the parent commit, same GPU visit", "sizes": {}}
    ok_all = True
    for size, res in new["sizes"].items():
        n = int(size.split("x")[0])
        row = {}
        for key in sorted(bases[0]["sizes"][size]):
            vals = [b["sizes"][size][key] for b in bases]
            med = statistics.median(vals)
            row["parent_" + key] = {"median_us": round(med, 2), "runs_us": vals, "spread": round((max(vals) - min(vals)) / med, 4)}
        for key, v in sorted(res.items()):
            ref = key.replace("_batched_", "_one_by_one_").replace("_coupled_", "_one_by_one_")
            base = row["parent_" + ref]
            ratio = v / base["median_us"]
            kind = "batched_vs_parent_one_by_one" if "_batched_" in key else "coupled_vs_parent_one_by_one" if "_coupled_" in key else "new_vs_parent"
            entry = {"us": v, "ratio_to_parent": round(ratio, 4), "kind": kind}
            if "_batched_" in key and n <= CONDITION_UP_TO:
                entry["condition_met"] = bool(v < min(base["runs_us"]))  # below the parent's lowest one-by-one run
            elif key.endswith("_single"):
                entry["condition_met"] = bool(abs(ratio - 1.0) <= base["spread"])  # within the parent's spread
            if "_coupled_" in key:
                entry["cost_over_uncoupled_group"] = round(v / res[key.replace("_coupled_", "_batched_")], 4)
            if "condition_met" in entry:
                ok_all = ok_all and entry["condition_met"]
            row[key] = entry
        doc["sizes"][size] = row
    doc["all_conditions_met"] = ok_all
    print(json.dumps(doc, indent=1))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("measure")
    m.add_argument("--root", default=ROOT)
    m.add_argument("--iters", type=int, default=10)
    m.add_argument("--reps", type=int, default=20)
    m.add_argument("--sizes", default="256,512,1024,2048,4096")
    m.add_argument("--counts", default="3,4")
    r = sub.add_parser("report")
    r.add_argument("files", nargs="+")
    args = ap.parse_args()
    measure(args) if args.cmd == "measure" else report(args)


if __name__ == "__main__":
    main()
