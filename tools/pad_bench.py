#!/usr/bin/env python3
"""Cost of the smooth padding (FDR_OPT_PAD_MODE = FDR_PAD_SMOOTH) of the Wiener call on one GPU: prints one JSON line.

For each case (a rows x cols window in an M x N fast-mode plan, motion 15/30 PSF, K = 0.01): the device time of fdr_wiener_f32_dev with
zero padding and with smooth padding (hipEvents around each call, median of `reps` calls after warm-up), their ratio, and with --passes
the per-pass device times of one call in each mode (fdr_plan_pass_times).  The measurement is repeated `rounds` times, the two modes
alternating, and the spread of the round medians ((max - min) / median) is reported beside them: a difference inside it is noise.

--zero-only measures zero padding alone and does not touch the option, so the same script runs against a library built from an earlier
commit (FDR_LIB_PATH=/path/to/libfdr.so) for a before / after comparison on the same machine.

usage: tools/pad_bench.py [--reps 20] [--rounds 5] [--cases 4096x4096:4096x4096,3000x4000:4096x4096,700x900:1024x1024] [--passes] [--zero-only]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_CASES = "4096x4096:4096x4096,3000x4000:4096x4096,700x900:1024x1024"


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


def summary(xs):
    med = statistics.median(xs)
    return {"us": round(med, 2), "rounds_us": [round(x, 2) for x in xs], "spread": round((max(xs) - min(xs)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--passes", action="store_true")
    ap.add_argument("--zero-only", action="store_true")
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"metric": "wiener_f32_dev_us_zero_vs_smooth_padding", "reps": args.reps, "rounds": args.rounds, "lib": os.path.realpath(fdr.LIB_PATH),
           "cases": {}}
    modes = [("zero", 0)] if args.zero_only else [("zero", fdr.PAD_ZERO), ("smooth", fdr.PAD_SMOOTH)]
    for case in args.cases.split(","):
        win, plan = case.split(":")
        rows, cols = (int(x) for x in win.split("x"))
        M, N = (int(x) for x in plan.split("x"))
        d_in = torch.rand((rows, cols), device="cuda", dtype=torch.float32)
        d_out = torch.empty_like(d_in)
        res = {}
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            p.set_psf_motion(15, 30.0, 0.01, stream=stream)

            def call():
                p.wiener_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), cols, fdr.NORM_CROPPED, stream=stream)
            ts = {name: [] for name, _ in modes}
            for _ in range(args.rounds):
                for name, value in modes:
                    if not args.zero_only:
                        p.set_option(fdr.OPT_PAD_MODE, value)
                    ts[name].append(timed(torch, call, args.reps))
            for name, _ in modes:
                res[name] = summary(ts[name])
            if not args.zero_only:
                res["smooth_over_zero"] = round(res["smooth"]["us"] / res["zero"]["us"], 4)
            if args.passes:
                for name, value in modes:
                    if not args.zero_only:
                        p.set_option(fdr.OPT_PAD_MODE, value)
                    p.profile(True)
                    for _ in range(5):
                        call()
                    torch.cuda.synchronize()
                    res[name]["passes_mean_us"] = {nm: round(ms * 1e3, 2) for nm, ms, cnt in p.pass_times() if cnt}
                    p.profile(False)
        out["cases"][case] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
