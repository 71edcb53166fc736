#!/usr/bin/env python3
"""The frame registration on one GPU (fdr_register_frames_f32_dev).

For each size (1024^2, 4096^2; full-plane frames, 15 px motion PSFs at K angles) and K in {2, 4, 8}: the device time of one call
(hipEvents around it, median of `reps` after warm-up) divided by its K - 1 non-reference frames is the time of the estimate per
frame, with and without PSFs.  One profiled run of the same call gives the pass times (fdr_plan_pass_times): the three new kernel
groups alone -- window (the pair pass of the pictures and of the PSFs, the zero-frame gate), cross-power (the pair sweep, its fold,
the normalising sweep) and peak (the sweep and the pick) -- beside the plan's transforms.  Their algorithmic bytes per bin of the
plan, per frame with PSFs: window 16 written + 8 read on the window, cross-power 24 + 16, peak 8: 72 at window = plan.  The rate they
imply stands beside the TV spatial kernel's (28 bytes per pixel), timed in the same run on the same plan: the project's usual yardstick
for a streaming kernel.

Prints one JSON document and writes it to --out (profiles/register_bench.json).

usage: tools/register_bench.py [--reps 10] [--sizes 1024,4096] [--counts 2,4,8] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd"
SPATIAL_PASS = "TV spatial: shrink+dual+div"
BYTES_SPATIAL = 28
NEW_PASSES = {"register window": 24, "register cross-power": 40, "register peak": 8}  # bytes per bin and frame, window = plan, with PSFs


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--counts", default="2,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    fdr = importlib.import_module(PKG)
    stream = torch.cuda.current_stream().cuda_stream
    counts = [int(c) for c in args.counts.split(",")]
    kmax = max(counts)
    out = {"metric": "register_frames_us_per_frame", "reps": args.reps, "bytes_per_bin": NEW_PASSES, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        px = n * n
        d_in = torch.rand((kmax, n, n), device="cuda", dtype=torch.float32) + 0.05
        d_tmp = torch.empty((n, n), device="cuda", dtype=torch.float32)
        d_psf = torch.from_numpy(np.stack([fdr.motionBlurKernel(15, 8.0 + 22.0 * k) for k in range(kmax)])).cuda()
        d_sh = torch.zeros(kmax * 24, dtype=torch.uint8, device="cuda")
        res = {}
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)
            p.profile(True)
            for _ in range(3):
                p.tv_deconv_dev(d_in.data_ptr(), n, n, n, d_tmp.data_ptr(), n, 100.0, 2.0, 4, False, stream=stream)
            torch.cuda.synchronize()
            sp = {name: ms * 1e3 for name, ms, _ in p.pass_times()}.get(SPATIAL_PASS, float("nan"))
            p.profile(False)
            sp_rate = BYTES_SPATIAL * px / (sp * 1e-6) / 1e12
            res.update({"tv_spatial_us": round(sp, 2), "tv_spatial_TBps": round(sp_rate, 3)})
            for K in counts:
                row = {}
                for tag, with_psfs in (("", True), ("_plain", False)):
                    def call():
                        p.register_frames_dev(d_in.data_ptr(), px, K, n, n, n, d_sh.data_ptr(), d_psfs=d_psf.data_ptr() if with_psfs else None,
                                              psf_pitch=225, prows=15, pcols=15, pstride=15, stream=stream)
                    row["us_per_frame" + tag] = round(timed(torch, call, args.reps) / (K - 1), 2)
                call = None
                p.profile(True)
                p.pass_times()  # (clears the records)
                for _ in range(3):
                    p.register_frames_dev(d_in.data_ptr(), px, K, n, n, n, d_sh.data_ptr(), d_psfs=d_psf.data_ptr(), psf_pitch=225, prows=15, pcols=15,
                                          pstride=15, stream=stream)
                torch.cuda.synchronize()
                frames = 3 * (K - 1)
                passes = {name: ms * 1e3 * cnt / frames for name, ms, cnt in p.pass_times() if name.startswith("register")}  # us per frame
                p.profile(False)
                new_us = sum(passes.get(name, float("nan")) for name in NEW_PASSES)
                new_rate = sum(NEW_PASSES.values()) * px / (new_us * 1e-6) / 1e12
                row.update({"pass_us_per_frame": {k: round(v, 2) for k, v in passes.items()}, "new_kernels_us_per_frame": round(new_us, 2),
                            "new_kernels_TBps": round(new_rate, 3), "new_kernels_over_tv_spatial_rate": round(new_rate / sp_rate, 3)})
                for name, nbytes in NEW_PASSES.items():
                    row[name.replace(" ", "_") + "_TBps"] = round(nbytes * px / (passes.get(name, float("nan")) * 1e-6) / 1e12, 3)
                res["K=%d" % K] = row
        out["sizes"]["%dx%d" % (n, n)] = res
        del d_in, d_tmp, d_psf, d_sh
    text = json.dumps(out, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
