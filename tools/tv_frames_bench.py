#!/usr/bin/env python3
"""Multi-frame TV deconvolution against K single free-boundary TV iterations on one GPU (after tools/rl_frames_bench.py).

For each size (1024^2, 2048^2, 4096^2; full-plane frames, motion 15 px PSFs at K angles), K in {1, 2, 3, 5, 8} and both data terms:
the device time of one fdr_tv_deconv_frames_f32_dev call with `iters` iterations minus the time with 1 (hipEvents around each call,
median of `reps` after warm-up; 1 and not 0, so that the table build of a call is in neither), divided by `iters` - 1, is the time of
ONE joint iteration; measured for the launch groups 1 and min(K, 8).  The comparison, timed in the same run and the same way, is K
times one iteration of fdr_tv_deconv_free_f32_dev on the same plan.  By counting transform passes a joint iteration is 5 K + 7 (per
frame: rows, H_k columns, rows back, rows of r_k, conj(H_k) columns; then one inverse row pass of the summed spectrum, the three
passes of the solve, and the sum, data and spatial launches beside them) against 11 K: the expected ratio is (5 K + 7) / (11 K).

Prints one JSON document and writes it to --out (profiles/tv_frames_bench.json).

usage: tools/tv_frames_bench.py [--iters 6] [--reps 10] [--sizes 1024,2048,4096] [--counts 1,2,3,5,8] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd"


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
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--counts", default="1,2,3,5,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tv_frames_bench.json"))
    args = ap.parse_args()
    assert args.iters >= 2
    sys.path.insert(0, ROOT)
    import torch
    fdr = importlib.import_module(PKG)
    stream = torch.cuda.current_stream().cuda_stream
    counts = [int(c) for c in args.counts.split(",")]
    kmax = max(counts)
    mu = 100.0
    out = {"metric": "tv_deconv_frames_us_per_joint_iteration", "iters": args.iters, "reps": args.reps, "sizes": {}}

    def per_iteration(call):
        return (timed(torch, call(args.iters), args.reps) - timed(torch, call(1), args.reps)) / (args.iters - 1)

    for n in (int(s) for s in args.sizes.split(",")):
        px = n * n
        d_in = torch.rand((kmax, n, n), device="cuda", dtype=torch.float32) + 0.05
        d_out = torch.empty((n, n), device="cuda", dtype=torch.float32)
        psfs = [fdr.motionBlurKernel(15, 8.0 + 22.0 * k) for k in range(kmax)]
        res = {}
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf(psfs[0])
            p.set_batching(1, 1)
            one = per_iteration(lambda k: lambda: p.tv_deconv_free_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, mu, iterations=k, stream=stream))
            res["single_free_iteration_us"] = round(one, 2)
            for K in counts:
                p.set_frame_psfs(psfs[:K])
                row = {"K_single_iterations_us": round(K * one, 2), "expected_ratio_by_passes": round((5 * K + 7) / (11.0 * K), 4)}
                for name, term in (("least_squares", fdr.TV_FRAMES_LEAST_SQUARES), ("poisson", fdr.TV_FRAMES_POISSON)):
                    for group in sorted({1, min(K, 8)}):
                        p.set_batching(1, group)
                        t = per_iteration(lambda k: lambda: p.tv_deconv_frames_dev(d_in.data_ptr(), px, K, n, n, n, d_out.data_ptr(), n, mu, k,
                                                                                   data_term=term, stream=stream))
                        row["%s group_%d" % (name, group)] = {"joint_iteration_us": round(t, 2), "ratio_to_K_single": round(t / (K * one), 4)}
                res["K=%d" % K] = row
        out["sizes"]["%dx%d" % (n, n)] = res
        del d_in, d_out
    text = json.dumps(out, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
