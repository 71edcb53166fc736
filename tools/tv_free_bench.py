#!/usr/bin/env python3
"""Free-boundary TV (ADMM, two splittings) iteration cost on one GPU: prints one JSON line.

For each plan (1024^2, 4096^2, 8192^2; motion 15/30 PSF; the window is the plan less the PSF's reach, n - 14 square, a dense random
image, so its rows have no 16-byte alignment): the device time of fdr_tv_deconv_free_f32_dev with `iters` iterations minus the time
with 0 (hipEvents around each call, median of `reps` after warm-up) divided by `iters` is one iteration, without weights and with a
0 / 1 mask; the periodic fdr_tv_deconv_f32_dev on the same plan and window is timed the same way in the same run.  The passes of
profiled calls (fdr_plan_pass_times) give the data kernel's own time and the rate of its 20 bytes per window pixel (24 with
weights), beside the spatial kernel's time and the rate of its 28 bytes per padded pixel in the same calls.

usage: tools/tv_free_bench.py [--iters 10] [--reps 20] [--sizes 1024,4096,8192]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rl_bench import timed  # noqa: E402

BYTES_SPATIAL = 28  # x 4 + w 8 + b 4 in, w 8 + rhs 4 out, per padded pixel
BYTES_DATA = 20     # c 4 + q 4 + d 4 in, q 4 + r 4 out, per window pixel; the weights add 4
BYTES_CHAIN = 52    # A 16, B' with its table 24, C 12: a blur or the solve, per padded pixel
DATA_PASS = "TVF data: s, q, r = 2s-e (window)"
SPATIAL_PASS = "TV spatial: shrink+dual+div (free)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--mu", type=float, default=500.0)
    ap.add_argument("--rho", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"metric": "tv_free_admm_us_per_iteration", "iters": args.iters, "reps": args.reps, "mu": args.mu, "rho": args.rho, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        m = n - 14
        d_in = torch.rand((m, m), device="cuda", dtype=torch.float32)
        d_w = (torch.rand((m, m), device="cuda", dtype=torch.float32) > 0.02).to(torch.float32)
        d_out = torch.empty((m, m), device="cuda", dtype=torch.float32)
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)

            def free(k, w=None):
                return lambda: p.tv_deconv_free_dev(d_in.data_ptr(), m, m, m, d_out.data_ptr(), m, args.mu, args.rho, k, w, m, stream=stream)

            def tv(k):
                return lambda: p.tv_deconv_dev(d_in.data_ptr(), m, m, m, d_out.data_ptr(), m, args.mu, args.rho, k, stream=stream)
            f_k, f_0 = timed(torch, free(args.iters), args.reps), timed(torch, free(0), args.reps)
            f_kw = timed(torch, free(args.iters, d_w.data_ptr()), args.reps)
            t_k, t_0 = timed(torch, tv(args.iters), args.reps), timed(torch, tv(0), args.reps)
            passes = {}
            for tag, w in (("", None), ("_weights", d_w.data_ptr())):
                p.profile(True)
                for _ in range(3):
                    free(args.iters, w)()
                torch.cuda.synchronize()
                passes[tag] = {name: round(ms * 1e3, 2) for name, ms, _ in p.pass_times()}
                p.profile(False)
        it, it_w, it_tv = (f_k - f_0) / args.iters, (f_kw - f_0) / args.iters, (t_k - t_0) / args.iters
        nbytes = (3 * BYTES_CHAIN + BYTES_SPATIAL) * n * n + BYTES_DATA * m * m
        row = {"window": "%dx%d" % (m, m), "us_per_iteration": round(it, 2), "us_per_iteration_weights": round(it_w, 2),
               "us_call_%d_iterations" % args.iters: round(f_k, 1), "us_call_0_iterations": round(f_0, 1), "bytes_per_iteration": nbytes,
               "implied_TBps": round(nbytes / (it * 1e-6) / 1e12, 3), "periodic_us_per_iteration": round(it_tv, 2),
               "iteration_over_periodic_iteration": round(it / it_tv, 2)}
        for tag, extra in (("", 0), ("_weights", 4)):
            da, sp = passes[tag].get(DATA_PASS, float("nan")), passes[tag].get(SPATIAL_PASS, float("nan"))
            d_rate, s_rate = (BYTES_DATA + extra) * m * m / (da * 1e-6) / 1e12, BYTES_SPATIAL * n * n / (sp * 1e-6) / 1e12
            row.update({"data_us" + tag: da, "data_TBps" + tag: round(d_rate, 3), "spatial_us" + tag: sp, "spatial_TBps" + tag: round(s_rate, 3),
                        "data_over_spatial_rate" + tag: round(d_rate / s_rate, 3)})
        row["pass_us"] = passes[""]
        out["sizes"]["%dx%d" % (n, n)] = row
        del d_in, d_w, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
