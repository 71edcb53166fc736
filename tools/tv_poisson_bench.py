#!/usr/bin/env python3
"""Poisson-likelihood TV (the free-boundary ADMM iteration with the Poisson data step) against the free form on one GPU: prints one
JSON line.

For each plan (1024^2, 2048^2, 4096^2; motion 15/30 PSF; the window is the plan less the PSF's reach, n - 14 square, a dense random
non-negative image, so its rows have no 16-byte alignment): the device time of fdr_tv_deconv_poisson_f32_dev with `iters` iterations
minus the time with 0 (hipEvents around each call, median of `reps` after warm-up) divided by `iters` is one iteration, without
weights and with a 0 / 1 mask; fdr_tv_deconv_free_f32_dev on the same plan and window is timed the same way in the same run.  The
passes of profiled calls (fdr_plan_pass_times) give each data kernel's own time and the rate of its 20 bytes per window pixel (24
with weights).  Then, at the first size, batches: 3 and 4 images in one launch group against the loop of single calls, and the
coupled group of 3 against the uncoupled one.

usage: tools/tv_poisson_bench.py [--iters 10] [--reps 20] [--sizes 1024,2048,4096]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rl_bench import timed  # noqa: E402

BYTES_DATA = 20  # c 4 + q 4 + d 4 in, q 4 + r 4 out, per window pixel; the weights add 4
POISSON_PASS = "TVP data: Poisson s, q, r = 2s-e (window)"
FREE_PASS = "TVF data: s, q, r = 2s-e (window)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--mu", type=float, default=16.0)
    ap.add_argument("--rho", type=float, default=2.0)
    ap.add_argument("--background", type=float, default=0.02)
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"metric": "tv_poisson_admm_us_per_iteration", "iters": args.iters, "reps": args.reps, "mu": args.mu, "rho": args.rho,
           "background": args.background, "sizes": {}}
    sizes = [int(s) for s in args.sizes.split(",")]
    for n in sizes:
        m = n - 14
        d_in = torch.rand((m, m), device="cuda", dtype=torch.float32)
        d_w = (torch.rand((m, m), device="cuda", dtype=torch.float32) > 0.02).to(torch.float32)
        d_out = torch.empty((m, m), device="cuda", dtype=torch.float32)
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)

            def poisson(k, w=None):
                return lambda: p.tv_deconv_poisson_dev(d_in.data_ptr(), m, m, m, d_out.data_ptr(), m, args.mu, args.rho, k, w, m,
                                                       background=args.background, stream=stream)

            def free(k, w=None):
                return lambda: p.tv_deconv_free_dev(d_in.data_ptr(), m, m, m, d_out.data_ptr(), m, args.mu, args.rho, k, w, m, stream=stream)
            row = {"window": "%dx%d" % (m, m)}
            for name, call in (("poisson", poisson), ("free", free)):
                t_k, t_0 = timed(torch, call(args.iters), args.reps), timed(torch, call(0), args.reps)
                t_kw = timed(torch, call(args.iters, d_w.data_ptr()), args.reps)
                row[name + "_us_per_iteration"] = round((t_k - t_0) / args.iters, 2)
                row[name + "_us_per_iteration_weights"] = round((t_kw - t_0) / args.iters, 2)
            row["iteration_over_free_iteration"] = round(row["poisson_us_per_iteration"] / row["free_us_per_iteration"], 3)
            for name, call, pass_name in (("poisson", poisson, POISSON_PASS), ("free", free, FREE_PASS)):
                for tag, w, extra in (("", None, 0), ("_weights", d_w.data_ptr(), 4)):
                    p.profile(True)
                    for _ in range(3):
                        call(args.iters, w)()
                    torch.cuda.synchronize()
                    us = {nm: ms * 1e3 for nm, ms, _ in p.pass_times()}.get(pass_name, float("nan"))
                    p.profile(False)
                    row[name + "_data_us" + tag] = round(us, 2)
                    row[name + "_data_TBps" + tag] = round((BYTES_DATA + extra) * m * m / (us * 1e-6) / 1e12, 3)
            row["data_rate_over_free"] = round(row["poisson_data_TBps"] / row["free_data_TBps"], 3)
            row["data_rate_over_free_weights"] = round(row["poisson_data_TBps_weights"] / row["free_data_TBps_weights"], 3)
        out["sizes"]["%dx%d" % (n, n)] = row
        del d_in, d_w, d_out
    # groups: `count` images in one launch group against the loop of single calls; the coupled group against the uncoupled one
    n = sizes[0]
    m = n - 14
    out["groups"] = {"plan": "%dx%d" % (n, n), "window": "%dx%d" % (m, m)}
    for count in (3, 4):
        d_in = torch.rand((count, m, m), device="cuda", dtype=torch.float32)
        d_out = torch.empty((count, m, m), device="cuda", dtype=torch.float32)
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)

            def batch(k, group, coupled=False):
                def run():
                    p.set_batching(1, group)
                    p.tv_deconv_poisson_batch_dev(d_in.data_ptr(), m * m, count, m, m, m, d_out.data_ptr(), m * m, m, args.mu, args.rho, k,
                                                  background=args.background, coupled=coupled, stream=stream)
                return run
            g_k, g_0 = timed(torch, batch(args.iters, count), args.reps), timed(torch, batch(0, count), args.reps)
            l_k, l_0 = timed(torch, batch(args.iters, 1), args.reps), timed(torch, batch(0, 1), args.reps)
            grp, loop = (g_k - g_0) / args.iters, (l_k - l_0) / args.iters
            res = {"group_us_per_iteration": round(grp, 2), "loop_us_per_iteration": round(loop, 2), "group_over_loop": round(grp / loop, 3)}
            if count == 3:
                c_k, c_0 = timed(torch, batch(args.iters, count, True), args.reps), timed(torch, batch(0, count, True), args.reps)
                res["coupled_us_per_iteration"] = round((c_k - c_0) / args.iters, 2)
                res["coupled_over_group"] = round((c_k - c_0) / args.iters / grp, 3)
        out["groups"]["count_%d" % count] = res
        del d_in, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
