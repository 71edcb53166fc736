#!/usr/bin/env python3
"""Total-variation (ADMM) iteration cost on one GPU: prints one JSON line.

For each plan (1024^2, 4096^2, 8192^2; full-plane random image, motion 15/30 PSF): the device time of fdr_tv_deconv_f32_dev with
`iters` iterations minus the time with 0 (hipEvents around each call, median of `reps` after warm-up) divided by `iters` is one
iteration (the one adjoint blur that builds b is spread over the iterations); the algorithmic bytes of an iteration (80 per padded
pixel: spatial kernel 28, solve 52) give the rate it implies.  A Richardson-Lucy iteration and
fdr_wiener_f32_dev on the same plan and image are timed the same way in the same run.  The passes of one profiled call
(fdr_plan_pass_times) give the spatial kernel's own time and the rate of its 28 bytes per pixel.

usage: tools/tv_bench.py [--iters 10] [--reps 20] [--sizes 1024,4096,8192]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rl_bench import timed  # noqa: E402

BYTES_SPATIAL = 28  # x 4 + w 8 + b 4 in, w 8 + rhs 4 out
BYTES_SOLVE = 52    # A 16, B' with its table 24, C 12
SPATIAL_PASS = "TV spatial: shrink+dual+div"


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
    out = {"metric": "tv_admm_us_per_iteration", "iters": args.iters, "reps": args.reps, "mu": args.mu, "rho": args.rho,
           "bytes_per_padded_pixel": BYTES_SPATIAL + BYTES_SOLVE, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        d_in = torch.rand((n, n), device="cuda", dtype=torch.float32)
        d_out = torch.empty_like(d_in)
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)
            p.set_psf_motion(15, 30.0, 0.01, stream=stream)

            def tv(k, aniso=False):
                return lambda: p.tv_deconv_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, args.mu, args.rho, k, aniso, stream=stream)

            def rl(k):
                return lambda: p.richardson_lucy_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, fdr.NORM_NONE, stream=stream)
            t_k, t_0 = timed(torch, tv(args.iters), args.reps), timed(torch, tv(0), args.reps)
            t_ka = timed(torch, tv(args.iters, True), args.reps)
            r_k, r_0 = timed(torch, rl(args.iters), args.reps), timed(torch, rl(0), args.reps)
            t_w = timed(torch, lambda: p.wiener_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, fdr.NORM_PADDED, stream=stream), args.reps)
            p.profile(True)
            for _ in range(3):
                tv(args.iters)()
            torch.cuda.synchronize()
            passes = {name: round(ms * 1e3, 2) for name, ms, _ in p.pass_times()}
            p.profile(False)
        it, it_a, it_rl = (t_k - t_0) / args.iters, (t_ka - t_0) / args.iters, (r_k - r_0) / args.iters
        nbytes = (BYTES_SPATIAL + BYTES_SOLVE) * n * n
        sp = passes.get(SPATIAL_PASS, float("nan"))
        out["sizes"]["%dx%d" % (n, n)] = {
            "us_per_iteration": round(it, 2), "us_per_iteration_anisotropic": round(it_a, 2), "us_call_%d_iterations" % args.iters: round(t_k, 1),
            "us_call_0_iterations": round(t_0, 1), "bytes_per_iteration": nbytes, "implied_TBps": round(nbytes / (it * 1e-6) / 1e12, 3),
            "spatial_us": sp, "spatial_TBps": round(BYTES_SPATIAL * n * n / (sp * 1e-6) / 1e12, 3), "rl_us_per_iteration": round(it_rl, 2),
            "iteration_over_rl_iteration": round(it / it_rl, 2), "wiener_us": round(t_w, 1), "pass_us": passes}
        del d_in, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
