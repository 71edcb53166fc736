#!/usr/bin/env python3
"""Noise-constrained TV (the free-boundary ADMM iteration with mu chosen per step) iteration cost on one GPU: prints one JSON line.

For each plan (1024^2, 4096^2, 8192^2; motion 15/30 PSF; the window is the plan less the PSF's reach, n - 14 square, a dense random
image, so its rows have no 16-byte alignment): the device time of fdr_tv_deconv_auto_f32_dev with `iters` iterations minus the time
with 0 (hipEvents around each call, median of `reps` after warm-up) divided by `iters` is one iteration, without weights and with a
0 / 1 mask; fdr_tv_deconv_free_f32_dev on the same plan and window, with the same nu, is timed the same way in the same run.  The
passes of profiled calls (fdr_plan_pass_times) give the time of the norm and mu launches (one name: the norm kernel's 12 bytes per
window pixel, 16 with weights, and the single-workgroup fold behind it -- the rate printed is therefore a lower bound of the norm
kernel's own) and of the auto data kernel, beside the free call's data kernel and the rate of its 20 bytes per window pixel (24 with
weights) in the same run.

usage: tools/tv_auto_bench.py [--iters 10] [--reps 20] [--sizes 1024,4096,8192]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rl_bench import timed  # noqa: E402

BYTES_NORM = 12  # c 4 + q 4 + d 4 in, per window pixel; the weights add 4
BYTES_DATA = 20  # c 4 + q 4 + d 4 in, q 4 + r 4 out, per window pixel; the weights add 4
NORM_PASS = "TVA norm+mu: res_e, res_c, S -> mu_k"
AUTO_DATA_PASS = "TVA data: s, q, r = 2s-e (mu_k)"
FREE_DATA_PASS = "TVF data: s, q, r = 2s-e (window)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--rho", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    nu = fdr.TV_AUTO_NU_RATIO * args.rho
    out = {"metric": "tv_auto_admm_us_per_iteration", "iters": args.iters, "reps": args.reps, "sigma": args.sigma, "rho": args.rho, "nu": nu, "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        m = n - 14
        d_in = torch.rand((m, m), device="cuda", dtype=torch.float32)
        d_w = (torch.rand((m, m), device="cuda", dtype=torch.float32) > 0.02).to(torch.float32)
        d_out = torch.empty((m, m), device="cuda", dtype=torch.float32)
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)

            def auto(k, w=None):
                return lambda: p.tv_deconv_auto_dev(d_in.data_ptr(), m, m, m, d_out.data_ptr(), m, args.sigma, args.rho, k, w, m, stream=stream)

            def free(k, w=None):
                return lambda: p.tv_deconv_free_dev(d_in.data_ptr(), m, m, m, d_out.data_ptr(), m, 100.0, args.rho, k, w, m, nu, stream=stream)
            # alternating, so that a drift of the clocks falls on both
            a_k, f_k = timed(torch, auto(args.iters), args.reps), timed(torch, free(args.iters), args.reps)
            a_0, f_0 = timed(torch, auto(0), args.reps), timed(torch, free(0), args.reps)
            a_kw, f_kw = timed(torch, auto(args.iters, d_w.data_ptr()), args.reps), timed(torch, free(args.iters, d_w.data_ptr()), args.reps)
            passes = {}
            for tag, w in (("", None), ("_weights", d_w.data_ptr())):
                p.profile(True)
                for _ in range(3):
                    auto(args.iters, w)()
                    free(args.iters, w)()
                torch.cuda.synchronize()
                passes[tag] = {name: round(ms * 1e3, 2) for name, ms, _ in p.pass_times()}
                p.profile(False)
        it_a, it_f = (a_k - a_0) / args.iters, (f_k - f_0) / args.iters
        it_aw, it_fw = (a_kw - a_0) / args.iters, (f_kw - f_0) / args.iters
        row = {"window": "%dx%d" % (m, m), "us_per_iteration": round(it_a, 2), "us_per_iteration_weights": round(it_aw, 2),
               "free_us_per_iteration": round(it_f, 2), "free_us_per_iteration_weights": round(it_fw, 2),
               "iteration_over_free_iteration": round(it_a / it_f, 3), "iteration_over_free_iteration_weights": round(it_aw / it_fw, 3)}
        for tag, extra in (("", 0), ("_weights", 4)):
            no, ad, fd = (passes[tag].get(k, float("nan")) for k in (NORM_PASS, AUTO_DATA_PASS, FREE_DATA_PASS))
            n_rate, a_rate, f_rate = ((b + extra) * m * m / (t * 1e-6) / 1e12 for b, t in ((BYTES_NORM, no), (BYTES_DATA, ad), (BYTES_DATA, fd)))
            row.update({"norm_mu_us" + tag: no, "norm_TBps" + tag: round(n_rate, 3), "auto_data_us" + tag: ad, "auto_data_TBps" + tag: round(a_rate, 3),
                        "free_data_us" + tag: fd, "free_data_TBps" + tag: round(f_rate, 3), "norm_over_free_data_rate" + tag: round(n_rate / f_rate, 3)})
        row["pass_us"] = passes[""]
        out["sizes"]["%dx%d" % (n, n)] = row
        del d_in, d_w, d_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
