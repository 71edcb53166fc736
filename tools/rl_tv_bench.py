#!/usr/bin/env python3
"""Cost of a Richardson-Lucy iteration with the total-variation prior on one GPU: prints one JSON line and writes it to
profiles/rl_tv_bench.json.

For each plan (1024^2, 4096^2, 8192^2; full-plane random image, motion 15/30 PSF), in one run: the device time of
fdr_richardson_lucy_tv_f32_dev with `iters` iterations minus the time with 0 (hipEvents around each call, median of `reps` after
warm-up) divided by `iters` is one regularised iteration, of the plain and of the free-boundary form (lambda = 0.01, eps = 1e-3);
the unregularised iteration of both forms is timed the same way, and the ratio of the two is set against the ratio of their
algorithmic bytes (76 / 64 and 80 / 68 per padded pixel): the check is ratio <= 1.15 x the byte ratio.  The
factor kernel alone (fdr_rl_tv_factor_f32_dev, with and without w) gives its own time and the rate of its 8 / 12 bytes per
pixel; tv_spatial_kernel's rate comes from the pass times of one profiled fdr_tv_deconv_f32_dev call (28 bytes per pixel), and the
factor kernel is held to 0.8 of it at 4096^2.  --passes adds the per-pass device times of one regularised call of each form.

usage: tools/rl_tv_bench.py [--iters 10] [--reps 20] [--sizes 1024,4096,8192] [--passes] [--no-write]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rl_bench import BYTES_PER_PIXEL, FREE_BYTES_PER_PIXEL, timed  # noqa: E402
from tv_bench import BYTES_SPATIAL, SPATIAL_PASS  # noqa: E402

TV_BYTES_PER_PIXEL = BYTES_PER_PIXEL + 8 + 4            # the factor kernel u in, factor out; the update reads the factor
TV_FREE_BYTES_PER_PIXEL = FREE_BYTES_PER_PIXEL + 12      # the factor kernel reads u and wgt and writes the factor, which the update reads in wgt's place
FACTOR_BYTES, FACTOR_W_BYTES = 8, 12
LAMBDA, EPS = 0.01, 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--passes", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"metric": "richardson_lucy_tv_us_per_iteration", "iters": args.iters, "reps": args.reps, "lambda": LAMBDA, "eps": EPS,
           "bytes_per_padded_pixel": {"plain": BYTES_PER_PIXEL, "tv": TV_BYTES_PER_PIXEL, "free": FREE_BYTES_PER_PIXEL, "tv_free": TV_FREE_BYTES_PER_PIXEL},
           "csrc": fdr.csrc_fingerprint(), "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        d_in = torch.rand((n, n), device="cuda", dtype=torch.float32) + 0.05
        d_out = torch.empty_like(d_in)
        d_w = torch.rand((n, n), device="cuda", dtype=torch.float32)
        with fdr.Plan(n, n, fdr.MODE_FAST) as p:
            p.set_operator_psf_motion(15, 30.0, stream=stream)

            def rl(k):
                return lambda: p.richardson_lucy_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, fdr.NORM_NONE, stream=stream)

            def free(k):
                return lambda: p.richardson_lucy_free_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, norm_area=fdr.NORM_NONE, stream=stream)

            def tv(k, fb):
                return lambda: p.richardson_lucy_tv_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, k, LAMBDA, EPS, free_boundary=fb,
                                                        norm_area=fdr.NORM_NONE, stream=stream)

            def per_iteration(f):
                return (timed(torch, f(args.iters), args.reps) - timed(torch, f(0), args.reps)) / args.iters
            it_rl, it_free = per_iteration(rl), per_iteration(free)
            it_tv, it_tvf = per_iteration(lambda k: tv(k, False)), per_iteration(lambda k: tv(k, True))
            t_f = timed(torch, lambda: fdr.rl_tv_factor_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, LAMBDA, EPS, stream=stream), args.reps)
            t_fw = timed(torch, lambda: fdr.rl_tv_factor_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, LAMBDA, EPS, d_w=d_w.data_ptr(),
                                                             stream=stream), args.reps)
            p.profile(True)
            for _ in range(3):
                p.tv_deconv_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, 500.0, 2.0, args.iters, False, stream=stream)
            torch.cuda.synchronize()
            sp = {name: ms * 1e3 for name, ms, cnt in p.pass_times() if cnt}.get(SPATIAL_PASS, float("nan"))
            passes = None
            if args.passes:
                passes = {}
                for fb in (False, True):
                    tv(args.iters, fb)()
                    torch.cuda.synchronize()
                    passes["free" if fb else "plain"] = {name: {"mean_us": round(ms * 1e3, 2), "launches": cnt} for name, ms, cnt in p.pass_times() if cnt}
            p.profile(False)
        px = n * n
        tbps = lambda nbytes, us: round(nbytes * px / (us * 1e-6) / 1e12, 3)  # noqa: E731
        r = {"tv_us_per_iteration": round(it_tv, 2), "plain_us_per_iteration": round(it_rl, 2), "tv_over_plain": round(it_tv / it_rl, 3),
             "byte_ratio_plain": round(TV_BYTES_PER_PIXEL / BYTES_PER_PIXEL, 3),
             "tv_over_plain_within_1.15x_bytes": bool(it_tv / it_rl <= 1.15 * TV_BYTES_PER_PIXEL / BYTES_PER_PIXEL),
             "tv_free_us_per_iteration": round(it_tvf, 2), "free_us_per_iteration": round(it_free, 2), "tv_free_over_free": round(it_tvf / it_free, 3),
             "byte_ratio_free": round(TV_FREE_BYTES_PER_PIXEL / FREE_BYTES_PER_PIXEL, 3),
             "tv_free_over_free_within_1.15x_bytes": bool(it_tvf / it_free <= 1.15 * TV_FREE_BYTES_PER_PIXEL / FREE_BYTES_PER_PIXEL),
             "tv_implied_TBps": tbps(TV_BYTES_PER_PIXEL, it_tv), "tv_free_implied_TBps": tbps(TV_FREE_BYTES_PER_PIXEL, it_tvf),
             "factor_us": round(t_f, 2), "factor_TBps": tbps(FACTOR_BYTES, t_f), "factor_w_us": round(t_fw, 2), "factor_w_TBps": tbps(FACTOR_W_BYTES, t_fw),
             "tv_spatial_us": round(sp, 2), "tv_spatial_TBps": tbps(BYTES_SPATIAL, sp),
             "factor_over_tv_spatial_rate": round(tbps(FACTOR_BYTES, t_f) / tbps(BYTES_SPATIAL, sp), 3),
             "factor_w_over_tv_spatial_rate": round(tbps(FACTOR_W_BYTES, t_fw) / tbps(BYTES_SPATIAL, sp), 3)}
        if passes is not None:
            r["passes"] = passes
        out["sizes"]["%dx%d" % (n, n)] = r
        del d_in, d_out, d_w
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, "profiles", "rl_tv_bench.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
