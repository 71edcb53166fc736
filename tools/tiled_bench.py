#!/usr/bin/env python3
"""Sectioned restoration on one GPU: prints one JSON line.

For each picture size n (default 4096) and each method (free-boundary Richardson-Lucy, free-boundary TV): the device time of
fdr_restore_tiled_f32_dev (tiles of --tile pixels, --overlap shared, `iters` iterations, launch groups of --group tiles; hipEvents
around each call, median of `reps` after warm-up) beside the whole-picture free call of the method on the plan that holds the
picture and the PSF's reach (sizes where that plan exists).  The blend kernel's own time comes from fdr_plan_pass_times of one
profiled tiled call, its rate from 4 bytes read per covering tile and 4 written per pixel (the coverage is counted from the layout),
beside the TV spatial kernel (28 bytes per pixel) timed in the same run on an n x n plan.  --beyond adds one tiled call on a picture
no plan holds (default 12288^2, TV).

usage: tools/tiled_bench.py [--sizes 4096] [--tile 1024] [--overlap 64] [--iters 10] [--reps 5] [--group 4] [--blend-sizes 4096,8192] [--beyond 12288]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLEND = "T blend: tiles -> picture"
SPATIAL = "TV spatial: shrink+dual+div (free)"


def timed(torch, fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))  # ms
    return statistics.median(ts)


def coverage(n, lay):
    """mean number of tiles that cover a pixel of an n x n picture"""
    return (lay.tiles_r * lay.win_rows / n) * (lay.tiles_c * lay.win_cols / n)


class Tiled:
    def __init__(self, fdr, torch, n, method, tile, overlap, iters, psf):
        self.prm = fdr.TiledParams.make(method, tile, overlap, iters, fdr.RL_SIGMA, 200.0, 2.0)
        self.lay = fdr.tiled_layout(n, n, psf.shape[0], psf.shape[1], self.prm)
        self.d_in = torch.rand((n, n), device="cuda", dtype=torch.float32) + 0.05
        self.d_out = torch.empty_like(self.d_in)
        self.d_work = torch.empty(self.lay.work_bytes + 256, dtype=torch.uint8, device="cuda")
        self.work = (self.d_work.data_ptr() + 255) & ~255
        self.d_psf = torch.from_numpy(psf).cuda()
        self.n, self.psf, self.fdr = n, psf, fdr

    def run(self, p, stream):
        pr, pc = self.psf.shape
        p.restore_tiled_dev(self.d_in.data_ptr(), self.n, self.n, self.n, self.d_psf.data_ptr(), pr * pc, 1, pr, pc, pc, self.d_out.data_ptr(),
                            self.n, self.prm, self.work, self.lay.work_bytes, stream=stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096")
    ap.add_argument("--blend-sizes", default="4096,8192")
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--beyond", type=int, default=12288)
    args = ap.parse_args()
    import torch
    fdr = importlib.import_module("parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd")
    stream = torch.cuda.current_stream().cuda_stream
    psf = fdr.motionBlurKernel(15, 30.0)
    methods = (("rl", fdr.TILED_RL_FREE), ("tv", fdr.TILED_TV_FREE))
    out = {"metric": "tiled_restoration_ms", "tile": args.tile, "overlap": args.overlap, "iters": args.iters, "reps": args.reps, "group": args.group,
           "sizes": {}, "blend": {}}
    for n in (int(s) for s in args.sizes.split(",") if s):
        res = {}
        for name, method in methods:
            t = Tiled(fdr, torch, n, method, args.tile, args.overlap, args.iters, psf)
            with fdr.Plan(t.lay.min_M, t.lay.min_N, fdr.MODE_FAST) as p:
                p.set_batching(1, args.group)
                res[name] = {"tiled_ms": round(timed(torch, lambda: t.run(p, stream), args.reps), 3), "tiles": t.lay.tiles_r * t.lay.tiles_c,
                             "tile_plan": [t.lay.min_M, t.lay.min_N]}
            M = fdr.nextPowerOfTwo(n + psf.shape[0] - 1)
            if M <= 8192:
                with fdr.Plan(M, M, fdr.MODE_FAST) as p:
                    p.set_operator_psf(psf)
                    if method == fdr.TILED_RL_FREE:
                        whole = lambda: p.richardson_lucy_free_dev(t.d_in.data_ptr(), n, n, n, t.d_out.data_ptr(), n, args.iters, stream=stream)  # noqa: E731
                    else:
                        whole = lambda: p.tv_deconv_free_dev(t.d_in.data_ptr(), n, n, n, t.d_out.data_ptr(), n, 200.0, 2.0, args.iters, stream=stream)  # noqa: E731
                    res[name]["whole_ms"] = round(timed(torch, whole, args.reps), 3)
                    res[name]["whole_plan"] = [M, M]
                    res[name]["tiled_over_whole"] = round(res[name]["tiled_ms"] / res[name]["whole_ms"], 3)
            del t
        out["sizes"]["%dx%d" % (n, n)] = res
    for n in (int(s) for s in args.blend_sizes.split(",") if s):
        t = Tiled(fdr, torch, n, fdr.TILED_RL_FREE, args.tile, args.overlap, 0, psf)
        with fdr.Plan(t.lay.min_M, t.lay.min_N, fdr.MODE_FAST) as p:
            p.set_batching(1, args.group)
            t.run(p, stream)
            torch.cuda.synchronize()
            p.profile(True)
            for _ in range(args.reps):
                t.run(p, stream)
            torch.cuda.synchronize()
            blend_ms = {nm: ms for nm, ms, c in p.pass_times() if c}[BLEND]
        cover = coverage(n, t.lay)
        del t
        entry = {"blend_us": round(blend_ms * 1e3, 1), "coverage": round(cover, 4), "bytes_per_pixel": round(4 * cover + 4, 3),
                 "blend_TBps": round((4 * cover + 4) * n * n / (blend_ms * 1e-3) / 1e12, 3)}
        if n <= 8192:  # the TV spatial kernel on an n x n plan, in the same run
            d_in = torch.rand((n, n), device="cuda", dtype=torch.float32) + 0.05
            d_out = torch.empty_like(d_in)
            with fdr.Plan(n, n, fdr.MODE_FAST) as p:
                p.set_operator_psf(psf)
                p.tv_deconv_free_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, 200.0, 2.0, 1, stream=stream)
                torch.cuda.synchronize()
                p.profile(True)
                p.tv_deconv_free_dev(d_in.data_ptr(), n, n, n, d_out.data_ptr(), n, 200.0, 2.0, args.reps, stream=stream)
                torch.cuda.synchronize()
                sp_ms = {nm: ms for nm, ms, c in p.pass_times() if c}[SPATIAL]
            del d_in, d_out
            entry.update({"tv_spatial_us": round(sp_ms * 1e3, 1), "tv_spatial_TBps": round(28.0 * n * n / (sp_ms * 1e-3) / 1e12, 3)})
            entry["blend_over_tv_spatial_rate"] = round(entry["blend_TBps"] / entry["tv_spatial_TBps"], 3)
        out["blend"]["%dx%d" % (n, n)] = entry
    if args.beyond > 0:
        n = args.beyond
        t = Tiled(fdr, torch, n, fdr.TILED_TV_FREE, args.tile, args.overlap, args.iters, psf)
        with fdr.Plan(t.lay.min_M, t.lay.min_N, fdr.MODE_FAST) as p:
            p.set_batching(1, args.group)
            ms = timed(torch, lambda: t.run(p, stream), max(1, args.reps // 2))
        out["beyond"] = {"size": [n, n], "method": "tv", "tiles": t.lay.tiles_r * t.lay.tiles_c, "tiled_ms": round(ms, 2),
                         "work_MiB": round(t.lay.work_bytes / 2 ** 20, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
