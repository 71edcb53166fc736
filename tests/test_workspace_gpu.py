"""The on-demand workspaces of a plan on the MI355X, all of them on one plan: every call that makes a workspace keeps its bits when
the workspaces around it are made, grown and used (three rounds on one 64 x 64 plan against fresh plans), and fdr_plan_destroy gives
every block back (three create / use / destroy cycles of a 1024 x 1024 plan against the device's free memory).  The layouts
themselves are checked without a device (test_workspace_host.py).  Cases print a `WS` line with their measured values (pytest -s)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
# Free memory lost per create / use / destroy cycle of the 1024 x 1024 plan.  Measured on the parent commit, whose fdr_plan_destroy
# named every block: 0 bytes in each of the three cycles, in two runs.  The smallest block such a plan makes with a plane in it is
# one M x N float plane, 4 MiB (the blind call's weights); half of it is the margin, so one such block lost per cycle shows.
PARENT_DRIFT = 0
LEAK_BOUND = PARENT_DRIFT + 2 * MIB


def _scene(M, N, rows, cols, seed=5):
    """a smooth positive picture and a second exposure of it (>= 0.05), weights with a hole, the PSFs"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    base = 0.5 + 0.3 * np.sin(x * (6.0 / cols)) * np.cos(y * (5.0 / rows)) + 0.1 * (((x // 8) + (y // 8)) % 2)
    imgs = [np.maximum(base * g + 0.02 * rng.standard_normal((rows, cols)), 0.05).astype(np.float32) for g in (1.0, 0.8, 1.2, 0.9)]
    w = np.ones((rows, cols), dtype=np.float32)
    w[rows // 3:rows // 3 + 4, cols // 2:cols // 2 + 5] = 0.0
    psfs = []
    for k in range(4):
        yy, xx = np.mgrid[-2:3, -2 - k % 2:3 + k % 2].astype(np.float64)
        g = np.exp(-(yy * yy + xx * xx) / (2.0 * (1.0 + 0.3 * k) ** 2))
        psfs.append((g / g.sum()).astype(np.float32))
    return imgs, w, psfs


def _calls(fdr, imgs, w, psfs, iters=3):
    """(name, run(plan) -> arrays): one call per workspace of a plan, in the order they are touched"""
    img = imgs[0]

    def frames(p, n):
        p.set_frame_psfs([np.pad(q, ((0, 0), (0, 7 - q.shape[1]))) for q in psfs[:n]])
        return imgs[:n]

    def auto(p):
        out, res, trace = p.richardson_lucy_auto(img, iters + 1, rule=fdr.RL_STOP_RESIDUAL, sigma=1e-4, free_boundary=True, weights=w)
        return [out, trace, np.array([res.iterations_done, res.stopped, res.sigma, res.target, res.statistic], dtype=np.float64)]

    def blind(p):
        out, psf = p.richardson_lucy_blind(img, psfs[1], iters, free_boundary=True, weights=w)
        return [out, psf]

    return [
        ("TV", lambda p: [p.tv_deconv(img, 20.0, iterations=iters)]),
        ("free TV", lambda p: [p.tv_deconv_free(img, 20.0, iterations=iters, weights=w)]),
        ("auto TV", lambda p: list(p.tv_deconv_auto(img, sigma=0.02, iterations=iters, weights=w)[::2])),
        ("Poisson TV", lambda p: [p.tv_deconv_poisson(img, 50.0, iterations=iters, weights=w, background=0.01)]),
        ("RL free", lambda p: [p.richardson_lucy_free(img, iters, weights=w)]),
        ("RL accelerated", lambda p: list(p.richardson_lucy(img, iters + 2, accelerate=True, return_alphas=True))),
        ("RL-TV", lambda p: [p.richardson_lucy_tv(img, iters, 0.002)]),
        ("RL auto with weights", auto),
        ("blind free-boundary", blind),
        ("motion estimate", lambda p: [p.estimate_motion(img, scores=True)[1]]),
        ("defocus estimate", lambda p: [p.estimate_defocus(img, return_profile=True)[1]]),
        ("choose regularisation", lambda p: [np.array(tuple(p.choose_regularisation(img, sigma=0.02)), dtype=np.float64)]),
        ("frames RL", lambda p: [p.richardson_lucy_frames(frames(p, 2), iters, weights=w, tv_lambda=0.002)]),
        ("frames TV", lambda p: [p.tv_deconv_frames(frames(p, 2), 20.0, iters, weights=w)]),
    ]


def _round(p, calls, psf):
    """every call of the list on the plan, each from the same operator PSF (the blind call leaves its own)"""
    out = {}
    for name, run in calls:
        p.set_operator_psf(psf)
        out[name] = [np.array(a, copy=True) for a in run(p)]
    return out


def _grow(fdr, p, imgs, w, psfs, iters=2):
    """the workspaces that can grow, grown: groups of 3, 4 frames, a finer angle step, an internal trace of more steps"""
    import torch
    p.set_operator_psf(psfs[0])
    p.set_batching(1, 3)
    three = np.stack(imgs[:3])
    outs = [p.tv_deconv_batch(three, 20.0, iterations=iters),
            p.tv_deconv_free_batch(three, 20.0, iterations=iters, weights=w),
            p.tv_deconv_auto_batch(three, sigma=0.02, iterations=iters, weights=w)[0],
            p.tv_deconv_poisson_batch(three, 50.0, iterations=iters, weights=w, background=0.01),
            p.richardson_lucy_batch(three, iters, free_boundary=True, weights=w),
            p.richardson_lucy_batch(three, iters + 2, accelerate=True),
            p.richardson_lucy_batch(three, iters + 2, free_boundary=True, weights=w, accelerate=True),
            p.richardson_lucy_tv_batch(three, iters, 0.002),
            p.richardson_lucy_tv_batch(three, iters, 0.002, free_boundary=True, weights=w)]
    p.set_frame_psfs([np.pad(q, ((0, 0), (0, 7 - q.shape[1]))) for q in psfs])
    outs.append(p.richardson_lucy_frames(imgs, iters, weights=w, tv_lambda=0.002))
    outs.append(p.tv_deconv_frames(imgs, 20.0, iters, weights=w))
    p.set_batching(1, 1)
    outs.append(p.estimate_motion(imgs[0], angle_step=0.25, scores=True)[1])
    # a rule and no trace of the caller's: the internal trace, for more steps than the 1024 it starts with (the large sigma stops it at
    # the first look)
    rows, cols = imgs[0].shape
    d_in = torch.from_numpy(imgs[0]).cuda()
    d_out = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    res = p.richardson_lucy_auto_dev(d_in.data_ptr(), rows, cols, cols, d_out.data_ptr(), cols, 1500, rule=fdr.RL_STOP_RESIDUAL, sigma=10.0)
    torch.cuda.synchronize()
    assert res.stopped and res.iterations_done < 1500, res
    outs.append(d_out.cpu().numpy())
    assert all(np.all(np.isfinite(o)) for o in outs)


def test_every_workspace_keeps_its_bits_through_growth(fdr):
    M = N = 64
    imgs, w, psfs = _scene(M, N, 40, 48)
    calls = _calls(fdr, imgs, w, psfs)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        first = _round(p, calls, psfs[0])
        _grow(fdr, p, imgs, w, psfs)
        third = _round(p, calls, psfs[0])
    for name, run in calls:
        with fdr.Plan(M, N, fdr.MODE_FAST) as fresh:
            alone = _round(fresh, [(name, run)], psfs[0])[name]
        for a, b, c in zip(first[name], third[name], alone):
            assert a.size and np.all(np.isfinite(a)), name
            assert a.tobytes() == b.tobytes(), "%s: not the bits of the first round after the workspaces grew" % name
            assert a.tobytes() == c.tobytes(), "%s: not the bits of the call on a fresh plan" % name
    print("WS %d calls, %d arrays: three rounds and fresh plans bit-identical" % (len(calls), sum(len(v) for v in first.values())))


def plan_cycles(fdr, cycles=3, M=1024, N=1024):
    """(free device memory before, and after each of `cycles` create / use / destroy rounds of an M x N plan that makes every
    workspace, after one small round, which loads every kernel; the least free memory seen while such a plan was alive)"""
    import torch
    small = _scene(64, 64, 40, 48)
    with fdr.Plan(64, 64, fdr.MODE_FAST) as p:
        _round(p, _calls(fdr, *small, iters=1), small[2][0])
        _grow(fdr, p, *small, iters=1)
    imgs, w, psfs = _scene(M, N, 200, 240)
    calls = _calls(fdr, imgs, w, psfs, iters=1)
    torch.cuda.synchronize()
    free, alive = [torch.cuda.mem_get_info()[0]], []
    for _ in range(cycles):
        with fdr.Plan(M, N, fdr.MODE_FAST) as p:
            _round(p, calls, psfs[0])
            _grow(fdr, p, imgs, w, psfs, iters=1)
            torch.cuda.synchronize()
            alive.append(torch.cuda.mem_get_info()[0])
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    return free, min(alive)


def test_plan_destroy_gives_every_block_back(fdr):
    free, alive = plan_cycles(fdr)
    drift = [a - b for a, b in zip(free, free[1:])]
    print("WS free memory %s MiB (%.1f with the plan alive), lost per cycle %s bytes (bound %d)" %
          (["%.1f" % (f / MIB) for f in free], alive / MIB, drift, LEAK_BOUND))
    # the measurement sees the plan's blocks at all: the workspaces' 65 M x N float planes alone (18 TV, 6 free TV, 8 multi-frame TV, 7
    # + 9 + 6 + 2 of the Richardson-Lucy forms, 6 of the frames, the blind weights, the motion estimate's complex plane) are 260 MiB
    assert free[0] - alive >= 260 * MIB, (free[0], alive)
    assert max(drift) <= LEAK_BOUND, drift
