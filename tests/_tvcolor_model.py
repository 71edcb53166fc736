"""float64 model of batched and colour total-variation deconvolution (fdr_tv_deconv_batch_f32*; include/fdr.h),
on the pieces of _tv_model.py.

Uncoupled, every image runs the iteration of _tv_model.py on its own.  Coupled (vectorial TV, FDR_TV_COUPLE_CHANNELS) the images are
the channels of one picture, TV(x) = sum over pixels of sqrt(sum over c of |grad x_c|^2), and one step of the iteration changes:

    m = sqrt(sum over c of gx_c^2 + gy_c^2), c = 0, 1, .. in that order;  s = m > t ? 1 - t / m : 0;  z_c = s g_c

b, the duals, v, the divergence, the solve with the one table, the clamp and the normalisation stay per channel.

Pinned in test_tvcolor_host.py (against tv_model, the proximal map, convergence, invariants, the float32 class, injected faults,
restoration quality) before it judges the GPU (test_tvcolor_gpu.py).  The GPU is held to TV_TOL of _tv_model.py: the coupled
iteration is of the same arithmetic class (the shrinkage is continuous at its threshold), so no new tolerance is introduced.
Largest errors of one run of test_tvcolor_gpu.py on an MI355X, max |got - model| / max |model| (normalised outputs: max-abs), per
plan, uncoupled / coupled: 8 x 32 1.9e-6 / 1.8e-6, 16 x 512 5.8e-6 / 4.7e-6, 64 x 256 6.4e-6 / 7.2e-6, 256 x 32 5.0e-6 / 5.4e-6,
128 x 512 with the window 100 x 333 5.7e-6 / 7.3e-6 (MEASURED_UNCOUPLED, MEASURED_COUPLED below: the maxima).  The same model in
float32 / complex64 on the CPU lies 1.2e-6 (n = 3) to 2.3e-6 (n = 100) from its float64 form (test_tvcolor_host.py)."""
import numpy as np

from _rl_model import NORM_CROPPED, NORM_NONE, NORM_PADDED, normalize, op_spectrum  # noqa: F401
from _tv_model import TV_TOL, dx, dxT, dy, dyT, shrink, solve_table  # noqa: F401

MEASURED_UNCOUPLED = 6.42e-6  # 64 x 256, see the docstring; nothing asserts on these two: TV_TOL is the bound
MEASURED_COUPLED = 7.27e-6    # 128 x 512, window 100 x 333, three channels

FAULTS = ("channelwise", "first_channel", "halo_own_norm", "sum_no_sqrt")


def tile_shape(M, N):
    """(rows, columns) of a workgroup's tile of the spatial kernels: 4 TY x 4 TX, TX = min(64, N / 4), TY = min(256 / TX, M / 4)"""
    TX = min(64, N // 4)
    TY = min(256 // TX, M // 4)
    return 4 * TY, 4 * TX


def joint_scale(gx, gy, t, fault=None):
    """s of the joint shrinkage from gx, gy [C, M, N]: one M x N plane (per channel, [C, M, N], for the channel-wise fault)"""
    dtype = gx.dtype
    if fault == "channelwise":
        m = np.sqrt(gx * gx + gy * gy)
    else:
        m2 = gx[0] * gx[0] + gy[0] * gy[0]
        for c in range(1, gx.shape[0] if fault != "first_channel" else 1):
            m2 = m2 + (gx[c] * gx[c] + gy[c] * gy[c])
        m = m2 if fault == "sum_no_sqrt" else np.sqrt(m2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m > t, 1 - t / np.where(m > t, m, 1), 0).astype(dtype)


def joint_shrink(gx, gy, t, fault=None):
    """the proximal map of t * ||.||_2 on R^(2C) at every pixel: all channels shortened by one factor"""
    s = joint_scale(gx, gy, t, fault)
    return s * gx, s * gy


def tvcolor_iterates(d, psf, M, N, mu, rho=2.0, iterations=50, coupled=False, dtype=np.float64, fault=None, anisotropic=False):
    """yields (x, zx, zy) [C, M, N] of every iteration; dtype float32 runs the formulas in single precision, as tv_iterates does.
    fault (coupled only, for the CPU pins): 'channelwise' (every channel its own norm), 'first_channel' (the norm of channel 0 for
    all), 'sum_no_sqrt' (m^2 in place of m) and 'halo_own_norm': the divergence takes vx from the left and vy from above with the
    channel-wise norm where the spatial kernel recomputes them, at the columns and rows that begin a tile (tile_shape)."""
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    d = np.asarray(d, dtype=dtype)
    C, rows, cols = d.shape
    H = op_spectrum(psf, M, N)
    T = solve_table(H, M, N, mu, rho).astype(dtype)
    pad = np.zeros((C, M, N), dtype=dtype)
    pad[:, :rows, :cols] = d
    Hb = np.conj(H).astype(cdt)
    b = np.stack([(dtype(mu) * np.fft.irfft2(np.fft.rfft2(pad[c]).astype(cdt) * Hb, s=(M, N)).astype(dtype)).astype(dtype) for c in range(C)])
    x = pad.copy()
    wx = np.zeros((C, M, N), dtype=dtype)
    wy = np.zeros((C, M, N), dtype=dtype)
    t = dtype(1.0) / dtype(rho)
    th, tw = tile_shape(M, N)
    yield x, None, None
    for _ in range(iterations):
        gx = np.stack([dx(x[c]) for c in range(C)]) + wx
        gy = np.stack([dy(x[c]) for c in range(C)]) + wy
        if coupled:
            zx, zy = joint_shrink(gx, gy, t, None if fault == "halo_own_norm" else fault)
        else:
            z = [shrink(gx[c], gy[c], t, anisotropic) for c in range(C)]
            zx, zy = np.stack([q[0] for q in z]), np.stack([q[1] for q in z])
        wx, wy = gx - zx, gy - zy
        vx, vy = zx - wx, zy - wy
        left, up = np.roll(vx, 1, axis=2), np.roll(vy, 1, axis=1)  # Dx^T v = left - v, Dy^T v = up - v
        if coupled and fault == "halo_own_norm":
            ox, oy = joint_shrink(gx, gy, t, "channelwise")
            left[:, :, ::tw] = np.roll(ox - (gx - ox), 1, axis=2)[:, :, ::tw]
            up[:, ::th, :] = np.roll(oy - (gy - oy), 1, axis=1)[:, ::th, :]
        x_new = []
        for c in range(C):
            div = (left[c] - vx[c]) + (up[c] - vy[c])
            rhs = (b[c] + dtype(rho) * div).astype(dtype)
            x_new.append(np.fft.irfft2(np.fft.rfft2(rhs).astype(cdt) * T, s=(M, N)).astype(dtype))
        x = np.stack(x_new)
        yield x, zx, zy


def tvcolor_model(d, psf, M, N, mu, rho=2.0, iterations=50, coupled=False, nonneg=False, norm_area=NORM_NONE, dtype=np.float64, fault=None,
                  anisotropic=False):
    """the output of fdr_tv_deconv_batch_f32 on the windows d [C, rows, cols]: x on each window, max(x, 0) with nonneg, every image
    normalised by norm_area on its own; [C, rows, cols] float64"""
    _, rows, cols = np.asarray(d).shape
    x = None
    for x, _, _ in tvcolor_iterates(d, psf, M, N, mu, rho, iterations, coupled, dtype, fault, anisotropic):
        pass
    out = np.asarray(x[:, :rows, :cols], dtype=np.float64)
    if nonneg:
        out = np.maximum(out, 0)
    return np.stack([normalize(o, norm_area, M, N) for o in out])


def vtv_value(x):
    """vectorial TV of x [C, M, N]"""
    g2 = sum(dx(x[c]) ** 2 + dy(x[c]) ** 2 for c in range(x.shape[0]))
    return float(np.sum(np.sqrt(g2)))


def colour_blocks(M, N, C, seed=0):
    """float64 [C, M, N] piecewise-constant colour picture: rectangles of one geometry in every channel, each with a level of its
    own per channel, on per-channel pedestals; values in [0.1, 1]"""
    rng = np.random.default_rng(seed)
    img = np.empty((C, M, N))
    img[:] = rng.uniform(0.15, 0.35, C)[:, None, None]
    for _ in range(12):
        h, w = max(1, int(rng.uniform(0.08, 0.3) * M)), max(1, int(rng.uniform(0.08, 0.3) * N))
        r, c = int(rng.uniform(0.05, 0.9) * (M - h)), int(rng.uniform(0.05, 0.9) * (N - w))
        img[:, r:r + h, c:c + w] = rng.uniform(0.1, 1.0, C)[:, None, None]
    return img


def colour_images(M, N, rows, cols, C, seed):
    """float32 [C, rows, cols] for the GPU cases: the window of colour_blocks with texture above the thresholds used there
    (1 / rho >= 0.1) and negative pixels, as tv_image of test_tv_gpu.py"""
    rng = np.random.default_rng(seed)
    return (colour_blocks(M, N, C, seed)[:, :rows, :cols] + 0.2 * rng.random((C, rows, cols)) - 0.15).astype(np.float32)


# the plans of test_tvcolor_gpu.py, the smallest that reach each tile geometry: (M, N, rows, cols); rows None = the full plane
GPU_PLANS = [(8, 32, None, None),      # one tile that wraps onto itself
             (16, 512, None, None),    # two tiles across
             (64, 256, None, None),    # four tiles down
             (256, 32, None, None),    # TX = 8, TY = 32: the largest xs
             (128, 512, 100, 333)]     # a cropped window (centred PSF)
