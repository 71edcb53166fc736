"""float64 / float32 model of multi-frame TV deconvolution (fdr_tv_deconv_frames_f32*; include/fdr.h): the
specification.

K frames d_k (rows x cols, all the same window at the plan's top-left corner) of one scene, each with its own PSF (H_k = DFT2 of PSF k
placed top-left in the M x N plan, sums NOT normalised) and its own weights m_k = pad(weights_k) (None: 1 on the window; one plane may
serve all frames).  One unknown x on the whole plan:

    minimise over x:  mu sum_k Phi_k(blur_k(x)) + TV(x)
      least squares:  Phi_k(s) = 1/2 sum m_k (s - pad(d_k))^2
      Poisson:        Phi_k(s) = sum m_k [ (s + b) - d_k+ log(s + b) ],   b >= 0 the known background

by ADMM with the splitting z = D x (dual w, penalty rho) and one splitting s_k = blur_k(x) per frame (duals q_k, penalty nu; nu = 0
selects rho):

    x = pad(d_0);  w = 0;  q_k = 0;  t = 1 / rho;  T = 1 / (nu sum_k |H_k|^2 + rho L);  n times:
        c_k = blur_k(x)
        e_k = c_k + q_k;  s_k = the data step of _tvfree_model.py / _tvpoisson_model.py with m_k;  q_k = e_k - s_k;  r_k = s_k - q_k
        b = sum_k blur_k^T(r_k)                                                  (ascending k)
        g = D x + w;  z = shrink(g, t);  w = g - z;  v = z - w
        x = IDFT2( DFT2(nu b + rho (Dx^T vx + Dy^T vy)) . T )

K = 1 is tvfree_iterates / tvpoisson_iterates, line by line.  Pinned in test_tvframes_host.py (those two, copies of one frame, the
normal equations, the objective from two starts, injected faults, quality) before it judges the GPU (test_tvframes_gpu.py).

Device against this model: max |got - model| / max |model| over the compared window (FDR_NORM_NONE) or max-abs (normalised outputs).
TVFR_TOL is at most 4x the largest value one run of test_tvframes_gpu.py measured on an MI355X, and that test also holds every case
within 10x of the float32 / complex64 CPU run of this model (dtype=np.float32) in the case's own metric.  Measured on the MI355X,
largest over n in {0, 1, 2, 10, 30}, both output windows, the three norm_area and the two data-term combinations of the case (in
brackets the float32 CPU run of the same output):
  8x32 win 8x32:      K=1 8.5e-7 (7.1e-7), K=2 4.7e-6 (2.7e-6), K=3 2.0e-6 (1.3e-6), K=5 1.5e-6 (6.5e-7), K=8 3.5e-6 (2.6e-6)
  16x32 win 9x30:     K=1 2.0e-6 (6.8e-7), K=2 1.7e-6 (7.4e-7), K=3 1.1e-6 (4.8e-7), K=5 4.7e-6 (1.5e-6), K=8 2.1e-6 (8.6e-7)
  64x128 win 37x101:  K=1 6.0e-6 (3.5e-6), K=2 5.5e-6 (1.6e-6), K=3 7.3e-6 (2.1e-6), K=5 5.5e-6 (1.1e-6), K=8 5.8e-6 (9.4e-7)
  the table seen through n = 1 on 8x32 (dense PSFs, K = 1 .. 8): 4.4e-7 .. 1.07e-6
  the joint quality case, n = 100: least squares model 42.324 dB, MI355X 42.324 dB; Poisson model 42.909 dB, MI355X 42.909 dB
The largest value is 7.31e-6 (64x128, K = 3, least squares mu 50 rho 1 nu 3, anisotropic, one weights plane, n = 30, the normalised
whole plan), 3.6x its float32 CPU run; the largest ratio to the CPU run is 6.1x (64x128, K = 8).  TVFR_TOL = 2e-5 is 2.7x the
largest value, the class of TVF_TOL and TVP_TOL (1.3e-5, 1.4e-5): the same kernels and the same arithmetic per frame, with K
adjoint spectra added in float32 on top.

The quality case (quality_case() of _frames_model.py: three 15 px lines at 30 / 90 / 150 degrees, 200 x 200 crop on 256^2, Poisson
noise at 1000 photons per unit), n = 100, rho = nu = 2, PSNR in dB against the truth at the best mu of QUALITY_MU (best value
interior), measured with this model in float64 (test_tvframes_host.py re-measures and asserts half of each gain):
  the crops themselves 21.70, 20.71, 21.70
  least squares: each frame alone 37.07 (mu 100), 34.95 (mu 40), 37.89 (mu 100); all three jointly 42.32 (mu 60): a gain of 4.43 dB
  Poisson:       each frame alone 38.15 (mu 40), 35.99 (mu 40), 38.78 (mu 60); all three jointly 42.91 (mu 40): a gain of 4.13 dB
  (multi-frame RL with its TV prior, section 37's table: 32.41 alone, 37.17 jointly)"""
import numpy as np

from _frames_model import MAX_FRAMES, frame_weights
from _rl_model import NORM_NONE, op_spectrum, psnr
from _tv_model import dx, dxT, dy, dyT, lap_symbol, shrink, tv_value
from _tvfree_model import finish, pad_to
from _tvpoisson_model import s_update as poisson_s_update

LEAST_SQUARES, POISSON = 0, 1  # FDR_TV_FRAMES_LEAST_SQUARES, FDR_TV_FRAMES_POISSON
TVFR_TOL = 2e-5  # 2.7x the largest error measured on the MI355X (7.31e-6): see the header

FAULTS = ("adjoint_H", "table_one", "swap01", "drop_last", "shared_q", "weights_ignored")


def frames_table(Hs, M, N, nu, rho):
    """1 / (nu sum_k |H_k|^2 + rho L), the |H_k|^2 added in ascending k; 0 where the denominator is 0"""
    h2 = None
    for H in Hs:
        t = np.abs(H) ** 2
        h2 = t if h2 is None else h2 + t
    den = nu * h2 + rho * lap_symbol(M, N)
    return np.where(den > 0, 1.0 / np.where(den > 0, den, 1), 0.0)


def tvframes_iterates(ds, psfs, M, N, mu, rho=2.0, iterations=50, weights=None, nu=0.0, data_term=LEAST_SQUARES, background=0.0,
                      anisotropic=False, dtype=np.float64, fault=None, x0=None):
    """yields dict(x, q (list), r (list), c (list), b, v) after the start (x alone) and after every iteration, all M x N planes.  dtype
    float32 runs the same formulas in single precision (float32 planes and table, complex64 spectra): the arithmetic class of the
    device.  x0: another start than pad(d_0) (the convergence pin).  fault (for the CPU pins only): 'adjoint_H' (the adjoints taken
    with H in place of conj(H)), 'table_one' (T from frame 0's |H|^2 alone), 'swap01' (the tables of frames 0 and 1 swapped on the
    adjoint side), 'drop_last' (the last frame missing from b), 'shared_q' (one q for all frames: every frame reads and overwrites
    it), 'weights_ignored' (weights = None)."""
    assert fault is None or fault in FAULTS, fault
    K = len(ds)
    assert 1 <= K <= MAX_FRAMES and len(psfs) == K
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    ds = [np.asarray(d, dtype=dtype) for d in ds]
    rows, cols = ds[0].shape
    nu = float(nu) if nu else float(rho)
    Hs = [op_spectrum(p, M, N) for p in psfs]
    T = frames_table(Hs[:1] if fault == "table_one" else Hs, M, N, nu, rho).astype(dtype)
    Hf = [H.astype(cdt) for H in Hs]
    Ha = list(Hs)
    if fault == "swap01" and K > 1:
        Ha[0], Ha[1] = Ha[1], Ha[0]
    Hb = [(H if fault == "adjoint_H" else np.conj(H)).astype(cdt) for H in Ha]
    pads = [pad_to(d, M, N, dtype) for d in ds]
    ws = frame_weights(None if fault == "weights_ignored" else weights, K, (rows, cols), dtype)
    ms = []
    for k in range(K):
        m = np.zeros((M, N), dtype=dtype)
        m[:rows, :cols] = ws[k]
        ms.append(m)
    inside = np.zeros((M, N), dtype=bool)
    inside[:rows, :cols] = True
    mu_, nu_, rho_ = dtype(mu), dtype(nu), dtype(rho)
    x = pads[0].copy() if x0 is None else np.asarray(x0, dtype=dtype).copy()
    wx = np.zeros((M, N), dtype=dtype)
    wy = np.zeros((M, N), dtype=dtype)
    qs = [np.zeros((M, N), dtype=dtype) for _ in range(K)]
    t = dtype(1.0) / rho_
    yield dict(x=x)
    for _ in range(iterations):
        cs, rs = [], []
        b = None
        for k in range(K):
            c = np.fft.irfft2(np.fft.rfft2(x).astype(cdt) * Hf[k], s=(M, N)).astype(dtype)
            qi = 0 if fault == "shared_q" else k
            e = c + qs[qi]
            if data_term == POISSON:
                s = poisson_s_update(e, pads[k], ms[k], mu, nu, background)
                q = (e - s).astype(dtype)
                r = (s - q).astype(dtype)
            else:
                a = mu_ * ms[k]
                s = np.where(inside, (a * pads[k] + nu_ * e) / (a + nu_), e).astype(dtype)
                q = np.where(inside, e - s, 0).astype(dtype)
                r = np.where(inside, s - q, c).astype(dtype)
            qs[qi] = q
            cs.append(c)
            rs.append(r)
            if fault == "drop_last" and K > 1 and k == K - 1:
                continue
            g = np.fft.irfft2(np.fft.rfft2(r).astype(cdt) * Hb[k], s=(M, N)).astype(dtype)
            b = g if b is None else (b + g).astype(dtype)
        gx, gy = dx(x) + wx, dy(x) + wy
        zx, zy = shrink(gx, gy, t, bool(anisotropic))
        wx, wy = gx - zx, gy - zy
        vx, vy = zx - wx, zy - wy
        rhs = (nu_ * b + rho_ * (dxT(vx) + dyT(vy))).astype(dtype)
        x = np.fft.irfft2(np.fft.rfft2(rhs).astype(cdt) * T, s=(M, N)).astype(dtype)
        yield dict(x=x, q=list(qs), r=rs, c=cs, b=b, v=(vx, vy), z=(zx, zy))


def tvframes_model(ds, psfs, M, N, mu, rho=2.0, iterations=50, weights=None, nu=0.0, data_term=LEAST_SQUARES, background=0.0,
                   anisotropic=False, nonneg=False, norm_area=NORM_NONE, out_shape=None, dtype=np.float64, fault=None):
    """the output of fdr_tv_deconv_frames_f32 on the frames ds: the top-left out_shape (default the frames' shape) of x"""
    st = None
    for st in tvframes_iterates(ds, psfs, M, N, mu, rho, iterations, weights, nu, data_term, background, anisotropic, dtype, fault):
        pass
    return finish(st["x"], out_shape or np.asarray(ds[0]).shape, nonneg, norm_area, M, N)


def frames_objective(x, ds, psfs, M, N, mu, weights=None, data_term=LEAST_SQUARES, background=0.0, anisotropic=False):
    """mu sum_k Phi_k(blur_k(x)) + TV(x) in float64"""
    K = len(ds)
    rows, cols = np.asarray(ds[0]).shape
    ws = frame_weights(weights, K, (rows, cols))
    total = tv_value(x, anisotropic)
    for k in range(K):
        c = np.fft.irfft2(np.fft.rfft2(x) * op_spectrum(psfs[k], M, N), s=(M, N))[:rows, :cols]
        d = np.asarray(ds[k], dtype=np.float64)
        if data_term == POISSON:
            u = c + background
            dp = np.maximum(d, 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                term = u - np.where(dp > 0, dp * np.log(np.where(u > 0, u, 1)), 0)
            if np.any(u[(ws[k] > 0) & (dp > 0)] <= 0):
                return np.inf
            total += mu * float(np.sum(ws[k] * term))
        else:
            total += 0.5 * mu * float(np.sum(ws[k] * (c - d) ** 2))
    return total


# ---- the short cases of test_tvframes_gpu.py, shared with the fault pins of test_tvframes_host.py ----
# (M, N, rows, cols, stride, wstride, out_stride, output windows): the packed column is most of the 8 x 32 table; a window short of the
# plan in both directions with odd strides; more than one workgroup of every window kernel with strides that leave no row aligned
SHORT = [(8, 32, 8, 32, 32, 32, 32, ((8, 32),)),
         (16, 32, 9, 30, 31, 33, 35, ((9, 30), (16, 32))),
         (64, 128, 37, 101, 103, 101, 131, ((37, 101), (64, 128)))]
SHORT_IDS = ["%dx%d-win%dx%d" % c[:4] for c in SHORT]
EXPOSURES = (0.5, 1.0, 2.0)  # PSF sums: a frame's sum is its exposure


def short_psfs(kind, K, M, N):
    """K PSFs of one shape: 'dense' 5 x 5 random planes top-left with the sums EXPOSURES in turn (their Nyquist responses are not
    zero), 'motion' centred 7 px lines at K angles (M x N planes)"""
    from _rl_model import centred_psf, dense_psf
    from _rltv_model import line_psf
    if kind == "dense":
        return [(dense_psf(11 + k, 5) * np.float32(EXPOSURES[k % 3])).astype(np.float32) for k in range(K)]
    return [centred_psf(line_psf(7, 180.0 * k / K + 15.0), M, N) for k in range(K)]


def short_frames(M, N, rows, cols, K, psfs, seed, positive=False):
    """K float32 windows: one scene with edges blurred by every PSF on the plan, cropped, plus a little noise of the frame's own
    (negative pixels unless `positive`)"""
    from _tv_model import blocks_scene
    rng = np.random.default_rng(seed)
    scene = blocks_scene(M, N, seed) + 0.1
    out = []
    for k in range(K):
        c = np.fft.irfft2(np.fft.rfft2(scene) * op_spectrum(psfs[k], M, N), s=(M, N))[:rows, :cols]
        d = c + 0.2 * rng.random((rows, cols)) - (0.0 if positive else 0.15)
        out.append(d.astype(np.float32))
    return out


def short_weights(kind, K, rows, cols, seed):
    """None, one 0 / 1 mask with 2 % zeros for all frames, or K planes with a different mask each (frame k odd: fractional weights)"""
    rng = np.random.default_rng(seed + 100)
    if kind == "none":
        return None
    if kind == "one":
        return (rng.random((rows, cols)) > 0.02).astype(np.float32)
    planes = []
    for k in range(K):
        planes.append((rng.random((rows, cols)) > 0.05).astype(np.float32) if k % 2 == 0 else rng.random((rows, cols)).astype(np.float32))
    return np.stack(planes)


WEIGHT_KINDS = ("none", "one", "per_frame")

# ---- the quality table: quality_case() of _frames_model.py ----
QUALITY_N, QUALITY_RHO = 100, 2.0
QUALITY_MU = {LEAST_SQUARES: (20.0, 40.0, 60.0, 100.0, 200.0), POISSON: (20.0, 40.0, 60.0, 100.0, 200.0)}
QUALITY_JOINT_MU = {LEAST_SQUARES: 60.0, POISSON: 40.0}  # the best mu of the grid for all three frames jointly
# PSNR in dB measured with this model in float64 at the best mu of the grid: (frame 0, frame 1, frame 2 alone, all three jointly)
QUALITY_MEASURED = {LEAST_SQUARES: (37.07, 34.95, 37.89, 42.32), POISSON: (38.15, 35.99, 38.78, 42.91)}


def quality_psnr(case, frames, mu, data_term, iterations=QUALITY_N, dtype=np.float64):
    """PSNR of the joint restoration of the frames `frames` (indices) of the case at mu"""
    ds = [case["ds"][k] for k in frames]
    psfs = [case["psfs"][k] for k in frames]
    out = tvframes_model(ds, psfs, case["M"], case["N"], mu, QUALITY_RHO, iterations, data_term=data_term, dtype=dtype)
    return psnr(out, case["truth"])
