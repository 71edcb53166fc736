"""float64 model of multi-frame Richardson-Lucy (fdr_set_frame_psfs*, fdr_blur_frames_f32_dev, fdr_richardson_lucy_frames_f32*;
include/fdr.h): the specification.

K frames d_k (rows x cols, all the same window at the plan's top-left corner) of one scene, each with its own PSF (H_k = DFT2 of PSF k
placed top-left in the M x N plan, PSF sums NOT normalised: a frame's sum is its relative exposure) and its own weights m_k (None =
all ones; one plane may serve all frames).  With fullblur / fullblur^T of _rlfree_model.py and the factor of _rltv_model.py:

    W_k = pad(m_k);  dw_k = pad(m_k . max(d_k, 0))
    alpha = sum_k fullblur_k^T(W_k);  seen = alpha > sigma K;  wgt = seen ? 1 / alpha : 0
    u = seen ? (sum_k sum dw_k) / (sum_k sum W_k) : 0
    n times:  c_k = window(fullblur_k(u));  r_k = c_k > TAU ? dw_k / c_k : 0 (0 outside the window)
              u = max(u . factor . sum_k fullblur_k^T(pad(r_k)), 0),   factor = wgt (lambda = 0) or wgt / g(u) (the TV prior)

sigma K is formed in float32, as the device forms it.  K = 1 is rlfree_state / rltv_free_state.  Pinned in test_frames_host.py
(those two, copies of one frame, the adjoint identity, the flux invariant, injected faults) before it judges the GPU
(test_frames_gpu.py).

Device against this model: max |got - model| / max |model| over the compared window (FDR_NORM_NONE) or max-abs (normalised outputs).
FRAMES_TOL and FRAMES_ADJ_TOL are at most 4x the largest value one run of test_frames_gpu.py measured on an MI355X, and the test also
holds every case within 10x of the float32 / complex64 CPU run of this model (dtype=np.float32).  Measured on the MI355X, sigma 1e-2,
PSF sums 0.5 / 1 / 2, largest over n, both output windows and the three norm_area (in brackets the float32 CPU run of the same case):
  64x128 win 37x101 (n <= 30):    K=2 no weights 1.3e-5 (4.2e-6), K=3 per-frame weights 6.3e-5 (1.9e-5), K=5 none 1.9e-5 (3.1e-6),
                                  K=8 none 3.0e-5 (1.4e-5)
  256^2 win 200x151 (n <= 30):    K=2 per frame 1.7e-5 (9.6e-6), K=3 one plane 9.0e-5 (3.6e-5), K=5 per frame 2.6e-5 (2.0e-5),
                                  K=8 per frame 3.1e-5 (2.3e-5); K=3 with the prior (lambda 0.02, eps 0.05, n <= 10) 3.4e-5 (2.2e-5)
  1024x512 win 1000x333 (n <= 30): K=2 one plane 9.3e-5 (5.7e-5), K=3 none 2.7e-4 (1.2e-4), K=5 one plane 1.2e-4 (5.5e-5),
                                  K=8 one plane 1.1e-4 (3.4e-5)
  4096^2 win 4000x3900, K=2, n=1: 2.3e-5 (9.8e-6)
  adjoint sum of K = 5 windows, relative to its largest value: 8x32 1.8e-7 (1.3e-7), 64x128 4.8e-7 (1.7e-7), 256^2 4.5e-7 (2.2e-7),
                                  1024x512 5.7e-7 (2.5e-7)
  the quality case (three frames, lambda 0.01, eps 1e-3, n = 100): model 37.174 dB, MI355X 37.164 dB
As in _rlfree_model.py the errors sit on the rim where the coverage is small and wgt = 1 / alpha magnifies the error of a float32
alpha; they grow with n on the top-left PSFs of the 1024 x 512 cases, where that rim lies inside the output window (K = 3: 2.0e-4
at n = 10, 2.7e-4 at n = 30).  The largest value is 2.65e-4, so FRAMES_TOL = 7.5e-4 lies below 4x of it; the normalised outputs are
held to the 10x bound in their own max-abs metric as well."""
import numpy as np

from _rl_model import NORM_NONE, TAU, normalize, op_spectrum, psnr
from _rlfree_model import SIGMA, fullblur
from _rltv_model import EPS, tv_factor

MAX_FRAMES = 8  # FDR_MAX_FRAMES
FAULTS = ("adjoint_H", "alpha_one", "sigma_single", "swap01", "drop_last")
FRAMES_TOL = 7.5e-4  # the class of RLFREE_TOL (1e-3)
FRAMES_ADJ_TOL = 2e-6  # the sum of K adjoint blurs, relative to its largest value (BLUR_TOL, one blur: 5e-6)
SIGMA_MARGIN = 1e-4  # per frame: no model alpha may lie within SIGMA_MARGIN * K of sigma * K


def frame_weights(weights, K, shape, dtype=np.float64):
    """the K weight planes: None -> ones, one 2-D plane -> that for every frame, K planes -> one each"""
    if weights is None:
        return [np.ones(shape, dtype=dtype)] * K
    w = np.asarray(weights, dtype=dtype)
    if w.ndim == 2:
        return [w] * K
    assert w.shape[0] == K
    return [w[k] for k in range(K)]


def threshold(sigma, K):
    """sigma K as the device forms it: a float32 product"""
    return float(np.float32(sigma) * np.float32(K))


def blur_frames(x, psfs, M, N, dtype=np.float64):
    """the K windows blur_k(x) of one window x"""
    x = np.asarray(x, dtype=dtype)
    rows, cols = x.shape
    X = np.zeros((M, N), dtype=dtype)
    X[:rows, :cols] = x
    return [fullblur(X, op_spectrum(p, M, N), dtype=dtype)[:rows, :cols] for p in psfs]


def blur_frames_adjoint(ys, psfs, M, N, dtype=np.float64):
    """the one window sum_k blur_k^T(y_k), added in ascending k"""
    rows, cols = np.asarray(ys[0]).shape
    acc = None
    for y, p in zip(ys, psfs):
        Y = np.zeros((M, N), dtype=dtype)
        Y[:rows, :cols] = np.asarray(y, dtype=dtype)
        g = fullblur(Y, op_spectrum(p, M, N), adjoint=True, dtype=dtype)
        acc = g if acc is None else (acc + g).astype(dtype)
    return acc[:rows, :cols]


def frames_state(ds, psfs, M, N, iterations, weights=None, sigma=SIGMA, lam=0.0, eps=EPS, dtype=np.float64, tau=TAU, fault=None, keep=(),
                 keep_r=False):
    """the whole state after `iterations` steps: dict(u, alpha, wgt, dw (list), W (list), us), planes M x N; us[n] is the estimate
    after n steps for every n in `keep` (one run then serves several iteration counts); with keep_r, rs[it][k] is the window of the
    ratio plane r_k of step it.  fault (for the CPU pins
    only): 'adjoint_H' (the last frame's adjoint with H in place of conj(H)), 'alpha_one' (the coverage from frame 0 alone),
    'sigma_single' (the threshold sigma in place of sigma K), 'swap01' (the tables of frames 0 and 1 swapped on the adjoint side),
    'drop_last' (the last frame missing from the sum of the update)"""
    K = len(ds)
    assert 1 <= K <= MAX_FRAMES and len(psfs) == K
    rows, cols = np.asarray(ds[0]).shape
    ms = frame_weights(weights, K, (rows, cols), dtype)
    Hs = [op_spectrum(p, M, N) for p in psfs]
    Ha = list(Hs)  # the tables of the adjoint side
    if fault == "swap01" and K > 1:
        Ha[0], Ha[1] = Ha[1], Ha[0]
    adj = [True] * K
    if fault == "adjoint_H":
        adj[K - 1] = False
    Ws, dws = [], []
    for k in range(K):
        W = np.zeros((M, N), dtype=dtype)
        W[:rows, :cols] = ms[k]
        dw = np.zeros((M, N), dtype=dtype)
        dw[:rows, :cols] = ms[k] * np.maximum(np.asarray(ds[k], dtype=dtype), 0)
        Ws.append(W)
        dws.append(dw)
    alpha = None
    for k in range(1 if fault == "alpha_one" else K):
        a = fullblur(Ws[k], Ha[k], adjoint=adj[k], dtype=dtype)
        alpha = a if alpha is None else (alpha + a).astype(dtype)
    thr = float(np.float32(sigma)) if fault == "sigma_single" else threshold(sigma, K)
    seen = alpha > thr
    wgt = np.where(seen, 1 / np.where(seen, alpha, 1), 0).astype(dtype)
    sw = sum(float(np.sum(W, dtype=np.float64)) for W in Ws)
    sd = sum(float(np.sum(dw, dtype=np.float64)) for dw in dws)
    u = np.where(seen, sd / sw if sw > 0 else 0.0, 0).astype(dtype)
    win = np.zeros((M, N), dtype=bool)
    win[:rows, :cols] = True
    us = {0: u} if 0 in keep else {}
    rs = []
    for it in range(iterations):
        factor = wgt if lam == 0 else tv_factor(u, lam, eps, w=wgt, dtype=dtype)
        if keep_r:
            rs.append([])
        g = None
        for k in range(K - 1 if fault == "drop_last" and K > 1 else K):
            c = fullblur(u, Hs[k], dtype=dtype)
            ok = win & (c > tau)
            r = np.where(ok, dws[k] / np.where(ok, c, 1), 0).astype(dtype)
            if keep_r:
                rs[-1].append(r[:rows, :cols])
            gk = fullblur(r, Ha[k], adjoint=adj[k], dtype=dtype)
            g = gk if g is None else (g + gk).astype(dtype)
        u = np.maximum(u * factor * g, 0).astype(dtype)
        if it + 1 in keep:
            us[it + 1] = u
    return dict(u=u, alpha=alpha, wgt=wgt, dw=dws, W=Ws, us=us, rs=rs)


def frames_model(ds, psfs, M, N, iterations, weights=None, sigma=SIGMA, lam=0.0, eps=EPS, out_shape=None, norm_area=NORM_NONE,
                 dtype=np.float64, fault=None):
    """the output of fdr_richardson_lucy_frames_f32: the top-left out_shape (default the frames' shape) of u, normalised"""
    st = frames_state(ds, psfs, M, N, iterations, weights, sigma, lam, eps, dtype, fault=fault)
    orows, ocols = np.asarray(ds[0]).shape if out_shape is None else out_shape
    return normalize(st["u"][:orows, :ocols], norm_area, M, N)


def flux_defect(st):
    """|sum(alpha u) / sum_k sum(dw_k) - 1| in float64: 0 after every iteration at lambda = 0 wherever c_k > tau"""
    a = float(np.sum(st["alpha"].astype(np.float64) * st["u"].astype(np.float64)))
    b = sum(float(np.sum(dw, dtype=np.float64)) for dw in st["dw"])
    return abs(a / b - 1.0)


def sigma_margin(alpha, sigma, K):
    """min |alpha - sigma K| over the plan"""
    return float(np.min(np.abs(np.asarray(alpha, dtype=np.float64) - threshold(sigma, K))))


# ---- the quality case: the "crop" scene of _rltv_model.py seen through three line PSFs ---------------------------------------------------
# rect_scene(512), blurred circularly on 512^2 by the 15 px line PSF at 30, 90 and 150 degrees, the 200 x 200 crop at (150, 170), Poisson
# noise at 1000 photons per unit from ONE default_rng(4) drawn frame after frame, restored on a 256^2 plan.  Measured with this model
# in float64, PSNR against the truth in dB (test_frames_host.py re-measures and asserts half of each gain):
#   the crops themselves 21.70, 20.71, 21.70
#   TV prior (lambda 0.01, eps 1e-3), n = 100: each frame alone 32.35, 30.20, 32.41; all three jointly 37.17
QUALITY_ANGLES = (30.0, 90.0, 150.0)
QUALITY_LAMBDA, QUALITY_EPS, QUALITY_N = 0.01, 1e-3, 100


def quality_case():
    """dict(truth, ds (float32 frames), psfs (the centred PSF planes of the plan), M, N)"""
    from _rl_model import centred_psf
    from _rltv_model import PHOTONS, line_psf, rect_scene
    scene = rect_scene(512)
    rng = np.random.default_rng(4)
    ds, psfs = [], []
    for a in QUALITY_ANGLES:
        psf = line_psf(15, a)
        blurred = np.fft.irfft2(np.fft.rfft2(scene) * np.fft.rfft2(centred_psf(psf, 512, 512).astype(np.float64)), s=scene.shape)
        noisy = rng.poisson(np.maximum(blurred, 0) * PHOTONS) / PHOTONS
        ds.append(noisy[150:350, 170:370].astype(np.float32))
        psfs.append(centred_psf(psf, 256, 256))
    return dict(truth=scene[150:350, 170:370], ds=ds, psfs=psfs, M=256, N=256)


def crop_quality_case():
    """the second scene: crop_scene(1024) of _rlfree_model.py, blurred circularly by 15 px lines at 0, 90 and 45 degrees, the 480 x 480
    crop at (200, 200), Poisson noise at 2000 photons per unit (default_rng(6), frame after frame), restored on a 512^2 plan"""
    from _rl_model import centred_psf
    from _rlfree_model import crop_scene
    from _rltv_model import line_psf
    scene = crop_scene(1024)
    rng = np.random.default_rng(6)
    ds, psfs = [], []
    for a in (0.0, 90.0, 45.0):
        psf = line_psf(15, a)
        blurred = np.fft.irfft2(np.fft.rfft2(scene) * np.fft.rfft2(centred_psf(psf, 1024, 1024).astype(np.float64)), s=scene.shape)
        ds.append((rng.poisson(np.maximum(blurred, 0) * 2000.0) / 2000.0)[200:680, 200:680].astype(np.float32))
        psfs.append(centred_psf(psf, 512, 512))
    return dict(truth=scene[200:680, 200:680], ds=ds, psfs=psfs, M=512, N=512)


def best_plain_iterate(case, frames, upto):
    """(k, PSNR) of the best iterate k <= upto of the joint restoration of the frames `frames` without a prior"""
    ds = [case["ds"][k] for k in frames]
    psfs = [case["psfs"][k] for k in frames]
    rows, cols = ds[0].shape
    us = frames_state(ds, psfs, case["M"], case["N"], upto, keep=range(1, upto + 1))["us"]
    return max(((k, psnr(u[:rows, :cols], case["truth"])) for k, u in us.items()), key=lambda t: t[1])


def quality_psnr(case, frames, iterations=QUALITY_N, lam=QUALITY_LAMBDA, eps=QUALITY_EPS, dtype=np.float64):
    """PSNR of the joint restoration of the frames `frames` (indices) of the case"""
    ds = [case["ds"][k] for k in frames]
    psfs = [case["psfs"][k] for k in frames]
    return psnr(frames_model(ds, psfs, case["M"], case["N"], iterations, lam=lam, eps=eps, dtype=dtype), case["truth"])
