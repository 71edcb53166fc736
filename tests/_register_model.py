"""float64 model of the frame registration (fdr_register_frames_f32*, fdr_psf_shift_f32*; include/fdr.h): the
specification.

K frames d_k (rows x cols, the window at the top-left of the M x N plan) of one scene, each seen through its own PSF p_k and moved by
its own translation s_k; for every k but the reference, with w = hann(rows) hann(cols)^T (numpy.hanning, as the motion estimate):

    a = pad(w . d_ref),  b = pad(w . d_k);  G_a, G_b their DFT2;  H_a, H_b the DFT2 of the PSFs top-left in the plan (1 without PSFs)
    C = conj(G_a) G_b H_a conj(H_b);  Chat = C / (|C| + eps_rel mean |C|);  r = Re IDFT2(Chat)
    (i*, j*) = argmax r over |dy| <= R_r, |dx| <= R_c, periodic; exact ties: the lowest (dy + R_r) (2 R_c + 1) + dx + R_c
    dy = i* + parabola(r[i* - 1, j*], r[i*, j*], r[i* + 1, j*]), dx alike;  parabola(m, z, p) = clamp(0.5 (m - p) / (m - 2 z + p))
    confidence = (r_peak - mean r) / std r

The reference gets (0, 0, 1, 0), an all-zero frame (mean |C| = 0) zeros.  psf_shift_model is the bilinear shift of a PSF into a plane
padded by `pad` on every side; with dtype=np.float32 it repeats the device's operations one by one (weights formed in double and
rounded once, four products each rounded, added in the kernel's order), so the device must give its bits.

FAULTS are wrong versions of the correlation plane and of the pick, for the CPU pins of test_register_host.py: each must move the
short case by far more than PLANE_TOL.  (Doubling C at the self-paired bins, or writing them twice, is NOT among them: the whitening
divides it out again and it changes r below float64 round-off; what a mishandled self-paired bin shows is 'self_unsplit'.)

Device against this model, the correlation plane r: max |got - model| over the plane (r is dimensionless, its peak at most 1).
PLANE_TOL is 4x the largest value test_register_gpu.py measured on an MI355X over its shapes, the factor covering the spread from
shape to shape; measured, worst frame of each case of GPU_CASES:
  32x32 win 16x16 8.4e-8, 32x32 win 20x27 7.3e-8, 64x32 win 50x32 (plain) 2.78e-7, 32x256 win 32x200 2.9e-8, 32x2048 whole 1.3e-8,
  45x75 win 40x61 1.8e-8, 48x80 whole (plain) 1.4e-7, 45x80 win 30x70 2.0e-8, 256^2 win 200^2 K = 8 4.0e-8
(r is a mean of M N unit phasors: its float32 error falls with the plan's size, and the two cases without PSFs, whose |C| spans the
whole range of |G|^2, are the largest).  The parabola turns a plane error into a shift error:  with every one of m, z, p off by at most t, the numerator 0.5 (m - p) is
off by at most t and the denominator D = m - 2 z + p by at most 4 t, so for |off| <= 0.5 and |D| > 4 t
    |off' - off| <= (t + |off| 4 t) / (|D| - 4 t) <= 3 t / (|D| - 4 t)                                                (shift_bound)
(the clamp to [-0.5, 0.5] only shortens the difference)."""
import numpy as np

from _motion_model import hann

MAX_FRAMES = 8         # FDR_MAX_FRAMES
EPS_REL = 1e-3         # FDR_REGISTER_EPS_REL (the float32 value is what the device uses)
MIN_WINDOW = 16
PLANE_TOL = 1.1e-6     # the correlation plane against this model, max-abs: 4x the largest measured (2.78e-7); see the docstring
FAULTS = ("conj_wrong", "no_psf", "swap_h", "no_window", "self_unsplit", "tie_high")


def default_range(rows, cols):
    return min(rows, cols) // 4


def window_plane(img, M, N, windowed=True):
    img = np.asarray(img, dtype=np.float64)
    rows, cols = img.shape
    x = np.zeros((M, N))
    x[:rows, :cols] = np.outer(hann(rows), hann(cols)) * img if windowed else img
    return x


def psf_spectrum(psf, M, N):
    plane = np.zeros((M, N))
    psf = np.asarray(psf, dtype=np.float64)
    plane[:psf.shape[0], :psf.shape[1]] = psf
    return np.fft.fft2(plane)


def self_paired(M, N):
    """the bins that are their own mirror image: row 0 or (M even) M / 2 with column 0 or (N even) N / 2"""
    return [(u, v) for u in ([0] + ([M // 2] if M % 2 == 0 else [])) for v in ([0] + ([N // 2] if N % 2 == 0 else []))]


def cross_power(d_ref, d_k, p_ref, p_k, M, N, fault=None):
    """C (M x N complex128)"""
    win = fault != "no_window"
    Ga, Gb = np.fft.fft2(window_plane(d_ref, M, N, win)), np.fft.fft2(window_plane(d_k, M, N, win))
    C = Ga * np.conj(Gb) if fault == "conj_wrong" else np.conj(Ga) * Gb
    if p_ref is not None and fault != "no_psf":
        Ha, Hb = psf_spectrum(p_ref, M, N), psf_spectrum(p_k, M, N)
        if fault == "swap_h":
            Ha, Hb = Hb, Ha
        C = C * Ha * np.conj(Hb)
    if fault == "self_unsplit":  # the pair spectrum Z = G_a + i G_b left where a lane did not separate it
        for u, v in self_paired(M, N):
            C[u, v] = Ga[u, v] + 1j * Gb[u, v]
    return C


def correlation_plane(d_ref, d_k, p_ref, p_k, M, N, eps_rel=EPS_REL, fault=None):
    """r (M x N float64); all zeros for an all-zero frame or reference"""
    C = cross_power(d_ref, d_k, p_ref, p_k, M, N, fault)
    mag = np.abs(C)
    mean = float(mag.mean())
    if not mean > 0:
        return np.zeros((M, N))
    den = mag + float(np.float32(eps_rel)) * mean
    return np.real(np.fft.ifft2(np.where(den > 0, C / np.where(den > 0, den, 1), 0)))


def parabola(m, z, p):
    den = m - 2.0 * z + p
    if den == 0:
        return 0.0
    return float(min(max(0.5 * (m - p) / den, -0.5), 0.5))


def pick(r, Rr, Rc, fault=None):
    """dict(dy, dx, peak, confidence, iy, ix (the whole-pixel peak), denom (the two parabola denominators), second (the largest r of
    the search window beside the peak, its neighbours included: stricter than leaving them out))"""
    M, N = r.shape
    dys, dxs = np.arange(-Rr, Rr + 1), np.arange(-Rc, Rc + 1)
    win = r[np.ix_(dys % M, dxs % N)]
    flat = win.ravel()
    best = flat.max()
    hits = np.flatnonzero(flat == best)
    idx = int(hits[-1] if fault == "tie_high" else hits[0])
    iy, ix = int(dys[idx // len(dxs)]), int(dxs[idx % len(dxs)])
    i, j = iy % M, ix % N
    z = r[i, j]
    m_y, p_y, m_x, p_x = r[(i - 1) % M, j], r[(i + 1) % M, j], r[i, (j - 1) % N], r[i, (j + 1) % N]
    mean, sd = float(r.mean()), float(r.std())
    mask = np.ones(win.shape, dtype=bool)
    mask[idx // len(dxs), idx % len(dxs)] = False
    return dict(dy=iy + parabola(m_y, z, p_y), dx=ix + parabola(m_x, z, p_x), peak=float(z), confidence=(float(z) - mean) / sd if sd > 0 else 0.0,
                iy=iy, ix=ix, denom=(float(m_y - 2 * z + p_y), float(m_x - 2 * z + p_x)), second=float(win[mask].max()) if mask.any() else -np.inf)


def register_model(frames, psfs, M, N, reference=0, max_shift=0, eps_rel=EPS_REL, fault=None, planes=False):
    """the K results as dicts (pick's, the reference's (0, 0, 1, 0)); with planes=True also the K correlation planes"""
    rows, cols = np.asarray(frames[0]).shape
    Rr, Rc = max_shift if isinstance(max_shift, (tuple, list)) else (max_shift, max_shift)
    Rr, Rc = Rr or default_range(rows, cols), Rc or default_range(rows, cols)
    assert 1 <= len(frames) <= MAX_FRAMES and 1 <= Rr and 2 * Rr < M and 1 <= Rc and 2 * Rc < N
    out, rs = [], []
    for k in range(len(frames)):
        if k == reference:
            out.append(dict(dy=0.0, dx=0.0, peak=1.0, confidence=0.0, iy=0, ix=0))
            rs.append(np.zeros((M, N)))
            continue
        r = correlation_plane(frames[reference], frames[k], None if psfs is None else psfs[reference], None if psfs is None else psfs[k], M, N,
                              eps_rel, fault)
        rs.append(r)
        if not np.any(r):
            out.append(dict(dy=0.0, dx=0.0, peak=0.0, confidence=0.0, iy=0, ix=0))
        else:
            out.append(pick(r, Rr, Rc, fault))
    return (out, rs) if planes else out


def shift_bound(denom, tol=PLANE_TOL):
    """the largest change of a parabola offset when its three values move by at most tol each (the docstring's derivation)"""
    assert abs(denom) > 8 * tol
    return 3 * tol / (abs(denom) - 4 * tol)


def psf_shift_model(psfs, shifts, pad_rows, pad_cols, dtype=np.float64):
    """the K shifted PSFs, (K, prows + 2 pad_rows, pcols + 2 pad_cols); shifts: (dy, dx) pairs.  float64: exact bilinear weights.
    float32: the device's arithmetic operation by operation"""
    psfs = [np.asarray(p, dtype=dtype) for p in psfs]
    pr, pc = psfs[0].shape
    out = np.zeros((len(psfs), pr + 2 * pad_rows, pc + 2 * pad_cols), dtype=dtype)
    for k, (p, s) in enumerate(zip(psfs, shifts)):
        dy, dx = float(s[0]), float(s[1])
        dy = 0.0 if dy != dy else min(max(dy, -float(pad_rows)), float(pad_rows - 1))
        dx = 0.0 if dx != dx else min(max(dx, -float(pad_cols)), float(pad_cols - 1))
        fy0, fx0 = np.floor(dy), np.floor(dx)
        fy, fx = dy - fy0, dx - fx0
        w = [dtype((1.0 - fy) * (1.0 - fx)), dtype((1.0 - fy) * fx), dtype(fy * (1.0 - fx)), dtype(fy * fx)]
        oy, ox = pad_rows + int(fy0), pad_cols + int(fx0)
        taps = []
        for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)):  # the output of tap (a, b): p laid at offset (oy + a, ox + b)
            t = np.zeros(out.shape[1:], dtype=dtype)
            y0, x0 = oy + a, ox + b
            ys, xs = slice(max(y0, 0), min(y0 + pr, t.shape[0])), slice(max(x0, 0), min(x0 + pc, t.shape[1]))
            t[ys, xs] = p[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0]
            taps.append(t)
        acc = (w[0] * taps[0]).astype(dtype)
        for i in (1, 2, 3):
            acc = (acc + (w[i] * taps[i]).astype(dtype)).astype(dtype)
        out[k] = acc
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def line(size, angle):
    from _rltv_model import line_psf
    return line_psf(size, angle)


def disk_psf(radius):
    from _defocus_model import disk, disk_size
    return disk(disk_size(radius), radius).astype(np.float32)


def embed(psf, size):
    """psf centred in a size x size plane (both odd): PSFs of one shape for one call"""
    out = np.zeros((size, size), dtype=np.float32)
    o = (size - psf.shape[0]) // 2
    out[o:o + psf.shape[0], o:o + psf.shape[1]] = psf
    return out


def _pair(a, b):
    size = max(a.shape[0], b.shape[0])
    return embed(a, size), embed(b, size)


PSF_PAIRS = {  # the accuracy table's pairs
    "lines-30-90": lambda: _pair(line(15, 30.0), line(15, 90.0)),
    "lines-30-150": lambda: _pair(line(15, 30.0), line(15, 150.0)),
    "lines-21-7": lambda: _pair(line(21, 30.0), line(7, 120.0)),
    "line-9-disk-4.5": lambda: _pair(line(9, 30.0), disk_psf(4.5)),
}
LINE_PAIRS = ("lines-30-90", "lines-30-150", "lines-21-7")
SHIFTS = [(3.3, -5.7), (0.5, 0.5), (-12.25, 8.5), (20.6, 17.4), (-0.4, 30.8)]
SCENE, CROP, CROP_AT, PLAN = 512, 200, (150, 170), 256


def translate(img, shift):
    """img moved by `shift` (rows down, columns right) on its torus: the phase ramp e^{-i w.s} on its DFT2, the exact translation of the
    periodic band-limited picture.  Neither the estimate nor the bilinear shift of a PSF is handed its own model by it."""
    fy, fx = np.fft.fftfreq(img.shape[0])[:, None], np.fft.fftfreq(img.shape[1])[None, :]
    return np.real(np.fft.ifft2(np.fft.fft2(img) * np.exp(-2j * np.pi * (fy * shift[0] + fx * shift[1]))))


def scene_blur(scene, psf, shift=(0.0, 0.0), pad=40):
    """the scene blurred periodically by the centred psf moved by `shift` (bilinear, psf_shift_model): (p * x)(r - s)"""
    q = psf_shift_model([psf], [shift], pad, pad)[0]
    plane = np.zeros(scene.shape)
    plane[:q.shape[0], :q.shape[1]] = q
    plane = np.roll(plane, (-(q.shape[0] // 2), -(q.shape[1] // 2)), axis=(0, 1))
    return np.fft.irfft2(np.fft.rfft2(scene) * np.fft.rfft2(plane), s=scene.shape)


def pair_frames(pair, shift, noise, seed=11):
    """(frames, psfs): the reference through the pair's first PSF, frame 1 through the second and moved by `shift` (translate),
    CROP x CROP crops of the 512^2 rectangle scene, Gaussian noise of deviation `noise` (default_rng(seed), frame after frame), float32"""
    from _rltv_model import rect_scene
    scene = rect_scene(SCENE)
    p0, p1 = PSF_PAIRS[pair]()
    rng = np.random.default_rng(seed)
    y, x = CROP_AT
    frames = []
    for p, s in ((p0, (0.0, 0.0)), (p1, shift)):
        f = translate(scene_blur(scene, p), s)[y:y + CROP, x:x + CROP]
        frames.append((f + noise * rng.standard_normal(f.shape)).astype(np.float32))
    return frames, [p0, p1]


def short_case(M, N, rows, cols, K, shifts, seed, psf_size=5):
    """(frames, psfs) for the device tests: a random texture (white noise: every shift has a sharp peak, also in a 16 x 16 window) on a
    torus twice the plan, K small random positive PSFs, frame k the scene through PSF k moved by shifts[k] (bilinear, psf_shift_model;
    shifts[reference] = (0, 0)), cropped to rows x cols; float32"""
    S0, S1 = 2 * M, 2 * N
    rng = np.random.default_rng(seed)
    scene = rng.uniform(0.0, 1.0, (S0, S1))
    psfs, frames = [], []
    pad_r, pad_c = int(max(abs(s[0]) for s in shifts)) + 2, int(max(abs(s[1]) for s in shifts)) + 2
    for k in range(K):
        p = rng.uniform(0.1, 1.0, (psf_size, psf_size))
        p = (p / p.sum()).astype(np.float32)
        q = psf_shift_model([p], [shifts[k]], pad_r, pad_c)[0]
        plane = np.zeros((S0, S1))
        plane[:q.shape[0], :q.shape[1]] = q
        plane = np.roll(plane, (-(q.shape[0] // 2), -(q.shape[1] // 2)), axis=(0, 1))
        f = np.fft.irfft2(np.fft.rfft2(scene) * np.fft.rfft2(plane), s=scene.shape)
        frames.append(f[M // 2:M // 2 + rows, N // 2:N // 2 + cols].astype(np.float32))
        psfs.append(p)
    return frames, psfs


# ---- the quality case: section 37's three frames, the second and third moved ------------------------------------------------------------
# rect_scene(512) through the 15 px line PSFs at 30 / 90 / 150 degrees, for frames 1 and 2 moved by QUALITY_SHIFTS (translate), the 200 x 200 crop at
# (150, 170), Poisson noise at 1000 photons per unit from ONE default_rng(4) drawn frame after frame, restored on a 256^2 plan by
# _frames_model.frames_model with the TV prior (lambda 0.01, eps 1e-3, n = 100).  Measured with these models in float64, PSNR against
# the truth in dB (test_register_host.py re-measures and asserts the relations):
#   shifts ignored 17.57; frame 0 alone 32.35; true shifts in the PSFs 35.62; estimated shifts in the PSFs 35.08
QUALITY_SHIFTS = [(0.0, 0.0), (3.3, -5.7), (-6.25, 8.5)]
QUALITY_PAD = 52  # max_shift + 2 for the default range of a 200 x 200 window


def quality_case():
    """dict(truth, ds (float32 frames), psfs (the compact 15 x 15 PSFs), M, N)"""
    from _frames_model import QUALITY_ANGLES
    from _rltv_model import PHOTONS, rect_scene
    scene = rect_scene(SCENE)
    rng = np.random.default_rng(4)
    y, x = CROP_AT
    ds, psfs = [], []
    for a, s in zip(QUALITY_ANGLES, QUALITY_SHIFTS):
        p = line(15, a)
        blurred = translate(scene_blur(scene, p), s)
        noisy = rng.poisson(np.maximum(blurred, 0) * PHOTONS) / PHOTONS
        ds.append(noisy[y:y + CROP, x:x + CROP].astype(np.float32))
        psfs.append(p)
    return dict(truth=scene[y:y + CROP, x:x + CROP], ds=ds, psfs=psfs, M=PLAN, N=PLAN)


def plan_psfs(psfs, shifts, M, N, pad=QUALITY_PAD, dtype=np.float64):
    """the M x N planes the restoration gets: PSF k moved by shifts[k] (psf_shift_model), laid top-left and rolled so that the centre tap
    of the unmoved PSF lies at (0, 0): the restoration stays where the reference frame is"""
    q = psf_shift_model(psfs, shifts, pad, pad, dtype=dtype)
    planes = np.zeros((len(psfs), M, N), dtype=q.dtype)
    planes[:, :q.shape[1], :q.shape[2]] = q
    return np.roll(planes, (-(q.shape[1] // 2), -(q.shape[2] // 2)), axis=(1, 2))


# ---- the device cases: the smallest shapes at which the kernels can still go wrong (test_register_gpu.py; test_register_host.py holds the
# model's peak of every frame of every case above all non-neighbours by PEAK_MARGIN x PLANE_TOL, so that the whole-pixel peak is decided) ----
# (id, M, N, rows, cols, mixed radix, reference, max_shift, with PSFs, per frame its shift; the reference's is (0, 0), seed)
PEAK_MARGIN = 10.0
GPU_CASES = [
    ("32x32-win16", 32, 32, 16, 16, False, 0, 0, True, [(0, 0), (0, 0), (2, -3), (-1.5, 0.5)], 1),                 # smallest plan and window
    ("32x32-win20x27", 32, 32, 20, 27, False, 0, (5, 6), True, [(0, 0), (5, -6), (-5, 6), (7.5, 2)], 2),          # at +-max_shift; beyond it
    ("64x32-win50x32", 64, 32, 50, 32, False, 1, 0, False, [(-3, 2.5), (0, 0)], 3),                               # non-square, plain, reference 1
    ("32x256-win32x200", 32, 256, 32, 200, False, 0, (7, 50), True, [(0, 0), (-7, 50), (3.5, -20.25)], 4),        # one row of workgroups
    ("32x2048-whole", 32, 2048, 32, 2048, False, 0, (7, 500), True, [(0, 0), (1, -300.25)], 5),                    # two column workgroups, window = plan
    ("45x75-win40x61", 45, 75, 40, 61, True, 0, 0, True, [(0, 0), (4.5, -7), (-10, 15)], 6),                      # odd lengths: no Nyquist bins
    ("48x80-whole", 48, 80, 48, 80, True, 0, 0, False, [(0, 0), (-3, 11.5)], 7),                                  # mixed radix, even lengths, window = plan
    ("45x80-win30x70", 45, 80, 30, 70, True, 0, 0, True, [(0, 0), (1, 2), (-0.5, -6.5)], 8),                      # mixed parity: one Nyquist column, no Nyquist row
    ("256-win200-K8", 256, 256, 200, 200, False, 3, 0, True,
     [(3.3, -5.7), (0.5, -2.5), (-12.25, 8.5), (0, 0), (20.6, 17.4), (-0.4, 30.8), (50, -50), (-6.25, 8.5)], 9),    # the accuracy case's size, K = 8
    ("32x32-K1", 32, 32, 16, 16, False, 0, 0, True, [(0, 0)], 10),                                                 # the reference alone
]
GPU_IDS = [c[0] for c in GPU_CASES]


def gpu_case(case):
    """(frames, psfs or None) of a GPU_CASES entry"""
    _, M, N, rows, cols, _, _, _, with_psfs, shifts, seed = case
    frames, psfs = short_case(M, N, rows, cols, len(shifts), shifts, seed)
    return frames, (psfs if with_psfs else None)
