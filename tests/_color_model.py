"""numpy model of the colour epilogue (csrc/fdr_color.hip: lab_mean_kernel + lab_apply_kernel behind fdr_white_balance_u8*):
BGR -> Lab, L of the restored picture scaled so that its mean meets the original's and clamped to [0, 100], Lab -> BGR, times 255.

    epilogue(orig, rest, dtype)  the three channels (B, G, R on the last axis) times 255 BEFORE rounding, as float64

One function of the kernel's formulae, operation by operation and in the kernel's order, evaluated in `dtype`: float32 restates the
kernel (every constant the float of its literal, every product and sum rounded to float32), float64 is the judge.  In both variants
the two L means are taken in float64 (the kernel sums doubles); the float32 variant rounds the gain once to float32, as the kernel does.

The rule the device is held to (test_aux_kernels_gpu.py), with v64 = epilogue(..., float64):

    |got - v64| <= 0.5 + DELTA      for every 8-bit value

so a device value may differ from rint(v64) only where v64 lies within DELTA of a tie.  DELTA is measured, not chosen: the largest
|v32 - v64| of the float32 variant against the float64 one over every input and shape below (test_aux_kernels_host.py measures it
again and fails if it has grown), times FACTOR for the device's powf and cbrtf, which are specified to a few ulp where numpy's are
within one (their real share of the gap is unmeasured).  Pinned on the CPU, fault variants included, before it judges the device."""
import numpy as np

# Largest |v32 - v64| over INPUTS x SHAPES and the two large shapes (uniform and gain_gt1 only), as test_aux_kernels_host.py
# measures it: 3.16e-3 on "uniform" (520 x 517), 2.2e-3 on "out_of_range", 2.0e-3 on "binary" (a channel near 0 after the matrix,
# where lin_to_srgb's slope of 12.92 x 255 meets the cancellation in 3.24 X - 1.54 Y - 0.50 Z); 3.7e-5 to 4.3e-4 on the other inputs.
MEASURED_GAP = 3.2e-3
FACTOR = 4          # the device's powf / cbrtf: a few ulp against numpy's one
DELTA = FACTOR * MEASURED_GAP
DELTA_MAX = 0.02    # above this the rule stops seeing a fourth-digit constant

INPUTS = ("uniform", "dark", "gain_gt1", "gain_lt1", "out_of_range", "rest_zero", "binary", "grey_ramp")
SHAPES = ((1, 1), (1, 257), (3, 5), (97, 203))
# 520 x 517 = 1051 workgroups' worth of pixels: the cap of 1024 partials; 1025 x 1024: lab_apply_kernel's loop takes a second trip
LARGE_SHAPES = ((520, 517), (1025, 1024))
LARGE_INPUTS = ("uniform", "gain_gt1")

FAULTS = ("y_green", "xn", "matrix_entry", "finv_threshold", "no_l_clamp", "ab_swapped", "br_swapped")


def color_input(name, rows, cols):
    """(orig, rest): two float32 arrays [3, rows, cols] (B, G, R planes), seeded by name and shape"""
    rng = np.random.default_rng([INPUTS.index(name), rows, cols])
    u = lambda lo, hi: (lo + (hi - lo) * rng.random((3, rows, cols))).astype(np.float32)
    if name == "uniform":
        return u(0, 1), u(0, 1)
    if name == "dark":            # the linear branches of srgb_to_lin, lab_f, L and lin_to_srgb
        return u(0, 0.06), u(0, 0.06)
    if name == "gain_gt1":        # bright original, dark restored: L clamps at 100, out-of-gamut values clamp
        return u(0.5, 1), u(0, 0.6)
    if name == "gain_lt1":
        return u(0, 0.3), u(0.4, 1)
    if name == "out_of_range":    # clamp01
        return u(-0.5, 1.5), u(-0.5, 1.5)
    if name == "rest_zero":       # gain = mean / 1e-6, output all zero
        return u(0, 1), np.zeros((3, rows, cols), dtype=np.float32)
    if name == "binary":
        return (rng.random((3, rows, cols)) < 0.5).astype(np.float32), (rng.random((3, rows, cols)) < 0.5).astype(np.float32)
    if name == "grey_ramp":
        ramp = np.linspace(0.0, 1.0, rows * cols, dtype=np.float64).reshape(rows, cols)
        grey = lambda p: np.repeat(p[None].astype(np.float32), 3, axis=0)
        return grey(ramp), grey(0.8 * ramp[::-1, ::-1] ** 1.5)
    raise ValueError(name)


def epilogue(orig, rest, dtype, fault=None):
    """orig, rest: [3, rows, cols] (B, G, R).  Returns float64 [rows, cols, 3]: B, G, R times 255, unrounded.
    fault (test_aux_kernels_host.py only): one of FAULTS."""
    T = np.dtype(dtype).type
    c = lambda v: T(v)  # a constant: the `dtype` of its decimal literal
    assert fault is None or fault in FAULTS
    Xn = c(0.950456)
    Zn = c(1.088754)
    Xn_fwd = c(0.9505) if fault == "xn" else Xn
    yg = c(0.7152) if fault == "y_green" else c(0.715160)
    rz = c(0.4985) if fault == "matrix_entry" else c(0.498535)
    finv_t = c(0.2) if fault == "finv_threshold" else c(0.206893)
    k16_116 = c(16) / c(116)

    def clamp01(v):
        return np.minimum(np.maximum(v, c(0)), c(1))

    def srgb_to_lin(v):
        return np.where(v <= c(0.04045), v / c(12.92), np.power((v + c(0.055)) / c(1.055), c(2.4)))

    def lin_to_srgb(v):
        with np.errstate(all="ignore"):
            return np.where(v <= c(0.0031308), c(12.92) * v, c(1.055) * np.power(v, c(1) / c(2.4)) - c(0.055))

    def lab_f(t):
        return np.where(t > c(0.008856), np.cbrt(t), c(7.787) * t + k16_116)

    def lab_finv(t):
        return np.where(t > finv_t, t * t * t, (t - k16_116) / c(7.787))

    def bgr_to_lab(p):
        b, g, r = (srgb_to_lin(clamp01(np.asarray(ch, dtype=T))) for ch in p)
        X = (c(0.412453) * r + c(0.357580) * g + c(0.180423) * b) / Xn_fwd
        Y = c(0.212671) * r + yg * g + c(0.072169) * b
        Z = (c(0.019334) * r + c(0.119193) * g + c(0.950227) * b) / Zn
        fx, fy, fz = lab_f(X), lab_f(Y), lab_f(Z)
        L = np.where(Y > c(0.008856), c(116) * fy - c(16), c(903.3) * Y)
        return L, c(500) * (fx - fy), c(200) * (fy - fz)

    Lo = bgr_to_lab(orig)[0]
    L, a, b = bgr_to_lab(rest)
    assert Lo.dtype == T and L.dtype == T and a.dtype == T
    n = float(L.size)
    gain = (np.sum(Lo, dtype=np.float64) / n) / (np.sum(L, dtype=np.float64) / n + 1e-6)
    if T is np.float32:
        gain = np.float32(gain)
    L = L * T(gain)
    if fault != "no_l_clamp":
        L = np.minimum(L, c(100))
    L = np.maximum(L, c(0))
    if fault == "ab_swapped":
        a, b = b, a

    fy = (L + c(16)) / c(116)
    fx, fz = fy + a / c(500), fy - b / c(200)
    Y = np.where(L > c(7.9996), fy * fy * fy, L / c(903.3))
    X, Z = lab_finv(fx) * Xn, lab_finv(fz) * Zn
    r = c(3.240479) * X - c(1.537150) * Y - rz * Z
    g = c(-0.969256) * X + c(1.875991) * Y + c(0.041556) * Z
    bb = c(0.055648) * X - c(0.204043) * Y + c(1.057311) * Z
    out = [lin_to_srgb(clamp01(ch)) for ch in (bb, g, r)]
    assert all(ch.dtype == T for ch in out)
    if fault == "br_swapped":
        out = out[::-1]
    return np.stack([ch.astype(np.float64) * 255.0 for ch in out], axis=-1)


def quantize(v, truncate=False):
    """convertTo(CV_8U): round half to even and saturate (truncate: the fault of test_aux_kernels_host.py)"""
    q = np.trunc(v) if truncate else np.rint(v)
    return np.clip(q, 0, 255).astype(np.uint8)


def rule(got_u8, v64, delta=DELTA):
    """(number of values that break |got - v64| <= 0.5 + delta, the largest |got - v64|)"""
    d = np.abs(got_u8.astype(np.float64) - v64)
    return int(np.count_nonzero(~(d <= 0.5 + delta))), float(d.max())
