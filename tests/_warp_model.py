"""numpy replay of the affine warp (csrc/fdr_image.hip: warp_affine_kernel, cv::warpAffine of the drop-in surface with its defaults,
and psf_motion_kernel, which is the same recipe on an analytic source):

    invert the forward 2 x 3 matrix in double, as invert_affine does;
    X0, Y0 (per row, + 16) and adelta, bdelta (per column) by rint with saturation to int32, held as int64;
    X = (X0 + adelta) >> 5, the pixel X >> 5 saturated to short, the fraction X & 31 (Y likewise);
    the four weights and the four products in float32, the sum as ((t0 + t1) + t2) + t3; zero outside the source.

Every step is an exactly rounded float32 or integer operation, so the device must equal the model bit for bit.  The model asserts that
X0 + adelta and Y0 + bdelta stay inside int32 (beyond that the kernel's int sum is not defined).

Pinned in test_aux_kernels_host.py before it judges the device: bit-equal to oracle.motion_blur_kernel on PSF_SIZES x PSF_ANGLES, and
within 1/16 of an exact float64 bilinear interpolation at the true inverse map on MATRICES; four fault variants must fail those pins."""
import numpy as np

PSF_SIZES = (1, 2, 3, 7, 8, 15, 40, 50, 64, 101, 513)
PSF_ANGLES = (0, 10, 30, 45, 90, 123.4, 180, 270, -30, 405, 359.999)

FAULTS = ("no_plus16", "w1_w2_swapped", "not_inverted", "floor")


def rotation_matrix(center, angle, scale):
    """cv::getRotationMatrix2D: center = (x, y) rounded to float as cv::Point2f, angle in degrees"""
    a = float(angle) * 3.1415926535897932384626433832795 / 180.0
    alpha, beta = np.cos(a) * scale, np.sin(a) * scale
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


# the three general matrices of the host pins and the device test (a 37 x 53 picture warped to 61 x 47)
MATRICES = {
    "rot17_scale1.3": rotation_matrix((20, 11), 17.0, 1.3),
    "shear": np.array([[1, 0.25, 3.3], [-0.1, 0.9, -2.7]], dtype=np.float64),
    "shrink": np.array([[0.4, 0, 0.5], [0, 0.6, 0.25]], dtype=np.float64),
}
SRC_SHAPE, DSIZE = (37, 53), (61, 47)  # rows x cols; cv::Size(width, height)
EXACT_GAP = 1.0 / 16                   # two 1/32 coordinate steps against a unit gradient


def invert_affine(fwd):
    """invertAffineTransform as cv::warpAffine applies it, in double and in its operation order"""
    M = [float(v) for v in np.asarray(fwd, dtype=np.float64).reshape(6)]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return M


def _cv_round(v, floor=False):
    """cvRound on a float64 array: round half to even, saturated to int32; returned as int64"""
    r = np.floor(v) if floor else np.rint(v)
    r = np.where(v >= 2147483647.0, 2147483647.0, np.where(v <= -2147483648.0, -2147483648.0, r))
    return r.astype(np.int64)


def warp_model(src, M, dsize, fault=None):
    """src float32 [rows, cols], M the forward 2 x 3 matrix, dsize = (width, height) -> float32 [height, width]"""
    assert fault is None or fault in FAULTS
    src = np.asarray(src, dtype=np.float32)
    srows, scols = src.shape
    dcols, drows = int(dsize[0]), int(dsize[1])
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)] if fault == "not_inverted" else invert_affine(M)
    floor = fault == "floor"
    x = np.arange(dcols, dtype=np.float64)[None, :]
    y = np.arange(drows, dtype=np.float64)[:, None]
    delta = 0 if fault == "no_plus16" else 16
    X0 = _cv_round((m[1] * y + m[2]) * 1024.0, floor) + delta
    Y0 = _cv_round((m[4] * y + m[5]) * 1024.0, floor) + delta
    adelta = _cv_round(m[0] * x * 1024.0, floor)
    bdelta = _cv_round(m[3] * x * 1024.0, floor)
    XS, YS = X0 + adelta, Y0 + bdelta
    assert max(np.abs(XS).max(), np.abs(YS).max()) < 2 ** 31, "coordinates times 1024 leave int32"
    X, Y = XS >> 5, YS >> 5
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx = (X & 31).astype(np.float32) * np.float32(1.0 / 32.0)
    fy = (Y & 31).astype(np.float32) * np.float32(1.0 / 32.0)
    one = np.float32(1)
    vx0, vx1, vy0, vy1 = one - fx, fx, one - fy, fy
    w0, w1, w2, w3 = vy0 * vx0, vy0 * vx1, vy1 * vx0, vy1 * vx1
    if fault == "w1_w2_swapped":
        w1, w2 = w2, w1

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < srows) & (xx >= 0) & (xx < scols)
        return np.where(inside, src[np.clip(yy, 0, srows - 1), np.clip(xx, 0, scols - 1)], np.float32(0))

    t0, t1, t2, t3 = tap(sy, sx) * w0, tap(sy, sx + 1) * w1, tap(sy + 1, sx) * w2, tap(sy + 1, sx + 1) * w3
    out = ((t0 + t1) + t2) + t3
    assert out.dtype == np.float32 and out.shape == (drows, dcols)
    return out


def psf_model(size, angle, fault=None):
    """utils.hpp:15-24 motionBlurKernel: row size / 2 of a size x size plane set to 1 / size, rotated about (size / 2, size / 2)"""
    k = np.zeros((size, size), dtype=np.float32)
    k[size // 2, :] = np.float32(1.0 / size)
    return warp_model(k, rotation_matrix((size // 2, size // 2), angle, 1.0), (size, size), fault)


def bilinear_exact(src, M, dsize):
    """float64 bilinear interpolation of src at the true inverse map of M (no fixed point), zero outside the source"""
    src = np.asarray(src, dtype=np.float64)
    srows, scols = src.shape
    fwd = np.vstack([np.asarray(M, dtype=np.float64).reshape(2, 3), [0, 0, 1]])
    inv = np.linalg.inv(fwd)
    x = np.arange(int(dsize[0]), dtype=np.float64)[None, :]
    y = np.arange(int(dsize[1]), dtype=np.float64)[:, None]
    u = inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]
    v = inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]
    iu, iv = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = u - iu, v - iv

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < srows) & (xx >= 0) & (xx < scols)
        return np.where(inside, src[np.clip(yy, 0, srows - 1), np.clip(xx, 0, scols - 1)], 0.0)

    return ((1 - fv) * ((1 - fu) * tap(iv, iu) + fu * tap(iv, iu + 1)) + fv * ((1 - fu) * tap(iv + 1, iu) + fu * tap(iv + 1, iu + 1)))
