// fdr_image.hip -- image utilities: the motion PSF and cv::warpAffine (one fixed-point bilinear replay), the counter-based
// synthetic image and the deterministic checksum of the batch runs.
#include "fdr_fft_core.hpp"
#include "fdr_kernels.hpp"

namespace fdr {

// ---- utils.hpp:15-24 motionBlurKernel on the device ----
// The source kernel (row size/2 set to 1/size) is analytic; the inverse affine map is prepared on
// the host in double exactly as cv::getRotationMatrix2D + cv::warpAffine do, and each destination
// pixel replays WarpAffineInvoker's 10-bit fixed-point coordinates and remapBilinear's 32x32
// float weights with BORDER_CONSTANT 0.
struct PsfMap { double m[6]; };

// the forward 2 x 3 matrix inverted (dst -> src) as invertAffineTransform does inside cv::warpAffine, in double on the host
static PsfMap invert_affine(const double fwd[6]) {
    double M[6];
    for (int i = 0; i < 6; ++i) M[i] = fwd[i];
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
    PsfMap map;
    for (int i = 0; i < 6; ++i) map.m[i] = M[i];
    return map;
}

__device__ __forceinline__ int cv_round_dev(double v) {
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return (-2147483647 - 1);
    return __double2int_rn(v);
}

// WarpAffineInvoker's source position of destination pixel (x, y) under the inverse map, declared in the caller's scope: the
// integer pixel (sx, sy) = SAT(X >> 5), SAT(Y >> 5) and remapBilinear's four weights of the 1/32 fractions (w0 = (sy, sx),
// w1 = (sy, sx + 1), w2 and w3 the row below).  SAT is what the caller does to the pixel: the warp saturates it to short, the PSF
// takes it as it is (the cast `int`: an identity function in its place changed psf_motion_kernel's schedule).  A macro with the
// statements in this order: as a function, and as a macro that left the pixel to the caller, the block changed the schedule of
// one of the two kernels.
#define FDR_AFFINE_BILINEAR(map, x, y, SAT)                                                                                \
    const int X0 = cv_round_dev((map.m[1] * y + map.m[2]) * 1024.0) + 16;                                                  \
    const int Y0 = cv_round_dev((map.m[4] * y + map.m[5]) * 1024.0) + 16;                                                  \
    const int adelta = cv_round_dev(map.m[0] * x * 1024.0), bdelta = cv_round_dev(map.m[3] * x * 1024.0);                  \
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;                                                              \
    const int sx = SAT(X >> 5), sy = SAT(Y >> 5), ax = X & 31, ay = Y & 31;                                                \
    const float fx = ax * (1.f / 32.f), fy = ay * (1.f / 32.f);                                                            \
    const float vx0 = 1.f - fx, vx1 = fx, vy0 = 1.f - fy, vy1 = fy;                                                        \
    const float w0 = vy0 * vx0, w1 = vy0 * vx1, w2 = vy1 * vx0, w3 = vy1 * vx1

__global__ void psf_motion_kernel(int size, PsfMap map, float* __restrict__ out) {
    const float line = (float)(1.0 / (double)size);
    const int cy = size / 2;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < size * size; idx += gridDim.x * blockDim.x) {
        const int y = idx / size, x = idx % size;
        FDR_AFFINE_BILINEAR(map, x, y, int);  // SAT = the functional cast int(..): the pixel as it is
        const bool x0in = sx >= 0 && sx < size, x1in = sx + 1 >= 0 && sx + 1 < size;
        const float s00 = (sy == cy && x0in) ? line : 0.f, s01 = (sy == cy && x1in) ? line : 0.f;
        const float s10 = (sy + 1 == cy && x0in) ? line : 0.f, s11 = (sy + 1 == cy && x1in) ? line : 0.f;
        const float t0 = s00 * w0, t1 = s01 * w1, t2 = s10 * w2, t3 = s11 * w3;
        float acc = t0 + t1;
        acc = acc + t2;
        acc = acc + t3;
        out[idx] = acc;
    }
}

hipError_t launch_psf_motion(int size, double angle_deg, float* d_out, hipStream_t s) {
    const double PI = 3.1415926535897932384626433832795;
    const double a = angle_deg * PI / 180.0;
    const double alpha = cos(a), beta = sin(a);
    const double cx = (double)(float)(size / 2), cy = (double)(float)(size / 2);
    const double M[6] = {alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy};  // cv::getRotationMatrix2D
    const PsfMap map = invert_affine(M);
    int blocks = (size * size + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(psf_motion_kernel, dim3(blocks), dim3(256), 0, s, size, map, d_out);
    return hipGetLastError();
}

// ---- cv::warpAffine(src, dst, M, dsize) with its defaults (INTER_LINEAR, BORDER_CONSTANT 0) for a single-channel float
// image, as utils.hpp:22 calls it: the same fixed-point replay as psf_motion_kernel, the source read from memory.
// `map` is the INVERTED matrix (dst -> src), prepared on the host in double as cv::warpAffine does.
__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
__global__ void warp_affine_kernel(const float* __restrict__ src, int srows, int scols, int sstride, PsfMap map, float* __restrict__ dst,
                                   int drows, int dcols, int dstride) {
    const long long total = (long long)drows * dcols;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(idx / dcols), x = (int)(idx % dcols);
        FDR_AFFINE_BILINEAR(map, x, y, sat_short);
        const bool x0in = sx >= 0 && sx < scols, x1in = sx + 1 >= 0 && sx + 1 < scols;
        const bool y0in = sy >= 0 && sy < srows, y1in = sy + 1 >= 0 && sy + 1 < srows;
        const float s00 = (y0in && x0in) ? src[(size_t)sy * sstride + sx] : 0.f;
        const float s01 = (y0in && x1in) ? src[(size_t)sy * sstride + sx + 1] : 0.f;
        const float s10 = (y1in && x0in) ? src[(size_t)(sy + 1) * sstride + sx] : 0.f;
        const float s11 = (y1in && x1in) ? src[(size_t)(sy + 1) * sstride + sx + 1] : 0.f;
        const float t0 = s00 * w0, t1 = s01 * w1, t2 = s10 * w2, t3 = s11 * w3;
        float acc = t0 + t1;
        acc = acc + t2;
        acc = acc + t3;
        dst[(size_t)y * dstride + x] = acc;
    }
}

hipError_t launch_warp_affine(const float* src, int srows, int scols, int sstride, const double fwd[6], float* dst, int drows, int dcols,
                              int dstride, hipStream_t s) {
    if (drows <= 0 || dcols <= 0) return hipSuccess;
    const PsfMap map = invert_affine(fwd);
    long long blocks = ((long long)drows * dcols + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(warp_affine_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, srows, scols, sstride, map, dst, drows, dcols, dstride);
    return hipGetLastError();
}

// ---- counter-based synthetic image: top 24 bits of splitmix64(seed + first + i) / 2^24 ----
__global__ void synth_kernel(uint64_t seed, uint64_t first, size_t count, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t x = seed + first + i;
        x += 0x9E3779B97F4A7C15ULL;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
        x = x ^ (x >> 31);
        out[i] = (float)(x >> 40) * (1.0f / 16777216.0f);
    }
}

hipError_t launch_synth(uint64_t seed, uint64_t first, size_t count, float* d_out, hipStream_t s) {
    if (count == 0) return hipSuccess;
    size_t blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(synth_kernel, dim3((unsigned)blocks), dim3(256), 0, s, seed, first, count, d_out);
    return hipGetLastError();
}

// ---- deterministic checksum of `count` floats (fdr_batch_run): per-block partial sums in double, folded on the host ----
__global__ void checksum_kernel(const float* __restrict__ x, size_t count, double* __restrict__ part) {
    __shared__ double red[4];
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) acc += (double)x[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

hipError_t launch_checksum(const float* x, size_t count, double* part, hipStream_t s) {
    hipLaunchKernelGGL(checksum_kernel, dim3(kChecksumParts), dim3(256), 0, s, x, count, part);
    return hipGetLastError();
}

}  // namespace fdr
