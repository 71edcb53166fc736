// fdr_motion.hip -- the motion-blur estimate (fdr_cepstrum_f32*, fdr_estimate_motion_f32*): the power cepstrum of the windowed
// picture and the score table over (angle, length) that the host picks the blur from.
//
//     x = hann(rows) hann(cols)^T . img on the window, 0 elsewhere in the M x N plane;  eps = 1e-6 sum |x|
//     c = Re IDFT2(log(|G| + eps)),  G = DFT2(x)        (IDFT2 includes 1 / (M N))
//     S[a, l] = c bilinearly at row -l sin(theta_a), column l cos(theta_a), periodic
//
// Passes: the Hann tables, the window / pad pass (complex plane + per-workgroup sum |x| partials), a fixed-order fold of the
// partials, the plan's complex 2-D transform forward, log |G| in place (times 1 / (M N), the imaginary part 0), the transform
// inverse, then the score gather from the real parts (or, for fdr_cepstrum_*, the real part of the plane).  No float atomics:
// every reduction runs in a fixed order, so results are bit-identical from call to call.
#include "fdr_kernels.hpp"

namespace fdr {

constexpr int kMoThreads = 256;
constexpr int kMoPadCols = 4 * kMoThreads;  // columns of one pad workgroup (4 per thread, 256 apart: coalesced)

// h[k] = 0.5 - 0.5 cos(2 pi k / (n - 1)) (numpy.hanning) for n = rows (h[0 .. rows)) and n = cols (h[rows .. rows + cols)), in double
__global__ __launch_bounds__(kMoThreads) void motion_hann_kernel(float* __restrict__ h, int rows, int cols) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rows + cols) return;
    const int n = k < rows ? rows : cols, i = k < rows ? k : k - rows;
    h[k] = (float)(0.5 - 0.5 * cospi(2.0 * (double)i / (double)(n - 1)));
}

// one row (blockIdx.y) of kMoPadCols columns (blockIdx.x) of the M x N plane: w . img on the window, 0 elsewhere; the
// workgroup's sum |x| (double, fixed-order tree) to part[blockIdx.y * gridDim.x + blockIdx.x]
__global__ __launch_bounds__(kMoThreads) void motion_pad_kernel(const float* __restrict__ img, int rows, int cols, int stride,
                                                                const float* __restrict__ hann, float2* __restrict__ plane, int N,
                                                                double* __restrict__ part) {
    __shared__ double red[kMoThreads];
    const int i = blockIdx.y;
    const bool in_rows = i < rows;
    const float hr = in_rows ? hann[i] : 0.f;
    const float* src = img + (size_t)(in_rows ? i : 0) * stride;
    float2* dst = plane + (size_t)i * N;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = blockIdx.x * kMoPadCols + k * kMoThreads + threadIdx.x;
        if (j >= N) break;
        float v = 0.f;
        if (in_rows && j < cols) {
            const float w = hr * hann[rows + j];
            v = w * src[j];
        }
        acc += (double)fabsf(v);
        dst[j] = make_float2(v, 0.f);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = kMoThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// one workgroup: part[n] = sum of part[0 .. n) (thread t adds t, t + 256, ... in order, then a fixed tree)
__global__ __launch_bounds__(kMoThreads) void motion_fold_kernel(double* __restrict__ part, int n) {
    __shared__ double red[kMoThreads];
    double acc = 0.0;
    for (int k = threadIdx.x; k < n; k += kMoThreads) acc += part[k];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = kMoThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[n] = red[0];
}

// G -> (log(|G| + eps) / (M N), 0) in place, eps = 1e-6 * (*sum); an all-zero window (sum 0) gives 0 (no log(0)).  |G| <= sum |x|:
// its square stays far inside the float range for any picture the plans take (2^70 at 8192^2 and 8-bit data)
__global__ __launch_bounds__(kMoThreads) void motion_log_kernel(float2* __restrict__ plane, size_t count, const double* __restrict__ sum,
                                                                float inv_mn) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const double s = *sum;
    const float eps = (float)(1e-6 * s);
    const float2 g = plane[k];
    const float re2 = g.x * g.x, im2 = g.y * g.y;
    const float mag = sqrtf(re2 + im2);
    const float v = s > 0.0 ? logf(mag + eps) * inv_mn : 0.f;
    plane[k] = make_float2(v, 0.f);
}

// one lane per (angle a, length l): S = c at (y, x) = (-l sin, l cos) bilinearly, periodic; trig = cos[n_angles] then sin[n_angles]
__global__ __launch_bounds__(kMoThreads) void motion_score_kernel(const float2* __restrict__ plane, int M, int N, const double* __restrict__ trig,
                                                                  int n_angles, int min_length, int n_lengths, float* __restrict__ table) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_angles * n_lengths) return;
    const int a = k / n_lengths, l = min_length + (k - a * n_lengths);
    const double y = -(double)l * trig[n_angles + a], x = (double)l * trig[a];
    const double fy0 = floor(y), fx0 = floor(x);
    const float fy = (float)(y - fy0), fx = (float)(x - fx0);
    int i0 = (int)fy0 % M, j0 = (int)fx0 % N;
    if (i0 < 0) i0 += M;
    if (j0 < 0) j0 += N;
    const int i1 = i0 + 1 == M ? 0 : i0 + 1, j1 = j0 + 1 == N ? 0 : j0 + 1;
    const float c00 = plane[(size_t)i0 * N + j0].x, c01 = plane[(size_t)i0 * N + j1].x;
    const float c10 = plane[(size_t)i1 * N + j0].x, c11 = plane[(size_t)i1 * N + j1].x;
    const float r0 = (1.f - fx) * c00 + fx * c01, r1 = (1.f - fx) * c10 + fx * c11;
    table[k] = (1.f - fy) * r0 + fy * r1;
}

int motion_pad_partials(int M, int N) { return M * ((N + kMoPadCols - 1) / kMoPadCols); }

hipError_t launch_motion_hann(float* hann, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(motion_hann_kernel, dim3((unsigned)((rows + cols + kMoThreads - 1) / kMoThreads)), dim3(kMoThreads), 0, s, hann, rows,
                       cols);
    return hipGetLastError();
}

hipError_t launch_motion_fold(double* part, int n, hipStream_t s) {
    hipLaunchKernelGGL(motion_fold_kernel, dim3(1), dim3(kMoThreads), 0, s, part, n);
    return hipGetLastError();
}

hipError_t launch_motion_window(const float* img, int rows, int cols, int stride, float* hann, float2* plane, int M, int N, double* part,
                                hipStream_t s) {
    hipError_t e = launch_motion_hann(hann, rows, cols, s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((N + kMoPadCols - 1) / kMoPadCols), (unsigned)M);
    hipLaunchKernelGGL(motion_pad_kernel, grid, dim3(kMoThreads), 0, s, img, rows, cols, stride, (const float*)hann, plane, N, part);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_motion_fold(part, motion_pad_partials(M, N), s);
}

hipError_t launch_motion_log(float2* plane, int M, int N, const double* sum, hipStream_t s) {
    const size_t count = (size_t)M * N;
    const float inv_mn = (float)(1.0 / (double)count);
    hipLaunchKernelGGL(motion_log_kernel, dim3((unsigned)((count + kMoThreads - 1) / kMoThreads)), dim3(kMoThreads), 0, s, plane, count, sum,
                       inv_mn);
    return hipGetLastError();
}

hipError_t launch_motion_score(const float2* plane, int M, int N, const double* trig, int n_angles, int min_length, int n_lengths, float* table,
                               hipStream_t s) {
    const int lanes = n_angles * n_lengths;
    hipLaunchKernelGGL(motion_score_kernel, dim3((unsigned)((lanes + kMoThreads - 1) / kMoThreads)), dim3(kMoThreads), 0, s, plane, M, N, trig,
                       n_angles, min_length, n_lengths, table);
    return hipGetLastError();
}

}  // namespace fdr
