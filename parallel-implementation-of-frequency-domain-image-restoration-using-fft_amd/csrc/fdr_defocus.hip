// fdr_defocus.hip -- the defocus estimate (fdr_psf_disk*, fdr_estimate_defocus_f32*, fdr_estimate_blur_f32*): the disk PSF and the
// angular median of the power cepstrum (fdr_motion.hip) on circles.
//
//     disk: out[i, j] = share of pixel (i, j)'s unit square inside the disk of radius R about c = size / 2, counted on 16 x 16
//           sub-samples in integers, over the total count
//     T[d] = median over a of S[a, d],  S the score table of fdr_motion.hip (c bilinearly at row -d sin(theta_a), column d cos(theta_a))
//
// A uniform disk has rings of zeros in |G|; in c they show as a negative ring of radius about 2 R, which T has as its minimum.
// No atomics: the count is an integer sum, the median a sort.
#include "fdr_kernels.hpp"

namespace fdr {

constexpr int kDfThreads = 256;
constexpr int kDiskThreads = 1024;
constexpr int kDiskSub = 16;  // sub-samples per pixel and axis; coordinates in units of 1 / (2 kDiskSub) px

__device__ __forceinline__ bool disk_inside(int X, int Y, double q) { return (double)(X * X + Y * Y) <= q; }

// one workgroup; thread t takes pixels t, t + 1024, ...: the count of each pixel into out (as an integer), the fixed-order fold of
// the counts, then out = count / total in double, rounded once.  q = (2 kDiskSub radius)^2.  A pixel whose four corners lie inside
// holds all 256 sub-samples (the disk is convex), one whose nearest point lies outside none: both skip the count.
__global__ __launch_bounds__(kDiskThreads) void psf_disk_kernel(int size, double q, float* __restrict__ out) {
    __shared__ int red[kDiskThreads];
    const int n = size * size, c = size / 2;
    int sum = 0;
    for (int p = threadIdx.x; p < n; p += kDiskThreads) {
        const int y0 = 2 * kDiskSub * (p / size - c) - kDiskSub, x0 = 2 * kDiskSub * (p % size - c) - kDiskSub;  // the pixel's low corner
        const int y1 = y0 + 2 * kDiskSub, x1 = x0 + 2 * kDiskSub;
        const int ny = y0 > 0 ? y0 : (y1 < 0 ? y1 : 0), nx = x0 > 0 ? x0 : (x1 < 0 ? x1 : 0);  // the square's point nearest the centre
        int count = 0;
        if (disk_inside(x0, y0, q) && disk_inside(x1, y0, q) && disk_inside(x0, y1, q) && disk_inside(x1, y1, q)) {
            count = kDiskSub * kDiskSub;
        } else if (disk_inside(nx, ny, q)) {
            for (int k = 0; k < kDiskSub; ++k)
                for (int l = 0; l < kDiskSub; ++l) count += disk_inside(x0 + 2 * l + 1, y0 + 2 * k + 1, q) ? 1 : 0;
        }
        out[p] = __int_as_float(count);
        sum += count;
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int h = kDiskThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    const double total = (double)red[0];
    for (int p = threadIdx.x; p < n; p += kDiskThreads) out[p] = (float)((double)__float_as_int(out[p]) / total);  // this thread's own pixels
}

// one workgroup per diameter d = min_diameter + blockIdx.x: the column S[., d] gathered from the real parts of the cepstrum plane (the
// arithmetic of motion_score_kernel), sorted ascending in LDS by a bitonic network on n_pad = the next power of two (+inf above
// n_angles), T[d] = 0.5 (s[(n - 1) / 2] + s[n / 2]).  trig = cos[n_angles] then sin[n_angles]; n_angles <= kDefocusMaxAngles.
// A compare-exchange at distance j < 32 would read its low elements 64 dwords wide per 32 lanes, two per bank; the lanes whose pair
// lies in the upper 32 dwords read the high element first instead, so each of the two reads covers every bank once.
__global__ __launch_bounds__(kDfThreads) void defocus_profile_kernel(const float2* __restrict__ plane, int M, int N, const double* __restrict__ trig,
                                                                     int n_angles, int n_pad, int min_diameter, float* __restrict__ T) {
    __shared__ float col[kDefocusMaxAngles];
    const int d = min_diameter + blockIdx.x;
    for (int a = threadIdx.x; a < n_pad; a += kDfThreads) {
        float v = __builtin_inff();
        if (a < n_angles) {
            const double y = -(double)d * trig[n_angles + a], x = (double)d * trig[a];
            const double fy0 = floor(y), fx0 = floor(x);
            const float fy = (float)(y - fy0), fx = (float)(x - fx0);
            int i0 = (int)fy0 % M, j0 = (int)fx0 % N;
            if (i0 < 0) i0 += M;
            if (j0 < 0) j0 += N;
            const int i1 = i0 + 1 == M ? 0 : i0 + 1, j1 = j0 + 1 == N ? 0 : j0 + 1;
            const float c00 = plane[(size_t)i0 * N + j0].x, c01 = plane[(size_t)i0 * N + j1].x;
            const float c10 = plane[(size_t)i1 * N + j0].x, c11 = plane[(size_t)i1 * N + j1].x;
            const float r0 = (1.f - fx) * c00 + fx * c01, r1 = (1.f - fx) * c10 + fx * c11;
            v = (1.f - fy) * r0 + fy * r1;
        }
        col[a] = v;
    }
    __syncthreads();
    for (int k = 2; k <= n_pad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < n_pad / 2; t += kDfThreads) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const bool high_first = j < 32 && (lo & 32) != 0;
                const int first = high_first ? hi : lo, second = high_first ? lo : hi;
                const float f = col[first], g = col[second];
                const float vlo = high_first ? g : f, vhi = high_first ? f : g;
                const bool ascending = (lo & k) == 0;
                if ((vlo > vhi) == ascending) {
                    col[first] = g;
                    col[second] = f;
                }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) T[blockIdx.x] = 0.5f * (col[(n_angles - 1) / 2] + col[n_angles / 2]);
}

hipError_t launch_psf_disk(int size, double radius, float* d_out, hipStream_t s) {
    if (size <= 0 || size > kDiskMaxSize || !(radius > 0.0)) return hipErrorInvalidValue;
    const double e = 2.0 * kDiskSub * radius;
    hipLaunchKernelGGL(psf_disk_kernel, dim3(1), dim3(kDiskThreads), 0, s, size, e * e, d_out);
    return hipGetLastError();
}

hipError_t launch_defocus_profile(const float2* plane, int M, int N, const double* trig, int n_angles, int min_diameter, int n_diameters,
                                  float* T, hipStream_t s) {
    if (n_angles <= 0 || n_angles > kDefocusMaxAngles || n_diameters <= 0) return hipErrorInvalidValue;
    int n_pad = 1;
    while (n_pad < n_angles) n_pad <<= 1;
    hipLaunchKernelGGL(defocus_profile_kernel, dim3((unsigned)n_diameters), dim3(kDfThreads), 0, s, plane, M, N, trig, n_angles, n_pad,
                       min_diameter, T);
    return hipGetLastError();
}

}  // namespace fdr
