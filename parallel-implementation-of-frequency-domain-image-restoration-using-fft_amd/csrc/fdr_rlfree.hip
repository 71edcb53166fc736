// fdr_rlfree.hip -- the small kernels of free-boundary, weighted Richardson-Lucy (fdr_richardson_lucy_free_f32*): the estimate u
// lives on the whole M x N plan, the data d (window rows x cols, weights m in [0, 1]) constrain it inside the window only, and the
// coverage alpha = fullblur^T(pad(m)) renormalises each update:
//
//     dw = m max(d, 0);  wgt = alpha > sigma ? 1 / alpha : 0;  u = alpha > sigma ? sum(dw) / sum(m) : 0
//     n times:  c = window(fullblur(u));  r = c > tau ? dw / c : 0;  u = max(u wgt fullblur^T(pad(r)), 0)
//
// The transforms are the operator passes of fdr_panel_rows.hip (the weighted update is a kind of the inverse row pass there).  Here:
// the setup pass (dw, W = m dense, and the two sums as per-workgroup double partials), their fixed-order fold, the start (wgt and
// u from alpha in one pointwise pass) and the crop of the result.  No float atomics: every sum runs in a fixed order.
#include "fdr_kernels.hpp"

namespace fdr {

constexpr int kRfThreads = 256;
constexpr int kRfCols = 4 * kRfThreads;  // columns of one setup workgroup (4 per thread, 256 apart: coalesced)

// one row (blockIdx.y) of kRfCols columns (blockIdx.x) of the window: dw and W (row stride cols; W may be m itself: a lane reads the
// element it writes), the workgroup's sums (double, fixed-order tree) to part[b] and part[n + b], b = blockIdx.y * gridDim.x + blockIdx.x
__global__ __launch_bounds__(kRfThreads) void rlfree_setup_kernel(const float* __restrict__ d, int stride, const float* m, int mstride, int cols,
                                                                  float* __restrict__ dw, float* W, double* __restrict__ part, int n) {
    __shared__ double red[2][kRfThreads];
    const size_t y = blockIdx.y;
    double sd = 0.0, sw = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = blockIdx.x * kRfCols + k * kRfThreads + threadIdx.x;
        if (x >= cols) break;
        const float w = m ? m[y * mstride + x] : 1.f;
        const float v = w * fmaxf(d[y * stride + x], 0.f);
        dw[y * cols + x] = v;
        W[y * cols + x] = w;
        sd += (double)v;
        sw += (double)w;
    }
    red[0][threadIdx.x] = sd;
    red[1][threadIdx.x] = sw;
    __syncthreads();
    for (int h = kRfThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[0][threadIdx.x] += red[0][threadIdx.x + h];
            red[1][threadIdx.x] += red[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const size_t b = y * gridDim.x + blockIdx.x;
        part[b] = red[0][0];
        part[(size_t)n + b] = red[1][0];
    }
}

// one workgroup: part[2 n] = sum of part[0 .. n), part[2 n + 1] = sum of part[n .. 2 n) (thread t adds t, t + 256, ... in order,
// then a fixed tree)
__global__ __launch_bounds__(kRfThreads) void rlfree_fold_kernel(double* __restrict__ part, int n) {
    __shared__ double red[2][kRfThreads];
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < n; k += kRfThreads) {
        a += part[k];
        b += part[(size_t)n + k];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int h = kRfThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[0][threadIdx.x] += red[0][threadIdx.x + h];
            red[1][threadIdx.x] += red[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * (size_t)n] = red[0][0];
        part[2 * (size_t)n + 1] = red[1][0];
    }
}

// four consecutive pixels per lane (count is a multiple of 4: N >= 32): alpha in `wgt` -> wgt and the start u
__global__ __launch_bounds__(kRfThreads) void rlfree_start_kernel(float4* __restrict__ wgt, float4* __restrict__ u, size_t count4, float sigma,
                                                                  const double* __restrict__ sums) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count4) return;
    const double sd = sums[0], sw = sums[1];
    const float mean = sw > 0.0 ? (float)(sd / sw) : 0.f;
    const float4 a = wgt[k];
    float4 w, v;
    w.x = a.x > sigma ? 1.f / a.x : 0.f;  v.x = a.x > sigma ? mean : 0.f;
    w.y = a.y > sigma ? 1.f / a.y : 0.f;  v.y = a.y > sigma ? mean : 0.f;
    w.z = a.z > sigma ? 1.f / a.z : 0.f;  v.z = a.z > sigma ? mean : 0.f;
    w.w = a.w > sigma ? 1.f / a.w : 0.f;  v.w = a.w > sigma ? mean : 0.f;
    wgt[k] = w;
    u[k] = v;
}

// the window rows x cols of u to out (one row per blockIdx.y)
__global__ __launch_bounds__(kRfThreads) void rlfree_crop_kernel(const float* __restrict__ u, int ustride, float* __restrict__ out, int cols,
                                                                 int out_stride) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t y = blockIdx.y;
    if (x < cols) out[y * out_stride + x] = u[y * ustride + x];
}

int rlfree_partials(int rows, int cols) { return rows * ((cols + kRfCols - 1) / kRfCols); }

hipError_t launch_rlfree_setup(const float* d, int stride, const float* m, int mstride, int rows, int cols, float* dw, float* W, double* part,
                               hipStream_t s) {
    if (rows <= 0 || cols <= 0) return hipErrorInvalidValue;
    const int n = rlfree_partials(rows, cols);
    const dim3 grid((unsigned)((cols + kRfCols - 1) / kRfCols), (unsigned)rows);
    hipLaunchKernelGGL(rlfree_setup_kernel, grid, dim3(kRfThreads), 0, s, d, stride, m, mstride, cols, dw, W, part, n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rlfree_fold_kernel, dim3(1), dim3(kRfThreads), 0, s, part, n);
    return hipGetLastError();
}

hipError_t launch_rlfree_start(float* wgt, float* u, size_t count, float sigma, const double* sums, hipStream_t s) {
    if ((count & 3) != 0) return hipErrorInvalidValue;
    const size_t count4 = count / 4;
    hipLaunchKernelGGL(rlfree_start_kernel, dim3((unsigned)((count4 + kRfThreads - 1) / kRfThreads)), dim3(kRfThreads), 0, s,
                       reinterpret_cast<float4*>(wgt), reinterpret_cast<float4*>(u), count4, sigma, sums);
    return hipGetLastError();
}

hipError_t launch_rlfree_crop(const float* u, int ustride, float* out, int rows, int cols, int out_stride, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(rlfree_crop_kernel, dim3((unsigned)((cols + kRfThreads - 1) / kRfThreads), (unsigned)rows), dim3(kRfThreads), 0, s, u,
                       ustride, out, cols, out_stride);
    return hipGetLastError();
}

}  // namespace fdr
