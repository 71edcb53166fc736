// fdr_rlstop.hip -- the fit trace of Richardson-Lucy (fdr_richardson_lucy_auto_f32*): the ratio pass of an iteration, run as
// ROW_OUT_RL_RATIO_STAT (fdr_panel_rows.hip), leaves one pair of double partials per workgroup,
//
//     res = sum w (d+ - c)^2,   kl = sum w (c - d+ + d+ ln(d+ / c))      over the window, c = blur(y_k)
//
// and the one kernel here folds them into trace[k] = (res_k, kl_k).  No atomics: every sum runs in a fixed order, so a trace is
// bit-identical from call to call.
#include "fdr_kernels.hpp"

namespace fdr {

constexpr int kRsThreads = 256;

// one workgroup: thread t adds the pairs t, t + 256, ... in order, then a fixed tree; out[0] = res, out[1] = kl
__global__ __launch_bounds__(kRsThreads) void rlstop_fold_kernel(const double2* __restrict__ part, int n, double* __restrict__ out) {
    __shared__ double red[2][kRsThreads];
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < n; k += kRsThreads) {
        const double2 v = part[k];
        a += v.x;
        b += v.y;
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int h = kRsThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[0][threadIdx.x] += red[0][threadIdx.x + h];
            red[1][threadIdx.x] += red[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = red[0][0];
        out[1] = red[1][0];
    }
}

hipError_t launch_rlstop_fold(const double* part, int n, double* out, hipStream_t s) {
    if (n <= 0 || !part || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rlstop_fold_kernel, dim3(1), dim3(kRsThreads), 0, s, reinterpret_cast<const double2*>(part), n, out);
    return hipGetLastError();
}

}  // namespace fdr
