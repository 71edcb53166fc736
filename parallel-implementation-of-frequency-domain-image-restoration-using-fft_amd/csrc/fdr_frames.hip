// fdr_frames.hip -- the kernels of multi-frame Richardson-Lucy (fdr_richardson_lucy_frames_f32*, fdr_blur_frames_f32_dev): K exposures of
// one scene, each with its own PSF, restored jointly,
//
//     u <- u / alpha . sum_k H_k^T( w_k d_k / (H_k u) ),   alpha = sum_k H_k^T w_k.
//
// Every transform is an operator pass of fdr_panel_rows.hip / fdr_panel_cols.hip.  Pass B' leaves a slot's spectrum linear in its
// input (the packed DC / Nyquist column is a real-linear packing), so the K adjoint results are added HERE, in that domain, and go
// through one inverse row pass instead of K.  The sum is a streaming kernel: (n + 1) 4 bytes per float ((n + 2) 4 when it accumulates),
// 16 bytes per lane and request, no LDS, no atomics; the adds run in ascending k whatever the launch, so the result does not depend
// on how the frames are cut into launch groups.  Beside it the fold of the frames' (sum dw, sum W) pairs, in the same fixed order.
#include "fdr_kernels.hpp"

#include <cstdint>

namespace fdr {

constexpr int kFsThreads = 256;
constexpr int kFsMaxBlocks = 2048;  // 8 workgroups per CU; the rest of a long spectrum by the grid stride

// N sources (a constant: the loop unrolls, every pointer is a scalar of the argument block and the N loads of an element are in
// flight together); ACC: dst is read and every source added to it, otherwise source 0 starts the sum.  n4 float4 elements, then the
// float2 tail of an n_floats that is 2 modulo 4.  dst may be one of the sources (a lane reads element i of every operand before it
// writes it), so it is not __restrict__.
template <int N, bool ACC>
__global__ __launch_bounds__(kFsThreads) void frames_sum_kernel(float* dst, FrameSrcs srcs, size_t n4, int tail) {
    const size_t step = (size_t)gridDim.x * kFsThreads;
    for (size_t i = (size_t)blockIdx.x * kFsThreads + threadIdx.x; i < n4; i += step) {
        float4 x[N];
#pragma unroll
        for (int k = 0; k < N; ++k) x[k] = reinterpret_cast<const float4*>(srcs.p[k])[i];
        float4 v = ACC ? reinterpret_cast<const float4*>(dst)[i] : x[0];
#pragma unroll
        for (int k = ACC ? 0 : 1; k < N; ++k) { v.x += x[k].x; v.y += x[k].y; v.z += x[k].z; v.w += x[k].w; }
        reinterpret_cast<float4*>(dst)[i] = v;
    }
    if (tail && blockIdx.x == 0 && threadIdx.x == 0) {
        const size_t i = 2 * n4;  // in float2 elements
        float2 x[N];
#pragma unroll
        for (int k = 0; k < N; ++k) x[k] = reinterpret_cast<const float2*>(srcs.p[k])[i];
        float2 v = ACC ? reinterpret_cast<const float2*>(dst)[i] : x[0];
#pragma unroll
        for (int k = ACC ? 0 : 1; k < N; ++k) { v.x += x[k].x; v.y += x[k].y; }
        reinterpret_cast<float2*>(dst)[i] = v;
    }
}

// one lane: out[j] = sums[j] + sums[pitch + j] + ... in ascending k
__global__ void frames_fold_kernel(const double* __restrict__ sums, size_t pitch, int n, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double a = sums[0], b = sums[1];
    for (int k = 1; k < n; ++k) {
        a += sums[(size_t)k * pitch];
        b += sums[(size_t)k * pitch + 1];
    }
    out[0] = a;
    out[1] = b;
}

namespace {

template <int N>
hipError_t frames_sum_n(float* dst, const FrameSrcs& srcs, size_t n_floats, bool accumulate, hipStream_t s) {
    const size_t n4 = n_floats / 4;
    const int tail = (n_floats & 3) != 0;
    const size_t want = (n4 + kFsThreads - 1) / kFsThreads;
    const unsigned blocks = (unsigned)(want < 1 ? 1 : want > (size_t)kFsMaxBlocks ? (size_t)kFsMaxBlocks : want);
    if (accumulate)
        hipLaunchKernelGGL((frames_sum_kernel<N, true>), dim3(blocks), dim3(kFsThreads), 0, s, dst, srcs, n4, tail);
    else
        hipLaunchKernelGGL((frames_sum_kernel<N, false>), dim3(blocks), dim3(kFsThreads), 0, s, dst, srcs, n4, tail);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_frames_sum(float* dst, const FrameSrcs& srcs, int n, size_t n_floats, bool accumulate, hipStream_t s) {
    // (the 16-byte requests need 16-byte aligned bases: the library's own operands, slot spectra and frames.acc, are hipMalloc bases)
    if (!dst || ((uintptr_t)dst & 15) != 0 || n < 1 || n > kMaxGroup || n_floats < 2 || (n_floats & 1) != 0) return hipErrorInvalidValue;
    for (int k = 0; k < n; ++k)
        if (!srcs.p[k] || ((uintptr_t)srcs.p[k] & 15) != 0) return hipErrorInvalidValue;
    switch (n) {
        case 1: return frames_sum_n<1>(dst, srcs, n_floats, accumulate, s);
        case 2: return frames_sum_n<2>(dst, srcs, n_floats, accumulate, s);
        case 3: return frames_sum_n<3>(dst, srcs, n_floats, accumulate, s);
        case 4: return frames_sum_n<4>(dst, srcs, n_floats, accumulate, s);
        case 5: return frames_sum_n<5>(dst, srcs, n_floats, accumulate, s);
        case 6: return frames_sum_n<6>(dst, srcs, n_floats, accumulate, s);
        case 7: return frames_sum_n<7>(dst, srcs, n_floats, accumulate, s);
        default: return frames_sum_n<8>(dst, srcs, n_floats, accumulate, s);
    }
}

hipError_t launch_frames_fold(const double* sums, size_t pitch, int n, double* out, hipStream_t s) {
    if (!sums || !out || n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(frames_fold_kernel, dim3(1), dim3(64), 0, s, sums, pitch, n, out);
    return hipGetLastError();
}

}  // namespace fdr
