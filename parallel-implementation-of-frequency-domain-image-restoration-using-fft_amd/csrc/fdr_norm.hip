// fdr_norm.hip -- min/max and normalisation: the fold of the per-workgroup (min, max) partials, cv::normalize to [0, 1] from a
// row-major and from a panel-major real plane (the last pass of every Wiener call), and the real-plane primitives of the slab mode.
#include "fdr_fft_core.hpp"
#include "fdr_kernels.hpp"

namespace fdr {

// ---- final min/max over the per-workgroup partials: one workgroup, fixed order => deterministic ----
__global__ void reduce_minmax_kernel(const float2* __restrict__ part, int n, float* __restrict__ mm) {
    __shared__ float2 red[16];
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float2 p = part[i];
        mn = fminf(mn, p.x);
        mx = fmaxf(mx, p.y);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float2(mn, mx);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
            mn = fminf(mn, red[w].x);
            mx = fmaxf(mx, red[w].y);
        }
        mm[0] = mn;
        mm[1] = mx;
    }
}

hipError_t launch_reduce_minmax(const float2* mm_part, int n_part, float* mm, hipStream_t s) {
    hipLaunchKernelGGL(reduce_minmax_kernel, dim3(1), dim3(1024), 0, s, mm_part, n_part, mm);
    return hipGetLastError();
}

// ---- cv::normalize(src, dst, 0, 1, NORM_MINMAX) (fft/fft_serial.cpp:246) + crop (serial.cpp:38) ----
// scale/shift exactly as OpenCV 4.x derives them for CV_32F: double min/max, scale rounded to
// float, shift = (float)dmin - (float)(smin*scale); applied as a float multiply then a float add.
// Every workgroup first folds the (few thousand) per-workgroup min/max partials itself -- a fixed
// order, so the result is deterministic -- which saves a separate reduce launch.
// the fold of the two normalise kernels: mn, mx = (min, max) over the n_part partials by a workgroup of 256 threads, through the
// kernel's own `red[4]`; every thread gets the result.  A macro: as a function it changed the registers of all four kernels.
#define FDR_FOLD_PARTIALS_256(part, n_part, red, mn, mx)                                \
    do {                                                                                \
        mn = __builtin_inff(); mx = -__builtin_inff();                                  \
        for (int i = threadIdx.x; i < n_part; i += 256) {                               \
            const float2 p = part[i];                                                   \
            mn = fminf(mn, p.x);                                                        \
            mx = fmaxf(mx, p.y);                                                        \
        }                                                                               \
        _Pragma("unroll")                                                               \
        for (int off = 32; off > 0; off >>= 1) {                                        \
            mn = fminf(mn, __shfl_xor(mn, off));                                        \
            mx = fmaxf(mx, __shfl_xor(mx, off));                                        \
        }                                                                               \
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float2(mn, mx);       \
        __syncthreads();                                                                \
        mn = fminf(fminf(red[0].x, red[1].x), fminf(red[2].x, red[3].x));               \
        mx = fmaxf(fmaxf(red[0].y, red[1].y), fmaxf(red[2].y, red[3].y));               \
    } while (0)

template <bool VEC4>
__global__ __launch_bounds__(256) void normalize_kernel(const float* __restrict__ raw, int N, const float2* __restrict__ part,
                                                        int n_part, const float* __restrict__ mm, float* __restrict__ out,
                                                        int rows, int cols, int out_stride, const NormBatch nb) {
    if (nb.nimg > 1) {  // blockIdx.y = image
        const int i = blockIdx.y;
        raw = FDR_PICK_IMAGE(nb.raw, i);
        part = FDR_PICK_IMAGE(nb.part, i);
        out = FDR_PICK_IMAGE(nb.out, i);
    }
    __shared__ float2 red[4];
    float mn, mx;
    if (part != nullptr) {
        FDR_FOLD_PARTIALS_256(part, n_part, red, mn, mx);
    } else {
        mn = mm[0]; mx = mm[1];
    }
    float fscale, fshift;
    minmax_to_scale_shift(mn, mx, fscale, fshift);

    constexpr int W = VEC4 ? 1024 : 256;               // elements per workgroup per segment
    const int segs_per_row = (cols + W - 1) / W;
    const long long nseg = (long long)rows * segs_per_row;
    for (long long sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
        const int y = (int)(sgi / segs_per_row);
        const int x = (int)(sgi % segs_per_row) * W + threadIdx.x * (VEC4 ? 4 : 1);
        if (VEC4) {
            if (x < cols) {  // cols % 4 == 0
                typedef float nf4 __attribute__((ext_vector_type(4)));
                const nf4 vv = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(raw + (size_t)y * N + x));  // last use
                const float4 v = make_float4(vv.x, vv.y, vv.z, vv.w);
                float4 o;
                o.x = v.x * fscale; o.y = v.y * fscale; o.z = v.z * fscale; o.w = v.w * fscale;
                o.x = o.x + fshift; o.y = o.y + fshift; o.z = o.z + fshift; o.w = o.w + fshift;
                nf4 oo; oo.x = o.x; oo.y = o.y; oo.z = o.z; oo.w = o.w;
                __builtin_nontemporal_store(oo, reinterpret_cast<nf4*>(out + (size_t)y * out_stride + x));  // written once, read by the caller
            }
        } else {
            if (x < cols) {
                const float p = raw[(size_t)y * N + x] * fscale;
                out[(size_t)y * out_stride + x] = p + fshift;
            }
        }
    }
}

hipError_t launch_normalize(const float* raw, int N, const float2* mm_part, int n_part, const float* mm, float* out,
                            int rows, int cols, int out_stride, hipStream_t s, const NormBatch* batch) {
    NormBatch nb{};
    if (batch) nb = *batch;
    const int ny = nb.nimg > 1 ? nb.nimg : 1;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    bool vec4 = (cols % 4 == 0) && (out_stride % 4 == 0) && (N % 4 == 0) &&
                ((reinterpret_cast<uintptr_t>(out) & 15) == 0) && ((reinterpret_cast<uintptr_t>(raw) & 15) == 0);
    for (int k = 0; k < nb.nimg; ++k)
        vec4 = vec4 && ((reinterpret_cast<uintptr_t>(nb.out[k]) & 15) == 0) && ((reinterpret_cast<uintptr_t>(nb.raw[k]) & 15) == 0);
    const int W = vec4 ? 1024 : 256;
    long long nseg = (long long)rows * ((cols + W - 1) / W);
    int grid = nseg > 2048 ? 2048 : (int)nseg;
    if (vec4)
        hipLaunchKernelGGL(normalize_kernel<true>, dim3(grid, ny), dim3(256), 0, s, raw, N, mm_part, n_part, mm, out, rows, cols, out_stride, nb);
    else
        hipLaunchKernelGGL(normalize_kernel<false>, dim3(grid, ny), dim3(256), 0, s, raw, N, mm_part, n_part, mm, out, rows, cols, out_stride, nb);
    return hipGetLastError();
}

// ---- the same normalisation from a PANEL-major real plane (the parity operator's layout): a workgroup takes 32 rows x 128
// columns, reads 32 panels x (32 rows x 16 bytes = 512 contiguous bytes), turns the block through LDS and writes 32 rows x
// 512 contiguous bytes.  scale / shift and the two roundings exactly as normalize_kernel.
template <bool VEC4>
__global__ __launch_bounds__(256) void normalize_panels_kernel(const float* __restrict__ raw, int M, const float2* __restrict__ part, int n_part,
                                                               const float* __restrict__ mm, float* __restrict__ out, int rows, int cols,
                                                               int out_stride) {
    __shared__ float tile[32][132];  // 32 rows x 128 columns (+4: the transposing accesses fall on distinct banks)
    __shared__ float2 red[4];
    float mn, mx;
    if (part != nullptr) {
        FDR_FOLD_PARTIALS_256(part, n_part, red, mn, mx);
    } else {
        mn = mm[0]; mx = mm[1];
    }
    float fscale, fshift;
    minmax_to_scale_shift(mn, mx, fscale, fshift);
    typedef float nf4 __attribute__((ext_vector_type(4)));
    const int cblocks = (cols + 127) / 128, rblocks = (rows + 31) / 32;
    for (long long bi = blockIdx.x; bi < (long long)cblocks * rblocks; bi += gridDim.x) {
        const int rb = (int)(bi / cblocks) * 32, cb = (int)(bi % cblocks) * 128;
        // read: 32 panels x 32 rows of 16 bytes; a wave takes two panels x 32 rows = two runs of 512 contiguous bytes
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = (int)threadIdx.x + 256 * k;  // 0 .. 1023
            const int pi = e >> 5, ri = e & 31;
            const int m = rb + ri, c0 = cb + pi * 4;
            nf4 v = {0.f, 0.f, 0.f, 0.f};
            if (m < rows && c0 < cols) v = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(raw + ((size_t)(c0 >> 2) * (size_t)M + (size_t)m) * 4));  // last use
            *reinterpret_cast<float4*>(&tile[ri][pi * 4]) = make_float4(v.x, v.y, v.z, v.w);
        }
        __syncthreads();
        // write: a row of the block is 128 columns = 512 contiguous bytes = 32 lanes x 16 bytes
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = (int)threadIdx.x + 256 * k;
            const int ri = e >> 5, ci = (e & 31) * 4;
            const int m = rb + ri, c = cb + ci;
            if (m < rows && c < cols) {
                const float4 t = *reinterpret_cast<const float4*>(&tile[ri][ci]);
                float4 o;
                o.x = t.x * fscale; o.y = t.y * fscale; o.z = t.z * fscale; o.w = t.w * fscale;
                o.x = o.x + fshift; o.y = o.y + fshift; o.z = o.z + fshift; o.w = o.w + fshift;
                float* dst = out + (size_t)m * out_stride + c;
                if (VEC4) {  // cols % 4 == 0, rows of the output 16-byte aligned
                    nf4 oo; oo.x = o.x; oo.y = o.y; oo.z = o.z; oo.w = o.w;
                    __builtin_nontemporal_store(oo, reinterpret_cast<nf4*>(dst));  // written once, read by the caller
                } else {
                    dst[0] = o.x;
                    if (c + 1 < cols) dst[1] = o.y;
                    if (c + 2 < cols) dst[2] = o.z;
                    if (c + 3 < cols) dst[3] = o.w;
                }
            }
        }
        __syncthreads();
    }
}

hipError_t launch_normalize_panels(const float* raw, int M, const float2* mm_part, int n_part, const float* mm, float* out,
                                   int rows, int cols, int out_stride, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    const long long nb = (long long)((cols + 127) / 128) * ((rows + 31) / 32);
    const int grid = nb > 4096 ? 4096 : (int)nb;
    const bool vec4 = (cols % 4 == 0) && (out_stride % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
    if (vec4)
        hipLaunchKernelGGL(normalize_panels_kernel<true>, dim3(grid), dim3(256), 0, s, raw, M, mm_part, n_part, mm, out, rows, cols, out_stride);
    else
        hipLaunchKernelGGL(normalize_panels_kernel<false>, dim3(grid), dim3(256), 0, s, raw, M, mm_part, n_part, mm, out, rows, cols, out_stride);
    return hipGetLastError();
}

// (min, max) partials of a real rows x ld plane over the counted window [0, mm_rows) x [0, mm_cols)
__global__ void minmax_real_kernel(const float* __restrict__ src, int rows, int ld, int mm_rows, int mm_cols, float2* __restrict__ part) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    if (x < ld && y < rows && y < mm_rows && x < mm_cols) { mn = mx = src[(size_t)y * ld + x]; }
    block_minmax_store(mn, mx, part);
}

hipError_t launch_minmax_real(const float* src, int rows, int ld, int mm_rows, int mm_cols, float2* part, int* n_part, hipStream_t s) {
    const dim3 grid((ld + 255) / 256, rows);
    *n_part = (int)(grid.x * grid.y);
    hipLaunchKernelGGL(minmax_real_kernel, grid, dim3(256), 0, s, src, rows, ld, mm_rows, mm_cols, part);
    return hipGetLastError();
}

__global__ void real_part_kernel(const float2* __restrict__ src, float* __restrict__ dst, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = src[i].x;
}

hipError_t launch_real_part(const float2* src, float* dst, size_t count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(real_part_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, src, dst, count);
    return hipGetLastError();
}

}  // namespace fdr
