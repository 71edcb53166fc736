// fdr_simple.hip -- the reference-shaped "simple path" (pad -> row FFT -> transpose -> row FFT -> transpose,
// fft/fft_gpu.cu:214-240), the on-device cross-check and the fallback for dimensions below 8, and the free-standing transforms
// beside it: the long row pass (more than 8192 points), the transposes, the pointwise Wiener quotient and filter, the O(n^2) DFT
// and the slab pack.
#include "fdr_fft_core.hpp"
#include "fdr_kernels.hpp"

namespace fdr {

// ---- preprocess_kernel equivalent (fft/fft_gpu.cu:85-103): real -> complex with zero padding ----
__global__ void pad_real_to_complex_kernel(const float* __restrict__ src, int rows, int cols, int stride,
                                           float2* __restrict__ dst, int M, int N) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x < N && y < M) {
        float p = 0.f;
        if (x < cols && y < rows) p = src[(size_t)y * stride + x];
        dst[(size_t)y * N + x] = make_float2(p, 0.f);
    }
}

hipError_t launch_pad_real_to_complex(const float* src, int rows, int cols, int stride, float2* dst, int M, int N,
                                      hipStream_t s) {
    const dim3 block(64, 4), grid((N + 63) / 64, (M + 3) / 4);
    hipLaunchKernelGGL(pad_real_to_complex_kernel, grid, block, 0, s, src, rows, cols, stride, dst, M, N);
    return hipGetLastError();
}

// ---- reference-shaped row FFT: whole row in LDS, explicit bit reversal, one radix-2 stage per
// barrier, flat butterfly index k (the shape of fft/fft_gpu.cu:108-148) but with the per-stage
// table so that parity mode reproduces fft/fft_serial.cpp:53-66 bit for bit.
template <class Pol>
__global__ void simple_rows_kernel(float2* __restrict__ data, int rows, int L, int logl, const float2* __restrict__ tw) {
    extern __shared__ float2 s_data[];  // tw: table of the requested direction (both modes)
    const int row = blockIdx.x;
    if (row >= rows) return;
    float2* p = data + (size_t)row * L;
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        const int rev = logl ? (int)(__brev((unsigned)i) >> (32 - logl)) : 0;
        s_data[rev] = p[i];
    }
    __syncthreads();
    for (int len = 2; len <= L; len <<= 1) {
        const int half = len >> 1;
        for (int k = threadIdx.x; k < (L >> 1); k += blockDim.x) {
            const int off = k & (half - 1);
            const int ui = ((k - off) << 1) + off, vi = ui + half;
            float2 u = s_data[ui], v = s_data[vi];
            Pol::bfly(u, v, tw[(half - 1) + off]);
            s_data[ui] = u;
            s_data[vi] = v;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < L; i += blockDim.x) p[i] = s_data[i];
}

hipError_t launch_simple_rows(float2* data, int rows, int L, int logl, const float2* tw, int mode, hipStream_t s) {
    const size_t smem = (size_t)L * sizeof(float2);
    int threads = L / 2;
    if (threads < 64) threads = 64;
    if (threads > 1024) threads = 1024;
    if (smem > 48 * 1024) {
        // opt in to a 64 KiB dynamic LDS row (the reference never does).  A function attribute belongs to the
        // CURRENT device's copy of the code object, and fdr_batch_run drives one host thread per device: set it on every such
        // launch (a host-side table write, no device work) instead of remembering a process-wide "done" flag
        hipError_t e = mode == 0 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&simple_rows_kernel<PolicyParity>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024)
                                 : hipFuncSetAttribute(reinterpret_cast<const void*>(&simple_rows_kernel<PolicyFast>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        if (e != hipSuccess) return e;
    }
    if (mode == 0)
        hipLaunchKernelGGL(simple_rows_kernel<PolicyParity>, dim3(rows), dim3(threads), smem, s, data, rows, L, logl, tw);
    else
        hipLaunchKernelGGL(simple_rows_kernel<PolicyFast>, dim3(rows), dim3(threads), smem, s, data, rows, L, logl, tw);
    return hipGetLastError();
}

// ---- transforms longer than one LDS row (L > 8192, a power of two): fft_serial::fft_radix2_inplace (fft/fft_serial.cpp:40-68)
// takes any power of two.  Its stages len = 2 .. L0 act inside aligned blocks of L0 = 8192 positions of the bit-reversed
// array, and block B of that array is the L0-point transform of the subsequence x[j S + bitrev(B)], S = L / L0: so the
// subsequences are gathered into blocks (long_gather_kernel), every block runs through the ordinary L0-point row kernels as a
// row of its own, and the remaining log2 S stages are plain butterflies over the whole row in global memory
// (long_stage_kernel), with the SAME per-stage twiddle table and butterfly as every other stage -- parity mode stays
// bit-identical to the serial recurrence.  Two extra passes over the data per transform plus one per stage above L0: the
// serial path "only gets slow" beyond 8192 points, and so does this one.
__global__ void long_gather_kernel(const float2* __restrict__ src, float2* __restrict__ dst, size_t rows, int L, int logs) {
    const int S = 1 << logs, L0 = L >> logs;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // over rows x L destination elements
    if (idx >= rows * (size_t)L) return;
    const size_t row = idx / (size_t)L;
    const int pos = (int)(idx - row * (size_t)L);
    const int B = pos / L0, j = pos - B * L0;
    const int h = logs ? (int)(__brev((unsigned)B) >> (32 - logs)) : 0;
    dst[idx] = src[row * (size_t)L + (size_t)j * S + h];
}

template <class Pol>
__global__ void long_stage_kernel(const float2* src, float2* dst, size_t rows, int L, int half,  // (src may be dst: own pair only)
                                  const float2* __restrict__ tw) {  // tw: table of the requested direction, all stages
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // over rows x L/2 butterflies
    const size_t per_row = (size_t)(L >> 1);
    if (idx >= rows * per_row) return;
    const size_t row = idx / per_row;
    const int k = (int)(idx - row * per_row);
    const int off = k & (half - 1);
    const size_t ui = row * (size_t)L + (size_t)(((k - off) << 1) + off), vi = ui + (size_t)half;
    float2 u = src[ui], v = src[vi];
    Pol::bfly(u, v, tw[(half - 1) + off]);
    dst[ui] = u;
    dst[vi] = v;
}

hipError_t launch_long_gather(const float2* src, float2* dst, size_t rows, int L, int logs, hipStream_t s) {
    const size_t n = rows * (size_t)L;
    hipLaunchKernelGGL(long_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, rows, L, logs);
    return hipGetLastError();
}

hipError_t launch_long_stage(const float2* src, float2* dst, size_t rows, int L, int half, const float2* tw, int mode, hipStream_t s) {
    const size_t n = rows * (size_t)(L >> 1);
    if (mode == 0)
        hipLaunchKernelGGL(long_stage_kernel<PolicyParity>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, rows, L, half, tw);
    else
        hipLaunchKernelGGL(long_stage_kernel<PolicyFast>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, rows, L, half, tw);
    return hipGetLastError();
}

// ---- tile transpose through LDS (fft/fft_gpu.cu:153-164), 64-lane friendly 32x32 tile, +1 pad; 4- or 8-byte elements ----
template <class E>
__global__ void transpose_any_kernel(const E* __restrict__ src, E* __restrict__ dst, int rows, int cols) {
    __shared__ E tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    int x = blockIdx.x * 32 + tx;
    for (int j = ty; j < 32; j += 8) {
        const int y = blockIdx.y * 32 + j;
        if (x < cols && y < rows) tile[j][tx] = src[(size_t)y * cols + x];
    }
    __syncthreads();
    x = blockIdx.y * 32 + tx;
    for (int j = ty; j < 32; j += 8) {
        const int y = blockIdx.x * 32 + j;
        if (x < rows && y < cols) dst[(size_t)y * rows + x] = tile[tx][j];
    }
}

hipError_t launch_transpose(const float2* src, float2* dst, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(transpose_any_kernel<float2>, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, s, src, dst, rows, cols);
    return hipGetLastError();
}

hipError_t launch_transpose_any(const void* src, void* dst, int rows, int cols, int elem_size, hipStream_t s) {
    if (elem_size != 4 && elem_size != 8) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    const dim3 grid((cols + 31) / 32, (rows + 31) / 32), block(256);
    if (elem_size == 8) hipLaunchKernelGGL(transpose_any_kernel<float2>, grid, block, 0, s, (const float2*)src, (float2*)dst, rows, cols);
    else hipLaunchKernelGGL(transpose_any_kernel<float>, grid, block, 0, s, (const float*)src, (float*)dst, rows, cols);
    return hipGetLastError();
}

// ---- Wiener quotient, pointwise (simple path); parity: fft/fft_serial.cpp:186-224 op order ----
__global__ void wiener_pointwise_kernel(float2* __restrict__ g, const float2* __restrict__ filt, size_t count, float K,
                                        int mode) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float2 G = g[i], h = filt[i];
    float2 o;
    if (mode == 0) {
        const float hr2 = h.x * h.x, hi2 = h.y * h.y;
        const float mag = sqrtf(hr2 + hi2);
        const float mag2 = mag * mag;
        const float denom = mag2 + K;
        const float chi = -h.y;
        const float p0 = G.x * h.x, p1 = G.y * chi, p2 = G.x * chi, p3 = G.y * h.x;
        const float nr = p0 - p1, ni = p2 + p3;
        o.x = denom != 0.0f ? nr / denom : 0.0f;
        o.y = denom != 0.0f ? ni / denom : 0.0f;
    } else {
        o.x = __builtin_fmaf(G.x, h.x, -(G.y * h.y));
        o.y = __builtin_fmaf(G.x, h.y, G.y * h.x);
    }
    g[i] = o;
}

hipError_t launch_wiener_pointwise(float2* g, const float2* filt, size_t count, float K, int mode, hipStream_t s) {
    hipLaunchKernelGGL(wiener_pointwise_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, g, filt, count, K,
                       mode);
    return hipGetLastError();
}

// ---- fast mode: W = conj(H) / (|H|^2 + K), evaluated in double, rounded once ----
__global__ void make_filter_fast_kernel(const float2* __restrict__ H, float2* __restrict__ W, size_t count, float K) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    W[i] = wiener_filter_fast(H[i], K);
}

hipError_t launch_make_filter_fast(const float2* H, float2* W, size_t count, float K, hipStream_t s) {
    hipLaunchKernelGGL(make_filter_fast_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, H, W, count, K);
    return hipGetLastError();
}

// ---- simple path: real plane + min/max (postprocess_kernel, fft/fft_gpu.cu:187-201, unscaled) ----
__global__ void real_minmax_kernel(const float2* __restrict__ src, float* __restrict__ dst, int M, int N, int mm_rows,
                                   int mm_cols, float2* __restrict__ mm_part) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    if (x < N && y < M) {
        const float r = src[(size_t)y * N + x].x;
        dst[(size_t)y * N + x] = r;
        if (y < mm_rows && x < mm_cols) { mn = r; mx = r; }
    }
    block_minmax_store(mn, mx, mm_part);
}

hipError_t launch_real_minmax(const float2* src, float* dst, int M, int N, int mm_rows, int mm_cols, float2* mm_part,
                              int* n_part, hipStream_t s) {
    const dim3 grid((N + 255) / 256, M);
    *n_part = (int)(grid.x * grid.y);
    hipLaunchKernelGGL(real_minmax_kernel, grid, dim3(256), 0, s, src, dst, M, N, mm_rows, mm_cols, mm_part);
    return hipGetLastError();
}

// ---- fft_serial::dft_naive_inplace (fft/fft_serial.cpp:71-87): one thread per output k, terms accumulated in the
// reference's order t = 0..n-1, every product and sum rounded separately (-ffp-contract=off).
// Table form (bit parity): table[t * n + k] = (cosf(ang), sinf(ang)) with ang = (float)(2.0f*CV_PI*k*t/n*sign) evaluated
// left to right in double -- generated on the HOST with the C library's cosf / sinf, the functions the serial path
// itself calls (the device's own cosf / sinf differ from them by up to 2 ulp).  Forward table only: the inverse angle
// is the exact negation, cosf is even and sinf odd.  Batched over rows (blockIdx.y); src and dst must differ.
__global__ void dft_naive_rows_kernel(const float2* __restrict__ src, float2* __restrict__ dst, int n, const float2* __restrict__ table,
                                      int inverse) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float2* __restrict__ row = src + (size_t)blockIdx.y * n;
    float sr = 0.f, si = 0.f;
    for (int t = 0; t < n; ++t) {
        const float2 w = table[(size_t)t * n + k];
        const float wr = w.x, wi = inverse ? -w.y : w.y;
        const float2 a = row[t];
        const float pr = a.x * wr - a.y * wi, pi = a.x * wi + a.y * wr;
        sr += pr;
        si += pi;
    }
    dst[(size_t)blockIdx.y * n + k] = make_float2(sr, si);
}

// the same with the angle's cosine and sine evaluated on the device (lengths whose n x n table would be too large):
// within 2 ulp per twiddle of the table form
__global__ void dft_naive_kernel(const float2* __restrict__ src, float2* __restrict__ dst, int n, int inverse) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double sign = inverse ? 1.0 : -1.0;
    float sr = 0.f, si = 0.f;
    for (int t = 0; t < n; ++t) {
        const float ang = (float)(2.0 * 3.1415926535897932384626433832795 * (double)k * (double)t / (double)n * sign);
        const float wr = cosf(ang), wi = sinf(ang);
        const float2 a = src[t];
        const float pr = a.x * wr - a.y * wi, pi = a.x * wi + a.y * wr;
        sr += pr;
        si += pi;
    }
    dst[k] = make_float2(sr, si);
}

hipError_t launch_dft_naive(const float2* src, float2* dst, int n, int inverse, hipStream_t s) {
    hipLaunchKernelGGL(dft_naive_kernel, dim3((n + 127) / 128), dim3(128), 0, s, src, dst, n, inverse);
    return hipGetLastError();
}

hipError_t launch_dft_naive_rows(const float2* src, float2* dst, int rows, int n, const float2* table, int inverse, hipStream_t s) {
    if (rows <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(dft_naive_rows_kernel, dim3((n + 127) / 128, rows), dim3(128), 0, s, src, dst, n, table, inverse);
    return hipGetLastError();
}

// ---- building blocks of the single-image multi-GPU mode (slab decomposition; the reference's
// fft/fft_mpi.cpp:170-307): pack the column blocks of a row slab for the all-to-all, transpose what came back ----
struct SlabParts { int parts; int counts[16]; int displs[16]; };

// dst = [block 0 | block 1 | ...], block p = src[:, displs[p] : displs[p] + counts[p]] stored row-major (rows x counts[p]);
// the send buffer of fft/fft_mpi.cpp:118-135 (displs are the prefix sums of counts, so block p starts at rows * displs[p])
template <class E>
__global__ void slab_pack_kernel(const E* __restrict__ src, int rows, int ld, SlabParts sp, E* __restrict__ dst) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c >= ld || r >= rows) return;
    int p = 0;
#pragma unroll
    for (int k = 1; k < 16; ++k)
        if (k < sp.parts && c >= sp.displs[k]) p = k;
    dst[(size_t)rows * sp.displs[p] + (size_t)r * sp.counts[p] + (c - sp.displs[p])] = src[(size_t)r * ld + c];
}

hipError_t launch_slab_pack(const void* src, int rows, int ld, int parts, const int* counts, int elem_size, void* dst, hipStream_t s) {
    if (parts < 1 || parts > 16 || (elem_size != 4 && elem_size != 8)) return hipErrorInvalidValue;
    SlabParts sp{};
    sp.parts = parts;
    int d = 0;
    for (int k = 0; k < parts; ++k) {
        if (counts[k] < 0) return hipErrorInvalidValue;  // (a negative block could still sum to ld)
        sp.counts[k] = counts[k]; sp.displs[k] = d; d += counts[k];
    }
    if (d != ld) return hipErrorInvalidValue;
    if (rows <= 0 || ld <= 0) return hipSuccess;
    const dim3 grid((ld + 255) / 256, rows), block(256);
    if (elem_size == 8) hipLaunchKernelGGL(slab_pack_kernel<float2>, grid, block, 0, s, (const float2*)src, rows, ld, sp, (float2*)dst);
    else hipLaunchKernelGGL(slab_pack_kernel<float>, grid, block, 0, s, (const float*)src, rows, ld, sp, (float*)dst);
    return hipGetLastError();
}

}  // namespace fdr
