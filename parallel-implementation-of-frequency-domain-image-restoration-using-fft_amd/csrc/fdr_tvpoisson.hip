// fdr_tvpoisson.hip -- Poisson-likelihood TV deconvolution on the free-boundary iteration (fdr_tv_deconv_poisson_f32*; driver in
// fdr_api_tvfree.hip, entry points in fdr_api_tvpoisson.hip), the one kernel it does not share with fdr_tv_deconv_free_f32: the data
// step of the splitting s = blur(x) for the term mu m [(s + b) - d+ log(s + b)],
//
//     e = c + q;  k = mu m / nu;  a = e + b - k;  y = the non-negative root of y^2 - a y - k d+ = 0;  s = y - b;  q = e - s;  r = s - q
//
// with c = blur(x) on entry and r in its place on exit (tvpoisson_data_pixel of fdr_kernels.hpp, which every kernel here calls).
// Outside the window, and where m is not above 0, the step is s = e: the launch covers the window alone, as the free call's does,
// and moves the same bytes (20 per pixel, 24 with weights).  d and the weights are read in place from the caller's strided windows.
// The group form makes the step of up to kMaxGroup images in one launch, blockIdx.z the image, with one weights window for all;
// the single kernel and the group kernel instantiate one device function, so an image has the same bits in a group as alone.
#include "fdr_kernels.hpp"

namespace fdr {

// A thread owns four consecutive pixels j .. j + 3 of window row i, exactly as tvfree_data_group4 (fdr_tvfree.hip) lays them out:
// c and q are dense M x N planes (N a multiple of 4, the base 256-byte aligned) and take 16-byte loads and stores; d (and w) take
// one 16-byte load when the group lies inside the window and the window's base and stride keep every row 16-byte aligned (dvec /
// wvec, decided on the host), scalar loads otherwise.  In the group that straddles column `cols` the pixels beyond it keep the c
// and q they were loaded with.
template <bool WEIGHTS>
__device__ __forceinline__ void tvpoisson_data_group4(float* __restrict__ c, float* __restrict__ q, const float* __restrict__ d, const int stride,
                                                      const float* __restrict__ w, const int wstride, const int rows, const int cols, const int N,
                                                      const float mu, const float nu, const float bg, const int dvec, const int wvec) {
    const int j = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= rows || j >= cols) return;
    const size_t at = (size_t)i * N + j;
    const float4 c4 = *reinterpret_cast<const float4*>(c + at), q4 = *reinterpret_cast<const float4*>(q + at);
    float cc[4] = {c4.x, c4.y, c4.z, c4.w}, qq[4] = {q4.x, q4.y, q4.z, q4.w};
    float dd[4] = {0.f, 0.f, 0.f, 0.f}, mm[4] = {1.f, 1.f, 1.f, 1.f};
    const bool whole = j + 3 < cols;
    const float* dr = d + (size_t)i * stride + j;
    if (whole && dvec) {
        const float4 v = *reinterpret_cast<const float4*>(dr);
        dd[0] = v.x; dd[1] = v.y; dd[2] = v.z; dd[3] = v.w;
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (j + l < cols) dd[l] = dr[l];
    }
    if (WEIGHTS) {
        const float* wr = w + (size_t)i * wstride + j;
        if (whole && wvec) {
            const float4 v = *reinterpret_cast<const float4*>(wr);
            mm[0] = v.x; mm[1] = v.y; mm[2] = v.z; mm[3] = v.w;
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (j + l < cols) mm[l] = wr[l];
        }
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (j + l < cols) tvpoisson_data_pixel(mu, nu, bg, mm[l], dd[l], cc[l], qq[l]);
    }
    *reinterpret_cast<float4*>(q + at) = make_float4(qq[0], qq[1], qq[2], qq[3]);
    *reinterpret_cast<float4*>(c + at) = make_float4(cc[0], cc[1], cc[2], cc[3]);
}
template <bool WEIGHTS>
__global__ __launch_bounds__(256) void tvpoisson_data_kernel(float* __restrict__ c, float* __restrict__ q, const float* __restrict__ d,
                                                             const int stride, const float* __restrict__ w, const int wstride, const int rows,
                                                             const int cols, const int N, const float mu, const float nu, const float bg,
                                                             const int dvec, const int wvec) {
    tvpoisson_data_group4<WEIGHTS>(c, q, d, stride, w, wstride, rows, cols, N, mu, nu, bg, dvec, wvec);
}

// entry i (uniform over the workgroup) of a per-image pointer array of a by-value kernel argument: a select chain on scalars,
// written on the member itself as in fdr_tvfree.hip (a dynamic index sends the argument block to scratch memory)
#define FDR_TP_PICK(arr, i) \
    ((i) < 4 ? ((i) == 0 ? arr[0] : (i) == 1 ? arr[1] : (i) == 2 ? arr[2] : arr[3]) : ((i) == 4 ? arr[4] : (i) == 5 ? arr[5] : (i) == 6 ? arr[6] : arr[7]))
static_assert(kMaxGroup == 8, "select chain written for 8 entries");

// the group form: image blockIdx.z on its planes and its window, the weights window shared.  Bit z of dvec says whether image z's
// window takes 16-byte loads: the images of a batch with an odd pitch differ in alignment.
struct TvPoissonPlanes {
    float* c[kMaxGroup];
    float* q[kMaxGroup];
    const float* d[kMaxGroup];
};
template <bool WEIGHTS>
__global__ __launch_bounds__(256) void tvpoisson_data_group_kernel(const TvPoissonPlanes pl, const int stride, const float* __restrict__ w,
                                                                   const int wstride, const int rows, const int cols, const int N, const float mu,
                                                                   const float nu, const float bg, const int dvec, const int wvec) {
    const int z = blockIdx.z;
    tvpoisson_data_group4<WEIGHTS>(FDR_TP_PICK(pl.c, z), FDR_TP_PICK(pl.q, z), FDR_TP_PICK(pl.d, z), stride, w, wstride, rows, cols, N, mu, nu, bg,
                                   (dvec >> z) & 1, wvec);
}

// rows x cols must lie within the M x N planes c and q (N a multiple of 4, the planes 16-byte aligned); d and w (null: weights of
// 1) are rows x cols windows with their own strides, of any alignment
hipError_t launch_tvpoisson_data(float* c, float* q, const float* d, int stride, const float* w, int wstride, int rows, int cols, int M, int N,
                                 float mu, float nu, float background, hipStream_t s) {
    if (!c || !q || !d || rows < 1 || cols < 1 || rows > M || cols > N || (N & 3) || stride < cols || (w && wstride < cols)) return hipErrorInvalidValue;
    if (((uintptr_t)c & 15) || ((uintptr_t)q & 15)) return hipErrorInvalidValue;
    const int groups = (cols + 3) / 4;
    const int tx = groups <= 64 ? 64 : groups <= 128 ? 128 : 256, ty = 256 / tx;
    const dim3 grid((unsigned)((groups + tx - 1) / tx), (unsigned)((rows + ty - 1) / ty));
    const int dvec = ((uintptr_t)d & 15) == 0 && (stride & 3) == 0;
    const int wvec = w && ((uintptr_t)w & 15) == 0 && (wstride & 3) == 0;
    if (w)
        hipLaunchKernelGGL((tvpoisson_data_kernel<true>), grid, dim3(tx, ty), 0, s, c, q, d, stride, w, wstride, rows, cols, N, mu, nu, background,
                           dvec, wvec);
    else
        hipLaunchKernelGGL((tvpoisson_data_kernel<false>), grid, dim3(tx, ty), 0, s, c, q, d, stride, w, wstride, rows, cols, N, mu, nu, background,
                           dvec, wvec);
    return hipGetLastError();
}

hipError_t launch_tvpoisson_data_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride,
                                   int rows, int cols, int M, int N, float mu, float nu, float background, hipStream_t s) {
    if (nimg < 1 || nimg > kMaxGroup) return hipErrorInvalidValue;
    if (nimg == 1) return launch_tvpoisson_data(c[0], q[0], d[0], stride, w, wstride, rows, cols, M, N, mu, nu, background, s);
    if (rows < 1 || cols < 1 || rows > M || cols > N || (N & 3) || stride < cols || (w && wstride < cols)) return hipErrorInvalidValue;
    TvPoissonPlanes pl;
    int dvec = 0;
    for (int k = 0; k < kMaxGroup; ++k) {
        const int i = k < nimg ? k : 0;
        if (!c[i] || !q[i] || !d[i] || ((uintptr_t)c[i] & 15) || ((uintptr_t)q[i] & 15)) return hipErrorInvalidValue;
        pl.c[k] = c[i]; pl.q[k] = q[i]; pl.d[k] = d[i];
        if (((uintptr_t)d[i] & 15) == 0 && (stride & 3) == 0) dvec |= 1 << k;
    }
    const int groups = (cols + 3) / 4;
    const int tx = groups <= 64 ? 64 : groups <= 128 ? 128 : 256, ty = 256 / tx;
    const dim3 grid((unsigned)((groups + tx - 1) / tx), (unsigned)((rows + ty - 1) / ty), (unsigned)nimg);
    const int wvec = w && ((uintptr_t)w & 15) == 0 && (wstride & 3) == 0;
    if (w)
        hipLaunchKernelGGL((tvpoisson_data_group_kernel<true>), grid, dim3(tx, ty), 0, s, pl, stride, w, wstride, rows, cols, N, mu, nu, background,
                           dvec, wvec);
    else
        hipLaunchKernelGGL((tvpoisson_data_group_kernel<false>), grid, dim3(tx, ty), 0, s, pl, stride, w, wstride, rows, cols, N, mu, nu, background,
                           dvec, wvec);
    return hipGetLastError();
}

}  // namespace fdr
