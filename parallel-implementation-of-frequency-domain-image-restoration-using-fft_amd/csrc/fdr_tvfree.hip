// fdr_tvfree.hip -- the window data step of the free-boundary ADMM iteration (driver in fdr_api_tvfree.hip), the one kernel the
// periodic iteration of fdr_tv.hip does not have: the step of the second splitting s = blur(x),
//
//     e = c + q;  s = the minimiser of the data term + nu / 2 (s - e)^2;  q = e - s;  r = s - q
//
// with c = blur(x) on entry and r in its place on exit.  One kernel makes it for the three data terms of the library, which differ in
// the arithmetic of a pixel alone (a step object, below): least squares with the weight mu an argument (fdr_tv_deconv_free_f32*),
// least squares with every image's mu read from the device, where the mu kernel of fdr_tvauto.hip left it (fdr_tv_deconv_auto_f32*),
// and the Poisson likelihood with a background (fdr_tv_deconv_poisson_f32*, fdr_tv_poisson_step*_f32_dev).  Outside the window, where
// the weights are 0, the step is s = e, q = 0, r = c: nothing to compute and nothing to store, so the launch covers the window alone
// and q, zero outside the window since the start, is never touched there; it moves 20 bytes per pixel, 24 with weights.  d and the
// weights are read in place from the caller's strided windows.  The group form makes the step of up to kMaxGroup images in one
// launch, blockIdx.z the image, with one weights window for all, or (the frames of fdr_tv_deconv_frames_f32*, whose exposures differ
// in their masks) with image z's own; the single kernel and the group kernels instantiate one device function, and a pixel is
// computed by tvfree_data_pixel or tvpoisson_data_pixel (fdr_kernels.hpp), so an image has the same bits in a group as alone.
#include "fdr_kernels.hpp"

namespace fdr {

// The data term of a step, a by-value kernel argument: image(z) runs once per thread that has pixels, before its loads, with the
// image of the launch group (0 in the single kernel); pixel() is the arithmetic on one pixel of weight m.
struct TvStepLeastSquares {
    float mu;
    __device__ __forceinline__ void image(int) {}
    __device__ __forceinline__ void pixel(float nu, float m, float d, float& c, float& q) const { tvfree_data_pixel(mu, nu, m, d, c, q); }
};
struct TvStepLeastSquaresDeviceMu {
    const float* mu_dev;  // one weight per image of the group
    float mu;             // this image's, loaded by image()
    __device__ __forceinline__ void image(int z) { mu = mu_dev[z]; }
    __device__ __forceinline__ void pixel(float nu, float m, float d, float& c, float& q) const { tvfree_data_pixel(mu, nu, m, d, c, q); }
};
struct TvStepPoisson {
    float mu, background;
    __device__ __forceinline__ void image(int) {}
    __device__ __forceinline__ void pixel(float nu, float m, float d, float& c, float& q) const {
        tvpoisson_data_pixel(mu, nu, background, m, d, c, q);
    }
};

// A thread owns four consecutive pixels j .. j + 3 of window row i.  c and q are dense M x N planes (N a multiple of 4, the base
// 16-byte aligned): 16-byte loads and stores.  d (and w) are loaded by tv_load_window4 under dvec (wvec), decided on the host.  In
// the group that straddles column `cols` the pixels beyond it keep the c and q they were loaded with.
template <bool WEIGHTS, class Step>
__device__ __forceinline__ void tv_data_group4(float* __restrict__ c, float* __restrict__ q, const float* __restrict__ d, const int stride,
                                               const float* __restrict__ w, const int wstride, const int rows, const int cols, const int N,
                                               const float nu, Step step, const int z, const int dvec, const int wvec) {
    const int j = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= rows || j >= cols) return;
    step.image(z);
    const size_t at = (size_t)i * N + j;
    const float4 c4 = *reinterpret_cast<const float4*>(c + at), q4 = *reinterpret_cast<const float4*>(q + at);
    float cc[4] = {c4.x, c4.y, c4.z, c4.w}, qq[4] = {q4.x, q4.y, q4.z, q4.w};
    float dd[4] = {0.f, 0.f, 0.f, 0.f}, mm[4] = {1.f, 1.f, 1.f, 1.f};
    const bool whole = j + 3 < cols;
    tv_load_window4(d + (size_t)i * stride + j, j, cols, whole, dvec, dd);
    if (WEIGHTS) tv_load_window4(w + (size_t)i * wstride + j, j, cols, whole, wvec, mm);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (j + l < cols) step.pixel(nu, mm[l], dd[l], cc[l], qq[l]);
    }
    *reinterpret_cast<float4*>(q + at) = make_float4(qq[0], qq[1], qq[2], qq[3]);
    *reinterpret_cast<float4*>(c + at) = make_float4(cc[0], cc[1], cc[2], cc[3]);
}
template <bool WEIGHTS, class Step>
__global__ __launch_bounds__(256) void tv_data_kernel(float* __restrict__ c, float* __restrict__ q, const float* __restrict__ d, const int stride,
                                                      const float* __restrict__ w, const int wstride, const int rows, const int cols, const int N,
                                                      const float nu, const Step step, const int dvec, const int wvec) {
    tv_data_group4<WEIGHTS>(c, q, d, stride, w, wstride, rows, cols, N, nu, step, 0, dvec, wvec);
}
// the group form: image blockIdx.z on its planes and its window, the weights window shared.  Bit z of dvec says whether image z's
// window takes 16-byte loads: the images of a batch with an odd pitch differ in alignment.
template <bool WEIGHTS, class Step>
__global__ __launch_bounds__(256) void tv_data_group_kernel(const TvWindowPlanes pl, const int stride, const float* __restrict__ w, const int wstride,
                                                            const int rows, const int cols, const int N, const float nu, const Step step,
                                                            const int dvec, const int wvec) {
    const int z = blockIdx.z;
    tv_data_group4<WEIGHTS>(FDR_PICK_IMAGE(pl.c, z), FDR_PICK_IMAGE(pl.q, z), FDR_PICK_IMAGE(pl.d, z), stride, w, wstride, rows, cols, N, nu, step, z,
                            (dvec >> z) & 1, wvec);
}

// the group form with a weights window per image: image blockIdx.z reads its own, bit z of wvec says whether it takes 16-byte loads
template <class Step>
__global__ __launch_bounds__(256) void tv_data_group_weights_kernel(const TvWindowPlanes pl, const int stride, const TvWindowWeights wp,
                                                                    const int wstride, const int rows, const int cols, const int N, const float nu,
                                                                    const Step step, const int dvec, const int wvec) {
    const int z = blockIdx.z;
    tv_data_group4<true>(FDR_PICK_IMAGE(pl.c, z), FDR_PICK_IMAGE(pl.q, z), FDR_PICK_IMAGE(pl.d, z), stride, FDR_PICK_IMAGE(wp.w, z), wstride, rows, cols,
                         N, nu, step, z, (dvec >> z) & 1, (wvec >> z) & 1);
}

bool tv_window_launch(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride, int rows, int cols,
                      int M, int N, TvWindowLaunch* L) {
    if (nimg < 1 || nimg > kMaxGroup || !c || !q || !d) return false;
    if (rows < 1 || cols < 1 || rows > M || cols > N || (N & 3) || stride < cols || (w && wstride < cols)) return false;
    L->dvec = 0;
    for (int k = 0; k < kMaxGroup; ++k) {
        const int i = k < nimg ? k : 0;
        if (!c[i] || !q[i] || !d[i] || ((uintptr_t)c[i] & 15) || ((uintptr_t)q[i] & 15)) return false;
        L->pl.c[k] = c[i]; L->pl.q[k] = q[i]; L->pl.d[k] = d[i];
        if (((uintptr_t)d[i] & 15) == 0 && (stride & 3) == 0) L->dvec |= 1 << k;
    }
    L->wvec = w && ((uintptr_t)w & 15) == 0 && (wstride & 3) == 0;
    tv_window_block(cols, &L->tx, &L->ty, &L->gx);
    return true;
}

namespace {

// one image makes the single kernel's launch, more make the group kernel's
template <class Step>
hipError_t launch_tv_data(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride, int rows, int cols,
                          int M, int N, float nu, const Step step, hipStream_t s) {
    TvWindowLaunch L;
    if (!tv_window_launch(nimg, c, q, d, stride, w, wstride, rows, cols, M, N, &L)) return hipErrorInvalidValue;
    const dim3 block((unsigned)L.tx, (unsigned)L.ty), grid((unsigned)L.gx, (unsigned)((rows + L.ty - 1) / L.ty), (unsigned)nimg);
    if (nimg == 1) {
        if (w) hipLaunchKernelGGL((tv_data_kernel<true, Step>), grid, block, 0, s, c[0], q[0], d[0], stride, w, wstride, rows, cols, N, nu, step, L.dvec & 1, L.wvec);
        else hipLaunchKernelGGL((tv_data_kernel<false, Step>), grid, block, 0, s, c[0], q[0], d[0], stride, w, wstride, rows, cols, N, nu, step, L.dvec & 1, L.wvec);
    } else {
        if (w) hipLaunchKernelGGL((tv_data_group_kernel<true, Step>), grid, block, 0, s, L.pl, stride, w, wstride, rows, cols, N, nu, step, L.dvec, L.wvec);
        else hipLaunchKernelGGL((tv_data_group_kernel<false, Step>), grid, block, 0, s, L.pl, stride, w, wstride, rows, cols, N, nu, step, L.dvec, L.wvec);
    }
    return hipGetLastError();
}

// the same with a weights window per image, wk[k] image k's (none null): one image makes the single kernel's launch on its window
template <class Step>
hipError_t launch_tv_data_weights(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* const* wk, int wstride,
                                  int rows, int cols, int M, int N, float nu, const Step step, hipStream_t s) {
    if (!wk || nimg < 1 || nimg > kMaxGroup) return hipErrorInvalidValue;
    for (int k = 0; k < nimg; ++k)
        if (!wk[k]) return hipErrorInvalidValue;
    if (nimg == 1) return launch_tv_data(1, c, q, d, stride, wk[0], wstride, rows, cols, M, N, nu, step, s);
    TvWindowLaunch L;
    if (!tv_window_launch(nimg, c, q, d, stride, wk[0], wstride, rows, cols, M, N, &L)) return hipErrorInvalidValue;
    TvWindowWeights wp;
    int wvec = 0;
    for (int k = 0; k < kMaxGroup; ++k) {
        wp.w[k] = wk[k < nimg ? k : 0];
        if (((uintptr_t)wp.w[k] & 15) == 0 && (wstride & 3) == 0) wvec |= 1 << k;
    }
    const dim3 block((unsigned)L.tx, (unsigned)L.ty), grid((unsigned)L.gx, (unsigned)((rows + L.ty - 1) / L.ty), (unsigned)nimg);
    hipLaunchKernelGGL((tv_data_group_weights_kernel<Step>), grid, block, 0, s, L.pl, stride, wp, wstride, rows, cols, N, nu, step, L.dvec, wvec);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tvfree_data_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride, int rows,
                                int cols, int M, int N, float mu, float nu, hipStream_t s) {
    return launch_tv_data(nimg, c, q, d, stride, w, wstride, rows, cols, M, N, nu, TvStepLeastSquares{mu}, s);
}

hipError_t launch_tvauto_data_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride, int rows,
                                int cols, int M, int N, const float* mu, float nu, hipStream_t s) {
    if (!mu) return hipErrorInvalidValue;
    return launch_tv_data(nimg, c, q, d, stride, w, wstride, rows, cols, M, N, nu, TvStepLeastSquaresDeviceMu{mu, 0.f}, s);
}

hipError_t launch_tvpoisson_data_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride,
                                   int rows, int cols, int M, int N, float mu, float nu, float background, hipStream_t s) {
    return launch_tv_data(nimg, c, q, d, stride, w, wstride, rows, cols, M, N, nu, TvStepPoisson{mu, background}, s);
}

hipError_t launch_tvfree_data_weights_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* const* w,
                                        int wstride, int rows, int cols, int M, int N, float mu, float nu, hipStream_t s) {
    return launch_tv_data_weights(nimg, c, q, d, stride, w, wstride, rows, cols, M, N, nu, TvStepLeastSquares{mu}, s);
}

hipError_t launch_tvpoisson_data_weights_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* const* w,
                                           int wstride, int rows, int cols, int M, int N, float mu, float nu, float background, hipStream_t s) {
    return launch_tv_data_weights(nimg, c, q, d, stride, w, wstride, rows, cols, M, N, nu, TvStepPoisson{mu, background}, s);
}

}  // namespace fdr
