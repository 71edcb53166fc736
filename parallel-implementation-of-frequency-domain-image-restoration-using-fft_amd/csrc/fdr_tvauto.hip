// fdr_tvauto.hip -- the kernels of noise-constrained TV deconvolution (fdr_tv_deconv_auto_f32*; driver in fdr_api_tvfree.hip, entry
// points in fdr_api_tvauto.hip): the free-boundary iteration with the weight of its data step chosen in every iteration so that s
// lands on the discrepancy ball  sum m (s - d)^2 <= c2 = tau sigma^2 sum m:
//
//     c = blur(x);  res_e = sum m (c + q - d)^2;  res_c = sum m (c - d)^2;  S = sum m                  (over the window, in double)
//     g = 0 for res_e <= c2;  kTvAutoMaxRatio for c2 = 0 or a quotient that is not finite;  else min(sqrt(res_e / c2) - 1, kTvAutoMaxRatio)
//     mu_k = float(nu g);  then the data step of fdr_tvfree.hip, which reads mu_k from the device
//
// Two kernels: the norm (the three sums as per-workgroup double partials) and mu (one workgroup folds the partials in index order,
// forms mu_k, writes the device scalar and the trace).  d and the weights are read in place from the caller's strided windows, on
// the planes, alignment bits and workgroups of the data step (tv_window_launch).  A thread adds its terms in one order whether it
// loads them as one 16-byte request or as four scalars, so the sums do not depend on the alignment of the caller's windows.  No
// atomics: every sum runs in a fixed order.  Each kernel has a group form (fdr_tv_deconv_auto_batch_f32*) for up to kMaxGroup images
// in one launch: the norm with blockIdx.z as the image, the fold with one workgroup per image; image z has its own partials, noise
// level, mu, sums and trace slot, and the single and the group kernel instantiate one device function, so an image has the same
// sums and bits in a group as alone.
#include "fdr_kernels.hpp"

#include <cstdint>

namespace fdr {

constexpr int kTaThreads = 256;
constexpr int kTaRows = 4;  // rows per thread of the norm kernel
constexpr int kTaFold = 8;  // partials of each sum a thread of the mu kernel has in flight
static_assert(kTaThreads == 256, "the norm kernel adds the sums of four waves, on tv_window_block's workgroups");
constexpr double kTvAutoMaxRatio = 1e6;  // FDR_TV_AUTO_MAX_RATIO of include/fdr.h

// four consecutive pixels of a window row for the sums (row = the row's base): one 16-byte load when the group lies inside the
// window and the host found every row aligned (`vec`), as tv_load_window4, else scalar loads at
// clamped columns -- a pixel beyond column `cols` reads the row's last one and is not counted -- so that no load hangs on a
// per-pixel condition and the loads of all the rows of a thread are in flight together.  (With per-pixel conditions the compiler
// waits for each row's loads before it issues the next row's.  The two forms load the same values, and it may merge them.)
__device__ __forceinline__ void ta_load_sum4(const float* row, int j, int cols, bool vec, float v[4]) {
    if (vec && j + 3 < cols) {
        const float4 t = *reinterpret_cast<const float4*>(row + j);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l) v[l] = row[min(j + l, cols - 1)];
    }
}

// A workgroup of blockDim.x x blockDim.y = 256 threads covers 4 blockDim.x columns of kTaRows blockDim.y rows of the window; thread
// (tx, ty) owns the columns j .. j + 3 of the rows r0 + ty, r0 + ty + blockDim.y, ...  c and q are the dense M x N planes (row
// stride N, a multiple of 4): 16-byte loads; pixels beyond column `cols` are loaded (they lie in the plane) and not counted.  The
// workgroup's sums go to part[b], part[n + b], part[2 n + b] (res_e, res_c, S), b = blockIdx.y gridDim.x + blockIdx.x,
// n = gridDim.x gridDim.y.
template <bool WEIGHTS>
__device__ __forceinline__ void tvauto_norm_block(const float* __restrict__ c, const float* __restrict__ q, const float* __restrict__ d,
                                                  const int stride, const float* __restrict__ w, const int wstride, const int rows, const int cols,
                                                  const int N, const int dvec, const int wvec, double* __restrict__ part) {
    __shared__ double red[3][kTaThreads / 64];
    const int j = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int r0 = blockIdx.y * (blockDim.y * kTaRows) + threadIdx.y;
    double s_e = 0.0, s_c = 0.0, s_m = 0.0;
    if (j < cols) {
        // every load of the thread's rows first (a row past the window reads the last row and is not counted), then the sums
        float cc[kTaRows][4], qq[kTaRows][4], dd[kTaRows][4], mm[kTaRows][4];
#pragma unroll
        for (int k = 0; k < kTaRows; ++k) {
            const int i = min(r0 + k * (int)blockDim.y, rows - 1);
            const size_t at = (size_t)i * N + j;
            const float4 c4 = *reinterpret_cast<const float4*>(c + at), q4 = *reinterpret_cast<const float4*>(q + at);
            cc[k][0] = c4.x; cc[k][1] = c4.y; cc[k][2] = c4.z; cc[k][3] = c4.w;
            qq[k][0] = q4.x; qq[k][1] = q4.y; qq[k][2] = q4.z; qq[k][3] = q4.w;
            ta_load_sum4(d + (size_t)i * stride, j, cols, dvec != 0, dd[k]);
            mm[k][0] = mm[k][1] = mm[k][2] = mm[k][3] = 1.f;
            if (WEIGHTS) ta_load_sum4(w + (size_t)i * wstride, j, cols, wvec != 0, mm[k]);
        }
#pragma unroll
        for (int k = 0; k < kTaRows; ++k) {
            const bool row_ok = r0 + k * (int)blockDim.y < rows;
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const bool ok = row_ok && j + l < cols;  // selects, not branches: a pixel that is not counted adds 0
                const double m = (double)mm[k][l];
                const double rc = (double)cc[k][l] - (double)dd[k][l];
                const double re = ((double)cc[k][l] + (double)qq[k][l]) - (double)dd[k][l];
                s_e += ok ? m * (re * re) : 0.0;
                s_c += ok ? m * (rc * rc) : 0.0;
                s_m += ok ? m : 0.0;
            }
        }
    }
    // a fixed tree: the 64 lanes of a wave by shuffles, then the four waves in order
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) {
        s_e += __shfl_down(s_e, h);
        s_c += __shfl_down(s_c, h);
        s_m += __shfl_down(s_m, h);
    }
    const int t = threadIdx.y * blockDim.x + threadIdx.x;
    if ((t & 63) == 0) {
        red[0][t >> 6] = s_e;
        red[1][t >> 6] = s_c;
        red[2][t >> 6] = s_m;
    }
    __syncthreads();
    if (t == 0) {
        const size_t n = (size_t)gridDim.x * gridDim.y, b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[b] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        part[n + b] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        part[2 * n + b] = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    }
}
template <bool WEIGHTS>
__global__ __launch_bounds__(kTaThreads) void tvauto_norm_kernel(const float* __restrict__ c, const float* __restrict__ q, const float* __restrict__ d,
                                                                 const int stride, const float* __restrict__ w, const int wstride, const int rows,
                                                                 const int cols, const int N, const int dvec, const int wvec,
                                                                 double* __restrict__ part) {
    tvauto_norm_block<WEIGHTS>(c, q, d, stride, w, wstride, rows, cols, N, dvec, wvec, part);
}

// the group form: image blockIdx.z on its planes and its window, the weights window shared; bit z of dvec says whether image z's
// window takes 16-byte loads.  The workgroup's place in the image is (blockIdx.x, blockIdx.y), as in the single kernel, so image
// z's partials, written to part + z 3 n, are those of its single launch.
template <bool WEIGHTS>
__global__ __launch_bounds__(kTaThreads) void tvauto_norm_group_kernel(const TvWindowPlanes pl, const int stride, const float* __restrict__ w,
                                                                       const int wstride, const int rows, const int cols, const int N, const int dvec,
                                                                       const int wvec, double* __restrict__ part) {
    const int z = blockIdx.z;
    const size_t n = (size_t)gridDim.x * gridDim.y;
    tvauto_norm_block<WEIGHTS>(FDR_PICK_IMAGE(pl.c, z), FDR_PICK_IMAGE(pl.q, z), FDR_PICK_IMAGE(pl.d, z), stride, w, wstride, rows, cols, N,
                               (dvec >> z) & 1, wvec, part + (size_t)z * 3 * n);
}

// one workgroup: res_e, res_c and S from the 3 n partials (thread t adds t, t + 256, ... in order, then a fixed tree), c2 and mu_k in
// double, mu_k rounded to float once into *mu; stat = (res_c, res_e, mu_k, S), and the first three to `trace` when that is not null
__device__ __forceinline__ void tvauto_mu_fold(const double* __restrict__ part, const int n, const double sigma, const double tau, const float nu,
                                               float* __restrict__ mu, double* __restrict__ stat, double* __restrict__ trace) {
    __shared__ double red[3][kTaThreads];
    double a = 0.0, b = 0.0, m = 0.0;
    // kTaFold partials of each sum per round, loaded together and added in index order: one workgroup is bound by the latency of
    // its loads, not by their bytes (a partial past n is a 0 that changes no sum)
    for (int k0 = threadIdx.x; k0 < n; k0 += kTaThreads * kTaFold) {
        double va[kTaFold], vb[kTaFold], vm[kTaFold];
#pragma unroll
        for (int u = 0; u < kTaFold; ++u) {
            const int k = k0 + u * kTaThreads;
            const bool in = k < n;
            const size_t at = in ? (size_t)k : 0;
            va[u] = part[at];
            vb[u] = part[(size_t)n + at];
            vm[u] = part[2 * (size_t)n + at];
            if (!in) va[u] = vb[u] = vm[u] = 0.0;
        }
#pragma unroll
        for (int u = 0; u < kTaFold; ++u) {
            a += va[u];
            b += vb[u];
            m += vm[u];
        }
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    red[2][threadIdx.x] = m;
    __syncthreads();
    for (int h = kTaThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[0][threadIdx.x] += red[0][threadIdx.x + h];
            red[1][threadIdx.x] += red[1][threadIdx.x + h];
            red[2][threadIdx.x] += red[2][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double res_e = red[0][0], res_c = red[1][0], S = red[2][0];
        const double c2 = tau * sigma * sigma * S;
        double g;
        if (res_e <= c2) {
            g = 0.0;
        } else {
            const double quot = res_e / c2;
            if (c2 == 0.0 || !(quot <= 1.7976931348623157e308)) g = kTvAutoMaxRatio;  // no ball, or NaN / infinite
            else g = fmin(sqrt(quot) - 1.0, kTvAutoMaxRatio);
        }
        const float v = (float)((double)nu * g);
        *mu = v;
        stat[0] = res_c; stat[1] = res_e; stat[2] = (double)v; stat[3] = S;
        if (trace) { trace[0] = res_c; trace[1] = res_e; trace[2] = (double)v; }
    }
}
__global__ __launch_bounds__(kTaThreads) void tvauto_mu_kernel(const double* __restrict__ part, const int n, const double sigma, const double tau,
                                                               const float nu, float* __restrict__ mu, double* __restrict__ stat,
                                                               double* __restrict__ trace) {
    tvauto_mu_fold(part, n, sigma, tau, nu, mu, stat, trace);
}
// the group form: workgroup z folds image z's partials with image z's noise level into mu[z], stat + 4 z and image z's trace slot
struct TvAutoLevels {
    double sigma[kMaxGroup];
    double* trace[kMaxGroup];  // null: no trace
};
__global__ __launch_bounds__(kTaThreads) void tvauto_mu_group_kernel(const double* __restrict__ part, const int n, const TvAutoLevels lv, const double tau,
                                                                     const float nu, float* __restrict__ mu, double* __restrict__ stat) {
    const int z = blockIdx.x;
    tvauto_mu_fold(part + (size_t)z * 3 * n, n, FDR_PICK_IMAGE(lv.sigma, z), tau, nu, mu + z, stat + 4 * z, FDR_PICK_IMAGE(lv.trace, z));
}

// the workgroups of the norm launch: tv_window_block's across the window, kTaRows rows per thread down it
int tvauto_partials(int rows, int cols) {
    int tx, ty, gx;
    tv_window_block(cols, &tx, &ty, &gx);
    return gx * ((rows + ty * kTaRows - 1) / (ty * kTaRows));
}

// no window of an M x N plan makes more partials: the widest workgroup, one row of threads
int tvauto_max_partials(int M, int N) { return ((N + 4 * kTaThreads - 1) / (4 * kTaThreads)) * ((M + kTaRows - 1) / kTaRows); }

hipError_t launch_tvauto_mu(const double* part, int n, double sigma, double tau, float nu, float* mu, double* stat, double* trace, hipStream_t s) {
    if (n <= 0 || !part || !mu || !stat) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tvauto_mu_kernel, dim3(1), dim3(kTaThreads), 0, s, part, n, sigma, tau, nu, mu, stat, trace);
    return hipGetLastError();
}

// one image makes the single kernel's launch, more make the group kernel's (the planes are only read)
hipError_t launch_tvauto_norm_n(int nimg, const float* const* c, const float* const* q, const float* const* d, int stride, const float* w, int wstride,
                                int rows, int cols, int M, int N, double* part, hipStream_t s) {
    TvWindowLaunch L;
    if (!part || !tv_window_launch(nimg, const_cast<float* const*>(c), const_cast<float* const*>(q), d, stride, w, wstride, rows, cols, M, N, &L))
        return hipErrorInvalidValue;
    const dim3 block((unsigned)L.tx, (unsigned)L.ty), grid((unsigned)L.gx, (unsigned)((rows + L.ty * kTaRows - 1) / (L.ty * kTaRows)), (unsigned)nimg);
    if (nimg == 1) {
        if (w) hipLaunchKernelGGL((tvauto_norm_kernel<true>), grid, block, 0, s, c[0], q[0], d[0], stride, w, wstride, rows, cols, N, L.dvec & 1, L.wvec, part);
        else hipLaunchKernelGGL((tvauto_norm_kernel<false>), grid, block, 0, s, c[0], q[0], d[0], stride, w, wstride, rows, cols, N, L.dvec & 1, L.wvec, part);
    } else {
        if (w) hipLaunchKernelGGL((tvauto_norm_group_kernel<true>), grid, block, 0, s, L.pl, stride, w, wstride, rows, cols, N, L.dvec, L.wvec, part);
        else hipLaunchKernelGGL((tvauto_norm_group_kernel<false>), grid, block, 0, s, L.pl, stride, w, wstride, rows, cols, N, L.dvec, L.wvec, part);
    }
    return hipGetLastError();
}

hipError_t launch_tvauto_mu_n(int nimg, const double* part, int n, const double* sigma, double tau, float nu, float* mu, double* stat,
                              double* const* trace, hipStream_t s) {
    if (nimg < 1 || nimg > kMaxGroup || !sigma) return hipErrorInvalidValue;
    if (nimg == 1) return launch_tvauto_mu(part, n, sigma[0], tau, nu, mu, stat, trace ? trace[0] : nullptr, s);
    if (n <= 0 || !part || !mu || !stat) return hipErrorInvalidValue;
    TvAutoLevels lv;
    for (int k = 0; k < kMaxGroup; ++k) {
        const int i = k < nimg ? k : 0;
        lv.sigma[k] = sigma[i];
        lv.trace[k] = trace ? trace[i] : nullptr;
    }
    hipLaunchKernelGGL(tvauto_mu_group_kernel, dim3((unsigned)nimg), dim3(kTaThreads), 0, s, part, n, lv, tau, nu, mu, stat);
    return hipGetLastError();
}

}  // namespace fdr
