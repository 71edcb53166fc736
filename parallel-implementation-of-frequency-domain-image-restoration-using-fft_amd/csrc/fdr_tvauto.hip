// fdr_tvauto.hip -- the kernels of noise-constrained TV deconvolution (fdr_tv_deconv_auto_f32*; driver in fdr_api_tvfree.hip, entry
// points in fdr_api_tvauto.hip): the free-boundary iteration of fdr_tvfree.hip with the weight of its data step chosen in every
// iteration so that s lands on the discrepancy ball  sum m (s - d)^2 <= c2 = tau sigma^2 sum m:
//
//     c = blur(x);  res_e = sum m (c + q - d)^2;  res_c = sum m (c - d)^2;  S = sum m                  (over the window, in double)
//     g = 0 for res_e <= c2;  kTvAutoMaxRatio for c2 = 0 or a quotient that is not finite;  else min(sqrt(res_e / c2) - 1, kTvAutoMaxRatio)
//     mu_k = float(nu g);  then the data step of fdr_tvfree.hip with mu_k
//
// Three kernels: the norm (the three sums as per-workgroup double partials), mu (one workgroup folds the partials in index order,
// forms mu_k, writes the device scalar and the trace) and the data step (reads that scalar).  d and the weights are read in place
// from the caller's strided windows, as tvfree_data_kernel reads them.  A thread adds its terms in one order whether it loads them
// as one 16-byte request or as four scalars, so the sums do not depend on the alignment of the caller's windows.  No atomics: every
// sum runs in a fixed order.  Each kernel has a group form (fdr_tv_deconv_auto_batch_f32*) for up to kMaxGroup images in one launch:
// the window kernels with blockIdx.z as the image, the fold with one workgroup per image; image z has its own partials, noise
// level, mu, sums and trace slot, and the single and the group kernel instantiate one device function, so an image has the same
// sums and bits in a group as alone.
#include "fdr_kernels.hpp"

#include <cstdint>

namespace fdr {

constexpr int kTaThreads = 256;
constexpr int kTaRows = 4;  // rows per thread of the norm kernel
constexpr int kTaFold = 8;  // partials of each sum a thread of the mu kernel has in flight
static_assert(kTaThreads == 256, "the norm kernel adds the sums of four waves");
constexpr double kTvAutoMaxRatio = 1e6;  // FDR_TV_AUTO_MAX_RATIO of include/fdr.h

// four consecutive pixels of a caller's window row (wr = the row's base + j): one 16-byte load when the group lies inside the
// window and the host found every row aligned (`vec`), scalar loads otherwise; pixels beyond column `cols` keep `fill`
__device__ __forceinline__ void ta_load_window4(const float* wr, int j, int cols, bool vec, float fill, float v[4]) {
    v[0] = v[1] = v[2] = v[3] = fill;
    if (j + 3 < cols && vec) {
        const float4 t = *reinterpret_cast<const float4*>(wr);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (j + l < cols) v[l] = wr[l];
    }
}

// the same four pixels for the sums (row = the window row's base): one 16-byte load under the same condition, else scalar loads at
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

// entry i (uniform over the workgroup) of a per-image array of a by-value kernel argument: pick_image's select chain on scalars,
// written on the member itself (a dynamic index, or pick_image's array reference, sends the argument block to scratch memory)
#define FDR_TA_PICK(arr, i) \
    ((i) < 4 ? ((i) == 0 ? arr[0] : (i) == 1 ? arr[1] : (i) == 2 ? arr[2] : arr[3]) : ((i) == 4 ? arr[4] : (i) == 5 ? arr[5] : (i) == 6 ? arr[6] : arr[7]))
static_assert(kMaxGroup == 8, "select chain written for 8 entries");

// the group forms of the window kernels: image blockIdx.z on its planes and its window, the weights window shared; bit z of dvec
// says whether image z's window takes 16-byte loads.  The workgroup's place in the image is (blockIdx.x, blockIdx.y), as in the
// single kernels, so image z's partials, written to part + z 3 n, are those of its single launch.
struct TvAutoPlanes {
    float* c[kMaxGroup];
    float* q[kMaxGroup];
    const float* d[kMaxGroup];
};
template <bool WEIGHTS>
__global__ __launch_bounds__(kTaThreads) void tvauto_norm_group_kernel(const TvAutoPlanes pl, const int stride, const float* __restrict__ w,
                                                                       const int wstride, const int rows, const int cols, const int N, const int dvec,
                                                                       const int wvec, double* __restrict__ part) {
    const int z = blockIdx.z;
    const size_t n = (size_t)gridDim.x * gridDim.y;
    tvauto_norm_block<WEIGHTS>(FDR_TA_PICK(pl.c, z), FDR_TA_PICK(pl.q, z), FDR_TA_PICK(pl.d, z), stride, w, wstride, rows, cols, N, (dvec >> z) & 1,
                               wvec, part + (size_t)z * 3 * n);
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
    tvauto_mu_fold(part + (size_t)z * 3 * n, n, FDR_TA_PICK(lv.sigma, z), tau, nu, mu + z, stat + 4 * z, FDR_TA_PICK(lv.trace, z));
}

// tvfree_data_kernel's step with mu read from the device scalar: a thread owns four consecutive pixels of one window row; in the
// group that straddles column `cols` the pixels beyond it keep the c and q they were loaded with
template <bool WEIGHTS>
__device__ __forceinline__ void tvauto_data_group4(float* __restrict__ c, float* __restrict__ q, const float* __restrict__ d, const int stride,
                                                   const float* __restrict__ w, const int wstride, const int rows, const int cols, const int N,
                                                   const float* __restrict__ mu_dev, const float nu, const int dvec, const int wvec) {
    const int j = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= rows || j >= cols) return;
    const float mu = *mu_dev;
    const size_t at = (size_t)i * N + j;
    const float4 c4 = *reinterpret_cast<const float4*>(c + at), q4 = *reinterpret_cast<const float4*>(q + at);
    float cc[4] = {c4.x, c4.y, c4.z, c4.w}, qq[4] = {q4.x, q4.y, q4.z, q4.w};
    float dd[4], mm[4] = {1.f, 1.f, 1.f, 1.f};
    ta_load_window4(d + (size_t)i * stride + j, j, cols, dvec != 0, 0.f, dd);
    if (WEIGHTS) ta_load_window4(w + (size_t)i * wstride + j, j, cols, wvec != 0, 1.f, mm);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (j + l < cols) tvfree_data_pixel(mu, nu, mm[l], dd[l], cc[l], qq[l]);
    }
    *reinterpret_cast<float4*>(q + at) = make_float4(qq[0], qq[1], qq[2], qq[3]);
    *reinterpret_cast<float4*>(c + at) = make_float4(cc[0], cc[1], cc[2], cc[3]);
}
template <bool WEIGHTS>
__global__ __launch_bounds__(kTaThreads) void tvauto_data_kernel(float* __restrict__ c, float* __restrict__ q, const float* __restrict__ d, const int stride,
                                                                 const float* __restrict__ w, const int wstride, const int rows, const int cols,
                                                                 const int N, const float* __restrict__ mu_dev, const float nu, const int dvec,
                                                                 const int wvec) {
    tvauto_data_group4<WEIGHTS>(c, q, d, stride, w, wstride, rows, cols, N, mu_dev, nu, dvec, wvec);
}
// the group form: image blockIdx.z with its own weight mu_dev[z]
template <bool WEIGHTS>
__global__ __launch_bounds__(kTaThreads) void tvauto_data_group_kernel(const TvAutoPlanes pl, const int stride, const float* __restrict__ w,
                                                                       const int wstride, const int rows, const int cols, const int N,
                                                                       const float* __restrict__ mu_dev, const float nu, const int dvec, const int wvec) {
    const int z = blockIdx.z;
    tvauto_data_group4<WEIGHTS>(FDR_TA_PICK(pl.c, z), FDR_TA_PICK(pl.q, z), FDR_TA_PICK(pl.d, z), stride, w, wstride, rows, cols, N, mu_dev + z, nu,
                                (dvec >> z) & 1, wvec);
}

namespace {
// the workgroup shape of both window kernels: tvfree_data_kernel's
void ta_block(int cols, int* tx, int* ty) {
    const int groups = (cols + 3) / 4;
    *tx = groups <= 64 ? 64 : groups <= 128 ? 128 : 256;
    *ty = kTaThreads / *tx;
}
bool ta_window_ok(const float* c, const float* q, const float* d, int stride, const float* w, int wstride, int rows, int cols, int M, int N) {
    return c && q && d && rows >= 1 && cols >= 1 && rows <= M && cols <= N && !(N & 3) && stride >= cols && !(w && wstride < cols);
}
}  // namespace

int tvauto_partials(int rows, int cols) {
    int tx, ty;
    ta_block(cols, &tx, &ty);
    const int groups = (cols + 3) / 4;
    return ((groups + tx - 1) / tx) * ((rows + ty * kTaRows - 1) / (ty * kTaRows));
}

// no window of an M x N plan makes more partials: the widest workgroup, one row of threads
int tvauto_max_partials(int M, int N) { return ((N + 4 * kTaThreads - 1) / (4 * kTaThreads)) * ((M + kTaRows - 1) / kTaRows); }

hipError_t launch_tvauto_norm(const float* c, const float* q, const float* d, int stride, const float* w, int wstride, int rows, int cols, int M, int N,
                              double* part, hipStream_t s) {
    if (!ta_window_ok(c, q, d, stride, w, wstride, rows, cols, M, N) || !part) return hipErrorInvalidValue;
    int tx, ty;
    ta_block(cols, &tx, &ty);
    const int groups = (cols + 3) / 4;
    const dim3 grid((unsigned)((groups + tx - 1) / tx), (unsigned)((rows + ty * kTaRows - 1) / (ty * kTaRows)));
    const int dvec = ((uintptr_t)d & 15) == 0 && (stride & 3) == 0;
    const int wvec = w && ((uintptr_t)w & 15) == 0 && (wstride & 3) == 0;
    if (w) hipLaunchKernelGGL((tvauto_norm_kernel<true>), grid, dim3(tx, ty), 0, s, c, q, d, stride, w, wstride, rows, cols, N, dvec, wvec, part);
    else hipLaunchKernelGGL((tvauto_norm_kernel<false>), grid, dim3(tx, ty), 0, s, c, q, d, stride, w, wstride, rows, cols, N, dvec, wvec, part);
    return hipGetLastError();
}

hipError_t launch_tvauto_mu(const double* part, int n, double sigma, double tau, float nu, float* mu, double* stat, double* trace, hipStream_t s) {
    if (n <= 0 || !part || !mu || !stat) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tvauto_mu_kernel, dim3(1), dim3(kTaThreads), 0, s, part, n, sigma, tau, nu, mu, stat, trace);
    return hipGetLastError();
}

hipError_t launch_tvauto_data(float* c, float* q, const float* d, int stride, const float* w, int wstride, int rows, int cols, int M, int N,
                              const float* mu, float nu, hipStream_t s) {
    if (!ta_window_ok(c, q, d, stride, w, wstride, rows, cols, M, N) || !mu) return hipErrorInvalidValue;
    int tx, ty;
    ta_block(cols, &tx, &ty);
    const int groups = (cols + 3) / 4;
    const dim3 grid((unsigned)((groups + tx - 1) / tx), (unsigned)((rows + ty - 1) / ty));
    const int dvec = ((uintptr_t)d & 15) == 0 && (stride & 3) == 0;
    const int wvec = w && ((uintptr_t)w & 15) == 0 && (wstride & 3) == 0;
    if (w) hipLaunchKernelGGL((tvauto_data_kernel<true>), grid, dim3(tx, ty), 0, s, c, q, d, stride, w, wstride, rows, cols, N, mu, nu, dvec, wvec);
    else hipLaunchKernelGGL((tvauto_data_kernel<false>), grid, dim3(tx, ty), 0, s, c, q, d, stride, w, wstride, rows, cols, N, mu, nu, dvec, wvec);
    return hipGetLastError();
}

namespace {
// the planes of a group for a kernel argument (entries past nimg repeat image 0) and the alignment bits of its windows
bool ta_group_planes(int nimg, float* const* c, float* const* q, const float* const* d, int stride, TvAutoPlanes* pl, int* dvec) {
    *dvec = 0;
    for (int k = 0; k < kMaxGroup; ++k) {
        const int i = k < nimg ? k : 0;
        if (!c[i] || !q[i] || !d[i]) return false;
        pl->c[k] = c[i]; pl->q[k] = q[i]; pl->d[k] = d[i];
        if (((uintptr_t)d[i] & 15) == 0 && (stride & 3) == 0) *dvec |= 1 << k;
    }
    return true;
}
}  // namespace

hipError_t launch_tvauto_norm_n(int nimg, const float* const* c, const float* const* q, const float* const* d, int stride, const float* w, int wstride,
                                int rows, int cols, int M, int N, double* part, hipStream_t s) {
    if (nimg < 1 || nimg > kMaxGroup) return hipErrorInvalidValue;
    if (nimg == 1) return launch_tvauto_norm(c[0], q[0], d[0], stride, w, wstride, rows, cols, M, N, part, s);
    if (!ta_window_ok(c[0], q[0], d[0], stride, w, wstride, rows, cols, M, N) || !part) return hipErrorInvalidValue;
    TvAutoPlanes pl;
    int dvec;
    if (!ta_group_planes(nimg, const_cast<float* const*>(c), const_cast<float* const*>(q), d, stride, &pl, &dvec)) return hipErrorInvalidValue;
    int tx, ty;
    ta_block(cols, &tx, &ty);
    const int groups = (cols + 3) / 4;
    const dim3 grid((unsigned)((groups + tx - 1) / tx), (unsigned)((rows + ty * kTaRows - 1) / (ty * kTaRows)), (unsigned)nimg);
    const int wvec = w && ((uintptr_t)w & 15) == 0 && (wstride & 3) == 0;
    if (w) hipLaunchKernelGGL((tvauto_norm_group_kernel<true>), grid, dim3(tx, ty), 0, s, pl, stride, w, wstride, rows, cols, N, dvec, wvec, part);
    else hipLaunchKernelGGL((tvauto_norm_group_kernel<false>), grid, dim3(tx, ty), 0, s, pl, stride, w, wstride, rows, cols, N, dvec, wvec, part);
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

hipError_t launch_tvauto_data_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride, int rows,
                                int cols, int M, int N, const float* mu, float nu, hipStream_t s) {
    if (nimg < 1 || nimg > kMaxGroup) return hipErrorInvalidValue;
    if (nimg == 1) return launch_tvauto_data(c[0], q[0], d[0], stride, w, wstride, rows, cols, M, N, mu, nu, s);
    if (!ta_window_ok(c[0], q[0], d[0], stride, w, wstride, rows, cols, M, N) || !mu) return hipErrorInvalidValue;
    TvAutoPlanes pl;
    int dvec;
    if (!ta_group_planes(nimg, c, q, d, stride, &pl, &dvec)) return hipErrorInvalidValue;
    int tx, ty;
    ta_block(cols, &tx, &ty);
    const int groups = (cols + 3) / 4;
    const dim3 grid((unsigned)((groups + tx - 1) / tx), (unsigned)((rows + ty - 1) / ty), (unsigned)nimg);
    const int wvec = w && ((uintptr_t)w & 15) == 0 && (wstride & 3) == 0;
    if (w) hipLaunchKernelGGL((tvauto_data_group_kernel<true>), grid, dim3(tx, ty), 0, s, pl, stride, w, wstride, rows, cols, N, mu, nu, dvec, wvec);
    else hipLaunchKernelGGL((tvauto_data_group_kernel<false>), grid, dim3(tx, ty), 0, s, pl, stride, w, wstride, rows, cols, N, mu, nu, dvec, wvec);
    return hipGetLastError();
}

}  // namespace fdr
