// fdr_blind.hip -- the kernels of blind Richardson-Lucy (fdr_richardson_lucy_blind_f32*; Fish, Brinicombe, Pike & Walker 1995,
// Holmes 1992): the PSF takes the same multiplicative step as the image, from the same ratio r,
//
//     corr_u(y) = crop( IDFT2( conj(DFT2(u)) . DFT2(y) ) )  to the top-left prows x pcols
//     plain form:  q = max(p . corr_u(pad(r)), 0)
//     free form:   num = corr_u(pad(r));  den = corr_u(W);  q = den > 0 ? max(p . num / den, 0) : 0
//     s = sum(q) in double;  p = s > 0 and finite ? q / s : p
//
// corr_u is passes A, B' and C of the operator path with conj(U) / (M N) as the table of pass B'.  Here: the column pass that
// makes that table from the row spectra pass A of u left in slot 0 (which it only reads), the start and the projection of the PSF
// (one workgroup each, sums in a fixed order: no atomics), the coverage weights of the free form and the Gaussian PSF.
#include "fdr_panel.hpp"

namespace fdr {

// The packed DC / Nyquist column of conj(U) * scale, in the layout of packed_column_filter_slot, which pass B' reads
// (fdr_panel_cols.hip): with C = U0 + i UN (U0 = U[., 0], UN = U[., N/2], both Hermitian along the column), ck = C[k], cmk = C[M - k],
//   S[k] = conj(U0[k]) (0 < k < M/2),  S[k] = conj(UN[M-k]) (M/2 < k < M),  S[0] = (U0[0], UN[0]),  S[M/2] = (U0[M/2], UN[M/2])
// (the slots at 0 and M/2 hold two real values: nothing to conjugate).
__device__ __forceinline__ float2 packed_column_conj_slot(float2 ck, float2 cmk, int k, int M, float scale) {
    const bool upper = k > M / 2;
    const float2 c = upper ? cmk : ck, cm = upper ? ck : cmk;          // C[j], C[M - j], j = min(k, M - k)
    const float u0r = 0.5f * (c.x + cm.x), u0i = 0.5f * (c.y - cm.y);  // U0 = (C + conj Cm) / 2
    const float unr = 0.5f * (c.y + cm.y), uni = 0.5f * (cm.x - c.x);  // UN = (C - conj Cm) / (2i)
    if (k == 0 || k == M / 2) return make_float2(u0r * scale, unr * scale);
    if (k < M / 2) return make_float2(u0r * scale, -(u0i * scale));
    return make_float2(unr * scale, -(uni * scale));
}

// The column pass of the image's table: forward column FFT of every panel of `src` (the row spectra of pass A; rows >= nvalid read
// as zero; never written), conj(U) * scale into `cdata`, row m of a panel at m * 4 (natural order): what
// fft_cols_panel_fwd_operator_kernel (fdr_rl.hip) stores as its second table, without its first one.
template <int LOGM>
__global__ __launch_bounds__(PanelGeom<LOGM>::THREADS) void fft_cols_panel_fwd_conj_kernel(
    const float2* __restrict__ src, float2* __restrict__ cdata, const float2* __restrict__ tw_fwd, const size_t pstride, const int npanels,
    const int nvalid, const float scale, const int packed0) {
    using St = Steps<LOGM>;
    using Geo = PanelGeom<LOGM>;
    constexpr int G = Geo::G, T = St::T;
    using Core = FftCore<LOGM, 4, 2, PolicyFast>;
    __shared__ float2 lds[G * 2 * St::BUF];
    const int g = threadIdx.x >> St::LOGT, tid = threadIdx.x & (T - 1);
    const int p = blockIdx.x * G + g;
    const bool active = p < npanels;
    const float2* sbase = src + (size_t)(active ? p : 0) * pstride;
    float2* cbase = cdata + (size_t)(active ? p : 0) * pstride;
    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);
    float2 v[4][8];
    FDR_PANEL_LOAD_VALID(Core, sbase, tid, nvalid, v)
    Core::template run<0, false>(v, lds + g * 2 * St::BUF, tw_fwd, bases, tid);
    const bool raw0 = packed0 && p == 0;  // uniform per thread group
    if (packed0 && blockIdx.x == 0) {     // uniform per workgroup: the packed column's slots need C[k] and C[M - k]
        float2* buf = lds + g * 2 * St::BUF;
        __syncthreads();  // the transform's last exchange has been read by every wave
        if (raw0) {
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) buf[Core::out_index(tid, u, q)] = v[0][u * Core::RHOL + q];
        }
        __syncthreads();
        if (raw0) {
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) {
                    const int s = u * Core::RHOL + q, k = Core::out_index(tid, u, q);
                    v[0][s] = packed_column_conj_slot(v[0][s], buf[(St::L - k) & (St::L - 1)], k, St::L, scale);
                }
        }
    }
    if (!active) return;
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) {
            const int s = u * Core::RHOL + q, m = Core::out_index(tid, u, q);
            float2 c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = (raw0 && j == 0) ? v[0][s] : make_float2(v[j][s].x * scale, -(v[j][s].y * scale));
            store4(cbase + (size_t)m * 4, c[0], c[1], c[2], c[3]);
        }
}

template <int LOGM>
static hipError_t launch_cols_panel_conj_t(const ColArgs& a, float2* conj_out, const float2* tw, hipStream_t s) {
    using Geo = PanelGeom<LOGM>;
    const int npanels = a.npanels > 0 ? a.npanels : a.N / 4;
    const int ntiles = (npanels + Geo::G - 1) / Geo::G;
    const float scale = (float)(1.0 / ((double)(1 << LOGM) * a.N));  // a power of two: exact
    hipLaunchKernelGGL((fft_cols_panel_fwd_conj_kernel<LOGM>), dim3(ntiles), dim3(Geo::THREADS), 0, s, (const float2*)a.data, conj_out, tw,
                       a.pstride, npanels, a.nvalid, scale, a.packed0);
    return hipGetLastError();
}

hipError_t launch_cols_panel_conj(int logm, const ColArgs& a, float2* conj_out, const float2* tw_fwd, hipStream_t s) {
    if (conj_out == nullptr || a.data == nullptr || conj_out == a.data) return hipErrorInvalidValue;
    FDR_DISPATCH_LOG(logm, launch_cols_panel_conj_t<LG>(a, conj_out, tw_fwd, s));
    return hipErrorInvalidValue;
}

// ---- the PSF's own kernels: one workgroup, n <= kBlindMaxPsf entries, dense (row stride pcols) ----
constexpr int kBlThreads = 1024;

// the workgroup's sum of `v` (every thread ends with it): a fixed tree over the threads
__device__ __forceinline__ double blind_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = kBlThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();  // red may be used again
    return s;
}

// the start: the caller's PSF (row stride pstride) dense into p; *status = 0 when it has no negative entry and a finite sum > 0
// (thread t adds entries t, t + 1024, ... in order, then the tree), else FDR_BLIND_BAD_START
__global__ __launch_bounds__(kBlThreads) void blind_psf_start_kernel(const float* __restrict__ psf, int pcols, int pstride, int n,
                                                                     float* __restrict__ p, int* __restrict__ status) {
    __shared__ double red[kBlThreads];
    double s = 0.0, neg = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlThreads) {
        const float v = psf[(size_t)(i / pcols) * pstride + i % pcols];
        p[i] = v;
        s += (double)v;
        if (v < 0.f) neg = 1.0;
    }
    const double sum = blind_block_sum(s, red);
    const double negs = blind_block_sum(neg, red);
    if (threadIdx.x == 0) *status = (negs == 0.0 && sum > 0.0 && sum <= 1.7976931348623157e308) ? 0 : 1;
}

// the projection: q from p, num (and den, free form; null in the plain form), s = sum(q) in double (thread t adds its entries in
// index order, then the tree), p = q / s when s is finite and > 0 -- else, and after a bad start, p stays.  With `out` not null the
// resulting PSF also goes there (row stride ostride): the caller's PSF, on the last step.
__device__ __forceinline__ float blind_q(float p, float num, const float* den, int i) {
    if (den == nullptr) return fmaxf(p * num, 0.f);
    const float d = den[i];
    return d > 0.f ? fmaxf(p * num / d, 0.f) : 0.f;
}
__global__ __launch_bounds__(kBlThreads) void blind_psf_project_kernel(float* __restrict__ p, const float* __restrict__ num,
                                                                       const float* __restrict__ den, int n, const int* __restrict__ status,
                                                                       float* __restrict__ out, int pcols, int ostride) {
    __shared__ double red[kBlThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlThreads) s += (double)blind_q(p[i], num[i], den, i);
    const double sum = blind_block_sum(s, red);
    const bool ok = *status == 0 && sum > 0.0 && sum <= 1.7976931348623157e308;
    for (int i = threadIdx.x; i < n; i += kBlThreads) {  // every thread rewrites the entries it read
        float v = p[i];
        if (ok) {
            v = (float)((double)blind_q(v, num[i], den, i) / sum);
            p[i] = v;
        }
        if (out) out[(size_t)(i / pcols) * ostride + i % pcols] = v;
    }
}

hipError_t launch_blind_psf_start(const float* psf, int prows, int pcols, int pstride, float* p, int* status, hipStream_t s) {
    if (prows <= 0 || pcols <= 0 || (size_t)prows * pcols > (size_t)kBlindMaxPsf) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blind_psf_start_kernel, dim3(1), dim3(kBlThreads), 0, s, psf, pcols, pstride, prows * pcols, p, status);
    return hipGetLastError();
}

hipError_t launch_blind_psf_project(float* p, const float* num, const float* den, int prows, int pcols, const int* status, float* out,
                                    int ostride, hipStream_t s) {
    if (prows <= 0 || pcols <= 0 || (size_t)prows * pcols > (size_t)kBlindMaxPsf) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blind_psf_project_kernel, dim3(1), dim3(kBlThreads), 0, s, p, num, den, prows * pcols, status, out, pcols, ostride);
    return hipGetLastError();
}

// free form: alpha in `wgt` -> wgt = alpha > sigma ? 1 / alpha : 0, the expression of rlfree_start_kernel (four pixels per lane)
__global__ __launch_bounds__(256) void blind_wgt_kernel(float4* __restrict__ wgt, size_t count4, float sigma) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count4) return;
    const float4 a = wgt[k];
    float4 w;
    w.x = a.x > sigma ? 1.f / a.x : 0.f;
    w.y = a.y > sigma ? 1.f / a.y : 0.f;
    w.z = a.z > sigma ? 1.f / a.z : 0.f;
    w.w = a.w > sigma ? 1.f / a.w : 0.f;
    wgt[k] = w;
}

hipError_t launch_blind_wgt(float* wgt, size_t count, float sigma, hipStream_t s) {
    if ((count & 3) != 0) return hipErrorInvalidValue;
    const size_t count4 = count / 4;
    hipLaunchKernelGGL(blind_wgt_kernel, dim3((unsigned)((count4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<float4*>(wgt), count4, sigma);
    return hipGetLastError();
}

// the Gaussian PSF of fdr_psf_gaussian: exp(-((i - c)^2 + (j - c)^2) / (2 sigma^2)), c = size / 2, in double, over its double sum
// (thread t adds entries t, t + 1024, ... in order, then the tree), rounded once
__global__ __launch_bounds__(kBlThreads) void psf_gaussian_kernel(int size, double sigma, float* __restrict__ out) {
    __shared__ double red[kBlThreads];
    const int n = size * size, c = size / 2;
    const double k = -1.0 / (2.0 * sigma * sigma);
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlThreads) {
        const double y = (double)(i / size - c), x = (double)(i % size - c);
        s += exp((y * y + x * x) * k);
    }
    const double sum = blind_block_sum(s, red);
    for (int i = threadIdx.x; i < n; i += kBlThreads) {
        const double y = (double)(i / size - c), x = (double)(i % size - c);
        out[i] = (float)(exp((y * y + x * x) * k) / sum);
    }
}

hipError_t launch_psf_gaussian(int size, double sigma, float* d_out, hipStream_t s) {
    if (size <= 0 || (size_t)size * size > (size_t)kBlindMaxPsf || !(sigma > 0.0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(psf_gaussian_kernel, dim3(1), dim3(kBlThreads), 0, s, size, sigma, d_out);
    return hipGetLastError();
}

}  // namespace fdr
