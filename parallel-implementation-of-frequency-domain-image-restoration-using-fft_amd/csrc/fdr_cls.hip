// fdr_cls.hip -- the constrained least-squares (CLS) filter of fdr_set_psf_cls* (fast mode):
//
//     W(u, v) = conj(H) / (|H|^2 + K + gamma L(u, v)^2),   L(u, v) = 4 sin^2(pi u / M) + 4 sin^2(pi v / N)
//
// L is the symbol of the periodic 5-point Laplacian.  The plan keeps a_u = 4 sin^2(pi u / M) (u < M) followed by
// b_v = 4 sin^2(pi v / N) (v < N) as a double table (fdr_api_wiener.hip, ensure_lap_table); cls_filter_fast / cls_reg
// (fdr_fft_core.hpp) evaluate the quotient in double and round once, as the Wiener filter does.  Two of the four filter
// sites live here, in a translation unit of their own so that the Wiener kernels of fdr_panel_cols.hip and fdr_simple.hip keep
// their code: the PSF column pass of the panel path (half and full spectrum) and the pointwise filter of the simple path.
// The mixed-radix site is the MIX_COLS_FILTER_CLS kind of fdr_mixed.hip.
#include "fdr_panel.hpp"

namespace fdr {

// The PSF column pass of the panel path (fft_cols_panel_fwd_filter_kernel of fdr_panel_cols.hip) with the CLS quotient: forward
// column FFT of every panel, in place, rows >= nvalid read as zero.  A value's row frequency is Core::out_index (the transform
// leaves in last-step order; W is stored at that row), its column 4 p + lane (v < N/2 in the half spectrum, v < N in the full
// one).  The packed DC / Nyquist column of the half spectrum (column 0 of panel 0) leaves as its filter slots
// (packed_column_cls_slot) with b_0 for W0 and b_{N/2} for WN.  No minimum occupancy in the launch bounds: the quotient with its
// table values needs more than 128 registers below LOGM 13, and this pass runs once per PSF.
template <int LOGM>
__global__ __launch_bounds__(PanelGeom<LOGM>::THREADS) void fft_cols_panel_fwd_cls_kernel(
    float2* __restrict__ data, const float2* __restrict__ tw_fwd, const size_t pstride, const int npanels, const int nvalid, const float K,
    const int packed0, const double* __restrict__ lap, const int N, const double gamma) {
    using St = Steps<LOGM>;
    using Geo = PanelGeom<LOGM>;
    constexpr int G = Geo::G, T = St::T;
    using Core = FftCore<LOGM, 4, 2, PolicyFast>;
    __shared__ float2 lds[G * 2 * St::BUF];
    const int g = threadIdx.x >> St::LOGT, tid = threadIdx.x & (T - 1);
    const int p = blockIdx.x * G + g;
    const bool active = p < npanels;
    float2* pbase = data + (size_t)(active ? p : 0) * pstride;
    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);
    float2 v[4][8];
    FDR_PANEL_LOAD_VALID(Core, pbase, tid, nvalid, v)
    Core::template run<0, false>(v, lds + g * 2 * St::BUF, tw_fwd, bases, tid);
    // opaque copy of tid: the row indices below are recomputed from it instead of living across the transform (at LOGM 13 the
    // kernel is held to 128 registers by its 1024 threads and would spill them)
    int otid = tid;
    asm volatile("" : "+v"(otid));
    const bool raw0 = packed0 && p == 0;  // uniform per thread group
    if (packed0 && blockIdx.x == 0) {     // uniform per workgroup: the packed column's slots need C[k] and C[M - k]
        float2* buf = lds + g * 2 * St::BUF;
        __syncthreads();  // the transform's last exchange has been read by every wave
        if (raw0) {
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) buf[Core::out_index(otid, u, q)] = v[0][u * Core::RHOL + q];
        }
        __syncthreads();
        if (raw0) {
            // one slot at a time (two double quotients each), from C in `buf` into the second buffer and back into the registers:
            // a thread reads back only the slots it wrote
            float2* slots = buf + St::BUF;
#pragma unroll 1
            for (int s = 0; s < Core::NUL * Core::RHOL; ++s) {
                const int k = Core::out_index(otid, s / Core::RHOL, s % Core::RHOL);
                const int j = k <= St::L / 2 ? k : St::L - k;
                slots[k] = packed_column_cls_slot(buf[k], buf[(St::L - k) & (St::L - 1)], k, St::L, K, cls_reg(lap, St::L, j, 0, gamma),
                                                  cls_reg(lap, St::L, j, N / 2, gamma));
            }
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) v[0][u * Core::RHOL + q] = slots[Core::out_index(otid, u, q)];
        }
    }
    int v0 = 4 * (active ? p : 0);  // an inactive thread group computes on panel 0 and stores nothing
    // from T = 64 on, a wave lies inside one thread group: its columns are wave-uniform and b_v comes by scalar loads
    if constexpr (T >= 64) v0 = __builtin_amdgcn_readfirstlane(v0);
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) {
            const int s = u * Core::RHOL + q, m = Core::out_index(otid, u, q);
            if (!raw0) v[0][s] = cls_filter_fast(v[0][s], K, cls_reg(lap, St::L, m, v0, gamma));
            v[1][s] = cls_filter_fast(v[1][s], K, cls_reg(lap, St::L, m, v0 + 1, gamma));
            v[2][s] = cls_filter_fast(v[2][s], K, cls_reg(lap, St::L, m, v0 + 2, gamma));
            v[3][s] = cls_filter_fast(v[3][s], K, cls_reg(lap, St::L, m, v0 + 3, gamma));
        }
    // row m of the panel at m * 4 (natural order).  Not panel_store_out (fdr_panel.hpp): its address form gives all eleven kernels
    // other registers and schedules (tools/kernel_diff.py)
    if (active) {
#pragma unroll
        for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHOL; ++q) {
                const int s = u * Core::RHOL + q;
                store4(pbase + (size_t)Core::out_index(otid, u, q) * 4, v[0][s], v[1][s], v[2][s], v[3][s]);
            }
    }
}

template <int LOGM>
static hipError_t launch_cols_panel_cls_t(const ColArgs& a, const double* lap, double gamma, const float2* tw, hipStream_t s) {
    using Geo = PanelGeom<LOGM>;
    const int npanels = a.npanels > 0 ? a.npanels : a.N / 4;
    const int ntiles = (npanels + Geo::G - 1) / Geo::G;
    hipLaunchKernelGGL((fft_cols_panel_fwd_cls_kernel<LOGM>), dim3(ntiles), dim3(Geo::THREADS), 0, s, a.data, tw, a.pstride, npanels, a.nvalid, a.K,
                       a.packed0, lap, a.N, gamma);
    return hipGetLastError();
}

hipError_t launch_cols_panel_cls(int logm, const ColArgs& a, const double* lap, double gamma, const float2* tw_fwd, hipStream_t s) {
    if (lap == nullptr) return hipErrorInvalidValue;
    FDR_DISPATCH_LOG(logm, launch_cols_panel_cls_t<LG>(a, lap, gamma, tw_fwd, s));
    return hipErrorInvalidValue;
}

// ---- simple path: the CLS quotient on the row-major M x N spectrum (make_filter_fast_kernel of fdr_simple.hip); element i is bin
// (i / N, i % N) ----
__global__ void make_filter_cls_kernel(const float2* __restrict__ H, float2* __restrict__ W, int M, int N, float K,
                                       const double* __restrict__ lap, double gamma) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)M * N) return;
    const int u = (int)(i / (size_t)N), v = (int)(i - (size_t)u * N);
    W[i] = cls_filter_fast(H[i], K, cls_reg(lap, M, u, v, gamma));
}

hipError_t launch_make_filter_cls(const float2* H, float2* W, int M, int N, float K, const double* lap, double gamma, hipStream_t s) {
    if (lap == nullptr) return hipErrorInvalidValue;
    const size_t count = (size_t)M * N;
    hipLaunchKernelGGL(make_filter_cls_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, H, W, M, N, K, lap, gamma);
    return hipGetLastError();
}

}  // namespace fdr
