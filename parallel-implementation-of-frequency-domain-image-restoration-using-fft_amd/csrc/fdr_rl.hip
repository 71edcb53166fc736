// fdr_rl.hip -- the forward blur operator and Richardson-Lucy deconvolution (fdr_blur_f32*, fdr_richardson_lucy_f32*; fast
// panel half-spectrum path):
//
//     blur(x)   = window( IDFT2( H       . DFT2(pad(x)) ) )
//     blur^T(y) = window( IDFT2( conj(H) . DFT2(pad(y)) ) )
//     RL:  u = max(d, 0);  n times:  c = blur(u);  r = c > tau ? max(d, 0) / c : 0;  u = max(u . blur^T(r), 0)
//
// A blur is passes A, B' and C of the Wiener operator (fdr_panel_*.hip) with the operator tables in place of W: B' runs unchanged
// on H / (M N) or conj(H) / (M N), and the inverse row pass ends in one of the operator kinds of rows4_rl_value (blur, ratio,
// update), cropped to the window.  Two kernels live here: the PSF column pass that writes both tables in one launch, and the
// initial estimate.  1 / (M N) is a power of two, so folding it into the tables is exact.
#include "fdr_panel.hpp"

namespace fdr {

// Filter slot S[k] of the packed DC / Nyquist column (column 0 of panel 0 carries C = H0 + i HN, H0 = H[., 0], HN = H[., N/2],
// both Hermitian along the column) for the operator H itself, scaled: the layout of packed_column_filter_slot, which pass B'
// reads (packed_column_filter of fdr_panel_cols.hip):
//   S[k] = H0[k] (0 < k < M/2),  S[k] = HN[M-k] (M/2 < k < M),  S[0] = (H0[0], HN[0]),  S[M/2] = (H0[M/2], HN[M/2])
// ck = C[k], cmk = C[M - k]; evaluated at j = min(k, M - k).  The conj(H) slot is its conjugate, except at 0 and M/2 (real parts).
__device__ __forceinline__ float2 packed_column_operator_slot(float2 ck, float2 cmk, int k, int M, float scale) {
    const bool upper = k > M / 2;
    const float2 c = upper ? cmk : ck, cm = upper ? ck : cmk;  // C[j], C[M - j]
    const float h0r = 0.5f * (c.x + cm.x), h0i = 0.5f * (c.y - cm.y);  // H0 = (C + conj Cm) / 2
    const float hnr = 0.5f * (c.y + cm.y), hni = 0.5f * (cm.x - c.x);  // HN = (C - conj Cm) / (2i)
    if (k == 0 || k == M / 2) return make_float2(h0r * scale, hnr * scale);
    if (k < M / 2) return make_float2(h0r * scale, h0i * scale);
    return make_float2(hnr * scale, hni * scale);
}

// The PSF column pass of the panel path (fft_cols_panel_fwd_filter_kernel of fdr_panel_cols.hip) for the operator tables: forward
// column FFT of every panel of `hdata` (the PSF's row spectra; rows >= nvalid read as zero), then H * scale back into `hdata`
// and conj(H) * scale into `cdata`, row m of a panel at m * 4 (natural order).  The packed column leaves as its slots
// (packed_column_operator_slot).  No minimum occupancy in the launch bounds: this pass runs once per PSF.
template <int LOGM>
__global__ __launch_bounds__(PanelGeom<LOGM>::THREADS) void fft_cols_panel_fwd_operator_kernel(
    float2* __restrict__ hdata, float2* __restrict__ cdata, const float2* __restrict__ tw_fwd, const size_t pstride, const int npanels,
    const int nvalid, const float scale, const int packed0) {
    using St = Steps<LOGM>;
    using Geo = PanelGeom<LOGM>;
    constexpr int G = Geo::G, T = St::T;
    using Core = FftCore<LOGM, 4, 2, PolicyFast>;
    __shared__ float2 lds[G * 2 * St::BUF];
    const int g = threadIdx.x >> St::LOGT, tid = threadIdx.x & (T - 1);
    const int p = blockIdx.x * G + g;
    const bool active = p < npanels;
    float2* hbase = hdata + (size_t)(active ? p : 0) * pstride;
    float2* cbase = cdata + (size_t)(active ? p : 0) * pstride;
    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);
    float2 v[4][8];
    FDR_PANEL_LOAD_VALID(Core, hbase, tid, nvalid, v)
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
                    v[0][s] = packed_column_operator_slot(v[0][s], buf[(St::L - k) & (St::L - 1)], k, St::L, scale);
                }
        }
    }
    if (!active) return;
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) {
            const int s = u * Core::RHOL + q, m = Core::out_index(tid, u, q);
            float2 h[4], c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h[j] = (raw0 && j == 0) ? v[0][s] : make_float2(v[j][s].x * scale, v[j][s].y * scale);
                c[j] = make_float2(h[j].x, -h[j].y);
            }
            // the packed column's slots at 0 and M/2 hold two real values, not one complex one: no conjugate there
            if (raw0 && (m == 0 || m == St::L / 2)) c[0] = h[0];
            store4(hbase + (size_t)m * 4, h[0], h[1], h[2], h[3]);
            store4(cbase + (size_t)m * 4, c[0], c[1], c[2], c[3]);
        }
}

template <int LOGM>
static hipError_t launch_cols_panel_operator_t(const ColArgs& a, float2* conj_out, const float2* tw, hipStream_t s) {
    using Geo = PanelGeom<LOGM>;
    const int npanels = a.npanels > 0 ? a.npanels : a.N / 4;
    const int ntiles = (npanels + Geo::G - 1) / Geo::G;
    const float scale = (float)(1.0 / ((double)(1 << LOGM) * a.N));  // a power of two: exact
    hipLaunchKernelGGL((fft_cols_panel_fwd_operator_kernel<LOGM>), dim3(ntiles), dim3(Geo::THREADS), 0, s, a.data, conj_out, tw, a.pstride,
                       npanels, a.nvalid, scale, a.packed0);
    return hipGetLastError();
}

hipError_t launch_cols_panel_operator(int logm, const ColArgs& a, float2* conj_out, const float2* tw_fwd, hipStream_t s) {
    if (conj_out == nullptr || a.data == nullptr) return hipErrorInvalidValue;
    FDR_DISPATCH_LOG(logm, launch_cols_panel_operator_t<LG>(a, conj_out, tw_fwd, s));
    return hipErrorInvalidValue;
}

// ---- the initial estimate u = max(d, 0) on the window (one row per blockIdx.y) ----
__global__ __launch_bounds__(256) void rl_init_kernel(const float* __restrict__ d, int cols, int stride, float* __restrict__ u, int ustride) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t y = blockIdx.y;
    if (x < cols) u[y * ustride + x] = fmaxf(d[y * stride + x], 0.f);
}

hipError_t launch_rl_init(const float* d, int rows, int cols, int stride, float* u, int ustride, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(rl_init_kernel, dim3((unsigned)((cols + 255) / 256), (unsigned)rows), dim3(256), 0, s, d, cols, stride, u, ustride);
    return hipGetLastError();
}

}  // namespace fdr
