// fdr_tvframes.hip -- the one kernel multi-frame TV deconvolution (fdr_tv_deconv_frames_f32*, driver in fdr_api_tvframes.hip) adds to
// those of fdr_tv.hip, fdr_tvfree.hip and fdr_frames.hip: the solve table of K exposures under one TV prior,
//
//     T = (1 / (M N)) / (nu sum_k |H_k|^2 + rho L),
//
// from the K frame tables H_k / (M N) of fdr_set_frame_psfs*, in the layout pass B' reads its filter from.  A bin's |H_k|^2 is
// formed as tv_table_kernel (fdr_tv.hip) forms it, with that kernel's case analysis of the packed DC / Nyquist column per frame;
// the K values are added in double in ascending k and the quotient is rounded once, so one frame gives the bytes of tv_table_kernel
// on that frame's table.  A streaming kernel: 8 K + 8 bytes per bin, 32 bytes per lane and table, no LDS, no atomics.
#include "fdr_kernels.hpp"

#include <cstdint>

namespace fdr {

// One thread per row m of a panel p, as tv_table_kernel: the four columns 4 p .. 4 p + 3 of every frame's table -> T at the same
// place.  K is a constant: the loops unroll, every table pointer is a scalar of the argument block and the 2 K 16-byte loads of a
// thread are in flight together.  In the packed column of panel 0 (slot m holds H0[m] below M / 2, HN[M - m] above, two real values
// at 0 and M / 2) the x and y parts of the rows 0 and M / 2 are two bins and are summed apart.
template <int K>
__global__ __launch_bounds__(256) void tv_frames_table_kernel(const FrameTables tabs, float2* __restrict__ T, const double* __restrict__ lap,
                                                              const int M, const int N, const size_t pstride, const int npanels, const double nu,
                                                              const double rho) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)npanels * M) return;
    const int p = (int)(idx / (size_t)M), m = (int)(idx - (size_t)p * M);
    const double mn = (double)M * (double)N, inv_mn = 1.0 / mn, mn2 = mn * mn;  // powers of two: exact
    const double* a = lap;
    const double* b = lap + M;
    const size_t at = (size_t)p * pstride + (size_t)m * 4;
    float4 h01[K], h23[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        h01[k] = *reinterpret_cast<const float4*>(tabs.p[k] + at);
        h23[k] = *reinterpret_cast<const float4*>(tabs.p[k] + at + 2);
    }
    const bool packed = p == 0, split = packed && (m == 0 || m == M / 2);
    double s[4] = {0.0, 0.0, 0.0, 0.0}, sy = 0.0;  // the bins' sums; sy: the second bin of a split packed slot
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float2 h[4] = {make_float2(h01[k].x, h01[k].y), make_float2(h01[k].z, h01[k].w), make_float2(h23[k].x, h23[k].y),
                             make_float2(h23[k].z, h23[k].w)};
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const double hx = h[l].x, hy = h[l].y;
            if (l == 0 && split) {
                const double tx = hx * hx * mn2, ty = hy * hy * mn2;
                s[0] = k == 0 ? tx : s[0] + tx;
                sy = k == 0 ? ty : sy + ty;
            } else {
                const double t = (hx * hx + hy * hy) * mn2;
                s[l] = k == 0 ? t : s[l] + t;
            }
        }
    }
    float2 t[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (packed && l == 0) {  // the packed column's slot S[m]
            if (split)
                t[l] = make_float2(tv_quotient(s[0], a[m] + b[0], nu, rho, inv_mn), tv_quotient(sy, a[m] + b[N / 2], nu, rho, inv_mn));
            else if (m < M / 2)
                t[l] = make_float2(tv_quotient(s[0], a[m] + b[0], nu, rho, inv_mn), 0.f);
            else
                t[l] = make_float2(tv_quotient(s[0], a[M - m] + b[N / 2], nu, rho, inv_mn), 0.f);
        } else {
            t[l] = make_float2(tv_quotient(s[l], a[m] + b[4 * p + l], nu, rho, inv_mn), 0.f);
        }
    }
    *reinterpret_cast<float4*>(T + at) = make_float4(t[0].x, t[0].y, t[1].x, t[1].y);
    *reinterpret_cast<float4*>(T + at + 2) = make_float4(t[2].x, t[2].y, t[3].x, t[3].y);
}

namespace {

template <int K>
hipError_t tv_frames_table_k(const FrameTables& tabs, float2* T, const double* lap, int M, int N, size_t pstride, int npanels, double nu, double rho,
                             hipStream_t s) {
    const size_t count = (size_t)npanels * M;
    hipLaunchKernelGGL((tv_frames_table_kernel<K>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, tabs, T, lap, M, N, pstride, npanels, nu,
                       rho);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tv_frames_table(const FrameTables& tabs, int count, float2* T, const double* lap, int M, int N, size_t pstride, int npanels,
                                  double nu, double rho, hipStream_t s) {
    if (!T || !lap || count < 1 || count > kMaxGroup || M < 2 || N < 2 || npanels < 1 || ((uintptr_t)T & 15) != 0) return hipErrorInvalidValue;
    for (int k = 0; k < count; ++k)
        if (!tabs.p[k] || ((uintptr_t)tabs.p[k] & 15) != 0) return hipErrorInvalidValue;
    switch (count) {
        case 1: return tv_frames_table_k<1>(tabs, T, lap, M, N, pstride, npanels, nu, rho, s);
        case 2: return tv_frames_table_k<2>(tabs, T, lap, M, N, pstride, npanels, nu, rho, s);
        case 3: return tv_frames_table_k<3>(tabs, T, lap, M, N, pstride, npanels, nu, rho, s);
        case 4: return tv_frames_table_k<4>(tabs, T, lap, M, N, pstride, npanels, nu, rho, s);
        case 5: return tv_frames_table_k<5>(tabs, T, lap, M, N, pstride, npanels, nu, rho, s);
        case 6: return tv_frames_table_k<6>(tabs, T, lap, M, N, pstride, npanels, nu, rho, s);
        case 7: return tv_frames_table_k<7>(tabs, T, lap, M, N, pstride, npanels, nu, rho, s);
        default: return tv_frames_table_k<8>(tabs, T, lap, M, N, pstride, npanels, nu, rho, s);
    }
}

}  // namespace fdr
