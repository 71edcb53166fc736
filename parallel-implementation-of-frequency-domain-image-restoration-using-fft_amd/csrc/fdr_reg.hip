// fdr_reg.hip -- choosing the regularisation weight of the Wiener / CLS filter from the picture (fdr_noise_sigma_f32*,
// fdr_reg_curve_f32*, fdr_choose_reg_f32*; fast panel half-spectrum path):
//
//     G = DFT2(pad(d));  P = |G|^2 / (M N)
//     t = K + gamma L^2;  q = t / (|H|^2 + t)   (0 for a denominator that is not positive)
//     rho(K, gamma) = sum over the M N bins of P q^2;  trace(K, gamma) = sum over the M N bins of q
//     sigma = sqrt(pi / 2) S / (6 (rows - 2)(cols - 2)),  S = sum over the interior of |d * [[1,-2,1],[-2,4,-2],[1,-2,1]]|
//
// Three kernels: the Immerkaer sum, the column pass that turns the row spectra of pass A into the power plane P (a sibling of
// fft_cols_panel_fwd_operator_kernel of fdr_rl.hip, not in place), and the sweep that evaluates rho and trace for C candidate
// pairs at once from P, the operator table H / (M N) and the Laplacian table.  Every sum is taken in double in a fixed order (per
// thread, per wave by shuffles, per workgroup, then one folding workgroup): no atomics, the same bits on every call.
#include "fdr_panel.hpp"

namespace fdr {

constexpr int kRegThreads = 256;
constexpr int kRegWaves = kRegThreads / 64;

// sum over the 64 lanes of a wave in a fixed order; lane 0 holds it
__device__ __forceinline__ double reg_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// ---- the noise estimate ----
// A tile is kRegThreads interior pixels of one interior row; workgroup b takes the tiles b, b + gridDim.x, ... in order and writes
// its sum of |d * n| (double) to part[b].
__global__ __launch_bounds__(kRegThreads) void reg_noise_kernel(const float* __restrict__ d, const int rows, const int cols, const int stride,
                                                                const int tiles_per_row, const int ntiles, double* __restrict__ part) {
    __shared__ double red[kRegWaves];
    double acc = 0.0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int i = 1 + t / tiles_per_row;
        const int j = 1 + (t - (i - 1) * tiles_per_row) * kRegThreads + (int)threadIdx.x;
        if (j < cols - 1) {
            const float* r0 = d + (size_t)(i - 1) * stride + j;
            const float* r1 = r0 + stride;
            const float* r2 = r1 + stride;
            const double corners = ((double)r0[-1] + (double)r0[1]) + ((double)r2[-1] + (double)r2[1]);
            const double edges = ((double)r0[0] + (double)r2[0]) + ((double)r1[-1] + (double)r1[1]);
            acc += fabs(corners - 2.0 * edges + 4.0 * (double)r1[0]);
        }
    }
    acc = reg_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
#pragma unroll
        for (int w = 1; w < kRegWaves; ++w) s += red[w];
        part[blockIdx.x] = s;
    }
}

// one workgroup: part[n] = sum of part[0 .. n) (thread t adds t, t + 256, ... in order, then waves, then the four wave sums)
__global__ __launch_bounds__(kRegThreads) void reg_noise_fold_kernel(double* __restrict__ part, const int n) {
    __shared__ double red[kRegWaves];
    double acc = 0.0;
    for (int k = threadIdx.x; k < n; k += kRegThreads) acc += part[k];
    acc = reg_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
#pragma unroll
        for (int w = 1; w < kRegWaves; ++w) s += red[w];
        part[n] = s;
    }
}

int reg_noise_partials(int rows, int cols) {
    if (rows < 3 || cols < 3) return 0;
    const long long tiles = (long long)(rows - 2) * ((cols - 2 + kRegThreads - 1) / kRegThreads);
    return (int)(tiles < kRegMaxPartials ? tiles : kRegMaxPartials);
}

hipError_t launch_reg_noise(const float* d, int rows, int cols, int stride, double* part, hipStream_t s) {
    if (!d || !part || rows < 3 || cols < 3 || stride < cols) return hipErrorInvalidValue;
    const int tiles_per_row = (cols - 2 + kRegThreads - 1) / kRegThreads;
    const int ntiles = (rows - 2) * tiles_per_row;  // <= 8190 * 32
    const int nb = reg_noise_partials(rows, cols);
    hipLaunchKernelGGL(reg_noise_kernel, dim3((unsigned)nb), dim3(kRegThreads), 0, s, d, rows, cols, stride, tiles_per_row, ntiles, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(reg_noise_fold_kernel, dim3(1), dim3(kRegThreads), 0, s, part, nb);
    return hipGetLastError();
}

// ---- the power plane ----
// Forward column FFT of every panel of `data` (the picture's row spectra of pass A; rows >= nvalid read as zero), then
// P = |G|^2 * scale (scale = 1 / (M N)) as ONE float per bin into `power`: row m of panel p at p * pstride + m * 4 floats.  `data` is
// only read.  Column 0 of panel 0 carries C = G0 + i GN (G0 = G[., 0], GN = G[., N/2], both Hermitian along the column); its slots:
//   k <= M/2: |G0[k]|^2 scale,   k > M/2: |GN[M - k]|^2 scale,   extras[0] = |GN[0]|^2 scale,  extras[1] = |GN[M/2]|^2 scale
// so that every non-redundant bin of the two columns has one slot.  C[k] and C[M - k] meet through LDS, as in
// fft_cols_panel_fwd_operator_kernel.
template <int LOGM>
__global__ __launch_bounds__(PanelGeom<LOGM>::THREADS) void fft_cols_panel_power_kernel(
    const float2* __restrict__ data, float* __restrict__ power, float* __restrict__ extras, const float2* __restrict__ tw_fwd,
    const size_t pstride, const int npanels, const int nvalid, const float scale, const int packed0) {
    using St = Steps<LOGM>;
    using Geo = PanelGeom<LOGM>;
    constexpr int G = Geo::G, T = St::T;
    using Core = FftCore<LOGM, 4, 2, PolicyFast>;
    __shared__ float2 lds[G * 2 * St::BUF];
    const int g = threadIdx.x >> St::LOGT, tid = threadIdx.x & (T - 1);
    const int p = blockIdx.x * G + g;
    const bool active = p < npanels;
    const float2* dbase = data + (size_t)(active ? p : 0) * pstride;
    float* pbase = power + (size_t)(active ? p : 0) * pstride;
    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);
    float2 v[4][8];
    FDR_PANEL_LOAD_VALID(Core, dbase, tid, nvalid, v)
    Core::template run<0, false>(v, lds + g * 2 * St::BUF, tw_fwd, bases, tid);
    const bool raw0 = packed0 && p == 0;  // uniform per thread group
    float p0[8];                          // the packed column's slots
    if (packed0 && blockIdx.x == 0) {     // uniform per workgroup
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
                    const float2 ck = v[0][s], cmk = buf[(St::L - k) & (St::L - 1)];
                    const bool upper = k > St::L / 2;
                    const float2 c = upper ? cmk : ck, cm = upper ? ck : cmk;          // C[j], C[M - j], j = min(k, M - k)
                    const float g0r = 0.5f * (c.x + cm.x), g0i = 0.5f * (c.y - cm.y);  // G0 = (C + conj Cm) / 2
                    const float gnr = 0.5f * (c.y + cm.y), gni = 0.5f * (cm.x - c.x);  // GN = (C - conj Cm) / (2i)
                    const float a0 = (g0r * g0r + g0i * g0i) * scale, an = (gnr * gnr + gni * gni) * scale;
                    p0[s] = upper ? an : a0;
                    if (k == 0) extras[0] = an;
                    if (k == St::L / 2) extras[1] = an;
                }
        }
    }
    if (!active) return;
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) {
            const int s = u * Core::RHOL + q, m = Core::out_index(tid, u, q);
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (v[j][s].x * v[j][s].x + v[j][s].y * v[j][s].y) * scale;
            if (raw0) o[0] = p0[s];
            *reinterpret_cast<float4*>(pbase + (size_t)m * 4) = make_float4(o[0], o[1], o[2], o[3]);
        }
}

template <int LOGM>
static hipError_t launch_cols_panel_power_t(const ColArgs& a, float* power, float* extras, const float2* tw, hipStream_t s) {
    using Geo = PanelGeom<LOGM>;
    const int npanels = a.npanels > 0 ? a.npanels : a.N / 4;
    const int ntiles = (npanels + Geo::G - 1) / Geo::G;
    const float scale = (float)(1.0 / ((double)(1 << LOGM) * a.N));  // a power of two: exact
    hipLaunchKernelGGL((fft_cols_panel_power_kernel<LOGM>), dim3(ntiles), dim3(Geo::THREADS), 0, s, (const float2*)a.data, power, extras, tw,
                       a.pstride, npanels, a.nvalid, scale, a.packed0);
    return hipGetLastError();
}

hipError_t launch_cols_panel_power(int logm, const ColArgs& a, float* power, float* extras, const float2* tw_fwd, hipStream_t s) {
    if (power == nullptr || extras == nullptr || a.data == nullptr || !a.packed0) return hipErrorInvalidValue;
    FDR_DISPATCH_LOG(logm, launch_cols_panel_power_t<LG>(a, power, extras, tw_fwd, s));
    return hipErrorInvalidValue;
}

// ---- the sweep ----
// q = t / (h2 + t) for one bin, and its terms: w q into tr, w P q^2 into rho (w = how many bins of the full spectrum the entry is)
__device__ __forceinline__ void reg_bin(double h2, double l2, double P, double w, double K, double gamma, double& rho, double& tr) {
    const double t = K + gamma * l2, den = h2 + t;
    const double q = den > 0.0 ? t / den : 0.0;
    tr += w * q;
    rho += (w * P) * (q * q);
}

// One thread per row m of a panel p, as tv_table_kernel: the four columns 4 p .. 4 p + 3 of op_h (H / (M N)) and of the power
// plane, for C candidate pairs cand[2 c] = K, cand[2 c + 1] = gamma.  Every entry stands for two bins of the full spectrum, (m, v) and
// (M - m, N - v); the four real bins (0, 0), (M/2, 0), (0, N/2), (M/2, N/2) stand for themselves, the last two through `extras`
// and the second halves of the H slots at 0 and M/2 of the packed column.  Workgroup b takes the entries b * 256 + t, then
// (b + gridDim.x) * 256 + t, ... and writes its 2 C sums (rho_c, trace_c) to part[b * 2 C ..).
template <int C>
__global__ __launch_bounds__(kRegThreads) void reg_curve_kernel(const float2* __restrict__ op_h, const float* __restrict__ power,
                                                                const float* __restrict__ extras, const double* __restrict__ lap,
                                                                const double* __restrict__ cand, const int M, const int N, const size_t pstride,
                                                                const int npanels, double* __restrict__ part) {
    __shared__ double red[kRegWaves][2 * C];
    const double mn = (double)M * (double)N, mn2 = mn * mn;  // powers of two: exact
    const double* a = lap;
    const double* b = lap + M;
    double rho[C], tr[C];
#pragma unroll
    for (int c = 0; c < C; ++c) rho[c] = tr[c] = 0.0;
    const size_t count = (size_t)npanels * M;
    for (size_t idx = (size_t)blockIdx.x * kRegThreads + threadIdx.x; idx < count; idx += (size_t)gridDim.x * kRegThreads) {
        const int p = (int)(idx / (size_t)M), m = (int)(idx - (size_t)p * M);
        const size_t at = (size_t)p * pstride + (size_t)m * 4;
        const float4 h01 = *reinterpret_cast<const float4*>(op_h + at), h23 = *reinterpret_cast<const float4*>(op_h + at + 2);
        const float4 pw = *reinterpret_cast<const float4*>(power + at);
        const float2 h[4] = {make_float2(h01.x, h01.y), make_float2(h01.z, h01.w), make_float2(h23.x, h23.y), make_float2(h23.z, h23.w)};
        const float pv[4] = {pw.x, pw.y, pw.z, pw.w};
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const double hx = h[l].x, hy = h[l].y;
            double h2 = (hx * hx + hy * hy) * mn2, lp = a[m] + b[4 * p + l], w = 2.0;
            if (p == 0 && l == 0) {  // the packed column's slot m
                if (m == 0 || m == M / 2) {
                    // two real bins: (m, 0) here, (m, N/2) from the slot's second half and the extra float
                    const double hn2 = hy * hy * mn2, ln = a[m] + b[N / 2], ln2 = ln * ln, pn = extras[m == 0 ? 0 : 1];
#pragma unroll
                    for (int c = 0; c < C; ++c) reg_bin(hn2, ln2, pn, 1.0, cand[2 * c], cand[2 * c + 1], rho[c], tr[c]);
                    h2 = hx * hx * mn2;
                    w = 1.0;
                } else if (m > M / 2) {
                    lp = a[M - m] + b[N / 2];
                }
            }
            const double l2 = lp * lp, P = pv[l];
#pragma unroll
            for (int c = 0; c < C; ++c) reg_bin(h2, l2, P, w, cand[2 * c], cand[2 * c + 1], rho[c], tr[c]);
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double r = reg_wave_sum(rho[c]), t = reg_wave_sum(tr[c]);
        if (lane == 0) { red[wave][2 * c] = r; red[wave][2 * c + 1] = t; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * C) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kRegWaves; ++w) s += red[w][threadIdx.x];
        part[(size_t)blockIdx.x * 2 * C + threadIdx.x] = s;
    }
}

// one workgroup: out[o] = sum over the nb workgroups of part[b * nv + o], o < nout (wave w folds o = w, w + 4, ...: lane l adds the
// workgroups l, l + 64, ... in order, then the fixed shuffle tree)
__global__ __launch_bounds__(kRegThreads) void reg_curve_fold_kernel(const double* __restrict__ part, const int nb, const int nv, const int nout,
                                                                     double* __restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int o = wave; o < nout; o += kRegWaves) {
        double acc = 0.0;
        for (int k = lane; k < nb; k += 64) acc += part[(size_t)k * nv + o];
        acc = reg_wave_sum(acc);
        if (lane == 0) out[o] = acc;
    }
}

int reg_curve_partials(int M, int npanels) {
    const size_t groups = ((size_t)npanels * M + kRegThreads - 1) / kRegThreads;
    return (int)(groups < (size_t)kRegMaxPartials ? groups : (size_t)kRegMaxPartials);
}

hipError_t launch_reg_curve(const float2* op_h, const float* power, const float* extras, const double* lap, const double* cand, int ncand, int M,
                            int N, size_t pstride, int npanels, double* part, double* out, hipStream_t s) {
    if (!op_h || !power || !extras || !lap || !cand || !part || !out || ncand < 1 || ncand > kRegCandidates) return hipErrorInvalidValue;
    const int nb = reg_curve_partials(M, npanels);
    hipLaunchKernelGGL((reg_curve_kernel<kRegCandidates>), dim3((unsigned)nb), dim3(kRegThreads), 0, s, op_h, power, extras, lap, cand, M, N,
                       pstride, npanels, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(reg_curve_fold_kernel, dim3(1), dim3(kRegThreads), 0, s, (const double*)part, nb, 2 * kRegCandidates, 2 * ncand, out);
    return hipGetLastError();
}

}  // namespace fdr
