// fdr_mixed.hip -- fast mode for plan sizes 2^a 3^b 5^c (FDR_FLAG_MIXED_RADIX): the sizes fft_serial::wienerDeblur_myfft
// pads to (getOptimalDFTSize, fft/fft_serial.cpp:153-154) instead of the next power of two.
//
// Transform core: Stockham autosort FFT with radices 4, 2, 3 and 5 on rows held in LDS, the factor schedule chosen on the
// host per length (MixLen::st).  Each stage reads every butterfly's inputs into registers, waits at a barrier, and writes
// its outputs in place, so one LDS buffer per transform is enough.  Twiddles exp(-2 pi i m / L) = lo[m mod 64] hi[m / 64]
// from a two-level table copied to LDS (entries double-generated and rounded once); the inverse is conj(FFT(conj(x))).
// Global loads are issued kMixU at a time per thread before their LDS writes (one load in flight per thread left the
// passes latency bound).
//
// Intermediate: the full complex spectrum, panel-major like the power-of-two fast path -- element (m, n) at
// (n / P) * pstride + m * P + n % P -- so that the column pass reads and writes one contiguous panel of P columns.
//   A  rows: two real rows per complex transform (x_a + i x_b), split into their spectra on store
//   B  cols: per panel, forward transform, multiply by W = conj(H) / (|H|^2 + K), inverse transform
//   C  rows: two spectrum rows per transform (their inverses are real), real parts of the cropped rows to a raw plane,
//      one (min, max) partial per workgroup
//   E  normalise + crop (launch_normalize, shared with the power-of-two path)
#include "../../include/fdr.h"
#include "fdr_kernels.hpp"
#include "fdr_fft_core.hpp"

namespace fdr {
namespace {

constexpr int kMixU = 8;  // global loads a thread keeps in flight before their LDS writes

__device__ __forceinline__ float2 mx_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 mx_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 mx_conj(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float2 mx_mul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}

// forward R-point DFTs in registers
template <int R> __device__ __forceinline__ void mx_dft(float2* v);
template <> __device__ __forceinline__ void mx_dft<2>(float2* v) {
    const float2 a = v[0], b = v[1];
    v[0] = mx_add(a, b);
    v[1] = mx_sub(a, b);
}
template <> __device__ __forceinline__ void mx_dft<3>(float2* v) {
    const float c = -0.5f, d = 0.866025403784438647f;  // w = exp(-2 pi i / 3) = c - i d
    const float2 s = mx_add(v[1], v[2]), t = mx_sub(v[1], v[2]);
    const float2 m = make_float2(fmaf(c, s.x, v[0].x), fmaf(c, s.y, v[0].y));
    v[0] = mx_add(v[0], s);
    v[1] = make_float2(fmaf(d, t.y, m.x), fmaf(-d, t.x, m.y));  // m - i d t
    v[2] = make_float2(fmaf(-d, t.y, m.x), fmaf(d, t.x, m.y));  // m + i d t
}
template <> __device__ __forceinline__ void mx_dft<4>(float2* v) {
    const float2 t0 = mx_add(v[0], v[2]), t1 = mx_sub(v[0], v[2]), t2 = mx_add(v[1], v[3]), d = mx_sub(v[1], v[3]);
    const float2 t3 = make_float2(d.y, -d.x);  // -i (a1 - a3)
    v[0] = mx_add(t0, t2);
    v[2] = mx_sub(t0, t2);
    v[1] = mx_add(t1, t3);
    v[3] = mx_sub(t1, t3);
}
template <> __device__ __forceinline__ void mx_dft<5>(float2* v) {
    const float c1 = 0.309016994374947424f, c2 = -0.809016994374947424f;  // cos(2 pi / 5), cos(4 pi / 5)
    const float s1 = 0.951056516295153572f, s2 = 0.587785252292473129f;   // sin(2 pi / 5), sin(4 pi / 5)
    const float2 a0 = v[0];
    const float2 b1 = mx_add(v[1], v[4]), b2 = mx_add(v[2], v[3]), d1 = mx_sub(v[1], v[4]), d2 = mx_sub(v[2], v[3]);
    const float2 t1 = make_float2(fmaf(c2, b2.x, fmaf(c1, b1.x, a0.x)), fmaf(c2, b2.y, fmaf(c1, b1.y, a0.y)));
    const float2 t2 = make_float2(fmaf(c1, b2.x, fmaf(c2, b1.x, a0.x)), fmaf(c1, b2.y, fmaf(c2, b1.y, a0.y)));
    const float2 u1 = make_float2(fmaf(s2, d2.x, s1 * d1.x), fmaf(s2, d2.y, s1 * d1.y));
    const float2 u2 = make_float2(fmaf(-s1, d2.x, s2 * d1.x), fmaf(-s1, d2.y, s2 * d1.y));
    v[0] = mx_add(a0, mx_add(b1, b2));
    v[1] = make_float2(t1.x + u1.y, t1.y - u1.x);  // t1 - i u1
    v[4] = make_float2(t1.x - u1.y, t1.y + u1.x);  // t1 + i u1
    v[2] = make_float2(t2.x + u2.y, t2.y - u2.x);  // t2 - i u2
    v[3] = make_float2(t2.x - u2.y, t2.y + u2.x);  // t2 + i u2
}

// One Stockham stage of radix R over a transform of length L at s[0..L): butterfly j (of L / R) reads s[j + r L / R],
// applies exp(-2 pi i r k / (ns R)) (k = j mod ns, ns = product of the earlier radices), and writes s[(j / ns) ns R + k + r ns].
// Thread lt of nt handles butterflies lt, lt + nt, ...: at most ceil(kMixMaxElems / R) of them (the host sizes nt).
template <int R>
__device__ __forceinline__ void mx_stage(float2* s, int L, int ns, unsigned magic, int twstep, const float2* __restrict__ tw, int lt,
                                         int nt) {
    constexpr int NIT = (kMixMaxElems + R - 1) / R;
    const int nb = L / R;
    float2 v[NIT][R];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int j = lt + it * nt;
        if (j < nb) {
#pragma unroll
            for (int r = 0; r < R; ++r) v[it][r] = s[j + r * nb];
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int j = lt + it * nt;
        if (j < nb) {
            const int q = magic ? (int)__umulhi((unsigned)j, magic) : j;  // j / ns (magic = 0: ns = 1)
            const int k = j - q * ns;
            const int tk = k * twstep;
#pragma unroll
            for (int r = 1; r < R; ++r) {
                const int m = r * tk;  // exp(-2 pi i m / L) = lo[m mod 64] * hi[m / 64]
                v[it][r] = mx_mul(v[it][r], mx_mul(tw[m & (kMixTwLo - 1)], tw[kMixTwLo + (m >> 6)]));
            }
            mx_dft<R>(v[it]);
            const int base = q * ns * R + k;
#pragma unroll
            for (int r = 0; r < R; ++r) s[base + r * ns] = v[it][r];
        }
    }
    __syncthreads();
}

// the two-level twiddle table of a length (kMixTwLo + L / 64 entries) into LDS; the caller's next barrier publishes it
__device__ __forceinline__ void mx_load_twiddles(float2* tw_lds, const MixLen& ml) {
    const int n = kMixTwLo + (ml.L + kMixTwLo - 1) / kMixTwLo;
    for (int i = threadIdx.x; i < n; i += blockDim.x) tw_lds[i] = ml.tw[i];
}

// forward transform of s[0..L) in place with the LDS twiddles tw; every thread of the workgroup calls it (same schedule:
// same barriers)
__device__ __forceinline__ void mx_fft(float2* s, const MixLen& ml, const float2* tw, int lt) {
    for (int i = 0; i < ml.nst; ++i) {
        const int4 sd = ml.st[i];  // uniform: scalar loads
        switch (sd.x) {
            case 4: mx_stage<4>(s, ml.L, sd.y, (unsigned)sd.z, sd.w, tw, lt, ml.nt); break;
            case 2: mx_stage<2>(s, ml.L, sd.y, (unsigned)sd.z, sd.w, tw, lt, ml.nt); break;
            case 3: mx_stage<3>(s, ml.L, sd.y, (unsigned)sd.z, sd.w, tw, lt, ml.nt); break;
            default: mx_stage<5>(s, ml.L, sd.y, (unsigned)sd.z, sd.w, tw, lt, ml.nt); break;
        }
    }
}

}  // namespace

// ---- row passes: a.B transforms of length N per workgroup, nt threads each --------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(1024) void mixed_rows_kernel(const MixRowArgs a) {
    extern __shared__ float2 mx_lds[];
    __shared__ float2 red[16];
    __shared__ float2 tw_lds[kMixTwLo + kMixMaxLen / kMixTwLo];
    mx_load_twiddles(tw_lds, a.len);
    const int N = a.len.L, nt = a.len.nt, P = 1 << a.logP;
    const int b = threadIdx.x / nt, lt = threadIdx.x - b * nt;
    float2* s = mx_lds + (size_t)b * N;
    const int npan = N >> a.logP;
    const int T = blockDim.x;

    if (KIND == MIX_ROWS_FWD_REAL) {
        // rows r0 + 2b (real part) and r0 + 2b + 1 (imaginary part), zero outside the source image
        const int ra = blockIdx.x * 2 * a.B + 2 * b, rb = ra + 1;
        const float* pa = a.src_real + (size_t)ra * a.src_stride;
        const float* pb = pa + a.src_stride;
        const bool va = ra < a.src_rows, vb = rb < a.src_rows;
        for (int n0 = lt; n0 < N; n0 += kMixU * nt) {
            float x[kMixU], y[kMixU];
#pragma unroll
            for (int u = 0; u < kMixU; ++u) {
                const int n = n0 + u * nt;
                const bool in = n < a.src_cols;
                x[u] = va && in ? pa[n] : 0.f;
                y[u] = vb && in ? pb[n] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kMixU; ++u)
                if (n0 + u * nt < N) s[n0 + u * nt] = make_float2(x[u], y[u]);
        }
    } else if (KIND == MIX_ROWS_C2C) {
        const int r = blockIdx.x * a.B + b;
        const float2* p = a.src_c + (size_t)r * N;
        for (int n0 = lt; n0 < N; n0 += kMixU * nt) {
            float2 z[kMixU];
#pragma unroll
            for (int u = 0; u < kMixU; ++u) z[u] = r < a.M && n0 + u * nt < N ? p[n0 + u * nt] : make_float2(0.f, 0.f);
#pragma unroll
            for (int u = 0; u < kMixU; ++u)
                if (n0 + u * nt < N) s[n0 + u * nt] = a.inverse ? mx_conj(z[u]) : z[u];
        }
    } else {  // MIX_ROWS_INV_REAL: spectrum rows m_a, m_b (panel-major) -> conj(h_a + i h_b)
        const int r0 = blockIdx.x * 2 * a.B;
        const int chunk = a.B << a.logP;  // (row pair, column) entries per panel
        const int tot = npan * chunk;
        for (int e0 = threadIdx.x; e0 < tot; e0 += kMixU * T) {
            float2 ha[kMixU], hb[kMixU];
#pragma unroll
            for (int u = 0; u < kMixU; ++u) {
                const int e = e0 + u * T;
                const int pn = e / chunk, w = e - pn * chunk;
                const int ma = r0 + 2 * (w >> a.logP), mb = ma + 1;
                const float2* src = a.src_c + (size_t)pn * a.pstride + (size_t)ma * P + (w & (P - 1));
                ha[u] = e < tot && ma < a.rows_in ? src[0] : make_float2(0.f, 0.f);
                hb[u] = e < tot && mb < a.rows_in ? src[P] : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < kMixU; ++u) {
                const int e = e0 + u * T;
                if (e >= tot) break;
                const int pn = e / chunk, w = e - pn * chunk;
                mx_lds[(size_t)(w >> a.logP) * N + pn * P + (w & (P - 1))] = make_float2(ha[u].x - hb[u].y, -(ha[u].y + hb[u].x));
            }
        }
    }
    __syncthreads();
    mx_fft(s, a.len, tw_lds, lt);

    if (KIND == MIX_ROWS_FWD_REAL || KIND == MIX_ROWS_C2C) {
        const int rpb = KIND == MIX_ROWS_FWD_REAL ? 2 * a.B : a.B;  // rows per workgroup
        const int r0 = blockIdx.x * rpb;
        const int chunk = rpb << a.logP;  // contiguous elements per panel
        for (int e = threadIdx.x; e < npan * chunk; e += T) {
            const int pn = e / chunk, w = e - pn * chunk;
            const int ml = w >> a.logP, c = w & (P - 1);
            const int m = r0 + ml;
            if (m >= a.M) continue;
            const int n = pn * P + c;
            float2 X;
            if (KIND == MIX_ROWS_FWD_REAL) {
                // Z = FFT(x_a + i x_b): X_a = (Z[n] + conj Z[-n]) / 2, X_b = (Z[n] - conj Z[-n]) / 2i
                const float2* sb = mx_lds + (size_t)(ml >> 1) * N;
                const float2 z = sb[n], zc = mx_conj(sb[n ? N - n : 0]);
                if ((ml & 1) == 0) X = make_float2(0.5f * (z.x + zc.x), 0.5f * (z.y + zc.y));
                else X = make_float2(0.5f * (z.y - zc.y), -0.5f * (z.x - zc.x));
            } else {
                const float2 z = mx_lds[(size_t)ml * N + n];
                X = a.inverse ? mx_conj(z) : z;
            }
            a.dst_c[(size_t)pn * a.pstride + (size_t)m * P + c] = X;
        }
        return;
    }

    // MIX_ROWS_INV_REAL: IFFT(h_a + i h_b) = conj(s) = f_a + i f_b, both real rows
    const int ma = blockIdx.x * 2 * a.B + 2 * b, mb = ma + 1;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int n = lt; n < N; n += nt) {
        const float2 z = s[n];
        const float fa = z.x * a.scale, fb = -z.y * a.scale;
        if (n < a.mm_cols) {
            if (ma < a.mm_rows) { mn = fminf(mn, fa); mx = fmaxf(mx, fa); }
            if (mb < a.mm_rows) { mn = fminf(mn, fb); mx = fmaxf(mx, fb); }
        }
        if (n < a.out_cols) {
            if (ma < a.out_rows) a.dst_real[(size_t)ma * a.dst_stride + n] = fa;
            if (mb < a.out_rows) a.dst_real[(size_t)mb * a.dst_stride + n] = fb;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float2(mn, mx);
    __syncthreads();
    if (threadIdx.x == 0) {
        float2 r = red[0];
        for (int k = 1; k < (T >> 6); ++k) { r.x = fminf(r.x, red[k].x); r.y = fmaxf(r.y, red[k].y); }
        a.mm_part[blockIdx.x] = r;
    }
}

// ---- column pass: one panel (P columns of length M) per workgroup, nt threads per column -------------------------------------
template <int KIND>
__global__ __launch_bounds__(1024) void mixed_cols_kernel(const MixColArgs a) {
    extern __shared__ float2 mx_lds[];
    __shared__ float2 tw_lds[kMixTwLo + kMixMaxLen / kMixTwLo];
    mx_load_twiddles(tw_lds, a.len);
    const int M = a.len.L, nt = a.len.nt, P = 1 << a.logP;
    const int c0 = threadIdx.x / nt, lt = threadIdx.x - c0 * nt;
    float2* s = mx_lds + (size_t)c0 * M;
    const int T = blockDim.x, tot = M << a.logP;
    const size_t base = (size_t)blockIdx.x * a.pstride;
    const float2* src = a.src + base;
    const bool conj_in = KIND == MIX_COLS_C2C && a.inverse;
    const int nin = a.rows_in << a.logP;  // rows >= rows_in are zero (and not read)
    for (int e0 = threadIdx.x; e0 < tot; e0 += kMixU * T) {
        float2 z[kMixU];
#pragma unroll
        for (int u = 0; u < kMixU; ++u) z[u] = e0 + u * T < nin ? src[e0 + u * T] : make_float2(0.f, 0.f);
#pragma unroll
        for (int u = 0; u < kMixU; ++u) {
            const int e = e0 + u * T;
            if (e < tot) mx_lds[(size_t)(e & (P - 1)) * M + (e >> a.logP)] = conj_in ? mx_conj(z[u]) : z[u];
        }
    }
    __syncthreads();
    mx_fft(s, a.len, tw_lds, lt);

    if (KIND == MIX_COLS_FILTER) {  // H -> W, in place over the whole panel
        for (int e = threadIdx.x; e < tot; e += T) {
            const int m = e >> a.logP, c = e & (P - 1);
            a.dst[base + e] = wiener_filter_fast(mx_lds[(size_t)c * M + m], a.K);
        }
        return;
    }
    if (KIND == MIX_COLS_FILTER_CLS) {  // the same with the CLS quotient: row m in natural order, column = the panel's first + c
        const int n0 = blockIdx.x << a.logP;
        for (int e = threadIdx.x; e < tot; e += T) {
            const int m = e >> a.logP, c = e & (P - 1);
            a.dst[base + e] = cls_filter_fast(mx_lds[(size_t)c * M + m], a.K, cls_reg(a.lap, M, m, n0 + c, a.gamma));
        }
        return;
    }
    if (KIND == MIX_COLS_C2C) {  // panel -> row-major M x N
        const int n0 = blockIdx.x << a.logP;
        for (int e = threadIdx.x; e < tot; e += T) {
            const int m = e >> a.logP, c = e & (P - 1);
            const float2 z = mx_lds[(size_t)c * M + m];
            a.dst[(size_t)m * a.N + n0 + c] = a.inverse ? mx_conj(z) : z;
        }
        return;
    }
    // MIX_COLS_FUSED: Y = X W, then IFFT(Y) = conj(FFT(conj(Y)))
    const float2* W = a.filt + base;
    for (int e0 = threadIdx.x; e0 < tot; e0 += kMixU * T) {
        float2 w[kMixU];
#pragma unroll
        for (int u = 0; u < kMixU; ++u) w[u] = e0 + u * T < tot ? W[e0 + u * T] : make_float2(0.f, 0.f);
#pragma unroll
        for (int u = 0; u < kMixU; ++u) {
            const int e = e0 + u * T;
            if (e < tot) {
                float2* p = mx_lds + (size_t)(e & (P - 1)) * M + (e >> a.logP);
                *p = mx_conj(mx_mul(*p, w[u]));
            }
        }
    }
    __syncthreads();
    mx_fft(s, a.len, tw_lds, lt);
    const int nout = a.rows_out << a.logP;
    for (int e = threadIdx.x; e < nout; e += T) {
        const int m = e >> a.logP, c = e & (P - 1);
        a.dst[base + e] = mx_conj(mx_lds[(size_t)c * M + m]);
    }
}

namespace {
template <class A>
hipError_t set_lds(void (*kernel)(const A), size_t smem) {
    // the attribute belongs to the current device's copy of the code object: set on every launch (host-side table write)
    if (smem <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
}

}  // namespace

hipError_t launch_mixed_rows(MixRowKind kind, const MixRowArgs& a, int blocks, hipStream_t s) {
    if (blocks <= 0) return hipSuccess;
    const int threads = a.B * a.len.nt;
    const size_t smem = (size_t)a.B * a.len.L * sizeof(float2);
    if (threads > 1024 || smem > kMixMaxLds) return hipErrorInvalidValue;
    void (*k)(const MixRowArgs) = kind == MIX_ROWS_FWD_REAL ? mixed_rows_kernel<MIX_ROWS_FWD_REAL>
                                : kind == MIX_ROWS_C2C      ? mixed_rows_kernel<MIX_ROWS_C2C>
                                                            : mixed_rows_kernel<MIX_ROWS_INV_REAL>;
    hipError_t e = set_lds(k, smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), smem, s, a);
    return hipGetLastError();
}

hipError_t launch_mixed_cols(MixColKind kind, const MixColArgs& a, int npanels, hipStream_t s) {
    const int threads = a.len.nt << a.logP;
    const size_t smem = ((size_t)a.len.L << a.logP) * sizeof(float2);
    if (threads > 1024 || smem > kMixMaxLds) return hipErrorInvalidValue;
    if (kind == MIX_COLS_FILTER_CLS && a.lap == nullptr) return hipErrorInvalidValue;
    void (*k)(const MixColArgs) = kind == MIX_COLS_FILTER     ? mixed_cols_kernel<MIX_COLS_FILTER>
                                : kind == MIX_COLS_FILTER_CLS ? mixed_cols_kernel<MIX_COLS_FILTER_CLS>
                                : kind == MIX_COLS_C2C        ? mixed_cols_kernel<MIX_COLS_C2C>
                                                              : mixed_cols_kernel<MIX_COLS_FUSED>;
    hipError_t e = set_lds(k, smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(npanels), dim3(threads), smem, s, a);
    return hipGetLastError();
}

}  // namespace fdr
