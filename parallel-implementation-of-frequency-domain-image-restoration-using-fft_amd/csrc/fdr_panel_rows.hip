// fdr_panel_rows.hip -- the row passes of the fast panel path (layout: fdr_panel.hpp).  Pass A: 4 real rows, padded on load -> row
// FFTs -> panel layout (the packed, persistent and split forward kernels, the smooth padding).  The inverse row passes: 4 rows
// gathered from the panels -> row IFFTs -> one of the RowOut kinds (passes C' / C1 / C2, the operator kinds).  One unit: the forward
// and the inverse kernels of a length share their FftCore, and compiled apart fft_rows4_inv_packed_kernel<13, false, .> comes out
// with other registers (tools/kernel_diff.py).
#include "fdr_panel.hpp"

namespace fdr {

// ---------------------------------------------------------------------------------------------
// rows, 4 at a time
// ---------------------------------------------------------------------------------------------
// Two-for-one row transforms (fast mode only; rounding differs from the serial path at the 1e-7
// level, far inside the 1e-4 budget).  The image rows are real, and after the inverse column pass
// every row spectrum is Hermitian, so two rows share one complex transform:
//   forward : z = x_a + i x_b  ->  Z = FFT(z);  X_a[n] = (Z[n] + conj Z[N-n]) / 2,
//                                               X_b[n] = (Z[n] - conj Z[N-n]) / (2i)
//             (Z[N-n] lives in another thread: one natural-order LDS round trip)
//   inverse : Z = Y_a + i Y_b  ->  z = IFFT(Z);  row a = Re z, row b = Im z   (no fix-up at all)
// A 4-row group therefore costs 2 complex transforms instead of 4.
//
// Cores whose first step is radix 2 (8192 = 2 x 16 x 16 x 16) and that span at least one wave do the first exchange with
// v_permlane32_swap instead of LDS (FftCore's SWAP0).
// ---------------------------------------------------------------------------------------------
// One-group row kernels (a workgroup lives for one 4-row group).
template <int LOGL, bool INV = false>
struct Rows4PackGeom {
    // values per thread (log2): 16 (radix-16 steps) from 4096 points on, for the inverse kernels from 2048 points on;
    // 8 below (LAB_NOTES "row kernel width")
    static constexpr int LOGV = LOGL >= (INV ? 11 : 12) ? 4 : 3;
    using St = Steps<LOGL, LOGV>;
    static constexpr int T = St::T;
    static constexpr int G = T >= 256 ? 1 : 256 / T;
    static constexpr int THREADS = T * G;
    // inverse kernels with 16 values per thread own ONE exchange buffer per thread group: the two packed pairs hand their
    // mirrored halves over one after the other (rows4_pack_mirror), so that more workgroups fit a CU; as many workgroups
    // per CU as the LDS admits, registers capped to match
    static constexpr bool ONE_BUF = INV && LOGV == 4;
    static constexpr int INV_LDS = G * St::BUF * 8;
    static constexpr int INV_WG_PER_CU = ONE_BUF ? ((160 * 1024) / INV_LDS > 4 ? 4 : (160 * 1024) / INV_LDS) : 1;
    static constexpr int INV_WAVES_PER_SIMD = INV_WG_PER_CU * THREADS / 256 > 0 ? (INV_WG_PER_CU * THREADS / 256 > 8 ? 8 : INV_WG_PER_CU * THREADS / 256) : 1;
};

// ---------------------------------------------------------------------------------------------
// Row passes for ONE small image (single-image calls, rows of 256 .. 2048 points, at most 2048 rows; BASELINE config 2).
// A lone 1024^2 image is 256 four-row groups: the packed kernels give each group to ONE thread group that runs its two
// packed transforms one after the other (128 workgroups of two groups at 1024 points), and with nothing else in flight the
// launch lasts as long as that dependent chain.  Here the two packed pairs of a group go to two thread groups of one
// workgroup (B = 1 transform each, twice the waves on half the chain, one workgroup per group: 256 of them at 1024^2); the
// step plan, policy and pack / separate formulas are those of the packed kernels, so the bits are the same.
// ---------------------------------------------------------------------------------------------
// (INV: the inverse kernel follows the batched inverse kernels' step plan (Rows4PackGeom<LOGL, true>::LOGV), so that ONE
// image restored alone and the same image inside a batch come out with identical bits.)
template <int LOGL, bool INV = false>
struct RowsSplitGeom {
    static constexpr int LOGV = Rows4PackGeom<LOGL, INV>::LOGV;
    using St = Steps<LOGL, LOGV>;
    static constexpr int T = St::T;
    static constexpr int THREADS = 2 * T;
    static constexpr bool SWAP = St::lr(0) == 1 && T >= 64;
};
static inline bool rows4_use_split(int logl, int M, int nimg, int half) {
    return nimg <= 1 && half && logl >= 8 && logl <= 11 && (M & 3) == 0 && M > 0 && M <= 2048;
}

// ---------------------------------------------------------------------------------------------
// What an inverse row pass does with its values, by RowOut kind (the inverse kernels and their epilogues are
// templated on the kind and ask these; a new kind is an enumerator, its answers here and its rows4_rl_value).
// ---------------------------------------------------------------------------------------------
constexpr bool row_out_stores_raw(RowOut o) { return o == ROW_OUT_REAL_MINMAX; }                              // the raw real plane
constexpr bool row_out_minmax(RowOut o) { return o == ROW_OUT_REAL_MINMAX || o == ROW_OUT_MINMAX_ONLY; }      // min/max partials
constexpr bool row_out_normalizes(RowOut o) { return o == ROW_OUT_NORMALIZED; }  // folds the partials, scales and shifts on store
constexpr bool row_out_operator(RowOut o) { return o >= ROW_OUT_BLUR; }          // half spectrum, >= 32 points, cropped
constexpr bool row_out_operator_group(RowOut o) { return row_out_operator(o) && o != ROW_OUT_RL_RATIO_STAT; }  // ... takes a group of images
constexpr bool row_out_reads_src(RowOut o) { return row_out_operator(o) && o != ROW_OUT_BLUR; }               // src_real
constexpr bool row_out_reads_src2(RowOut o) { return o == ROW_OUT_RL_UPDATE_W; }                              // src_real2 as well
constexpr bool row_out_fit_sums(RowOut o) { return o == ROW_OUT_RL_RATIO_STAT; }  // src_real2 when not null, (res, kl) partials

// ---------------------------------------------------------------------------------------------
// pass A
// ---------------------------------------------------------------------------------------------
// Reads every register of a prefetched set through an empty asm: the compiler places the wait for those loads HERE (with
// the exact vmcnt for this point of the program) and treats them as landed afterwards.  Used at the bottom of the
// persistent loop, right behind the stores of the group just finished: the prefetch is older than those stores, so the
// wait is vmcnt(#stores) and the stores keep draining; left to the first use (copies at the loop top, where the state
// of the first iteration merges in) the compiler emits vmcnt(0..1) and the stores drain before the next transform.
template <int R, int C>
__device__ __forceinline__ void landed_f(const float (&d)[R][C]) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < C; c += 4) asm volatile("" ::"v"(d[r][c]), "v"(d[r][c + 1]), "v"(d[r][c + 2]), "v"(d[r][c + 3]));
}

// ---------------------------------------------------------------------------------------------
// Smooth padding (RowArgs::pad_mode, FDR_PAD_SMOOTH of fdr.h): outside the rows x cols window the
// padded plane e continues the picture periodically instead of dropping to zero.  With ramp(n)[j] = 0.5 - 0.5 cos(pi (j + 1) / (n + 1)):
//     r < rows, c >= cols :  t = ramp(N - cols)[c - cols];  e[r, c] = (1 - t) d[r, cols-1] + t d[r, 0]
//     r >= rows           :  s = ramp(M - rows)[r - rows];  e[r, c] = (1 - s) e[rows-1, c] + s e[0, c]
// so an element needs at most four source values (three of them shared along a row or a column: PadRows).  Only the edge branches of the pass A kernels evaluate it (template parameter
// PAD); their interior branches and every PAD = 0 instantiation are the zero-padding code.  The weights come from cospif in the
// kernel: no table, nothing to upload, nothing that a stream capture would have to know about.
// ---------------------------------------------------------------------------------------------
constexpr int kPadZero = 0, kPadSmooth = 1;  // FDR_PAD_ZERO, FDR_PAD_SMOOTH
__device__ __forceinline__ float pad_ramp(int j, int n) { return 0.5f - 0.5f * cospif((float)(j + 1) / (float)(n + 1)); }
// What NR consecutive rows r0 .. r0+NR-1 of the extended plane share (uniform over the thread group, so these are scalar loads): column 0
// of each row (of row rows-1 below the picture), d[0, 0], the row weights, and whether any of the rows lies below the picture.
template <int NR>
struct PadRows {
    float c0[NR], rs[NR], d00;
    bool below[NR], any_below;
};
template <int NR>
__device__ __forceinline__ void pad_rows_init(PadRows<NR>& g, const float* __restrict__ src, int stride, int rows, int r0, int M) {
    g.d00 = src[0];
    g.any_below = r0 + NR - 1 >= rows;
#pragma unroll
    for (int b = 0; b < NR; ++b) {
        const int r = r0 + b;
        g.below[b] = r >= rows;
        g.c0[b] = src[(size_t)(r < rows ? r : rows - 1) * stride];
        g.rs[b] = r >= rows ? pad_ramp(r - rows, M - rows) : 0.f;
    }
}
// Column n of those rows: v[b] = d[min(r0 + b, rows-1), min(n, cols-1)] on entry (the element itself inside the picture, else the
// first of its source values), e[r0 + b, n] on return; ncp = N - cols.  One more load (d[0, .]) only below the picture, one cospif only
// to the right of it; every address lies inside the picture.
template <int NR>
__device__ __forceinline__ void pad_smooth_rows(float (&v)[NR], const PadRows<NR>& g, const float* __restrict__ src, int cols, int n, int ncp) {
    const bool right = n >= cols;
    float t = 0.f;
    if (right) {
        t = pad_ramp(n - cols, ncp);
#pragma unroll
        for (int b = 0; b < NR; ++b) v[b] = (1.f - t) * v[b] + t * g.c0[b];
    }
    if (g.any_below) {
        float w = src[right ? cols - 1 : n];
        if (right) w = (1.f - t) * w + t * g.d00;
#pragma unroll
        for (int b = 0; b < NR; ++b) v[b] = g.below[b] ? (1.f - g.rs[b]) * v[b] + g.rs[b] * w : v[b];
    }
}

// HALF: keep only the non-redundant half of each Hermitian row spectrum -- columns 0 .. N/2-1 in panels
// 0 .. N/8-1.  X[m,0] and X[m,N/2] are real for a real row, so the Nyquist column rides in the imaginary
// part of column 0: stored(m, 0) = X[m,0] + i X[m,N/2]  ("packed column", undone in passes B' and C').
// PAD: what the edge branch puts outside the picture (kPadZero / kPadSmooth, see pad_smooth_rows).
template <int LOGL, bool HALF, int PAD = kPadZero>
__global__ __launch_bounds__(Rows4PackGeom<LOGL>::THREADS) void fft_rows4_fwd_packed_kernel(const RowArgs a0,
                                                                                          const float2* __restrict__ tw_fwd) {
    RowArgs a = a0;
    if (a0.batch.nimg > 1) {  // blockIdx.y = image
        a.src_real = pick_image(a0.batch.src_real, blockIdx.y);
        a.dst_c = pick_image(a0.batch.spec, blockIdx.y);
    }
    using Geo = Rows4PackGeom<LOGL>;
    using St = typename Geo::St;
    constexpr int G = Geo::G, T = St::T, L = St::L;
    using Core = FftCore<LOGL, 2, 2, PolicyFast, Geo::LOGV, (St::lr(0) == 1 && T >= 64)>;
    __shared__ float2 lds[G * 2 * St::BUF];
    const int g = threadIdx.x >> St::LOGT, tid = Core::thread_index(threadIdx.x & (T - 1));
    float2* grp_lds = lds + g * 2 * St::BUF;
    const int M = a.M;
    const int r0 = (blockIdx.x * G + g) * 4;
    const bool active = r0 < M;
    const int rr = active ? r0 : 0;

    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);

    float2 z[2][Core::V];
    // common case first: all four rows and all L columns inside the image -> 32 unpredicated loads
    // from four wave-uniform row bases with one 32-bit per-thread offset
    const bool interior = (rr + 3 < a.src_rows) && (a.src_cols >= L);
    if (interior) {
        const float* row0 = a.src_real + (size_t)rr * a.src_stride;
        const float* row1 = row0 + a.src_stride;
        const float* row2 = row1 + a.src_stride;
        const float* row3 = row2 + a.src_stride;
#pragma unroll
        for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHO0; ++q) {
                const int s = u * Core::RHO0 + q;
                const unsigned n = (unsigned)Core::in_index(tid, u, q);
                // the image is read exactly once: keep it out of the caches that hold the intermediates
                z[0][s] = make_float2(__builtin_nontemporal_load(row0 + n), __builtin_nontemporal_load(row1 + n));
                z[1][s] = make_float2(__builtin_nontemporal_load(row2 + n), __builtin_nontemporal_load(row3 + n));
            }
    } else if constexpr (PAD == kPadSmooth) {
        PadRows<4> pr;
        pad_rows_init(pr, a.src_real, a.src_stride, a.src_rows, rr, M);
        const float* rowp[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) rowp[b] = a.src_real + (size_t)(rr + b < a.src_rows ? rr + b : a.src_rows - 1) * a.src_stride;
#pragma unroll
        for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHO0; ++q) {
                const int s = u * Core::RHO0 + q;
                const int n = Core::in_index(tid, u, q);
                const int nc = n < a.src_cols ? n : a.src_cols - 1;
                float x[4] = {rowp[0][nc], rowp[1][nc], rowp[2][nc], rowp[3][nc]};
                pad_smooth_rows(x, pr, a.src_real, a.src_cols, n, L - a.src_cols);
                z[0][s] = make_float2(x[0], x[1]);
                z[1][s] = make_float2(x[2], x[3]);
            }
    } else {
#pragma unroll
        for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHO0; ++q) {
                const int s = u * Core::RHO0 + q;
                const int n = Core::in_index(tid, u, q);
                float x[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    x[b] = 0.f;
                    if (rr + b < a.src_rows && n < a.src_cols) x[b] = a.src_real[(size_t)(rr + b) * a.src_stride + n];
                }
                z[0][s] = make_float2(x[0], x[1]);
                z[1][s] = make_float2(x[2], x[3]);
            }
    }

    Core::template run<0, false>(z, grp_lds, tw_fwd, bases, tid);

    // Separate the two real rows of each packed transform and store all four spectra panel-major.
    constexpr int SEQ1 = Core::SLOTS;
    if constexpr (T >= 4) {
        // Both packed spectra go to LDS in natural order; then the threads re-partition the work so
        // that a quad of lanes owns one 128-byte line (4 rows x 4 columns of a panel): lane j of the
        // quad builds row j's four columns (32 contiguous bytes).  Every store instruction of a wave
        // then covers 16 complete lines instead of 64 scattered 8-byte pieces.
        // The buffer of pair b = 1 is the one the transform's LAST exchange read from: a barrier has to separate those
        // reads from this write (pair b = 0 goes to the other buffer, which the last barrier of the transform already
        // protects).  Without it a wave that runs ahead overwrites values a slower wave is still picking up -- rows 2, 3
        // of the group came out wrong for a few lanes' columns whenever a second stream's kernels shared the CUs.
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float2* buf = grp_lds + ((SEQ1 + b) & 1) * St::BUF;
#ifndef FDR_DEBUG_OMIT_SEPARATION_BARRIER  // (the race fuzzer's own check: with the barrier left out it must find the race)
            if (b == 1) __syncthreads();
#endif
            FDR_JITTER(2001 + b);
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) buf[Core::out_index(tid, u, q)] = z[b][u * Core::RHOL + q];
        }
        __syncthreads();
        FDR_JITTER(2003);
        const int j = tid & 3;                                    // row inside the 4-row group
        const float2* buf = grp_lds + ((SEQ1 + (j >> 1)) & 1) * St::BUF;  // packed pair holding row j
        const bool odd = (j & 1) != 0;                            // row b of the pair (else row a)
#pragma unroll
        for (int i = 0; i < (HALF ? L / 8 : L / 4) / (T / 4); ++i) {
            const int c = (tid >> 2) + (T / 4) * i;  // panel
            const int n0 = c * 4;
            float2 o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float2 zn = buf[n0 + k];
                const float2 zm = buf[(L - n0 - k) & (L - 1)];
                o[k] = odd ? make_float2(0.5f * (zn.y + zm.y), 0.5f * (zm.x - zn.x))
                           : make_float2(0.5f * (zn.x + zm.x), 0.5f * (zn.y - zm.y));
            }
            if (HALF && n0 == 0) {  // packed column: (X[0], X[N/2]), both real: Re/Im of Z[0] and Z[N/2]
                const float2 z0 = buf[0], zq = buf[L / 2];
                o[0] = odd ? make_float2(z0.y, zq.y) : make_float2(z0.x, zq.x);
            }
            if (active) store4(a.dst_c + (size_t)c * a.pstride + (size_t)(r0 + j) * 4, o[0], o[1], o[2], o[3]);
        }
        } else {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float2* buf = grp_lds + ((SEQ1 + b) & 1) * St::BUF;
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) buf[Core::out_index(tid, u, q)] = z[b][u * Core::RHOL + q];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) {
                    const int s = u * Core::RHOL + q;
                    const int n = Core::out_index(tid, u, q);
                    const float2 zn = z[b][s];
                    const float2 zm = buf[(L - n) & (L - 1)];
                    const float2 xa = make_float2(0.5f * (zn.x + zm.x), 0.5f * (zn.y - zm.y));
                    const float2 xb = make_float2(0.5f * (zn.y + zm.y), 0.5f * (zm.x - zn.x));
                    if (active) {
                        float2* p = a.dst_c + (size_t)(n >> 2) * a.pstride + (size_t)(r0 + 2 * b) * 4 + (n & 3);
                        p[0] = xa;
                        p[4] = xb;
                    }
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Persistent form of pass A (8192-point rows: one thread group = one workgroup).  A launch of the kernel above runs in
// lockstep -- every workgroup loads, then every workgroup transforms, then every workgroup stores -- so HBM idles while
// the CUs compute and the CUs idle while HBM streams.  Here a workgroup walks over its row groups and requests the NEXT
// group's four image rows (4 V floats per thread) before it transforms the current one; the stores of the current group
// drain behind the next group's transform.  The prefetch is unconditional (clamped addresses, collapsed onto one element
// when there is no next group; zero padding is applied when the values are packed): a conditional load would make the
// compiler wait for it right away.
// 16 values per thread, T = L/16 threads: 8192-point rows as ONE 512-thread workgroup per CU with a 256-register budget
// (the 8-value form needs 1024 threads at 128 registers and cannot hold a prefetch).  Shorter rows gain nothing from
// the persistent form (LAB_NOTES "persistent row passes").
// ---------------------------------------------------------------------------------------------
constexpr int kRowsFwdPersMinLog = 13;  // shortest rows (log2) whose forward pass is persistent
constexpr int kRowsFwdPersLogV = 4;     // values per thread (log2) of the persistent forward kernel
template <int LOGL, int LOGV>
struct RowsPersGeom {
    using St = Steps<LOGL, LOGV>;
    static constexpr int T = St::T;
    static_assert(T >= 256, "one thread group per workgroup");
    static_assert(LOGV == 4, "16 values per thread");
    static constexpr int THREADS = T;
    static constexpr int LDS_BYTES = 2 * St::BUF * 8;
    static constexpr int BY_LDS = (160 * 1024) / LDS_BYTES;
    static constexpr int BY_REGS = 2 * 256 / THREADS;  // 256 registers per lane
    static constexpr int WG_PER_CU = BY_LDS < BY_REGS ? (BY_LDS < 1 ? 1 : BY_LDS) : (BY_REGS < 1 ? 1 : BY_REGS);
    static constexpr int WAVES_PER_SIMD = WG_PER_CU * THREADS / 256;
};

template <int LOGL, int LOGV, bool HALF, bool INTERIOR, int PAD = kPadZero>
__global__ __launch_bounds__((RowsPersGeom<LOGL, LOGV>::THREADS), (RowsPersGeom<LOGL, LOGV>::WAVES_PER_SIMD)) void fft_rows4_fwd_pers_kernel(
    const RowArgs a, const float2* __restrict__ tw_fwd, const int ngroups, const int total) {
    using St = Steps<LOGL, LOGV>;
    constexpr int T = St::T, L = St::L, V = St::V;
    using Core = FftCore<LOGL, 2, 2, PolicyFast, LOGV, (St::lr(0) == 1)>;  // 8192 points: wave-local first exchange
    __shared__ float2 lds[2 * St::BUF];
    const int tid = Core::thread_index(threadIdx.x);
    const int nimg = a.batch.nimg > 1 ? a.batch.nimg : 1;

    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);

    // group gi = (image, 4-row group); advanced by scalar add / subtract (no division on the vector unit)
    int gi = blockIdx.x;
    if (gi >= total) return;
    int img = 0, grp = gi;
    while (grp >= ngroups) { grp -= ngroups; ++img; }
    auto src_of = [&](int im) -> const float* { return nimg > 1 ? pick_image(a.batch.src_real, im) : a.src_real; };
    auto dst_of = [&](int im) -> float2* { return nimg > 1 ? pick_image(a.batch.spec, im) : a.dst_c; };

    // four image rows of group `g` of image `im`: unconditional loads from clamped coordinates; scale = 0 collapses
    // every address onto element 0 of the image (a prefetch with nothing to fetch: conditional loads would make the
    // compiler wait for them on the spot)
    float x[4][V];
    auto request = [&](const float* __restrict__ src, int g, unsigned scale) __attribute__((always_inline)) {
        const int r0 = g * 4;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            int r = r0 + b;
            if (!INTERIOR) r = r < a.src_rows ? r : a.src_rows - 1;
            const float* __restrict__ row = src + (size_t)r * (size_t)a.src_stride * scale;
#pragma unroll
            for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHO0; ++q) {
                    const int s = u * Core::RHO0 + q;
                    unsigned n = (unsigned)Core::in_index(tid, u, q);
                    if (!INTERIOR) n = n < (unsigned)a.src_cols ? n : (unsigned)a.src_cols - 1u;
                    x[b][s] = __builtin_nontemporal_load(row + n * scale);  // the image is read exactly once
                }
        }
    };
    // z[0] = rows 0 + i 1, z[1] = rows 2 + i 3 of group g of the image at `src` (the padding is applied here).  Smooth padding: the
    // prefetched value of an element outside the picture is the clamped one, d[min(r, rows-1), min(n, cols-1)] -- the first of the (at
    // most four) source values; the others are fetched here, by the padded elements only (pad_smooth_rows).
    float2 z[2][V];
    auto pack = [&](const float* __restrict__ src, int g) __attribute__((always_inline)) {
        const int r0 = g * 4;
        PadRows<4> pr;
        // (opaque copy of the thread index: the column weights and offsets below depend on the column alone, and hoisted out of the
        // group loop they would stay in ~40 registers across the transform, beside the prefetched rows -- more than the budget holds)
        int tp = tid;
        if constexpr (!INTERIOR && PAD == kPadSmooth) {
            asm volatile("" : "+v"(tp));
            pad_rows_init(pr, src, a.src_stride, a.src_rows, r0, a.M);
        }
#pragma unroll
        for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHO0; ++q) {
                const int s = u * Core::RHO0 + q;
                float v0 = x[0][s], v1 = x[1][s], v2 = x[2][s], v3 = x[3][s];
                if constexpr (!INTERIOR && PAD == kPadSmooth) {
                    float v[4] = {v0, v1, v2, v3};
                    pad_smooth_rows(v, pr, src, a.src_cols, Core::in_index(tp, u, q), L - a.src_cols);
                    v0 = v[0]; v1 = v[1]; v2 = v[2]; v3 = v[3];
                } else if (!INTERIOR) {
                    const bool cok = Core::in_index(tid, u, q) < a.src_cols;
                    v0 = (cok && r0 + 0 < a.src_rows) ? v0 : 0.f;
                    v1 = (cok && r0 + 1 < a.src_rows) ? v1 : 0.f;
                    v2 = (cok && r0 + 2 < a.src_rows) ? v2 : 0.f;
                    v3 = (cok && r0 + 3 < a.src_rows) ? v3 : 0.f;
                }
                z[0][s] = make_float2(v0, v1);
                z[1][s] = make_float2(v2, v3);
            }
    };
    // transform the packed pair in z, separate the two real rows of each transform and store all four spectra
    // panel-major: both packed spectra go to LDS in natural order, then a quad of lanes owns one 128-byte line (4 rows x
    // 4 columns of a panel): lane j of the quad builds row j's four columns (see fft_rows4_fwd_packed_kernel)
    auto body = [&](int im, int g) __attribute__((always_inline)) {
        {
            int tr = tid;  // opaque copy: the exchange addresses are recomputed per group, not carried across the loop
            asm volatile("" : "+v"(tr));
            Core::template run<0, false>(z, lds, tw_fwd, bases, tr);
        }
        constexpr int SEQ1 = Core::SLOTS;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float2* buf = lds + ((SEQ1 + b) & 1) * St::BUF;
            if (b == 1) __syncthreads();  // pair 1's buffer was read by the transform's last exchange (see fft_rows4_fwd_packed_kernel)
            FDR_JITTER(2011 + b);
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) buf[Core::out_index(tid, u, q)] = z[b][u * Core::RHOL + q];
        }
        __syncthreads();
        FDR_JITTER(2013);
        float2* __restrict__ dst = dst_of(im);
        const int r0 = g * 4;
        // (opaque copy of the thread index: the LDS and panel addresses below are loop invariant, and hoisted out of
        // the group loop they would occupy ~25 registers for the whole kernel -- recomputing them costs a few adds)
        int tq = tid;
        asm volatile("" : "+v"(tq));
        const int j = tq & 3;                                            // row inside the 4-row group
        const float2* buf = lds + ((SEQ1 + (j >> 1)) & 1) * St::BUF;     // packed pair holding row j
        const bool odd = (j & 1) != 0;                                   // row b of the pair (else row a)
        constexpr int NIT = (HALF ? L / 8 : L / 4) / (T / 4);            // panels per lane
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int c = (tq >> 2) + (T / 4) * i;  // panel
            const int n0 = c * 4;
            float2 o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float2 zn = buf[n0 + k];
                const float2 zm = buf[(L - n0 - k) & (L - 1)];
                o[k] = odd ? make_float2(0.5f * (zn.y + zm.y), 0.5f * (zm.x - zn.x))
                           : make_float2(0.5f * (zn.x + zm.x), 0.5f * (zn.y - zm.y));
            }
            if (HALF && n0 == 0) {  // packed column: (X[0], X[N/2]), both real: Re/Im of Z[0] and Z[N/2]
                const float2 z0 = buf[0], zq = buf[L / 2];
                o[0] = odd ? make_float2(z0.y, zq.y) : make_float2(z0.x, zq.x);
            }
            store4(dst + (size_t)c * a.pstride + (size_t)(r0 + j) * 4, o[0], o[1], o[2], o[3]);
        }
    };

    // Loop shape: the wait for a prefetch sits at the BOTTOM of the loop (pack), behind the stores of the group just
    // finished.  vmcnt counts loads and stores in issue order and the prefetch is older than those stores, so the wait
    // there is vmcnt(#stores) and the stores keep draining behind the next transform; with the wait at the loop top the
    // compiler has to merge it with the first iteration's state (no stores yet) and emits vmcnt(0).
    request(src_of(img), grp, 1u);
    landed_f(x);  // (also here: the loop top must see landed values on both of its entries, or it waits again)
    pack(src_of(img), grp);
    while (true) {
        const bool more = gi + (int)gridDim.x < total;
        int nimg_i = img, ngrp = grp;
        if (more) {
            ngrp += (int)gridDim.x;
            while (ngrp >= ngroups) { ngrp -= ngroups; ++nimg_i; }
        }
        request(src_of(nimg_i), more ? ngrp : 0, more ? 1u : 0u);
        body(img, grp);
        if (!more) break;
        landed_f(x);      // wait for the prefetch here, behind this group's stores
        __syncthreads();  // the separation's reads are done before the next transform's first exchange writes
        pack(src_of(nimg_i), ngrp);
        gi += (int)gridDim.x; img = nimg_i; grp = ngrp;
    }
}

// Pass A for ONE small image: the two packed pairs of a 4-row group on two thread groups (RowsSplitGeom).
template <int LOGL, int PAD = kPadZero>
__global__ __launch_bounds__(RowsSplitGeom<LOGL>::THREADS) void fft_rows4_fwd_split_kernel(const RowArgs a, const float2* __restrict__ tw_fwd) {
    using Geo = RowsSplitGeom<LOGL>;
    using St = typename Geo::St;
    constexpr int T = St::T, L = St::L;
    using Core = FftCore<LOGL, 1, 2, PolicyFast, 3, Geo::SWAP>;
    __shared__ float2 lds[2 * 2 * St::BUF];
    const int p = (int)(threadIdx.x >> St::LOGT);  // packed pair of the group: rows 2p, 2p + 1
    const int tid = Core::thread_index((int)(threadIdx.x & (T - 1)));
    float2* grp_lds = lds + p * 2 * St::BUF;
    const int r0 = (int)blockIdx.x * 4;
    const int ra = r0 + 2 * p, rb = ra + 1;

    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);

    float2 z[1][8];
    if constexpr (PAD == kPadSmooth) {
        PadRows<2> pr;
        pad_rows_init(pr, a.src_real, a.src_stride, a.src_rows, ra, a.M);
        const float* __restrict__ rowa = a.src_real + (size_t)(ra < a.src_rows ? ra : a.src_rows - 1) * a.src_stride;
        const float* __restrict__ rowb = a.src_real + (size_t)(rb < a.src_rows ? rb : a.src_rows - 1) * a.src_stride;
#pragma unroll
        for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHO0; ++q) {
                const int n = Core::in_index(tid, u, q);
                const int nc = n < a.src_cols ? n : a.src_cols - 1;
                float x[2] = {rowa[nc], rowb[nc]};
                pad_smooth_rows(x, pr, a.src_real, a.src_cols, n, L - a.src_cols);
                z[0][u * Core::RHO0 + q] = make_float2(x[0], x[1]);
            }
    } else {
        const float* __restrict__ rowa = a.src_real + (size_t)(ra < a.src_rows ? ra : 0) * a.src_stride;
        const float* __restrict__ rowb = a.src_real + (size_t)(rb < a.src_rows ? rb : 0) * a.src_stride;
#pragma unroll
        for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHO0; ++q) {
                const int n = Core::in_index(tid, u, q);
                float xa = 0.f, xb = 0.f;
                if (n < a.src_cols) {
                    if (ra < a.src_rows) xa = __builtin_nontemporal_load(rowa + n);
                    if (rb < a.src_rows) xb = __builtin_nontemporal_load(rowb + n);
                }
                z[0][u * Core::RHO0 + q] = make_float2(xa, xb);
            }
    }

    Core::template run<0, false>(z, grp_lds, tw_fwd, bases, tid);

    // the pair's packed spectrum in natural order into the buffer the last exchange did NOT use (free: its last readers
    // passed that exchange's barrier), then the whole workgroup separates: a quad of lanes owns one 128-byte line
    constexpr int SEQ1 = Core::SLOTS;
    float2* mine = grp_lds + (SEQ1 & 1) * St::BUF;
    FDR_JITTER(2031);
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) mine[Core::out_index(tid, u, q)] = z[0][u * Core::RHOL + q];
    __syncthreads();
    FDR_JITTER(2032);
    const int w = (int)threadIdx.x;
    const int j = w & 3;                                                        // row inside the 4-row group
    const float2* buf = lds + (j >> 1) * 2 * St::BUF + (SEQ1 & 1) * St::BUF;    // packed pair holding row j
    const bool odd = (j & 1) != 0;                                              // row b of the pair (else row a)
    constexpr int NIT = (L / 8) / (2 * T / 4);                                  // panels per lane (half spectrum)
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int c = (w >> 2) + (2 * T / 4) * i;  // panel
        const int n0 = c * 4;
        float2 o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float2 zn = buf[n0 + k];
            const float2 zm = buf[(L - n0 - k) & (L - 1)];
            o[k] = odd ? make_float2(0.5f * (zn.y + zm.y), 0.5f * (zm.x - zn.x))
                       : make_float2(0.5f * (zn.x + zm.x), 0.5f * (zn.y - zm.y));
        }
        if (n0 == 0) {  // packed column: (X[0], X[N/2]), both real: Re/Im of Z[0] and Z[N/2]
            const float2 z0 = buf[0], zq = buf[L / 2];
            o[0] = odd ? make_float2(z0.y, zq.y) : make_float2(z0.x, zq.x);
        }
        store4(a.dst_c + (size_t)c * a.pstride + (size_t)(r0 + j) * 4, o[0], o[1], o[2], o[3]);
    }
}

template <int LOGL>
static hipError_t launch_rows4_fwd_t(const RowArgs& a, const float2* tw, hipStream_t s) {
    using Geo = Rows4PackGeom<LOGL>;
    const int groups = (a.M + 3) / 4;
    const int nimg = a.batch.nimg > 1 ? a.batch.nimg : 1;
    const dim3 grid((groups + Geo::G - 1) / Geo::G, nimg), block(Geo::THREADS);
    // smooth padding: pass A of a picture smaller than the plan, all M rows (a full window has nothing to fill and runs the
    // zero-padding kernels: same bits by construction)
    const bool smooth = a.pad_mode == kPadSmooth && (a.src_rows < a.M || a.src_cols < (1 << LOGL));
    if (smooth && (a.src_rows <= 0 || a.src_cols <= 0 || a.src_rows > a.M || a.src_cols > (1 << LOGL))) return hipErrorInvalidValue;
    if constexpr (LOGL >= 8 && LOGL <= 11) {
        if (rows4_use_split(LOGL, a.M, nimg, a.half)) {  // one small image: two thread groups per 4-row group (RowsSplitGeom)
            const dim3 sgrid(a.M / 4), sblock(RowsSplitGeom<LOGL>::THREADS);
            if (a.src_rows <= 0 || a.src_cols <= 0) return hipErrorInvalidValue;
            if (smooth) hipLaunchKernelGGL((fft_rows4_fwd_split_kernel<LOGL, kPadSmooth>), sgrid, sblock, 0, s, a, tw);
            else hipLaunchKernelGGL((fft_rows4_fwd_split_kernel<LOGL>), sgrid, sblock, 0, s, a, tw);
            return hipGetLastError();
        }
    }
    if constexpr (LOGL >= kRowsFwdPersMinLog) {  // persistent, prefetching form (see fft_rows4_fwd_pers_kernel)
        constexpr int LOGV = kRowsFwdPersLogV;
        using PG = RowsPersGeom<LOGL, LOGV>;
        const int total = groups * nimg;
        int g = (a.num_cu > 0 ? a.num_cu : 256) * PG::WG_PER_CU;
        if ((a.M & 3) == 0 && a.src_rows > 0 && a.src_cols > 0) {
            if (g > total) g = total;
            const bool interior = a.src_rows >= a.M && a.src_cols >= (1 << LOGL);
            const dim3 pgrid(g), pblock(PG::THREADS);
            if (smooth) {  // (never interior)
                if (a.half) hipLaunchKernelGGL((fft_rows4_fwd_pers_kernel<LOGL, LOGV, true, false, kPadSmooth>), pgrid, pblock, 0, s, a, tw, groups, total);
                else hipLaunchKernelGGL((fft_rows4_fwd_pers_kernel<LOGL, LOGV, false, false, kPadSmooth>), pgrid, pblock, 0, s, a, tw, groups, total);
            } else if (a.half) {
                if (interior) hipLaunchKernelGGL((fft_rows4_fwd_pers_kernel<LOGL, LOGV, true, true>), pgrid, pblock, 0, s, a, tw, groups, total);
                else hipLaunchKernelGGL((fft_rows4_fwd_pers_kernel<LOGL, LOGV, true, false>), pgrid, pblock, 0, s, a, tw, groups, total);
            } else {
                if (interior) hipLaunchKernelGGL((fft_rows4_fwd_pers_kernel<LOGL, LOGV, false, true>), pgrid, pblock, 0, s, a, tw, groups, total);
                else hipLaunchKernelGGL((fft_rows4_fwd_pers_kernel<LOGL, LOGV, false, false>), pgrid, pblock, 0, s, a, tw, groups, total);
            }
            return hipGetLastError();
        }
    }
    if (smooth) {
        if (a.half) hipLaunchKernelGGL((fft_rows4_fwd_packed_kernel<LOGL, true, kPadSmooth>), grid, block, 0, s, a, tw);
        else hipLaunchKernelGGL((fft_rows4_fwd_packed_kernel<LOGL, false, kPadSmooth>), grid, block, 0, s, a, tw);
    } else if (a.half) hipLaunchKernelGGL((fft_rows4_fwd_packed_kernel<LOGL, true>), grid, block, 0, s, a, tw);
    else hipLaunchKernelGGL((fft_rows4_fwd_packed_kernel<LOGL, false>), grid, block, 0, s, a, tw);
    return hipGetLastError();
}

static hipError_t launch_rows4_fwd(int logl, const RowArgs& a, const float2* tw_fwd, hipStream_t s) {
    FDR_DISPATCH_LOG(logl, launch_rows4_fwd_t<LG>(a, tw_fwd, s));
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// the inverse row passes
// ---------------------------------------------------------------------------------------------
// Four Hermitian row spectra (rows rr .. rr+3) rebuilt from the panel-major (half) spectrum and packed two rows per
// complex transform, in two steps so that the loads of the NEXT row group can be issued (into y) before the values
// are touched:  rows4_load_raw -> y[row][slot] (first-step operand order, stored column of slot s),
//               rows4_pack     -> z[0] = Y_a + i Y_b (rows rr, rr+1), z[1] = rows rr+2, rr+3.
//
// Instruction count matters here (a VALU instruction costs 4 cycles per wave, and these kernels run 2 waves per SIMD):
// which half of the spectrum a slot lies in is a compile-time property of its q (n = tid + u T + q 2^LOGR0, and
// q >= RHO0/2  <=>  n >= L/2), so the mirrored slots (n > L/2: stored column L-n, conjugated) need no per-lane
// selects; only lane tid = 0 differs (n = 0: DC, n = L/2: Nyquist -- both live in the packed column 0) and is
// patched separately.  Addresses: one uniform base per slot + two per-lane 32-bit offsets (direct / mirrored).
template <int LOGL, bool HALF, class Core>
__device__ __forceinline__ void rows4_load_raw(const RowArgs& a, int rr, int tid, float2 (&y)[4][Core::V]) {
    constexpr int L = Steps<LOGL>::L;
    if constexpr (!HALF || LOGL < 5) {  // (half-spectrum plans need N >= 32; smaller instantiations are never launched)
#pragma unroll
        for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHO0; ++q) {
                const int s = u * Core::RHO0 + q;
                const int n = Core::in_index(tid, u, q);
                const float2* p = a.src_c + ((size_t)(n >> 2) * a.pstride + (size_t)rr * 4 + (n & 3));
                y[0][s] = p[0]; y[1][s] = p[4]; y[2][s] = p[8]; y[3][s] = p[12];
            }
    } else {
        static_assert(Core::RHO0 >= 2 && Core::LOGR0 >= 2, "n = t + q Q with Q a multiple of 4");
        const unsigned ps = (unsigned)a.pstride;
        constexpr unsigned PMID = (unsigned)(L / 8);  // panel of column L/2 (one past the stored panels)
        unsigned off_d[Core::NU0], off_m[Core::NU0];
#pragma unroll
        for (int u = 0; u < Core::NU0; ++u) {
            const unsigned t = (unsigned)(tid + u * Core::T);        // n = t + q Q,  Q = 2^LOGR0 (a multiple of 4)
            const unsigned ta = t >> 2, tb = t & 3u;
            // direct half: stored column t + qQ -> panel qQ/4 + ta, column tb
            off_d[u] = ta * ps + tb + (unsigned)rr * 4u;
            // mirrored half: stored column (RHO0 - q) Q - t -> panel (RHO0-q)Q/4 - ta - (tb != 0), column (4 - tb) & 3,
            // relative to q = RHO0/2 (panel L/8)
            const unsigned pm = PMID - ta - (tb != 0u ? 1u : 0u);     // panel of the mirrored column at q = RHO0/2
            off_m[u] = pm * ps + ((4u - tb) & 3u) + (unsigned)rr * 4u;
        }
        auto load_slot = [&](int u, int q) __attribute__((always_inline)) {
            const int s = u * Core::RHO0 + q;
#ifdef FDR_DEBUG_SKIP_MEM  // timing-only builds
            y[0][s] = y[1][s] = y[2][s] = y[3][s] = make_float2((float)(off_d[u] + q), (float)(off_m[u]));
#else
            const float2* p;
            if (q < Core::RHO0 / 2) {
                p = a.src_c + (size_t)((q << Core::LOGR0) >> 2) * ps + off_d[u];
            } else if (q == Core::RHO0 / 2) {
                // n = L/2 (lane t = 0 of the u = 0 slot): the Nyquist value rides in column 0 of panel 0
                const unsigned off_n = (u == 0 && tid == 0) ? (unsigned)rr * 4u : off_m[u];
                p = a.src_c + off_n;
            } else {  // (RHO0 - q) Q = L/2 - (q - RHO0/2) Q: uniform step back from the q = RHO0/2 panel
                p = a.src_c - (size_t)(((q - Core::RHO0 / 2) << Core::LOGR0) >> 2) * ps + off_m[u];
            }
            y[0][s] = p[0]; y[1][s] = p[4]; y[2][s] = p[8]; y[3][s] = p[12];
#endif
        };
        // Issue order: every stored line is read twice by the workgroup, once for a direct slot and once for the mirrored
        // slot that covers the same block of panels -- direct (u, q) and mirrored (NU0-1-u, RHO0-1-q).  Requested back to
        // back the second touch finds the line in (or on its way into) L1 / L2; in slot order the two are half a tile of
        // loads apart and the second one goes out to the fabric again (LAB_NOTES "pass C' reads").
#pragma unroll
        for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHO0 / 2; ++q) {
                load_slot(u, q);
                load_slot(Core::NU0 - 1 - u, Core::RHO0 - 1 - q);
#ifndef FDR_DEBUG_SKIP_MEM
                asm volatile("" ::: "memory");
#endif
            }
    }
}
template <int LOGL, bool HALF, class Core>
__device__ __forceinline__ void rows4_pack(int tid, const float2 (&y)[4][Core::V], float2 (&z)[2][Core::V]) {
#pragma unroll
    for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHO0; ++q) {
            const int s = u * Core::RHO0 + q;
            const float2 y0 = y[0][s], y1 = y[1][s], y2 = y[2][s], y3 = y[3][s];
            if (HALF && LOGL >= 5 && q >= Core::RHO0 / 2) {  // mirrored column: conjugate, then Y_a + i Y_b
                z[0][s] = make_float2(y0.x + y1.y, y1.x - y0.y);
                z[1][s] = make_float2(y2.x + y3.y, y3.x - y2.y);
            } else {
                z[0][s] = make_float2(y0.x - y1.y, y0.y + y1.x);  // Y_a + i Y_b
                z[1][s] = make_float2(y2.x - y3.y, y2.y + y3.x);
            }
        }
    if (HALF && LOGL >= 5 && tid == 0) {  // n = 0 (DC) and n = L/2 (Nyquist): real values packed as (DC, Nyquist) in column 0
        constexpr int SN = Core::RHO0 / 2;  // slot of n = L/2 (u = 0)
        z[0][0] = make_float2(y[0][0].x, y[1][0].x);
        z[1][0] = make_float2(y[2][0].x, y[3][0].x);
        z[0][SN] = make_float2(y[0][SN].y, y[1][SN].y);
        z[1][SN] = make_float2(y[2][SN].y, y[3][SN].y);
    }
}

// ---------------------------------------------------------------------------------------------
// The same rebuild WITHOUT the second touch of memory (half-spectrum plans, rows of 32 points and more).  The packed
// input of the inverse transform is Z[n] = Y_a[n] + i Y_b[n]; for the upper half, Z[N-n] = conj(Y_a[n]) + i conj(Y_b[n])
// -- a function of the SAME two stored values.  So a thread loads only its direct slots (stored columns n < N/2: half
// the gathers of rows4_load_raw, every stored line requested once), forms Z[n] for itself and Z[N-n] for whichever
// thread owns index N-n, and hands the latter over through LDS in natural order (the exchange buffers are idle at that
// point): 4 V / 8 writes + reads per thread and two barriers, against V/2 x 4 eight-byte gathers that went out to the
// fabric a second time (LAB_NOTES "pass C' reads").
//   y[row][j], j = u (RHO0/2) + q : stored column in_index(tid, u, q), q < RHO0/2
// ---------------------------------------------------------------------------------------------
// How the four rows reach the registers at 4096 and 8192 points.  The transform wants lane t to hold COLUMN t & 3 of the
// four rows of its panel; loaded that way every lane issues four 8-byte loads and a 128-byte line (4 rows x 4 columns of a
// panel) is requested in sixteen pieces.  Instead lane t loads ROW t & 3 -- four columns, two 16-byte loads, a quad of lanes
// requests the whole line -- and the quad transposes its 4 x 4 block in registers: two rounds of `v_cndmask_b32_dpp`
// (quad_perm [1,0,3,2], then [2,3,0,1]), 16 VALU instructions per panel and lane, no LDS.  Shorter rows keep the gathers
// (LAB_NOTES "row loads").

// r[c] = (row l, column c) on lane l of the quad  ->  q[r] = (row r, column l)
// d = (lane in MASK) ? keep : (value of `from` on the lane quad_perm points at), both halves of two float2: four
// v_cndmask_b32_dpp (select and cross-lane read in ONE instruction; hipcc emits v_mov_b32_dpp + v_cndmask_b32 for the
// same thing written in C, twice the VALU work).  s_nop 1: a DPP operand written by the preceding VALU instruction needs
// two wait states, and the hazard recogniser does not look into inline asm.
#define FDR_QUAD_SEL(MASK, PERM, d0, d1, from0, from1, keep0, keep1)                                                        \
    asm("s_nop 1\n\ts_mov_b32 vcc_lo, " MASK "\n\ts_mov_b32 vcc_hi, " MASK "\n\t"                                          \
        "v_cndmask_b32_dpp %0, %4, %8, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"                              \
        "v_cndmask_b32_dpp %1, %5, %9, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"                              \
        "v_cndmask_b32_dpp %2, %6, %10, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"                             \
        "v_cndmask_b32_dpp %3, %7, %11, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf"                                  \
        : "=&v"(d0.x), "=&v"(d0.y), "=&v"(d1.x), "=&v"(d1.y)                                                               \
        : "v"(from0.x), "v"(from0.y), "v"(from1.x), "v"(from1.y), "v"(keep0.x), "v"(keep0.y), "v"(keep1.x), "v"(keep1.y)   \
        : "vcc")
// (the masks are the physical lane's low bits, which the logical thread index keeps)
__device__ __forceinline__ void quad_transpose(const float2 (&r)[4], float2& q0, float2& q1, float2& q2, float2& q3) {
#if defined(__HIP_DEVICE_COMPILE__)
    float2 a00, a01, a10, a11;
    FDR_QUAD_SEL("0x55555555", "[1,0,3,2]", a00, a10, r[1], r[3], r[0], r[2]);  // even lanes keep columns 0 / 2, odd lanes take the
    FDR_QUAD_SEL("0xaaaaaaaa", "[1,0,3,2]", a01, a11, r[0], r[2], r[1], r[3]);  // neighbour's 1 / 3 (and the other way round)
    FDR_QUAD_SEL("0x33333333", "[2,3,0,1]", q0, q1, a10, a11, a00, a01);
    FDR_QUAD_SEL("0xcccccccc", "[2,3,0,1]", q2, q3, a00, a01, a10, a11);
#else
    (void)r; (void)q0; (void)q1; (void)q2; (void)q3;  // host pass of the translation unit: device code only
#endif
}

template <int LOGL, class Core>
__device__ __forceinline__ void rows4_load_direct(const RowArgs& a, int rr, int tid, float2 (&y)[4][Core::V / 2]) {
    static_assert(Core::RHO0 >= 2 && Core::LOGR0 >= 2, "n = t + q Q with Q a multiple of 4");
    constexpr int HQ = Core::RHO0 / 2;
    constexpr bool kRowLoads = LOGL >= 12;  // whole 32-byte rows of a panel + quad transpose (see above)
    const unsigned ps = (unsigned)a.pstride;
#pragma unroll
    for (int u = 0; u < Core::NU0; ++u) {
        const unsigned t = (unsigned)(tid + u * Core::T);  // stored column t + q Q -> panel q Q / 4 + t / 4, column t & 3
        // kRowLoads: row rr + (t & 3) of the panel, its 4 columns; else column t & 3 of rows rr .. rr + 3
        const unsigned off = kRowLoads ? (t >> 2) * ps + ((unsigned)rr + (t & 3u)) * 4u : (t >> 2) * ps + (t & 3u) + (unsigned)rr * 4u;
#pragma unroll
        for (int q = 0; q < HQ; ++q) {
            const int j = u * HQ + q;
#ifdef FDR_DEBUG_SKIP_MEM  // timing-only builds
            y[0][j] = y[1][j] = y[2][j] = y[3][j] = make_float2((float)(off + q), 1.0f);
#else
            const float2* p = a.src_c + (size_t)((q << Core::LOGR0) >> 2) * ps + off;
            if constexpr (kRowLoads) {
                const float4 lo = reinterpret_cast<const float4*>(p)[0], hi = reinterpret_cast<const float4*>(p)[1];
                y[0][j] = make_float2(lo.x, lo.y); y[1][j] = make_float2(lo.z, lo.w);
                y[2][j] = make_float2(hi.x, hi.y); y[3][j] = make_float2(hi.z, hi.w);
            } else {
                y[0][j] = p[0]; y[1][j] = p[4]; y[2][j] = p[8]; y[3][j] = p[12];
            }
#endif
        }
    }
#ifndef FDR_DEBUG_SKIP_MEM
    if constexpr (kRowLoads) {  // (every load of the group is requested before the first transpose)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < Core::NU0 * HQ; ++j) {
            // one panel after the other: left alone hipcc interleaves all the transposes and their temporaries push a
            // 128-register kernel over the edge (this asm makes panel j's inputs depend on panel j-1's results)
            if (j > 0)
                asm volatile("" : "+v"(y[0][j].x), "+v"(y[0][j].y), "+v"(y[1][j].x), "+v"(y[1][j].y), "+v"(y[2][j].x), "+v"(y[2][j].y),
                             "+v"(y[3][j].x), "+v"(y[3][j].y), "+v"(y[0][j - 1].x), "+v"(y[1][j - 1].y), "+v"(y[2][j - 1].x), "+v"(y[3][j - 1].y));
            const float2 r[4] = {y[0][j], y[1][j], y[2][j], y[3][j]};
            quad_transpose(r, y[0][j], y[1][j], y[2][j], y[3][j]);
        }
    }
#endif
}
// z[0] = Y_a + i Y_b of rows 0, 1, z[1] of rows 2, 3; grp_lds: the thread group's two exchange buffers.  Barriers inside
// (every thread of the workgroup must come here); returns with both buffers free again.
// ONE_BUF: the thread group owns a single exchange buffer (more workgroups per CU): the two packed pairs hand their mirrored
// halves over one after the other (two more barriers), same values.
template <int LOGL, class Core, bool ONE_BUF = false>
__device__ __forceinline__ void rows4_pack_mirror(int tid, const float2 (&y)[4][Core::V / 2], float2 (&z)[2][Core::V], float2* grp_lds) {
    using St = typename Core::St;
    constexpr int L = St::L, HQ = Core::RHO0 / 2;
    if constexpr (ONE_BUF) {
        float2* m = grp_lds;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            FDR_JITTER(3011 + p);
#pragma unroll
            for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
                for (int q = 0; q < HQ; ++q) {
                    const int j = u * HQ + q, s = u * Core::RHO0 + q;
                    const int n = Core::in_index(tid, u, q);
                    const float2 ya = y[2 * p][j], yb = y[2 * p + 1][j];
                    z[p][s] = make_float2(ya.x - yb.y, ya.y + yb.x);  // Y_a + i Y_b
                    const int k = (L - n) & (L - 1);
                    if (!(u == 0 && q == 0) || tid != 0) m[k] = make_float2(ya.x + yb.y, yb.x - ya.y);
                }
            __syncthreads();
            FDR_JITTER(3013 + p);
#pragma unroll
            for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
                for (int q = HQ; q < Core::RHO0; ++q) z[p][u * Core::RHO0 + q] = m[Core::in_index(tid, u, q)];
            if (tid == 0) {
                z[p][0] = make_float2(y[2 * p][0].x, y[2 * p + 1][0].x);
                z[p][HQ] = make_float2(y[2 * p][0].y, y[2 * p + 1][0].y);
            }
            __syncthreads();  // the next pair's hand-over (or the transform's first exchange) overwrites the buffer
        }
        return;
    }
    float2* m0 = grp_lds;
    float2* m1 = grp_lds + St::BUF;
    FDR_JITTER(3001);
#pragma unroll
    for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
        for (int q = 0; q < HQ; ++q) {
            const int j = u * HQ + q, s = u * Core::RHO0 + q;
            const int n = Core::in_index(tid, u, q);
            const float2 y0 = y[0][j], y1 = y[1][j], y2 = y[2][j], y3 = y[3][j];
            z[0][s] = make_float2(y0.x - y1.y, y0.y + y1.x);  // Y_a + i Y_b
            z[1][s] = make_float2(y2.x - y3.y, y2.y + y3.x);
            // conj(Y_a) + i conj(Y_b) belongs to index N - n (n = 0 has no mirror: it is the packed DC / Nyquist column)
            const int k = (L - n) & (L - 1);
            if (!(u == 0 && q == 0) || tid != 0) {
                m0[k] = make_float2(y0.x + y1.y, y1.x - y0.y);
                m1[k] = make_float2(y2.x + y3.y, y3.x - y2.y);
            }
        }
    __syncthreads();
    FDR_JITTER(3002);
#pragma unroll
    for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
        for (int q = HQ; q < Core::RHO0; ++q) {
            const int s = u * Core::RHO0 + q;
            const int k = Core::in_index(tid, u, q);
            z[0][s] = m0[k];
            z[1][s] = m1[k];
        }
    if (tid == 0) {  // n = 0 (DC) and n = L/2 (Nyquist): real values packed as (DC, Nyquist) in stored column 0
        constexpr int SN = HQ;  // slot of n = L/2 (u = 0, q = RHO0/2); its LDS cell was never written
        z[0][0] = make_float2(y[0][0].x, y[1][0].x);
        z[1][0] = make_float2(y[2][0].x, y[3][0].x);
        z[0][SN] = make_float2(y[0][0].y, y[1][0].y);
        z[1][SN] = make_float2(y[2][0].y, y[3][0].y);
    }
    __syncthreads();  // the transform's first exchange may overwrite either buffer
}

// Epilogue of the inverse row passes for one 4-row group (z = two packed transforms: rows r0, r0+1 and r0+2, r0+3).
//   ROW_OUT_REAL_MINMAX (pass C') : real plane + running min/max
//   ROW_OUT_MINMAX_ONLY (pass C1) : running min/max only -- nothing is stored
//   ROW_OUT_NORMALIZED  (pass C2) : value * fscale + fshift (two roundings, as normalize_kernel) to the cropped result, non-temporal
template <class Core, RowOut OUT, int V>
__device__ __forceinline__ void rows4_inv_epilogue(const RowArgs& a, const int r0, const int tq, const float2 (&z)[2][V], const float fscale,
                                                   const float fshift, float& mn, float& mx) {
    constexpr int T = Core::T, L = T * V;
    if constexpr (row_out_stores_raw(OUT)) {
        // four row bases + the lane's column: the stores need no per-element 64-bit address arithmetic
        float* o0 = a.dst_real + (size_t)r0 * L + tq;
        float* o1 = o0 + L;
        float* o2 = o1 + L;
        float* o3 = o2 + L;
#pragma unroll
        for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHOL; ++q) {
                const int s = u * Core::RHOL + q;
                const int c = u * T + (q << Core::LOGOUT);
                o0[c] = z[0][s].x; o1[c] = z[0][s].y; o2[c] = z[1][s].x; o3[c] = z[1][s].y;
            }
    }
    if constexpr (row_out_normalizes(OUT)) {
        float* o0 = a.out + (size_t)r0 * a.out_stride + tq;
        float* o1 = o0 + a.out_stride;
        float* o2 = o1 + a.out_stride;
        float* o3 = o2 + a.out_stride;
        if (r0 + 3 < a.out_rows && a.out_cols >= L) {  // nothing cropped in this group
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) {
                    const int s = u * Core::RHOL + q;
                    const int c = u * T + (q << Core::LOGOUT);
                    const float p0 = z[0][s].x * fscale, p1 = z[0][s].y * fscale, p2 = z[1][s].x * fscale, p3 = z[1][s].y * fscale;
                    __builtin_nontemporal_store(p0 + fshift, o0 + c);
                    __builtin_nontemporal_store(p1 + fshift, o1 + c);
                    __builtin_nontemporal_store(p2 + fshift, o2 + c);
                    __builtin_nontemporal_store(p3 + fshift, o3 + c);
                }
        } else {
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) {
                    const int s = u * Core::RHOL + q;
                    const int c = u * T + (q << Core::LOGOUT);
                    if (tq + c < a.out_cols) {
                        const float p0 = z[0][s].x * fscale, p1 = z[0][s].y * fscale, p2 = z[1][s].x * fscale, p3 = z[1][s].y * fscale;
                        if (r0 + 0 < a.out_rows) o0[c] = p0 + fshift;
                        if (r0 + 1 < a.out_rows) o1[c] = p1 + fshift;
                        if (r0 + 2 < a.out_rows) o2[c] = p2 + fshift;
                        if (r0 + 3 < a.out_rows) o3[c] = p3 + fshift;
                    }
                }
        }
    } else {
        if (r0 + 3 < a.mm_rows && a.mm_cols >= L) {  // whole group counted (always, with FDR_NORM_PADDED)
#pragma unroll
            for (int s = 0; s < V; ++s) {
                mn = fdr_min3(fdr_min3(mn, z[0][s].x, z[0][s].y), z[1][s].x, z[1][s].y);
                mx = fdr_max3(fdr_max3(mx, z[0][s].x, z[0][s].y), z[1][s].x, z[1][s].y);
            }
        } else {
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) {
                    const int s = u * Core::RHOL + q;
                    const int n = Core::out_index(tq, u, q);
                    const float r[4] = {z[0][s].x, z[0][s].y, z[1][s].x, z[1][s].y};
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (r0 + b < a.mm_rows && n < a.mm_cols) {
                            mn = fminf(mn, r[b]);
                            mx = fmaxf(mx, r[b]);
                        }
                }
        }
    }
}

// The operator kinds of the inverse row passes (the blur / Richardson-Lucy calls of fdr_rl.hip; a group of images per launch for all
// but ROW_OUT_RL_RATIO_STAT, each image with its own src_real and out and the bits it gets alone), the
// value v of the inverse transform at (r, n) of the window out_rows x out_cols, src = src_real + r src_stride + n:
//   ROW_OUT_BLUR        : v
//   ROW_OUT_RL_RATIO    : v > kRlTau ? max(d, 0) / v : 0, d = *src (the input image)
//   ROW_OUT_RL_UPDATE   : max(u v, 0), u = *src (the estimate; src may be the output itself: read and written by the same lane)
//   ROW_OUT_RL_UPDATE_W (free boundary) : max(u w v, 0), u = *src as ROW_OUT_RL_UPDATE, w = *src2 = src_real2 + r src_stride + n
template <RowOut OUT>
__device__ __forceinline__ float rows4_rl_value(const float v, const float* src, const float* src2 = nullptr) {
    if constexpr (OUT == ROW_OUT_BLUR) return v;
    else if constexpr (OUT == ROW_OUT_RL_RATIO) return v > kRlTau ? fmaxf(*src, 0.f) / v : 0.f;
    else if constexpr (OUT == ROW_OUT_RL_UPDATE) return fmaxf(*src * v, 0.f);
    else if constexpr (OUT == ROW_OUT_RL_UPDATE_W) return fmaxf(*src * *src2 * v, 0.f);
    else static_assert(OUT != OUT, "an operator kind without its value");
}
// ROW_OUT_RL_RATIO_STAT: the ratio of ROW_OUT_RL_RATIO on d = *src (src2 null) or, free boundary, on dw = w max(d, 0), w = *src2 (the
// float product of rlfree_setup_kernel, so the same bits as the ratio on the stored dw), and the pixel's terms of the two fit
// sums, added in double: res += w (d+ - c)^2, kl += w (c - d+ + (d+ > 0 && c > kRlTau ? d+ ln(d+ / c) : 0)).
// The logarithm without double transcendentals: q = d+ / c rounded to float leaves the residual d+ - q c exactly in one FMA, so
// ln(d+ / c) = ln(q) + ln(1 + delta), delta = (d+ - q c) / (q c) <= 2^-24, ln(1 + delta) = delta to 2^-48; logf (not the
// hardware's log2: it keeps its RELATIVE accuracy near q = 1, where the three terms cancel to d+ e^2 / 2, e = d+ / c - 1)
// gives ln(q) to an ulp, i.e. the term to about 1.2e-7 / |e| -- below what the float32 c itself leaves of it (2e-6 / |e|).
__device__ __forceinline__ float rows4_rl_ratio_stat(const float v, const float* src, const float* src2, double& res, double& kl) {
    const float dp = fmaxf(*src, 0.f);
    const bool ok = v > kRlTau;
    float num = dp, q = ok ? dp / v : 0.f, r = q;
    double w = 1.0;
    if (src2) {
        const float wf = *src2;
        num = wf * dp;
        r = ok ? num / v : 0.f;
        w = (double)wf;
    }
    const double c = (double)v, d = (double)dp, e = d - c;
    double t = c - d;
    if (dp > 0.f && ok) t += d * ((double)logf(q) + (double)__fdividef(fmaf(-q, v, dp), dp));
    res += w * (e * e);
    kl += w * t;
    return r;
}
// The workgroup's two sums (every wave is whole): an xor tree within each wave -- both partners form the same sum, so every lane
// ends with the same bits -- then thread 0 adds the waves in index order and writes the pair to part[index].
__device__ __forceinline__ void block_sum2_store(double s0, double s1, double2* __restrict__ part, int index) {
    __shared__ double2 sum_red[16];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off);
        s1 += __shfl_xor(s1, off);
    }
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) sum_red[wave] = make_double2(s0, s1);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) {
            s0 += sum_red[w].x;
            s1 += sum_red[w].y;
        }
        part[index] = make_double2(s0, s1);
    }
}
// rows4_inv_epilogue for those kinds: cropped on store as ROW_OUT_NORMALIZED, no min/max; res and kl: the thread's fit sums
// (ROW_OUT_RL_RATIO_STAT only), rows in order and the columns of a row in order
template <class Core, RowOut OUT, int V>
__device__ __forceinline__ void rows4_rl_epilogue(const RowArgs& a, const int r0, const int tq, const float2 (&z)[2][V], double& res,
                                                  double& kl) {
    constexpr int T = Core::T;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int r = r0 + b;
        if (r < a.out_rows) {
            float* o = a.out + (size_t)r * a.out_stride + tq;
            const float* in = row_out_reads_src(OUT) ? a.src_real + (size_t)r * a.src_stride + tq : nullptr;
            const float* in2 = (row_out_reads_src2(OUT) || (row_out_fit_sums(OUT) && a.src_real2)) ? a.src_real2 + (size_t)r * a.src_stride + tq : nullptr;
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) {
                    const int s = u * Core::RHOL + q;
                    const int c = u * T + (q << Core::LOGOUT);
                    const float v = b == 0 ? z[0][s].x : b == 1 ? z[0][s].y : b == 2 ? z[1][s].x : z[1][s].y;
                    if (tq + c < a.out_cols) {
                        if constexpr (row_out_fit_sums(OUT)) o[c] = rows4_rl_ratio_stat(v, in + c, in2 ? in2 + c : nullptr, res, kl);
                        else if constexpr (row_out_reads_src2(OUT)) o[c] = rows4_rl_value<OUT>(v, in + c, in2 + c);
                        else o[c] = rows4_rl_value<OUT>(v, in + c);
                    }
                }
        }
    }
}

// HALF: the row spectra hold columns 0 .. N/2-1 only, column 0 packed as Y[m,0] + i Y[m,N/2] (see the forward
// kernel); the upper half is rebuilt as the conjugate of the mirrored column (rows4_pack_mirror).
template <int LOGL, bool HALF, RowOut OUT>
__global__ __launch_bounds__((Rows4PackGeom<LOGL, true>::THREADS), (HALF ? Rows4PackGeom<LOGL, true>::INV_WAVES_PER_SIMD : 1)) void fft_rows4_inv_packed_kernel(const RowArgs a0,
                                                                                          const float2* __restrict__ tw_fwd) {
    RowArgs a = a0;
    if (a0.batch.nimg > 1) {  // blockIdx.y = image
        a.src_c = pick_image(a0.batch.spec, blockIdx.y);
        if constexpr (row_out_stores_raw(OUT)) a.dst_real = pick_image(a0.batch.raw, blockIdx.y);
        if constexpr (row_out_normalizes(OUT)) a.out = pick_image(a0.batch.out, blockIdx.y);
        a.mm_part = pick_image(a0.batch.mm_part, blockIdx.y);
        if constexpr (row_out_operator_group(OUT)) {  // its own real source (d, dw or u) and destination; src_real2 is the group's
            a.out = pick_image(a0.batch.out, blockIdx.y);  // (wgt: src2_pitch = 0) or the image's own (its factor plane)
            if constexpr (row_out_reads_src(OUT)) a.src_real = pick_image(a0.batch.src_real, blockIdx.y);
            if constexpr (row_out_reads_src2(OUT)) a.src_real2 = a0.src_real2 + (size_t)blockIdx.y * (size_t)a0.src2_pitch;
        }
    }
    float fscale = 0.f, fshift = 0.f;
    using Geo = Rows4PackGeom<LOGL, true>;
    using St = typename Geo::St;
    constexpr int G = Geo::G, T = St::T;
    constexpr int NBUF = (HALF && Geo::ONE_BUF) ? 1 : 2;  // 1: one exchange buffer per thread group (more workgroups per CU)
    using Core = FftCore<LOGL, 2, NBUF, PolicyFast, Geo::LOGV, (St::lr(0) == 1 && T >= 64)>;
    __shared__ float2 lds[G * NBUF * St::BUF];
    const int g = threadIdx.x >> St::LOGT, tid = Core::thread_index(threadIdx.x & (T - 1));
    const int M = a.M;
    const int r0 = (blockIdx.x * G + g) * 4;
    const bool active = r0 < M;
    const int rr = active ? r0 : 0;

    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);

    float2 z[2][Core::V];
    if constexpr (HALF && LOGL >= 5) {  // direct half from memory, mirrored half through LDS
        float2 y[4][Core::V / 2];
        rows4_load_direct<LOGL, Core>(a, rr, tid, y);
        // pass C2: the partials are folded BEHIND the group's own loads (a workgroup lives for one group here: a fold in
        // front of them adds its full memory latency to every workgroup)
        if constexpr (row_out_normalizes(OUT)) block_fold_partials(a.mm_part, a.n_part, fscale, fshift);
        rows4_pack_mirror<LOGL, Core, NBUF == 1>(tid, y, z, lds + g * NBUF * St::BUF);
    } else {
        float2 y[4][Core::V];
        rows4_load_raw<LOGL, HALF, Core>(a, rr, tid, y);
        if constexpr (row_out_normalizes(OUT)) block_fold_partials(a.mm_part, a.n_part, fscale, fshift);
        rows4_pack<LOGL, HALF, Core>(tid, y, z);
    }

    Core::template run<0, true>(z, lds + g * NBUF * St::BUF, tw_fwd, bases, tid);

    float mn = __builtin_inff(), mx = -__builtin_inff();
    double res = 0.0, kl = 0.0;  // row_out_fit_sums: an inactive thread group adds nothing
    if constexpr (row_out_operator(OUT)) {
        if (active) rows4_rl_epilogue<Core, OUT, Core::V>(a, r0, tid, z, res, kl);
    } else if (active) rows4_inv_epilogue<Core, OUT, Core::V>(a, r0, tid, z, fscale, fshift, mn, mx);
    if constexpr (row_out_minmax(OUT)) block_minmax_store(mn, mx, a.mm_part, (int)blockIdx.x);
    if constexpr (row_out_fit_sums(OUT)) {
        static_assert(Geo::THREADS % 64 == 0, "block_sum2_store: whole waves");
        block_sum2_store(res, kl, reinterpret_cast<double2*>(a.mm_part), (int)blockIdx.x);
    }
}

// The inverse row pass for ONE small image: the two packed pairs of a 4-row group on two thread groups (RowsSplitGeom).  OUT as in rows4_inv_epilogue and rows4_rl_value.
template <int LOGL, RowOut OUT>
__global__ __launch_bounds__((RowsSplitGeom<LOGL, true>::THREADS)) void fft_rows4_inv_split_kernel(const RowArgs a, const float2* __restrict__ tw_fwd) {
    using Geo = RowsSplitGeom<LOGL, true>;
    using St = typename Geo::St;
    constexpr int T = St::T, L = St::L, V = St::V;
    using Core = FftCore<LOGL, 1, 2, PolicyFast, Geo::LOGV, Geo::SWAP>;
    static_assert(Core::RHO0 >= 2 && Core::LOGR0 >= 2, "n = t + q Q with Q a multiple of 4");
    constexpr int HQ = Core::RHO0 / 2;
    __shared__ float2 lds[2 * 2 * St::BUF];
    const int p = (int)(threadIdx.x >> St::LOGT);
    const int tid = Core::thread_index((int)(threadIdx.x & (T - 1)));
    float2* grp_lds = lds + p * 2 * St::BUF;
    const int r0 = (int)blockIdx.x * 4;
    const int ra = r0 + 2 * p, rb = ra + 1;

    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);

    // direct half of the pair's two Hermitian row spectra (stored columns n < L/2), see rows4_load_direct
    float2 ya[V / 2], yb[V / 2];
    const unsigned ps = (unsigned)a.pstride;
#pragma unroll
    for (int u = 0; u < Core::NU0; ++u) {
        const unsigned t = (unsigned)(tid + u * Core::T);
        const unsigned off_d = (t >> 2) * ps + (t & 3u) + (unsigned)ra * 4u;
#pragma unroll
        for (int q = 0; q < HQ; ++q) {
            const float2* ptr = a.src_c + (size_t)((q << Core::LOGR0) >> 2) * ps + off_d;
            ya[u * HQ + q] = ptr[0];
            yb[u * HQ + q] = ptr[4];
        }
    }
    float fscale = 0.f, fshift = 0.f;
    if constexpr (row_out_normalizes(OUT)) block_fold_partials(a.mm_part, a.n_part, fscale, fshift);  // behind the group's own loads

    // Z[n] = Y_a[n] + i Y_b[n] for the direct half; conj(Y_a) + i conj(Y_b) belongs to index L - n: handed over in LDS
    float2 z[1][V];
    float2* m = grp_lds;
    FDR_JITTER(3021);
#pragma unroll
    for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
        for (int q = 0; q < HQ; ++q) {
            const int jj = u * HQ + q, s = u * Core::RHO0 + q;
            const int n = Core::in_index(tid, u, q);
            const float2 y0 = ya[jj], y1 = yb[jj];
            z[0][s] = make_float2(y0.x - y1.y, y0.y + y1.x);
            const int k = (L - n) & (L - 1);
            if (!(u == 0 && q == 0) || tid != 0) m[k] = make_float2(y0.x + y1.y, y1.x - y0.y);
        }
    __syncthreads();
    FDR_JITTER(3022);
#pragma unroll
    for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
        for (int q = HQ; q < Core::RHO0; ++q) z[0][u * Core::RHO0 + q] = m[Core::in_index(tid, u, q)];
    if (tid == 0) {  // n = 0 (DC) and n = L/2 (Nyquist): real values packed as (DC, Nyquist) in stored column 0
        z[0][0] = make_float2(ya[0].x, yb[0].x);
        z[0][HQ] = make_float2(ya[0].y, yb[0].y);
    }
    __syncthreads();  // the transform's first exchange may overwrite the buffer

    Core::template run<0, true>(z, grp_lds, tw_fwd, bases, tid);

    float mn = __builtin_inff(), mx = -__builtin_inff();
    double res = 0.0, kl = 0.0;  // row_out_fit_sums: the thread's terms, columns in order, row ra before rb
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) {
            const int n = Core::out_index(tid, u, q);
            const float va = z[0][u * Core::RHOL + q].x, vb = z[0][u * Core::RHOL + q].y;  // rows ra, rb
            if constexpr (row_out_stores_raw(OUT)) {
                a.dst_real[(size_t)ra * L + n] = va;
                a.dst_real[(size_t)rb * L + n] = vb;
            }
            if constexpr (row_out_fit_sums(OUT)) {  // (rows4_rl_ratio_stat)
                if (n < a.out_cols) {
                    if (ra < a.out_rows)
                        a.out[(size_t)ra * a.out_stride + n] = rows4_rl_ratio_stat(
                            va, a.src_real + (size_t)ra * a.src_stride + n, a.src_real2 ? a.src_real2 + (size_t)ra * a.src_stride + n : nullptr, res, kl);
                    if (rb < a.out_rows)
                        a.out[(size_t)rb * a.out_stride + n] = rows4_rl_ratio_stat(
                            vb, a.src_real + (size_t)rb * a.src_stride + n, a.src_real2 ? a.src_real2 + (size_t)rb * a.src_stride + n : nullptr, res, kl);
                }
            } else if constexpr (row_out_operator(OUT)) {  // (rows4_rl_value)
                if (n < a.out_cols) {
                    if (ra < a.out_rows)
                        a.out[(size_t)ra * a.out_stride + n] =
                            rows4_rl_value<OUT>(va, row_out_reads_src(OUT) ? a.src_real + (size_t)ra * a.src_stride + n : nullptr,
                                                row_out_reads_src2(OUT) ? a.src_real2 + (size_t)ra * a.src_stride + n : nullptr);
                    if (rb < a.out_rows)
                        a.out[(size_t)rb * a.out_stride + n] =
                            rows4_rl_value<OUT>(vb, row_out_reads_src(OUT) ? a.src_real + (size_t)rb * a.src_stride + n : nullptr,
                                                row_out_reads_src2(OUT) ? a.src_real2 + (size_t)rb * a.src_stride + n : nullptr);
                }
            } else if constexpr (row_out_normalizes(OUT)) {
                const float pa = va * fscale, pb = vb * fscale;
                if (n < a.out_cols) {
                    if (ra < a.out_rows) __builtin_nontemporal_store(pa + fshift, a.out + (size_t)ra * a.out_stride + n);
                    if (rb < a.out_rows) __builtin_nontemporal_store(pb + fshift, a.out + (size_t)rb * a.out_stride + n);
                }
            } else {
                if (n < a.mm_cols) {
                    if (ra < a.mm_rows) { mn = fminf(mn, va); mx = fmaxf(mx, va); }
                    if (rb < a.mm_rows) { mn = fminf(mn, vb); mx = fmaxf(mx, vb); }
                }
            }
        }
    if constexpr (row_out_minmax(OUT)) block_minmax_store(mn, mx, a.mm_part, (int)blockIdx.x);
    if constexpr (row_out_fit_sums(OUT)) {
        static_assert(Geo::THREADS % 64 == 0, "block_sum2_store: whole waves");
        block_sum2_store(res, kl, reinterpret_cast<double2*>(a.mm_part), (int)blockIdx.x);
    }
}

// One inverse row pass of kind OUT.  The guards: ROW_OUT_REAL_MINMAX alone has a full-spectrum form; the operator kinds take rows of
// 32 points and more, and ROW_OUT_RL_RATIO_STAT (one pair of fit sums per launch) one image per launch.
template <int LOGL, RowOut OUT>
static hipError_t launch_rows4_inv_kind(const RowArgs& a, const float2* tw, hipStream_t s) {
    using Geo = Rows4PackGeom<LOGL, true>;
    const int groups = (a.M + 3) / 4;
    const int nimg = a.batch.nimg > 1 ? a.batch.nimg : 1;
    const dim3 grid((groups + Geo::G - 1) / Geo::G, nimg), block(Geo::THREADS);
    if constexpr (LOGL >= 8 && LOGL <= 11) {
        if (rows4_use_split(LOGL, a.M, nimg, a.half)) {  // one small image: two thread groups per 4-row group (RowsSplitGeom)
            hipLaunchKernelGGL((fft_rows4_inv_split_kernel<LOGL, OUT>), dim3(a.M / 4), dim3(RowsSplitGeom<LOGL, true>::THREADS), 0, s, a, tw);
            return hipGetLastError();
        }
    }
    if constexpr (row_out_operator(OUT) && LOGL < 5) {
        return hipErrorInvalidValue;
    } else {
        if (row_out_operator(OUT) && !row_out_operator_group(OUT) && nimg > 1) return hipErrorInvalidValue;
        if (a.half) hipLaunchKernelGGL((fft_rows4_inv_packed_kernel<LOGL, true, OUT>), grid, block, 0, s, a, tw);
        else if constexpr (row_out_stores_raw(OUT)) hipLaunchKernelGGL((fft_rows4_inv_packed_kernel<LOGL, false, OUT>), grid, block, 0, s, a, tw);
        else return hipErrorInvalidValue;  // half-spectrum path only
        return hipGetLastError();
    }
}

// the kind as a template argument: every enumerator after ROW_OUT_COMPLEX is an inverse kind
template <int LOGL, RowOut OUT = ROW_OUT_REAL_MINMAX>
static hipError_t launch_rows4_inv_t(RowOut out, const RowArgs& a, const float2* tw, hipStream_t s) {
    if (out == OUT) return launch_rows4_inv_kind<LOGL, OUT>(a, tw, s);
    if constexpr (OUT < ROW_OUT_LAST) return launch_rows4_inv_t<LOGL, (RowOut)(OUT + 1)>(out, a, tw, s);
    return hipErrorInvalidValue;
}

static hipError_t launch_rows4_inv(int logl, RowOut out, const RowArgs& a, const float2* tw_fwd, hipStream_t s) {
    FDR_DISPATCH_LOG(logl, launch_rows4_inv_t<LG>(out, a, tw_fwd, s));
    return hipErrorInvalidValue;
}

template <int LOGL>
static int rows4_partials_t(int M, int nimg, int half) {
    if (rows4_use_split(LOGL, M, nimg, half)) return M / 4;  // one workgroup, one partial per 4-row group
    return ((M + 3) / 4 + Rows4PackGeom<LOGL, true>::G - 1) / Rows4PackGeom<LOGL, true>::G;
}

int rows4_minmax_partials(int logl, int M, int nimg, int half) {
    FDR_DISPATCH_LOG(logl, rows4_partials_t<LG>(M, nimg, half));
    return 0;
}

hipError_t launch_rows4(int logl, RowIn in, RowOut out, const RowArgs& a, const float2* tw_fwd, hipStream_t s) {
    if (in == ROW_IN_REAL && out == ROW_OUT_COMPLEX) return launch_rows4_fwd(logl, a, tw_fwd, s);
    if (in == ROW_IN_COMPLEX) return launch_rows4_inv(logl, out, a, tw_fwd, s);
    return hipErrorInvalidValue;
}

}  // namespace fdr
