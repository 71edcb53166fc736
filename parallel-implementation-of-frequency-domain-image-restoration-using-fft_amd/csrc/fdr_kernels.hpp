// fdr_kernels.hpp -- argument blocks and launcher declarations shared between the kernel
// translation units (compiled for gfx950 with -ffp-contract=off) and the host-side plan code.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "fdr_mixed_plan.hpp"

namespace fdr {

enum RowIn { ROW_IN_REAL = 0, ROW_IN_COMPLEX = 1 };
enum RowOut {
    ROW_OUT_COMPLEX = 0,
    ROW_OUT_REAL_MINMAX = 1,  // pass C': real plane + min/max partials
    ROW_OUT_MINMAX_ONLY = 2,  // pass C1 (two-sweep normalisation): min/max partials, nothing stored
    ROW_OUT_NORMALIZED = 3,   // pass C2: the transform again, normalised with the folded partials and cropped on store
    // the blur operator and Richardson-Lucy (fdr_rl.hip; half-spectrum rows of 32 points and more): cropped to the
    // window out_rows x out_cols on store (row stride out_stride), no min/max.  A group of images (batch.nimg > 1) takes spec[], out[]
    // and, for the kinds that read it, src_real[] from the batch block; ROW_OUT_RL_RATIO_STAT is one image per launch
    ROW_OUT_BLUR = 4,         // the value to `out`
    ROW_OUT_RL_RATIO = 5,     // r = c > kRlTau ? max(d, 0) / c : 0 to `out`; d read from src_real (row stride src_stride)
    ROW_OUT_RL_UPDATE = 6,    // max(u g, 0) to `out`; u read from src_real (row stride src_stride; may be `out` itself)
    // free-boundary Richardson-Lucy (fdr_rlfree.hip): max(u wgt g, 0) to `out`; u from src_real as ROW_OUT_RL_UPDATE, wgt from
    // src_real2 (same row stride; one plane for every image of a group, or with src2_pitch image k's own plane, the TV prior's factor)
    ROW_OUT_RL_UPDATE_W = 7,
    // the ratio that also measures the fit (fdr_rlstop.hip): d from src_real, the pixel's weight w from src_real2 (same row stride;
    // null: w = 1); r = c > kRlTau ? (w max(d, 0)) / c : 0 to `out` -- the bits of ROW_OUT_RL_RATIO on d (w = 1) or on dw = w max(d, 0)
    // -- and the workgroup's sums over the window of w (d+ - c)^2 and w (c - d+ + d+ ln(d+ / c)) as ONE pair of doubles at
    // mm_part (read as double2*), index blockIdx.x; rows4_minmax_partials(logl, M, 1, 1) of them
    ROW_OUT_RL_RATIO_STAT = 8,
    ROW_OUT_LAST = ROW_OUT_RL_RATIO_STAT
};
// the guard of the Richardson-Lucy ratio (FDR_RL_TAU of fdr.h): a blurred estimate at or below it gives r = 0
constexpr float kRlTau = 1e-7f;
enum ColKind {
    COL_FWD = 0,         // forward column FFT, complex in place (PSF spectrum, fft2d)
    COL_INV = 1,         // inverse column FFT, complex in place (fft2d)
    COL_FWD_WIENER = 2,  // parity pass B: forward column FFT then the Wiener quotient against H
    COL_INV_REAL = 3,    // parity pass D: inverse column FFT, real part to the raw plane, min/max
    COL_FUSED = 4,       // fast pass B' (panel kernels only): forward column FFT, multiply by W, inverse column FFT
    COL_FWD_FILTER = 5   // PSF spectrum (panel kernels only): rows >= nvalid taken as zero, forward column FFT, W = conj(H)/(|H|^2+K)
};

// several images per launch of the fast row passes / the normalisation (blockIdx.y = image): small images are launch
// bound, one launch per pass and GROUP of images fills the chip.  nimg <= 1: the single-image fields are used.
constexpr int kMaxGroup = 8;  // images per launch (fdr_plan_set_batching)
// entry `i` (uniform over the workgroup) of a kernel-argument array as a select chain on scalars: a dynamic index would
// send the array to scratch memory
template <class P>
__host__ __device__ __forceinline__ P pick_image(P const (&p)[kMaxGroup], int i) {
    static_assert(kMaxGroup == 8, "select chain written for 8 entries");
    const P lo = i == 0 ? p[0] : i == 1 ? p[1] : i == 2 ? p[2] : p[3];
    const P hi = i == 4 ? p[4] : i == 5 ? p[5] : i == 6 ? p[6] : p[7];
    return i < 4 ? lo : hi;
}
// The same chain written on the member itself, for the per-image arrays of a struct that is a by-value kernel argument
// (FDR_PICK_IMAGE(pl.c, z)): a macro and not pick_image, because pick_image's array reference, like a dynamic index, sends the whole
// argument block to scratch memory.
#define FDR_PICK_IMAGE(arr, i) \
    ((i) < 4 ? ((i) == 0 ? arr[0] : (i) == 1 ? arr[1] : (i) == 2 ? arr[2] : arr[3]) : ((i) == 4 ? arr[4] : (i) == 5 ? arr[5] : (i) == 6 ? arr[6] : arr[7]))
static_assert(kMaxGroup == 8, "FDR_PICK_IMAGE's select chain is written for 8 entries");
struct RowBatch {
    const float* src_real[kMaxGroup];  // pass A input; operator kinds of the inverse pass: the real source (d, dw or u)
    float2* spec[kMaxGroup];           // pass A output / pass C' input (panel-major spectrum)
    float* raw[kMaxGroup];             // pass C' output
    float2* mm_part[kMaxGroup];        // pass C' min/max partials
    float* out[kMaxGroup];             // pass C2 output (normalised, cropped); operator kinds: the cropped result
    int nimg;
};
struct NormBatch {
    const float* raw[kMaxGroup];
    const float2* part[kMaxGroup];
    float* out[kMaxGroup];
    int nimg;
};

// Workgroups that touch the same 128-byte lines -- `share` consecutive tiles -- are placed on ONE XCD (workgroup b lands
// on XCD b % 8) and dispatched back to back, so that their partial lines meet in that XCD's L2: tile of workgroup b.
__host__ __device__ __forceinline__ int col_tile_of_block(int b, int ntiles, int share) {
    if (share <= 1 || (ntiles % (8 * share)) != 0) return b;
    const int grp = b / (8 * share), r = b % (8 * share);
    return grp * 8 * share + (r % 8) * share + (r / 8);
}

struct RowArgs {
    // input
    const float* src_real;  // ROW_IN_REAL: rows x cols image, zero-padded on the fly to M x L
    int src_rows, src_cols, src_stride;
    const float2* src_c;  // ROW_IN_COMPLEX: M x L
    // output
    float2* dst_c;    // ROW_OUT_COMPLEX: M x L
    union {
        float* dst_real;         // ROW_OUT_REAL_MINMAX: M x L real plane
        const float* src_real2;  // ROW_OUT_RL_UPDATE_W, ROW_OUT_RL_RATIO_STAT: the second real source (row stride src_stride); shares the slot of dst_real,
                                 // which that kind does not use, so the argument block of every other kernel keeps its layout
    };
    float2* mm_part;  // one (min, max) partial per workgroup (ROW_OUT_RL_RATIO_STAT: one double2 (res, kl) per workgroup)
    int mm_rows, mm_cols;
    float* out;       // ROW_OUT_NORMALIZED: out_rows x out_cols result, row stride out_stride; mm_part holds n_part partials
    int out_rows, out_cols, out_stride, n_part;
    int M;              // number of rows to transform
    int src2_pitch;     // rows4 packed kernels, ROW_OUT_RL_UPDATE_W on a group: image k reads src_real2 + k src2_pitch floats (0: one
                        // plane for the group).  In the four bytes of padding between M and pstride: the block's size and every
                        // other field's offset are unchanged
    size_t pstride;     // rows4 kernels: panel stride of the panel-major spectrum, in float2 elements
    int half;           // rows4 packed kernels: half (Hermitian) spectrum, N/8 panels
    int num_cu;         // rows4 persistent kernels: CUs of the device
    RowBatch batch;     // rows4 packed kernels: several images per launch
    int panel_c;        // launch_rows (parity operator): the complex side(s) are PANEL-major, full spectrum: element (m, n) at
                        // (n >> 2) * pstride + m * 4 + (n & 3) -- the column passes then work on contiguous tiles
    int pad_mode;       // rows4 forward kernels (pass A): FDR_PAD_ZERO / FDR_PAD_SMOOTH -- what stands outside the picture.  In the tail
                        // padding of the block: its size and every other field's offset are unchanged
};
// Every rows4 kernel takes the block by value with the twiddle table behind it: a block that grew would move that pointer in the
// argument segment of all of them, so pad_mode sits in the tail padding and src2_pitch in the padding behind M.
static_assert(sizeof(RowArgs) == 448 && offsetof(RowArgs, src2_pitch) == offsetof(RowArgs, M) + sizeof(int) &&
                  offsetof(RowArgs, pstride) == offsetof(RowArgs, M) + 2 * sizeof(int),
              "pad_mode and src2_pitch fit the padding of RowArgs: the argument blocks keep their size and layout");

// up to kMaxGroup images' spectra handled by ONE pass-B' launch (their panels form one tile sequence)
struct PanelBatch {
    float2* data[kMaxGroup];
    int nimg;  // 0 or 1: use ColArgs::data only
};

struct ColArgs {
    float2* data;        // M x N complex, transformed in place
    const float2* filt;  // H (parity) or W (fast), M x N
    float K;
    float* dst_real;  // COL_INV_REAL: M x N real plane
    float2* mm_part;  // one (min, max) partial per workgroup
    int mm_rows, mm_cols;
    int N;  // row length (number of columns)
    int npanels;      // panel kernels: number of panels (0 = N/4)
    PanelBatch batch; // panel kernels, COL_FUSED: several images per launch
    int packed0;      // panel kernels: column 0 of panel 0 is the packed DC + i Nyquist column (half spectrum)
    int nvalid;       // COL_FWD_FILTER: rows of the panels that hold data (a multiple of 4); the others are read as zero
    size_t pstride;   // panel kernels: panel stride in float2 elements
    int num_cu;       // CUs of the device (persistent pass B' launches one workgroup per CU)
    int panel_c;      // launch_cols (parity operator): data / filt panel-major (pstride), dst_real panel-major with stride 4 M floats
};

// `return expr;` with LG = the value of `var` as a constant, for the transform lengths the kernels are instantiated for
// (log2 = 3..13); falls through for any other value
#define FDR_DISPATCH_LOG(var, expr)                                                     \
    switch (var) {                                                                      \
        case 3: { constexpr int LG = 3; return expr; }                                  \
        case 4: { constexpr int LG = 4; return expr; }                                  \
        case 5: { constexpr int LG = 5; return expr; }                                  \
        case 6: { constexpr int LG = 6; return expr; }                                  \
        case 7: { constexpr int LG = 7; return expr; }                                  \
        case 8: { constexpr int LG = 8; return expr; }                                  \
        case 9: { constexpr int LG = 9; return expr; }                                  \
        case 10: { constexpr int LG = 10; return expr; }                                \
        case 11: { constexpr int LG = 11; return expr; }                                \
        case 12: { constexpr int LG = 12; return expr; }                                \
        case 13: { constexpr int LG = 13; return expr; }                                \
        default: break;                                                                 \
    }

// launchers (fdr_rows.hip / fdr_cols.hip); logl = log2 of the transform length, 3..13
// tw: parity mode -> table of the requested direction; fast mode -> the forward table (inverse = conjugate)
hipError_t launch_rows(int logl, int mode, RowIn in, RowOut out, bool inverse, const RowArgs& a, const float2* tw,
                       hipStream_t s);
hipError_t launch_cols(int logm, int mode, ColKind kind, const ColArgs& a, const float2* tw_fwd, const float2* tw_inv,
                       hipStream_t s);

// fast-mode passes on the panel-major intermediate (fdr_panel_rows.hip, fdr_panel_cols.hip; layout in fdr_panel.hpp);
// tw_fwd = forward table
// rows4: (ROW_IN_REAL -> ROW_OUT_COMPLEX[panel]) forward, (ROW_IN_COMPLEX[panel] -> ROW_OUT_REAL_MINMAX) inverse
hipError_t launch_rows4(int logl, RowIn in, RowOut out, const RowArgs& a, const float2* tw_fwd, hipStream_t s);
// min/max partials pass C' writes per image when `nimg` images share a launch
int rows4_minmax_partials(int logl, int M, int nimg, int half);
// cols_panel: COL_FWD_FILTER (PSF spectrum -> W, in place) or COL_FUSED (FFT . W . IFFT)
hipError_t launch_cols_panel(int logm, ColKind kind, const ColArgs& a, const float2* tw_fwd, hipStream_t s);
// (fdr_cls.hip) the COL_FWD_FILTER pass with the constrained least-squares quotient W = conj(H) / (|H|^2 + K + gamma L^2) instead: lap = the
// Laplacian table of the plan (a_u = 4 sin^2(pi u / M), u < M, then b_v = 4 sin^2(pi v / N), v < N; doubles, device memory)
hipError_t launch_cols_panel_cls(int logm, const ColArgs& a, const double* lap, double gamma, const float2* tw_fwd, hipStream_t s);
// (fdr_rl.hip) the operator tables of the blur / Richardson-Lucy calls: the PSF column pass of COL_FWD_FILTER (a.data = the row
// spectra of the PSF, a.nvalid rows, half spectrum) writing H / (M N) in place and conj(H) / (M N) to `conj_out`, both in the
// layout pass B' reads W from (packed column 0 of panel 0 included)
hipError_t launch_cols_panel_operator(int logm, const ColArgs& a, float2* conj_out, const float2* tw_fwd, hipStream_t s);
// (fdr_rl.hip) u = max(d, 0) on a rows x cols window (row strides `stride` / `ustride`)
hipError_t launch_rl_init(const float* d, int rows, int cols, int stride, float* u, int ustride, hipStream_t s);
// (fdr_rlfree.hip) free-boundary, weighted Richardson-Lucy.  setup: dw = m max(d, 0) and W = m on the rows x cols window (m = 1 for a
// null pointer; both dense, row stride cols; W may be m itself), their sums in double as rlfree_partials(rows, cols) per-workgroup
// partials each, folded in a fixed order into part[2 n] = sum dw, part[2 n + 1] = sum W (part holds 2 n + 2 doubles).  start: the
// M x N plane `wgt` holds alpha on entry; wgt = alpha > sigma ? 1 / alpha : 0, u = alpha > sigma ? sum dw / sum W : 0 (0 for sum W = 0).
// crop: the window rows x cols of u (row stride ustride) to `out`.
int rlfree_partials(int rows, int cols);
hipError_t launch_rlfree_setup(const float* d, int stride, const float* m, int mstride, int rows, int cols, float* dw, float* W, double* part,
                               hipStream_t s);
hipError_t launch_rlfree_start(float* wgt, float* u, size_t count, float sigma, const double* sums, hipStream_t s);
hipError_t launch_rlfree_crop(const float* u, int ustride, float* out, int rows, int cols, int out_stride, hipStream_t s);
// (fdr_rltv.hip) Richardson-Lucy with a total-variation prior: out = w / (1 - lambda div(grad u / sqrt(|grad u|^2 + eps^2))) on the
// rows x cols domain of u (forward differences, replicated at the far edges; u and w with row stride `stride`, w = 1 for a null
// pointer; out is neither).  Any size, stride and alignment.
hipError_t launch_rltv_factor(const float* u, int rows, int cols, int stride, const float* w, float lambda, float eps, float* out,
                              int out_stride, hipStream_t s);
// the same on a group of 1 <= count <= kMaxGroup planes in one launch: plane k's u and out lie k u_pitch and k out_pitch floats
// behind those given, w is the group's.  Uncoupled every plane gets the bits of launch_rltv_factor on it (one plane is that launch);
// `coupled`: the planes are the channels of one picture and share m = sqrt(eps^2 + sum_c |grad u_c|^2), added in channel order.
hipError_t launch_rltv_factor_group(const float* u, size_t u_pitch, int count, int rows, int cols, int stride, const float* w, float lambda,
                                    float eps, float* out, size_t out_pitch, int out_stride, bool coupled, hipStream_t s);
// (fdr_frames.hip) multi-frame Richardson-Lucy.  sum: dst[i] = (accumulate ? dst[i] : src_0[i]) + src_k[i] for the remaining k < n in
// ascending order, plain float adds, i < n_floats (even, >= 2; every pointer 16-byte aligned; dst may be a source exactly): the
// spectra pass B' left for the frames of a launch group, added in the domain where the inverse row pass is still to come.  fold:
// out[j] = sum_k sums[k pitch + j], j = 0, 1, in ascending k (the (sum dw, sum W) pairs of the frames; out may not be one of them).
struct FrameSrcs { const float* p[kMaxGroup]; };
hipError_t launch_frames_sum(float* dst, const FrameSrcs& srcs, int n, size_t n_floats, bool accumulate, hipStream_t s);
hipError_t launch_frames_fold(const double* sums, size_t pitch, int n, double* out, hipStream_t s);
// (fdr_tvframes.hip) multi-frame TV deconvolution: T = (1 / (M N)) / (nu sum_k |H_k|^2 + rho L) from the `count` (1 .. kMaxGroup)
// frame tables H_k / (M N) (16-byte aligned, the layout of launch_tv_table's op_h), summed in double in ascending k and rounded
// once; one table gives the bytes of launch_tv_table on it
struct FrameTables { const float2* p[kMaxGroup]; };
hipError_t launch_tv_frames_table(const FrameTables& tabs, int count, float2* T, const double* lap, int M, int N, size_t pstride, int npanels,
                                  double nu, double rho, hipStream_t s);
// (fdr_rlaccel.hip) accelerated Richardson-Lucy, on rows x cols windows with their own row strides.  direction: g = u1 - y over the
// previous g; with `part` not null also sum(g_new g_old) and sum(g_old g_old) in double as rlaccel_partials(rows, cols)
// per-workgroup partials each (part holds 2 n doubles); with a null `part` the old g is not read.  alpha: one workgroup folds the
// partials in index order, alpha = clamp(num / den, 0, amax) (0 for den = 0 or a quotient that is not finite) to *alpha and, when
// not null, *record.  extrapolate: y = max(u1 + alpha (u1 - u0), 0), alpha read from the device.
int rlaccel_partials(int rows, int cols);
hipError_t launch_rlaccel_direction(const float* u1, int u1s, const float* y, int ys, float* g, int gs, int rows, int cols, double* part,
                                    hipStream_t s);
hipError_t launch_rlaccel_alpha(const double* part, int n, float amax, float* alpha, float* record, hipStream_t s);
hipError_t launch_rlaccel_extrapolate(const float* u1, int u1s, const float* u0, int u0s, const float* alpha, float* y, int ys, int rows,
                                      int cols, hipStream_t s);
// the same on a group of 1 <= nimg <= kMaxGroup images in one launch each (blockIdx.z = image; one image is the single-image launch):
// per-image planes with one row stride per operand, image z's partials at part + z 2 n (n = rlaccel_partials(rows, cols)), its alpha
// at alpha[z] and, when `record` is not null, at record[z alpha_pitch].  Every image gets the bits of the single-image kernels.
hipError_t launch_rlaccel_direction_n(int nimg, const float* const* u1, int u1s, const float* const* y, int ys, float* const* g, int gs, int rows,
                                      int cols, double* part, hipStream_t s);
hipError_t launch_rlaccel_alpha_n(int nimg, const double* part, int n, float amax, float* alpha, float* record, size_t alpha_pitch, hipStream_t s);
hipError_t launch_rlaccel_extrapolate_n(int nimg, const float* const* u1, int u1s, const float* const* u0, int u0s, const float* alpha,
                                        float* const* y, int ys, int rows, int cols, hipStream_t s);
// (fdr_rlstop.hip) the fit trace of Richardson-Lucy: one workgroup folds the n (res, kl) pairs ROW_OUT_RL_RATIO_STAT left in `part`
// in index order (thread t adds t, t + 256, ... in order, then a fixed tree) into out[0] = res, out[1] = kl
hipError_t launch_rlstop_fold(const double* part, int n, double* out, hipStream_t s);
// (fdr_blind.hip) blind Richardson-Lucy.  conj: the column pass of launch_cols_panel_operator on the row spectra a.data (a.nvalid rows,
// half spectrum; only read), storing conj(U) / (M N) alone, to `conj_out` (not a.data), in the layout pass B' reads its filter from.
// start: the caller's prows x pcols PSF (row stride pstride) dense into p, *status = 0 when no entry is negative and the double sum is
// finite and > 0, else 1.  project: q = max(p . num, 0) (den null) or den > 0 ? max(p . num / den, 0) : 0, s = sum(q) in double in a
// fixed order, p = q / s when s is finite and > 0 and *status is 0 (else p stays); the PSF also to `out` (row stride ostride) when
// that is not null.  wgt: alpha in `wgt` (count floats, a multiple of 4) -> alpha > sigma ? 1 / alpha : 0.  gaussian: fdr_psf_gaussian.
constexpr int kBlindMaxPsf = 65536;  // entries of a PSF the one-workgroup kernels take
hipError_t launch_cols_panel_conj(int logm, const ColArgs& a, float2* conj_out, const float2* tw_fwd, hipStream_t s);
hipError_t launch_blind_psf_start(const float* psf, int prows, int pcols, int pstride, float* p, int* status, hipStream_t s);
hipError_t launch_blind_psf_project(float* p, const float* num, const float* den, int prows, int pcols, const int* status, float* out,
                                    int ostride, hipStream_t s);
hipError_t launch_blind_wgt(float* wgt, size_t count, float sigma, hipStream_t s);
hipError_t launch_psf_gaussian(int size, double sigma, float* d_out, hipStream_t s);
// (fdr_tv.hip) total-variation deconvolution.  table: T = (1 / (M N)) / (mu |H|^2 + rho L) from op_h = H / (M N) (the operator table
// of launch_cols_panel_operator) and the Laplacian table `lap` of launch_cols_panel_cls, in the layout pass B' reads its filter
// from.  init: x = pad(d) over the M x N plan (row stride N), wx = wy = 0.  spatial: one ADMM half-step on full M x N planes --
// reads x, (wx, wy), b, writes the new duals (nwx, nwy; not the planes read) and rhs = mu b + rho D^T v (not x).  output: the window
// of x to `out`, clamped at 0 with nonneg.
hipError_t launch_tv_table(const float2* op_h, float2* T, const double* lap, int M, int N, size_t pstride, int npanels, double mu, double rho,
                           hipStream_t s);
// an entry of that table and of the frames' (fdr_tvframes.hip): (1 / (M N)) / (mu h2 + rho lap) in double, rounded once; a zero (or
// negative) denominator gives 0, as the CLS filter does
__device__ __forceinline__ float tv_quotient(double h2, double lap, double mu, double rho, double inv_mn) {
    const double den = mu * h2 + rho * lap;
    return den > 0.0 ? (float)(inv_mn / den) : 0.f;
}
hipError_t launch_tv_init(const float* d, int rows, int cols, int stride, float* x, float* wx, float* wy, int M, int N, hipStream_t s);
hipError_t launch_tv_spatial(const float* x, const float* wx, const float* wy, const float* b, float* nwx, float* nwy, float* rhs, int M, int N,
                             float mu, float rho, int anisotropic, hipStream_t s);
hipError_t launch_tv_output(const float* x, int N, float* out, int rows, int cols, int out_stride, int nonneg, hipStream_t s);
// the same on a group of 1 <= nimg <= kMaxGroup images in one launch each (blockIdx.z = image; one image is the single-image launch):
// per-image planes (spatial: those of image k lie k * stride floats behind those of image 0, its rhs is rhs[k]), every image with the
// bits of the single-image kernels.  spatial with `coupled` (isotropic only; any nimg >= 1):
// the images are the channels of one picture and share the shrinkage, z_c = s g_c, s = max(1 - t / m, 0), m^2 = the sum over the
// channels, in their order, of gx_c^2 + gy_c^2 (vectorial TV); one channel gives the bits of the single-image kernel.
hipError_t launch_tv_init_n(int nimg, const float* const* d, int rows, int cols, int stride, float* const* x, float* const* wx, float* const* wy,
                            int M, int N, hipStream_t s);
hipError_t launch_tv_spatial_n(int nimg, const float* x, const float* wx, const float* wy, const float* b, float* nwx, float* nwy, size_t stride,
                               float* const* rhs, int M, int N, float mu, float rho, int anisotropic, int coupled, hipStream_t s);
hipError_t launch_tv_output_n(int nimg, const float* const* x, int N, float* const* out, int rows, int cols, int out_stride, int nonneg,
                              hipStream_t s);
// (fdr_tvfree.hip) the window launches of the free-boundary TV forms: the data step, and the norm of fdr_tvauto.hip on the same
// window.  The planes of a launch group as a kernel argument, and what the host decides for a launch: the planes (entries past nimg
// repeat image 0), the alignment bits (bit z of dvec: image z's window d takes 16-byte loads; wvec: the one weights window does),
// the workgroup of tx x ty = 256 threads, four pixels of a row each, and gx, the workgroups across the window (tv_window_block; the
// workgroups down the window are the kernel's own: the norm kernel gives a thread several rows).  tv_window_launch fills it, or returns false for what no window kernel takes: nimg outside 1 .. kMaxGroup, a null plane or window, planes c and q
// that are not 16-byte aligned, a window outside the M x N planes, N no multiple of 4, a stride below cols.
struct TvWindowPlanes {
    float* c[kMaxGroup];
    float* q[kMaxGroup];
    const float* d[kMaxGroup];
};
struct TvWindowWeights { const float* w[kMaxGroup]; };  // a weights window per image (entries past nimg repeat image 0's)
struct TvWindowLaunch {
    TvWindowPlanes pl;
    int dvec, wvec;
    int tx, ty, gx;
};
inline void tv_window_block(int cols, int* tx, int* ty, int* gx) {
    const int groups = (cols + 3) / 4;
    *tx = groups <= 64 ? 64 : groups <= 128 ? 128 : 256;
    *ty = 256 / *tx;
    *gx = (groups + *tx - 1) / *tx;
}
bool tv_window_launch(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride, int rows, int cols,
                      int M, int N, TvWindowLaunch* L);
// four consecutive pixels of a caller's window row (wr = the row's base + j): one 16-byte load when the group lies inside the
// window (`whole`: j + 3 < cols) and the host found every row aligned (`vec`), scalar loads otherwise; pixels beyond column `cols`
// keep what v held
__device__ __forceinline__ void tv_load_window4(const float* wr, int j, int cols, bool whole, int vec, float v[4]) {
    if (whole && vec) {
        const float4 t = *reinterpret_cast<const float4*>(wr);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (j + l < cols) v[l] = wr[l];
    }
}
// The data step on the rows x cols window of the dense M x N planes c and q (row stride N, 16-byte aligned) of 1 <= nimg <= kMaxGroup
// images in one launch (blockIdx.z = image; one image makes the single kernel's launch): per-image planes c, q and windows d (one
// stride, any alignment each), ONE weights window w (null: 1) for all, read in place with their own strides; nothing outside the
// window is read or written, and every image gets the bits it gets alone.  Least squares: e = c + q; s = (mu w d + nu e) / (mu w +
// nu); q = e - s; c = s - q.
hipError_t launch_tvfree_data_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride, int rows,
                                int cols, int M, int N, float mu, float nu, hipStream_t s);
// the same with image z's weight read from the device, mu[z] (where launch_tvauto_mu_n left it)
hipError_t launch_tvauto_data_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride, int rows,
                                int cols, int M, int N, const float* mu, float nu, hipStream_t s);
// the arithmetic of the least-squares step on one pixel, shared by every launch of it (single and group, fixed and device mu) so
// that all of them round alike: c = blur(x) and q on entry, r = s - q and the new q on exit; m is the pixel's weight
__device__ __forceinline__ void tvfree_data_pixel(const float mu, const float nu, const float m, const float d, float& c, float& q) {
    const float e = c + q;
    const float a = mu * m;
    const float s = (a * d + nu * e) / (a + nu);
    q = e - s;
    c = s - q;
}
// the data step of Poisson-likelihood TV deconvolution, on the same window, planes and caller's windows: the minimiser over s of
// mu m [(s + b) - d+ log(s + b)] + nu / 2 (s - e)^2, b = background >= 0, then q = e - s; c = s - q
hipError_t launch_tvpoisson_data_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* w, int wstride,
                                   int rows, int cols, int M, int N, float mu, float nu, float background, hipStream_t s);
// both steps with a weights window per image, w[k] image k's (none null; one stride, any alignment each): the exposures of
// fdr_tv_deconv_frames_f32*, whose masks differ.  Every image gets the bits of the launches above on its own window; one image makes
// the single kernel's launch.
hipError_t launch_tvfree_data_weights_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* const* w,
                                        int wstride, int rows, int cols, int M, int N, float mu, float nu, hipStream_t s);
hipError_t launch_tvpoisson_data_weights_n(int nimg, float* const* c, float* const* q, const float* const* d, int stride, const float* const* w,
                                           int wstride, int rows, int cols, int M, int N, float mu, float nu, float background, hipStream_t s);
// The arithmetic of that step on one pixel, shared by every launch of it.  Every operation is one correctly rounded
// float operation (no contraction), in this order:
//     e  = c + q
//     m > 0 (a pixel that counts):
//         k  = (mu * m) / nu
//         dp = d < 0 ? 0 : d                      (a NaN stays)
//         a  = (e + b) - k
//         t  = k * dp
//         rt = sqrtf(a * a + 4 * t)
//         y  = a >= 0 ? 0.5 * (a + rt) : (2 * t) / (rt - a)      (the root of y^2 - a y - t = 0 that is >= 0, without cancellation)
//         s  = y - b
//     otherwise s = e
//     q  = e - s
//     c  = s - q
__device__ __forceinline__ void tvpoisson_data_pixel(const float mu, const float nu, const float b, const float m, const float d, float& c,
                                                     float& q) {
    const float e = c + q;
    float s = e;
    if (m > 0.f) {
        const float k = (mu * m) / nu;
        const float dp = d < 0.f ? 0.f : d;
        const float a = (e + b) - k;
        const float t = k * dp;
        const float rt = sqrtf(a * a + 4.f * t);
        const float y = a >= 0.f ? 0.5f * (a + rt) : (2.f * t) / (rt - a);
        s = y - b;
    }
    q = e - s;
    c = s - q;
}
// (fdr_tvauto.hip) noise-constrained TV deconvolution, on the same window, planes and caller's windows.  norm: res_e = sum w (c + q -
// d)^2, res_c = sum w (c - d)^2 and S = sum w in double as tvauto_partials(rows, cols) per-workgroup partials each (part holds 3 n
// doubles; no window of an M x N plan needs more than tvauto_max_partials(M, N)).  mu: one workgroup folds the partials in index
// order; with c2 = tau sigma^2 S, g = 0 for res_e <= c2, 1e6 for c2 = 0 or a quotient that is not finite, else min(sqrt(res_e / c2)
// - 1, 1e6); *mu = float(nu g), stat[0 .. 3] = (res_c, res_e, mu, S) and, when not null, trace[0 .. 2] = (res_c, res_e, mu).  The
// data step that reads that mu is launch_tvauto_data_n above.
int tvauto_partials(int rows, int cols);
int tvauto_max_partials(int M, int N);
hipError_t launch_tvauto_mu(const double* part, int n, double sigma, double tau, float nu, float* mu, double* stat, double* trace, hipStream_t s);
// on a group of 1 <= nimg <= kMaxGroup images in one launch each (one image makes the single kernel's launch), every image with the
// bits of the single kernels: image z's partials at part + z 3 n (n = tvauto_partials(rows, cols)), its noise level sigma[z], its
// weight at mu[z], its sums at stat + 4 z and, where trace[z] is not null, there (trace itself may be null).  The mu launch runs one
// workgroup per image.
hipError_t launch_tvauto_norm_n(int nimg, const float* const* c, const float* const* q, const float* const* d, int stride, const float* w, int wstride,
                                int rows, int cols, int M, int N, double* part, hipStream_t s);
hipError_t launch_tvauto_mu_n(int nimg, const double* part, int n, const double* sigma, double tau, float nu, float* mu, double* stat,
                              double* const* trace, hipStream_t s);

// (fdr_motion.hip) the motion-blur estimate.  window: the Hann tables into hann[rows + cols], w . img on the window and 0 elsewhere
// into the row-major M x N complex plane, sum |x| partials (motion_pad_partials of them) folded in a fixed order into
// part[motion_pad_partials(M, N)] (part holds one more double).  log: G -> (log(|G| + 1e-6 sum) / (M N), 0) in place (0 for sum 0).
// score: table[a * n_lengths + l - min_length] = the real parts bilinearly at (-l sin, l cos), periodic; trig = cos[n_angles], sin[n_angles]
int motion_pad_partials(int M, int N);
hipError_t launch_motion_window(const float* img, int rows, int cols, int stride, float* hann, float2* plane, int M, int N, double* part,
                                hipStream_t s);
hipError_t launch_motion_log(float2* plane, int M, int N, const double* sum, hipStream_t s);
// the two stages of the window launch that the frame registration shares: the Hann tables alone, and part[n] = the sum of part[0 .. n) in
// the fixed order of one workgroup
hipError_t launch_motion_hann(float* hann, int rows, int cols, hipStream_t s);
hipError_t launch_motion_fold(double* part, int n, hipStream_t s);
hipError_t launch_motion_score(const float2* plane, int M, int N, const double* trig, int n_angles, int min_length, int n_lengths, float* table,
                               hipStream_t s);
// (fdr_register.hip) registering the frames of a burst; the formulas are in that file's header.  pair: re = w . a, im = w . b on the rows x
// cols window (w the Hann tables, or 1 for hann == null), 0 elsewhere in the M x N plane; with `part` (2 register_peak_partials(M, N)
// doubles) also *gate = 1 when neither windowed picture is all zero, else 0.  cross: Z = DFT2 of such a picture pair (in
// place -> C), P = DFT2 of the PSF pair (null: H_a = H_b = 1), the sum |C| partials (register_cross_partials of them) folded into
// part[register_cross_partials(M, N)].  normalize: C -> C / (|C| + eps_rel mean |C|) / (M N) in place (0 for sum[0] = 0 or a gate
// sum[1] = 0; the peak pass reads the same pair).  peak: the real
// parts of the plane -> the frame's result (24 bytes: double dy, dx; float peak, confidence) at `result`; part holds 4
// register_peak_partials(M, N) doubles.  reference: the result (0, 0, 1, 0).  psf_shift: see fdr_psf_shift_f32 in include/fdr.h.
int register_cross_partials(int M, int N);
int register_peak_partials(int M, int N);
hipError_t launch_register_pair(const float* a, const float* b, int rows, int cols, int stride, const float* hann, float2* plane, int M, int N,
                                double* part, double* gate, hipStream_t s);
hipError_t launch_register_cross(float2* Z, const float2* P, int M, int N, double* part, hipStream_t s);
hipError_t launch_register_normalize(float2* plane, int M, int N, const double* sum, float eps_rel, hipStream_t s);
hipError_t launch_register_peak(const float2* plane, int M, int N, int range_rows, int range_cols, const double* sum, double* part, void* result,
                                hipStream_t s);
hipError_t launch_register_reference(void* result, hipStream_t s);
hipError_t launch_psf_shift(const float* psfs, size_t psf_pitch, int count, int prows, int pcols, int pstride, const void* shifts, int pad_rows,
                            int pad_cols, float* out, size_t out_pitch, int out_stride, hipStream_t s);
// (fdr_defocus.hip) the defocus estimate.  disk: fdr_psf_disk (size <= kDiskMaxSize, radius > 0; one workgroup).  profile: T[d -
// min_diameter] = the median over a of the score launch_motion_score would put at table[a * n_diameters + d - min_diameter], from the
// same plane and trig table; one workgroup per diameter, n_angles <= kDefocusMaxAngles
constexpr int kDiskMaxSize = 256;
constexpr int kDefocusMaxAngles = 4096;  // one column of scores in LDS: 16 KB
hipError_t launch_psf_disk(int size, double radius, float* d_out, hipStream_t s);
hipError_t launch_defocus_profile(const float2* plane, int M, int N, const double* trig, int n_angles, int min_diameter, int n_diameters,
                                  float* T, hipStream_t s);

// (fdr_reg.hip) choosing the regularisation weight.  noise: the Immerkaer sum S of |d * [[1,-2,1],[-2,4,-2],[1,-2,1]]| over the interior
// of the rows x cols window (rows, cols >= 3) as reg_noise_partials(rows, cols) double partials, folded in a fixed order into
// part[reg_noise_partials(rows, cols)] (part holds one more double; at most kRegMaxPartials + 1).  power: the forward column FFT of
// a.data (the row spectra of pass A, a.nvalid rows, half spectrum, only read) and |G|^2 / (M N) as one float per bin into `power`
// (row m of panel p at p * pstride + m * 4 floats); the packed column's slots hold |G0[k]|^2 for k <= M/2 and |GN[M - k]|^2 above,
// extras[0 .. 1] = |GN[0]|^2, |GN[M/2]|^2 (all scaled).  curve: rho and trace of `ncand` <= kRegCandidates pairs (cand holds
// kRegCandidates (K, gamma) pairs of doubles; the pairs past ncand are evaluated and dropped) into out[2 c], out[2 c + 1], through
// reg_curve_partials(M, npanels) * 2 kRegCandidates double partials in `part`.
constexpr int kRegCandidates = 16;    // candidate pairs per sweep of the spectrum
constexpr int kRegMaxPartials = 1024;  // workgroups of the noise and curve kernels
int reg_noise_partials(int rows, int cols);
hipError_t launch_reg_noise(const float* d, int rows, int cols, int stride, double* part, hipStream_t s);
hipError_t launch_cols_panel_power(int logm, const ColArgs& a, float* power, float* extras, const float2* tw_fwd, hipStream_t s);
int reg_curve_partials(int M, int npanels);
hipError_t launch_reg_curve(const float2* op_h, const float* power, const float* extras, const double* lap, const double* cand, int ncand, int M,
                            int N, size_t pstride, int npanels, double* part, double* out, hipStream_t s);

// the reference-shaped simple path and the free-standing transforms (fdr_simple.hip)
hipError_t launch_pad_real_to_complex(const float* src, int rows, int cols, int stride, float2* dst, int M, int N,
                                      hipStream_t s);
hipError_t launch_simple_rows(float2* data, int rows, int L, int logl, const float2* tw, int mode, hipStream_t s);
hipError_t launch_transpose(const float2* src, float2* dst, int rows, int cols, hipStream_t s);
// transforms of more than 8192 points (fdr_simple.hip): subsequences gathered into 8192-point blocks, and one radix-2 stage
// (butterfly distance `half`) over rows of length L in global memory; tw = table of the requested direction (both modes)
constexpr int kMaxLdsLog = 13;    // longest transform the row / column kernels hold on chip
constexpr int kMaxLongLog = 15;   // longest transform at all (32768 points)
hipError_t launch_long_gather(const float2* src, float2* dst, size_t rows, int L, int logs, hipStream_t s);
hipError_t launch_long_stage(const float2* src, float2* dst, size_t rows, int L, int half, const float2* tw, int mode, hipStream_t s);
hipError_t launch_wiener_pointwise(float2* g, const float2* filt, size_t count, float K, int mode, hipStream_t s);
hipError_t launch_make_filter_fast(const float2* H, float2* W, size_t count, float K, hipStream_t s);
// (fdr_cls.hip) the same with the CLS quotient on a row-major M x N spectrum (simple path); lap as launch_cols_panel_cls
hipError_t launch_make_filter_cls(const float2* H, float2* W, int M, int N, float K, const double* lap, double gamma, hipStream_t s);
hipError_t launch_real_minmax(const float2* src, float* dst, int M, int N, int mm_rows, int mm_cols, float2* mm_part,
                              int* n_part, hipStream_t s);
// min/max and normalisation (fdr_norm.hip)
hipError_t launch_reduce_minmax(const float2* mm_part, int n_part, float* mm, hipStream_t s);
// number of (min,max) partials the row / column real-output passes write for an M x N plan
int rows_minmax_partials(int logl, int M);
int cols_minmax_partials(int logm, int N);
// mm_part != nullptr: every workgroup folds the n_part partials itself; else mm = {min, max} from launch_reduce_minmax
hipError_t launch_normalize(const float* raw, int N, const float2* mm_part, int n_part, const float* mm, float* out,
                            int rows, int cols, int out_stride, hipStream_t s, const NormBatch* batch = nullptr);
// the same from a PANEL-major real plane (panel p = columns 4 p .. 4 p + 3, M rows of 4 floats, panels 4 M floats apart)
hipError_t launch_normalize_panels(const float* raw, int M, const float2* mm_part, int n_part, const float* mm, float* out,
                                   int rows, int cols, int out_stride, hipStream_t s);
// image utilities (fdr_image.hip: the motion PSF, the affine warp, launch_synth and launch_checksum below)
hipError_t launch_psf_motion(int size, double angle_deg, float* d_out, hipStream_t s);
// cv::warpAffine defaults (bilinear, constant 0 border) on a single-channel float image; fwd = the 2 x 3 matrix as cv::warpAffine takes it
hipError_t launch_warp_affine(const float* src, int srows, int scols, int sstride, const double fwd[6], float* dst, int drows, int dcols,
                              int dstride, hipStream_t s);
// slab mode (single image over several GPUs): column blocks of a row slab packed for the all-to-all, dense transposes
// of 4- or 8-byte elements (fdr_simple.hip), real part, min/max partials of a real plane (fdr_norm.hip)
hipError_t launch_slab_pack(const void* src, int rows, int ld, int parts, const int* counts, int elem_size, void* dst, hipStream_t s);
hipError_t launch_transpose_any(const void* src, void* dst, int rows, int cols, int elem_size, hipStream_t s);
hipError_t launch_real_part(const float2* src, float* dst, size_t count, hipStream_t s);
hipError_t launch_minmax_real(const float* src, int rows, int ld, int mm_rows, int mm_cols, float2* part, int* n_part, hipStream_t s);

// colour epilogue of the drivers (fdr_color.hip): planar float BGR in [0,1] -> Lab white balance -> interleaved 8-bit BGR
struct ColorArgs {
    const float* orig[3];  // blurred input planes B, G, R (the white-balance reference)
    const float* rest[3];  // restored planes B, G, R
    int rows, cols, stride;
    unsigned char* out;    // rows x cols x 3, row stride out_stride bytes
    int out_stride;
};
int color_partials(int rows, int cols);
hipError_t launch_color_epilogue(const ColorArgs& a, double2* part, hipStream_t s);
hipError_t launch_synth(uint64_t seed, uint64_t first, size_t count, float* d_out, hipStream_t s);
// sum of `count` floats as kChecksumParts double partials in `part` (fixed order: the same bits on every run)
constexpr int kChecksumParts = 1024;
hipError_t launch_checksum(const float* x, size_t count, double* part, hipStream_t s);
hipError_t launch_dft_naive(const float2* src, float2* dst, int n, int inverse, hipStream_t s);
// table[t * n + k], forward direction, host generated (see fdr_simple.hip); rows transforms of length n, src != dst
hipError_t launch_dft_naive_rows(const float2* src, float2* dst, int rows, int n, const float2* table, int inverse, hipStream_t s);

// mixed-radix fast mode (fdr_mixed.hip, FDR_FLAG_MIXED_RADIX): transform lengths 2^a 3^b 5^c up to 8192, rows in LDS
// (kMixMaxElems, kMixMaxLds, kMixMaxLen, kMixTwLo and the host-built tables: fdr_mixed_plan.hpp)
struct MixLen {            // one transform length, device tables built by the plan
    const float2* tw;      // exp(-2 pi i m / L) as lo[i] = m = i (i < 64), hi[i] = m = 64 i (i < ceil(L / 64)); double-generated
    const int4* st;        // per Stockham stage {radix, ns (product of the earlier radices), ceil(2^32 / ns) or 0 for ns = 1, L / (ns radix)}
    int L, nst;            // length, number of stages
    int nt;                // threads per transform (a multiple of 64, >= L / kMixMaxElems)
};
enum MixRowKind {
    MIX_ROWS_FWD_REAL = 0,  // pass A: real rows (zero padded on load) -> panel-major spectrum, two rows per transform
    MIX_ROWS_C2C = 1,       // fdr_fft2d_c2c: row-major complex rows -> panel-major, forward or inverse
    MIX_ROWS_INV_REAL = 2   // pass C: panel-major spectrum -> inverse, real parts of the cropped rows, (min, max) partials
};
enum MixColKind {
    MIX_COLS_FILTER = 0,  // PSF spectrum: forward columns, W = conj(H) / (|H|^2 + K) in place
    MIX_COLS_FUSED = 1,   // pass B: forward columns, multiply by W, inverse columns
    MIX_COLS_C2C = 2,     // fdr_fft2d_c2c: panel-major -> columns forward or inverse -> row-major M x N
    MIX_COLS_FILTER_CLS = 3  // MIX_COLS_FILTER with the CLS quotient W = conj(H) / (|H|^2 + K + gamma L^2) (lap, gamma)
};
struct MixRowArgs {
    MixLen len;          // length N
    int B;               // transforms per workgroup (FWD_REAL / INV_REAL: two image rows each)
    int M, logP;         // plan rows, log2 of the panel width
    size_t pstride;      // panel stride in float2 elements
    const float* src_real; int src_rows, src_cols, src_stride;  // FWD_REAL
    const float2* src_c;  // C2C: row-major M x N; INV_REAL: panel-major spectrum
    int rows_in;          // INV_REAL: spectrum rows read (the others are taken as zero)
    int inverse;          // C2C
    float2* dst_c;        // FWD_REAL / C2C: panel-major spectrum
    float* dst_real; int dst_stride, out_rows, out_cols;  // INV_REAL: raw real plane of the cropped rows x cols
    int mm_rows, mm_cols; float2* mm_part; float scale;    // INV_REAL: min/max window, one partial per workgroup, 1 / (M N)
};
struct MixColArgs {
    MixLen len;           // length M
    int N, logP;
    size_t pstride;
    const float2* src;    // panel-major input
    float2* dst;          // FILTER / FUSED: panel-major (may be src); C2C: row-major M x N
    const float2* filt;   // FUSED: W, panel-major
    float K;              // FILTER
    int rows_in;          // rows of src that hold data (the others are taken as zero)
    int rows_out;         // FUSED: rows written back
    int inverse;          // C2C
    const double* lap;    // FILTER_CLS: the Laplacian table (as launch_cols_panel_cls: M + N doubles)
    double gamma;         // FILTER_CLS
};
// blocks = workgroups (rows / (2 B) or rows / B, rounded up); npanels = N / P
hipError_t launch_mixed_rows(MixRowKind kind, const MixRowArgs& a, int blocks, hipStream_t s);
hipError_t launch_mixed_cols(MixColKind kind, const MixColArgs& a, int npanels, hipStream_t s);

// (fdr_tiled.hip) sectioned restoration (fdr_restore_tiled_f32*): the blend of the staged tile windows into the picture and the roll
// that centres a PSF in a plane.
// What covers one picture row (or column): the first covering tile, how many follow it (0 .. 3; 0 only in the padding of the column
// table) and their normalised weights, in tile order.  Built on the host (fdr_api_tiled.hip), 32 bytes so that an entry is two 16-byte loads.
constexpr int kTiledMaxCover = 3;
struct alignas(16) TiledCover {
    int first, count;
    float w[kTiledMaxCover];
    int pad[3];
};
static_assert(sizeof(TiledCover) == 32, "an entry is two 16-byte loads");
// One axis of the tiling: n tiles of `win` pixels, tile a at min(a step, last)
struct TiledAxis { int n, win, step, last; };
__host__ __device__ __forceinline__ int tiled_origin(const TiledAxis& ax, int a) {
    const long long o = (long long)a * ax.step;
    return o < ax.last ? (int)o : ax.last;
}
// out[y, x] = sum over the covering tile rows a (outer) and tile columns b (inner), ascending, of (Wy_a(y) Wx_b(x)) o_ab[y - y_a, x - x_b],
// every product and sum rounded on its own, from +0.  `stage` holds the windows dense, tile (a, b) at (a ac.n + b) ar.win ac.win;
// rtab has `rows` entries, ctab `cols` rounded up to a multiple of four (count 0 in the padding).  Any out pointer and stride.
hipError_t launch_tiled_blend(const float* stage, const TiledCover* rtab, const TiledCover* ctab, TiledAxis ar, TiledAxis ac, float* out, int rows,
                              int cols, int out_stride, hipStream_t s);
// plane (M x N, dense) = the prows x pcols PSF (row stride pstride) rolled by (-(prows / 2), -(pcols / 2)), zero elsewhere; prows <= M, pcols <= N
hipError_t launch_tiled_psf_centre(const float* psf, int prows, int pcols, int pstride, float* plane, int M, int N, hipStream_t s);

}  // namespace fdr
