// fdr_register.hip -- registering the frames of a burst (fdr_register_frames_f32*): the translation of frame k against the reference
// frame by PSF-aware phase correlation, and the bilinear shift of a PSF (fdr_psf_shift_f32*) that puts the estimate into the frame's PSF.
//
//     a = pad(w . d_ref),  b = pad(w . d_k)          w = hann(rows) hann(cols)^T, the tables of fdr_motion.hip
//     G_a = DFT2(a), G_b = DFT2(b);  H_a = DFT2(pad(p_ref)), H_b = DFT2(pad(p_k))     (both 1 without PSFs)
//     C   = conj(G_a) G_b H_a conj(H_b)              = |H_a|^2 |H_b|^2 |X|^2 e^{-i w.s}: the phases of the PSFs cancel
//     Chat = C / (|C| + eps_rel mean |C|),  r = Re IDFT2(Chat)                        (IDFT2 includes 1 / (M N))
//     (i*, j*) = argmax r over |dy| <= R_r, |dx| <= R_c (periodic; exact ties: the lowest (dy + R_r) (2 R_c + 1) + dx + R_c)
//     dy = i* + parabola(r[i* - 1, j*], r[i*, j*], r[i* + 1, j*]),  dx likewise;  confidence = (r_peak - mean r) / std r
//
// Passes per frame k != reference: the pair window pass (z = w d_ref + i w d_k: two real pictures ride one complex transform) and,
// with PSFs, the same pass without a window on (p_ref, p_k); the plan's complex 2-D transform of both planes; the cross-power pass,
// one lane per bin pair (f, -f); a fixed-order fold of its sum |C| partials; the normalising sweep; the inverse transform; the peak
// pass and its one-workgroup fold.  No atomics: every reduction runs in a fixed order, so results are bit-identical from call to call.
//
// The float formulas (every product and sum rounded separately: this file is compiled without contraction).  With z = Z(f), y = Z(-f)
// of the transformed picture pair, -f = ((M - u) % M, (N - v) % N):
//     A = (0.5 (z.x + y.x), 0.5 (z.y - y.y))          = G_a(f)
//     B = (0.5 (z.y + y.y), 0.5 (y.x - z.x))          = G_b(f)
//     T = (A.x B.x + A.y B.y,  A.x B.y - A.y B.x)     = conj(G_a) G_b
// H_a, H_b from the transformed PSF pair in the same way, Q = (Ha.x Hb.x + Ha.y Hb.y,  Ha.y Hb.x - Ha.x Hb.y) = H_a conj(H_b), or (1, 0),
//     C(f) = (T.x Q.x - T.y Q.y,  T.x Q.y + T.y Q.x),   C(-f) = conj C(f),   |C| = sqrt((double)C.x^2 + (double)C.y^2) in double
// (|G|^4 leaves the float range for an 8-bit 8192^2 picture; the double magnitude does not).  sum |C| over all M N bins in double, a
// bin pair counted as |C| + |C|, a self-paired bin once.  With e = (double)eps_rel (sum / (M N)):
//     den = (float)(|C| + e);  Chat / (M N) = ((C.x / den) inv_mn, (C.y / den) inv_mn),   inv_mn = (float)(1 / (double)(M N))
// and 0 where den = 0, and everywhere when the sum is 0 or one of the two windowed pictures is all zero (told from sum |w d| of the pair
// pass: the pair transform leaks round-off of one picture into the other's spectrum, so sum |C| cannot tell).  The peak is taken from
// the float real parts; the parabola, mean and deviation are formed in double from them:  off = 0.5 (m - p) / (m - 2 z + p), 0 for a
// denominator of 0, clamped to [-0.5, 0.5].
#include "fdr_kernels.hpp"

#include <climits>

namespace fdr {

constexpr int kRgThreads = 256;
constexpr int kRgCols = 4 * kRgThreads;  // columns of one workgroup of the pair and peak passes (4 per thread, 256 apart: coalesced)

// the workgroup's double sum in a fixed tree; every thread returns it
__device__ __forceinline__ double register_block_sum(double acc, double* red) {
    __syncthreads();  // (a sum before this one may still be read)
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = kRgThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    return red[0];
}

// one row (blockIdx.y) of kRgCols columns (blockIdx.x) of the M x N plane: (w . a, w . b) on the window, 0 elsewhere; hann null: w = 1.
// part not null: the workgroup's sum |w a| and sum |w b| (double, fixed tree) to part[2 g], part[2 g + 1]
__global__ __launch_bounds__(kRgThreads) void register_pair_kernel(const float* __restrict__ a, const float* __restrict__ b, int rows, int cols,
                                                                   int stride, const float* __restrict__ hann, float2* __restrict__ plane,
                                                                   int N, double* __restrict__ part) {
    __shared__ double red[kRgThreads];
    double sa = 0.0, sb = 0.0;
    const int i = blockIdx.y;
    const bool in_rows = i < rows;
    const float hr = in_rows && hann ? hann[i] : 1.f;
    const size_t row = (size_t)(in_rows ? i : 0) * stride;
    float2* dst = plane + (size_t)i * N;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = blockIdx.x * kRgCols + k * kRgThreads + threadIdx.x;
        if (j >= N) break;
        float2 v = make_float2(0.f, 0.f);
        if (in_rows && j < cols) {
            const float w = hann ? hr * hann[rows + j] : 1.f;
            v = make_float2(w * a[row + j], w * b[row + j]);
        }
        sa += (double)fabsf(v.x);
        sb += (double)fabsf(v.y);
        dst[j] = v;
    }
    if (!part) return;
    const double ta = register_block_sum(sa, red), tb = register_block_sum(sb, red);
    if (threadIdx.x == 0) {
        const size_t g = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[2 * g] = ta; part[2 * g + 1] = tb;
    }
}

// one workgroup: *gate = 1 when both pictures of the pair have a sample that is not 0 under the window, else 0 (the n pairs of partials
// folded: thread t takes t, t + 256, .. in order, then a fixed tree).  The pair transform leaks round-off of one picture into the
// spectrum of the other, so an all-zero frame is told here, where it is exact, and not from sum |C|
__global__ __launch_bounds__(kRgThreads) void register_gate_kernel(const double* __restrict__ part, int n, double* __restrict__ gate) {
    __shared__ double red[kRgThreads];
    double sa = 0.0, sb = 0.0;
    for (int k = threadIdx.x; k < n; k += kRgThreads) { sa += part[2 * (size_t)k]; sb += part[2 * (size_t)k + 1]; }
    const double ta = register_block_sum(sa, red), tb = register_block_sum(sb, red);
    if (threadIdx.x == 0) *gate = ta > 0.0 && tb > 0.0 ? 1.0 : 0.0;
}

// the two real spectra that ride one complex transform, at bin f: z = Z(f), y = Z(-f)
__device__ __forceinline__ void register_split(float2 z, float2 y, float2& A, float2& B) {
    A = make_float2(0.5f * (z.x + y.x), 0.5f * (z.y - y.y));
    B = make_float2(0.5f * (z.y + y.y), 0.5f * (y.x - z.x));
}

// One lane per bin pair (f, -f): row u = blockIdx.y of the upper half (0 .. M / 2), column v.  The rows 0 and (M even) M / 2 pair with
// themselves: there the lanes v <= (N - v) % N do the work, and v = 0 and (N even) v = N / 2 are the self-paired bins, written once.
// Both reads of a wave are contiguous (ascending at f, descending at -f), and the lane owns both bins, so C replaces Z in place.
__global__ __launch_bounds__(kRgThreads) void register_cross_kernel(float2* __restrict__ Z, const float2* __restrict__ P, int M, int N,
                                                                    double* __restrict__ part) {
    __shared__ double red[kRgThreads];
    const int u = blockIdx.y, v = blockIdx.x * kRgThreads + threadIdx.x;
    const int u2 = u ? M - u : 0;
    double acc = 0.0;
    if (v < N) {
        const int v2 = v ? N - v : 0;
        if (!(u2 == u && v2 < v)) {
            const bool self = u2 == u && v2 == v;
            const size_t k1 = (size_t)u * N + v, k2 = (size_t)u2 * N + v2;
            float2 A, B;
            register_split(Z[k1], Z[k2], A, B);
            const float2 T = make_float2(A.x * B.x + A.y * B.y, A.x * B.y - A.y * B.x);
            float2 C = T;
            if (P) {
                float2 Ha, Hb;
                register_split(P[k1], P[k2], Ha, Hb);
                const float2 Q = make_float2(Ha.x * Hb.x + Ha.y * Hb.y, Ha.y * Hb.x - Ha.x * Hb.y);
                C = make_float2(T.x * Q.x - T.y * Q.y, T.x * Q.y + T.y * Q.x);
            }
            const double mag = sqrt((double)C.x * (double)C.x + (double)C.y * (double)C.y);
            Z[k1] = C;
            if (self) {
                acc = mag;
            } else {
                Z[k2] = make_float2(C.x, -C.y);
                acc = mag + mag;
            }
        }
    }
    const double sum = register_block_sum(acc, red);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// C -> C / (|C| + eps_rel mean |C|) / (M N) in place; 0 where the denominator is 0 and everywhere for an all-zero frame (sum 0 or gate 0)
__global__ __launch_bounds__(kRgThreads) void register_normalize_kernel(float2* __restrict__ plane, size_t count, const double* __restrict__ sum,
                                                                        float eps_rel, float inv_mn) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const double s = sum[1] > 0.0 ? sum[0] : 0.0;  // (sum[1]: the gate)
    const double e = (double)eps_rel * (s / (double)count);
    const float2 c = plane[k];
    const double mag = sqrt((double)c.x * (double)c.x + (double)c.y * (double)c.y);
    const float den = (float)(mag + e);
    float2 out = make_float2(0.f, 0.f);
    if (s > 0.0 && den > 0.f) out = make_float2((c.x / den) * inv_mn, (c.y / den) * inv_mn);
    plane[k] = out;
}

// the better of two candidates (value, index of the search window): the larger value, on an exact tie the lower index
__device__ __forceinline__ bool register_better(float v, int idx, float bv, int bidx) { return v > bv || (v == bv && idx < bidx); }

// one row (blockIdx.y) of kRgCols columns (blockIdx.x): the workgroup's sum r, sum r^2 (double, fixed tree) and its best candidate of
// the search window to part[4 w .. 4 w + 3] (value and window index as doubles; index INT_MAX: none)
__global__ __launch_bounds__(kRgThreads) void register_peak_kernel(const float2* __restrict__ plane, int M, int N, int Rr, int Rc,
                                                                   double* __restrict__ part) {
    __shared__ double red[kRgThreads];
    __shared__ float bestv[kRgThreads];
    __shared__ int besti[kRgThreads];
    const int i = blockIdx.y;
    const int dy = i <= Rr ? i : i - M;  // (R_r < M / 2: at most one of the two lies in the range)
    const bool row_in = dy >= -Rr && dy <= Rr;
    const float2* src = plane + (size_t)i * N;
    double s1 = 0.0, s2 = 0.0;
    float bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = blockIdx.x * kRgCols + k * kRgThreads + threadIdx.x;
        if (j >= N) break;
        const float r = src[j].x;
        s1 += (double)r;
        s2 += (double)r * (double)r;
        const int dx = j <= Rc ? j : j - N;
        if (row_in && dx >= -Rc && dx <= Rc) {
            const int idx = (dy + Rr) * (2 * Rc + 1) + dx + Rc;
            if (register_better(r, idx, bv, bi)) { bv = r; bi = idx; }
        }
    }
    const double t1 = register_block_sum(s1, red), t2 = register_block_sum(s2, red);
    bestv[threadIdx.x] = bv;
    besti[threadIdx.x] = bi;
    __syncthreads();
    for (int h = kRgThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h && register_better(bestv[threadIdx.x + h], besti[threadIdx.x + h], bestv[threadIdx.x], besti[threadIdx.x])) {
            bestv[threadIdx.x] = bestv[threadIdx.x + h];
            besti[threadIdx.x] = besti[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = part + 4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = t1; o[1] = t2; o[2] = (double)bestv[0]; o[3] = (double)besti[0];
    }
}

__device__ __forceinline__ double register_parabola(float m, float z, float p) {
    const double den = (double)m - 2.0 * (double)z + (double)p;
    if (den == 0.0) return 0.0;
    const double off = 0.5 * ((double)m - (double)p) / den;
    return off < -0.5 ? -0.5 : off > 0.5 ? 0.5 : off;  // (a NaN stays one: the caller's data held one)
}

__device__ __forceinline__ void register_store(void* result, double dy, double dx, float peak, float confidence) {
    double* d = static_cast<double*>(result);
    float* f = reinterpret_cast<float*>(d + 2);
    d[0] = dy; d[1] = dx; f[0] = peak; f[1] = confidence;
}

// one workgroup: the n partials folded (thread t takes t, t + 256, .. in order, then a fixed tree; the better candidate is the same
// whatever the order), the four neighbours of the peak, the parabolas and the result
__global__ __launch_bounds__(kRgThreads) void register_pick_kernel(const float2* __restrict__ plane, int M, int N, int Rr, int Rc,
                                                                   const double* __restrict__ sum, const double* __restrict__ part, int n,
                                                                   void* __restrict__ result) {
    __shared__ double red[kRgThreads];
    __shared__ float bestv[kRgThreads];
    __shared__ int besti[kRgThreads];
    double s1 = 0.0, s2 = 0.0;
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int k = threadIdx.x; k < n; k += kRgThreads) {
        const double* o = part + 4 * (size_t)k;
        s1 += o[0];
        s2 += o[1];
        const float v = (float)o[2];
        const int idx = (int)o[3];
        if (register_better(v, idx, bv, bi)) { bv = v; bi = idx; }
    }
    const double t1 = register_block_sum(s1, red), t2 = register_block_sum(s2, red);
    bestv[threadIdx.x] = bv;
    besti[threadIdx.x] = bi;
    __syncthreads();
    for (int h = kRgThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h && register_better(bestv[threadIdx.x + h], besti[threadIdx.x + h], bestv[threadIdx.x], besti[threadIdx.x])) {
            bestv[threadIdx.x] = bestv[threadIdx.x + h];
            besti[threadIdx.x] = besti[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const int idx = besti[0];
    if (!(sum[0] > 0.0 && sum[1] > 0.0) || idx == INT_MAX) {  // an all-zero frame (or data without a single comparable value): the defined zero result
        register_store(result, 0.0, 0.0, 0.f, 0.f);
        return;
    }
    const int wc = 2 * Rc + 1;
    const int dy = idx / wc - Rr, dx = idx % wc - Rc;
    const int i = dy < 0 ? dy + M : dy, j = dx < 0 ? dx + N : dx;
    const int iu = i == 0 ? M - 1 : i - 1, id = i + 1 == M ? 0 : i + 1;
    const int jl = j == 0 ? N - 1 : j - 1, jr = j + 1 == N ? 0 : j + 1;
    const float z = plane[(size_t)i * N + j].x;
    const double oy = register_parabola(plane[(size_t)iu * N + j].x, z, plane[(size_t)id * N + j].x);
    const double ox = register_parabola(plane[(size_t)i * N + jl].x, z, plane[(size_t)i * N + jr].x);
    const double cnt = (double)M * (double)N;
    const double mean = t1 / cnt, var = t2 / cnt - mean * mean;
    const double sd = var > 0.0 ? sqrt(var) : 0.0;
    register_store(result, (double)dy + oy, (double)dx + ox, z, sd > 0.0 ? (float)(((double)z - mean) / sd) : 0.f);
}

__global__ void register_reference_kernel(void* result) { register_store(result, 0.0, 0.0, 1.f, 0.f); }

// One lane per element (oi, oj) of frame blockIdx.z's output, (prows + 2 pad_rows) x (pcols + 2 pad_cols): a gather of the four taps
// whose bilinear footprint covers it.  With (dy, dx) the frame's shift (NaN: 0; clamped to [-pad, pad - 1], so that no value in device
// memory indexes outside the planes), fy0 = floor(dy), fy = dy - fy0 in double (fx alike) and the weights rounded once,
//     w00 = (float)((1 - fy) (1 - fx)), w01 = (float)((1 - fy) fx), w10 = (float)(fy (1 - fx)), w11 = (float)(fy fx),
// and si = oi - pad_rows - fy0, sj = oj - pad_cols - fx0, p = 0 outside the PSF:
//     out = ((w00 p[si, sj] + w01 p[si, sj - 1]) + w10 p[si - 1, sj]) + w11 p[si - 1, sj - 1]      (float, no contraction)
__global__ __launch_bounds__(kRgThreads) void psf_shift_kernel(const float* __restrict__ psfs, size_t psf_pitch, int prows, int pcols, int pstride,
                                                               const char* __restrict__ shifts, int pad_rows, int pad_cols, float* __restrict__ out,
                                                               size_t out_pitch, int out_stride) {
    const int orows = prows + 2 * pad_rows, ocols = pcols + 2 * pad_cols;
    const int oj = blockIdx.x * kRgThreads + threadIdx.x, oi = blockIdx.y, k = blockIdx.z;
    if (oj >= ocols || oi >= orows) return;
    const double* sh = reinterpret_cast<const double*>(shifts + (size_t)k * 24);
    double dy = sh[0], dx = sh[1];
    if (!(dy == dy)) dy = 0.0;
    if (!(dx == dx)) dx = 0.0;
    dy = dy < -(double)pad_rows ? -(double)pad_rows : dy > (double)(pad_rows - 1) ? (double)(pad_rows - 1) : dy;
    dx = dx < -(double)pad_cols ? -(double)pad_cols : dx > (double)(pad_cols - 1) ? (double)(pad_cols - 1) : dx;
    const double fy0 = floor(dy), fx0 = floor(dx);
    const double fy = dy - fy0, fx = dx - fx0;
    const float w00 = (float)((1.0 - fy) * (1.0 - fx)), w01 = (float)((1.0 - fy) * fx);
    const float w10 = (float)(fy * (1.0 - fx)), w11 = (float)(fy * fx);
    const int si = oi - pad_rows - (int)fy0, sj = oj - pad_cols - (int)fx0;
    const float* p = psfs + (size_t)k * psf_pitch;
    const auto tap = [&](int i, int j) { return i >= 0 && i < prows && j >= 0 && j < pcols ? p[(size_t)i * pstride + j] : 0.f; };
    float acc = w00 * tap(si, sj);
    acc = acc + w01 * tap(si, sj - 1);
    acc = acc + w10 * tap(si - 1, sj);
    acc = acc + w11 * tap(si - 1, sj - 1);
    out[(size_t)k * out_pitch + (size_t)oi * out_stride + oj] = acc;
}

int register_cross_partials(int M, int N) { return (M / 2 + 1) * ((N + kRgThreads - 1) / kRgThreads); }
int register_peak_partials(int M, int N) { return M * ((N + kRgCols - 1) / kRgCols); }

hipError_t launch_register_pair(const float* a, const float* b, int rows, int cols, int stride, const float* hann, float2* plane, int M, int N,
                                double* part, double* gate, hipStream_t s) {
    const dim3 grid((unsigned)((N + kRgCols - 1) / kRgCols), (unsigned)M);
    hipLaunchKernelGGL(register_pair_kernel, grid, dim3(kRgThreads), 0, s, a, b, rows, cols, stride, hann, plane, N, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !part) return e;
    hipLaunchKernelGGL(register_gate_kernel, dim3(1), dim3(kRgThreads), 0, s, (const double*)part, register_peak_partials(M, N), gate);
    return hipGetLastError();
}

hipError_t launch_register_cross(float2* Z, const float2* P, int M, int N, double* part, hipStream_t s) {
    const dim3 grid((unsigned)((N + kRgThreads - 1) / kRgThreads), (unsigned)(M / 2 + 1));
    hipLaunchKernelGGL(register_cross_kernel, grid, dim3(kRgThreads), 0, s, Z, P, M, N, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_motion_fold(part, register_cross_partials(M, N), s);
}

hipError_t launch_register_normalize(float2* plane, int M, int N, const double* sum, float eps_rel, hipStream_t s) {
    const size_t count = (size_t)M * N;
    const float inv_mn = (float)(1.0 / (double)count);
    hipLaunchKernelGGL(register_normalize_kernel, dim3((unsigned)((count + kRgThreads - 1) / kRgThreads)), dim3(kRgThreads), 0, s, plane, count,
                       sum, eps_rel, inv_mn);
    return hipGetLastError();
}

hipError_t launch_register_peak(const float2* plane, int M, int N, int range_rows, int range_cols, const double* sum, double* part, void* result,
                                hipStream_t s) {
    const dim3 grid((unsigned)((N + kRgCols - 1) / kRgCols), (unsigned)M);
    hipLaunchKernelGGL(register_peak_kernel, grid, dim3(kRgThreads), 0, s, plane, M, N, range_rows, range_cols, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(register_pick_kernel, dim3(1), dim3(kRgThreads), 0, s, plane, M, N, range_rows, range_cols, sum, (const double*)part,
                       register_peak_partials(M, N), result);
    return hipGetLastError();
}

hipError_t launch_register_reference(void* result, hipStream_t s) {
    hipLaunchKernelGGL(register_reference_kernel, dim3(1), dim3(1), 0, s, result);
    return hipGetLastError();
}

hipError_t launch_psf_shift(const float* psfs, size_t psf_pitch, int count, int prows, int pcols, int pstride, const void* shifts, int pad_rows,
                            int pad_cols, float* out, size_t out_pitch, int out_stride, hipStream_t s) {
    const int orows = prows + 2 * pad_rows, ocols = pcols + 2 * pad_cols;
    const dim3 grid((unsigned)((ocols + kRgThreads - 1) / kRgThreads), (unsigned)orows, (unsigned)count);
    hipLaunchKernelGGL(psf_shift_kernel, grid, dim3(kRgThreads), 0, s, psfs, psf_pitch, prows, pcols, pstride, static_cast<const char*>(shifts),
                       pad_rows, pad_cols, out, out_pitch, out_stride);
    return hipGetLastError();
}

}  // namespace fdr
