// fdr_rlaccel.hip -- the kernels of accelerated Richardson-Lucy (fdr_richardson_lucy_accel_f32*, fdr_richardson_lucy_free_accel_f32*):
// Biggs & Andrews' vector extrapolation (Applied Optics 36, 1997) around the unchanged iteration step of either form,
//
//     k < 2 :  alpha_k = 0;  y_k = u_k
//     k >= 2:  alpha_k = clamp( sum(g_(k-1) g_(k-2)) / sum(g_(k-2) g_(k-2)), 0, FDR_RL_ACCEL_MAX )   (0 for a zero denominator or a
//              quotient that is not finite);  y_k = max(u_k + alpha_k (u_k - u_(k-1)), 0)
//     every k: u_(k+1) = step(y_k);  g_k = u_(k+1) - y_k
//
// Three kernels: the direction (g_k over g_(k-1), and the two inner products as per-workgroup double partials), alpha (one
// workgroup folds the partials in index order, clamps, writes the device scalar) and the extrapolation (reads that scalar).  The
// planes are windows with arbitrary row strides.  A thread owns four consecutive columns of kRaRows rows and adds its products
// in that order whether it loads them as one 16-byte request or as four scalars, so the sums do not depend on the alignment of
// the caller's planes.  No float atomics: every sum runs in a fixed order.
//
// Each kernel has a group form for 2 .. kMaxGroup images per launch (fdr_richardson_lucy_batch_accel_f32*): blockIdx.z is the image,
// the per-image planes travel by value in the argument block and are picked by a select chain on scalars, image z has its own 2 n
// partials at part + z 2 n and its own alpha[z].  Both forms expand the same per-tile code on the same tiling, so an image of a
// group comes out with the bits it gets alone.
#include "fdr_kernels.hpp"

#include <cstdint>

namespace fdr {

constexpr int kRaThreads = 256;
constexpr int kRaCols = 4 * kRaThreads;  // columns of one workgroup: four consecutive ones per thread
constexpr int kRaRows = 8;               // rows of one workgroup

template <bool VEC>
__device__ __forceinline__ float4 ra_load4(const float* row, int x, int cols) {
    if (VEC && x + 4 <= cols) return *reinterpret_cast<const float4*>(row + x);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x < cols) v.x = row[x];
    if (x + 1 < cols) v.y = row[x + 1];
    if (x + 2 < cols) v.z = row[x + 2];
    if (x + 3 < cols) v.w = row[x + 3];
    return v;
}
template <bool VEC>
__device__ __forceinline__ void ra_store4(float* row, int x, int cols, float4 v) {
    if (VEC && x + 4 <= cols) {
        *reinterpret_cast<float4*>(row + x) = v;
        return;
    }
    if (x < cols) row[x] = v.x;
    if (x + 1 < cols) row[x + 1] = v.y;
    if (x + 2 < cols) row[x + 2] = v.z;
    if (x + 3 < cols) row[x + 3] = v.w;
}

// the planes of a group, by value in the argument block.  direction: u1, y (read), g; extrapolation: u1, u0 (read), yw (written).
struct RaPlanes {
    const float* u1[kMaxGroup];
    const float* y[kMaxGroup];
    const float* u0[kMaxGroup];
    float* g[kMaxGroup];
    float* yw[kMaxGroup];
};

// The per-tile code of each kernel is a macro, expanded in the single-image kernel and in its group form: as an inlined function it
// changed the register allocation of the single-image kernels, whose code must stay what it was (tools/kernel_diff.py).  A macro
// takes the operands by the names the kernel gives them and may return from the kernel.

// kRaRows rows (blockIdx.y) of kRaCols columns (blockIdx.x) of the window: g = u1 - y over the previous g (same index), and with
// PARTIALS the workgroup's sum(g_new g_old) to part[b] and sum(g_old g_old) to part[n + b] (double, fixed-order tree),
// b = blockIdx.y * gridDim.x + blockIdx.x.  Without PARTIALS (the first direction of a call) g is written only, not read.
// Columns past `cols` load as zeros and add nothing.
#define FDR_RA_DIRECTION_TILE(u1, u1s, y, ys, g, gs, rows, cols, part, n) \
    do {                                                                                        \
        __shared__ double red[2][kRaThreads];                                                   \
        const int x = blockIdx.x * kRaCols + 4 * (int)threadIdx.x;                              \
        const int r0 = blockIdx.y * kRaRows;                                                    \
        double s_no = 0.0, s_oo = 0.0;                                                          \
        if (x < cols) {                                                                         \
            for (int i = 0; i < kRaRows; ++i) {                                                 \
                const size_t r = (size_t)(r0 + i);                                              \
                if (r0 + i >= rows) break;                                                      \
                const float4 a = ra_load4<VEC>(u1 + r * u1s, x, cols);                          \
                const float4 b = ra_load4<VEC>(y + r * ys, x, cols);                            \
                const float4 gn = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);      \
                if (PARTIALS) {                                                                 \
                    const float4 go = ra_load4<VEC>(g + r * gs, x, cols);                       \
                    s_no += (double)gn.x * (double)go.x;  s_oo += (double)go.x * (double)go.x;  \
                    s_no += (double)gn.y * (double)go.y;  s_oo += (double)go.y * (double)go.y;  \
                    s_no += (double)gn.z * (double)go.z;  s_oo += (double)go.z * (double)go.z;  \
                    s_no += (double)gn.w * (double)go.w;  s_oo += (double)go.w * (double)go.w;  \
                }                                                                               \
                ra_store4<VEC>(g + r * gs, x, cols, gn);                                        \
            }                                                                                   \
        }                                                                                       \
        if (!PARTIALS) return;                                                                  \
        red[0][threadIdx.x] = s_no;                                                             \
        red[1][threadIdx.x] = s_oo;                                                             \
        __syncthreads();                                                                        \
        for (int h = kRaThreads / 2; h > 0; h >>= 1) {                                          \
            if ((int)threadIdx.x < h) {                                                         \
                red[0][threadIdx.x] += red[0][threadIdx.x + h];                                 \
                red[1][threadIdx.x] += red[1][threadIdx.x + h];                                 \
            }                                                                                   \
            __syncthreads();                                                                    \
        }                                                                                       \
        if (threadIdx.x == 0) {                                                                 \
            const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;                       \
            part[b] = red[0][0];                                                                \
            part[(size_t)n + b] = red[1][0];                                                    \
        }                                                                                       \
    } while (0)
template <bool VEC, bool PARTIALS>
__global__ __launch_bounds__(kRaThreads) void rlaccel_direction_kernel(const float* __restrict__ u1, int u1s, const float* __restrict__ y, int ys,
                                                                       float* __restrict__ g, int gs, int rows, int cols,
                                                                       double* __restrict__ part, int n) {
    FDR_RA_DIRECTION_TILE(u1, u1s, y, ys, g, gs, rows, cols, part, n);
}
// the group form: image blockIdx.z on its planes, its partials at part + z 2 n
template <bool VEC, bool PARTIALS>
__global__ __launch_bounds__(kRaThreads) void rlaccel_direction_group_kernel(const RaPlanes pl, int u1s, int ys, int gs, int rows, int cols,
                                                                             double* __restrict__ part0, int n) {
    const int z = blockIdx.z;
    const float* __restrict__ u1 = FDR_PICK_IMAGE(pl.u1, z);
    const float* __restrict__ y = FDR_PICK_IMAGE(pl.y, z);
    float* __restrict__ g = FDR_PICK_IMAGE(pl.g, z);
    double* __restrict__ part = PARTIALS ? part0 + (size_t)z * 2 * (size_t)n : part0;
    FDR_RA_DIRECTION_TILE(u1, u1s, y, ys, g, gs, rows, cols, part, n);
}

// one workgroup: num = sum of part[0 .. n), den = sum of part[n .. 2 n) (thread t adds t, t + 256, ... in order, then a fixed
// tree); alpha = clamp(num / den, 0, max) rounded to float once, 0 for den = 0 or a quotient that is not finite; to *alpha and,
// when `record` is not null, to *record
#define FDR_RA_ALPHA_FOLD(part, n, amax, alpha, record) \
    do {                                                                                                             \
        __shared__ double red[2][kRaThreads];                                                                        \
        double a = 0.0, b = 0.0;                                                                                     \
        for (int k = threadIdx.x; k < n; k += kRaThreads) {                                                          \
            a += part[k];                                                                                            \
            b += part[(size_t)n + k];                                                                                \
        }                                                                                                            \
        red[0][threadIdx.x] = a;                                                                                     \
        red[1][threadIdx.x] = b;                                                                                     \
        __syncthreads();                                                                                             \
        for (int h = kRaThreads / 2; h > 0; h >>= 1) {                                                               \
            if ((int)threadIdx.x < h) {                                                                              \
                red[0][threadIdx.x] += red[0][threadIdx.x + h];                                                      \
                red[1][threadIdx.x] += red[1][threadIdx.x + h];                                                      \
            }                                                                                                        \
            __syncthreads();                                                                                         \
        }                                                                                                            \
        if (threadIdx.x == 0) {                                                                                      \
            const double num = red[0][0], den = red[1][0];                                                           \
            double q = den != 0.0 ? num / den : 0.0;                                                                 \
            if (!(q >= 0.0) || q > 1.7976931348623157e308) q = 0.0;  /* negative, NaN or infinite: no extrapolation */\
            if (q > (double)amax) q = (double)amax;                                                                  \
            const float v = (float)q;                                                                                \
            *alpha = v;                                                                                              \
            if (record) *record = v;                                                                                 \
        }                                                                                                            \
    } while (0)
__global__ __launch_bounds__(kRaThreads) void rlaccel_alpha_kernel(const double* __restrict__ part, int n, float amax, float* __restrict__ alpha,
                                                                   float* __restrict__ record) {
    FDR_RA_ALPHA_FOLD(part, n, amax, alpha, record);
}
// the group form, one workgroup per image (blockIdx.z): its partials at part + z 2 n, to alpha[z] and record[z alpha_pitch]
__global__ __launch_bounds__(kRaThreads) void rlaccel_alpha_group_kernel(const double* __restrict__ part0, int n, float amax,
                                                                         float* __restrict__ alpha0, float* __restrict__ record0,
                                                                         size_t alpha_pitch) {
    const size_t z = blockIdx.z;
    const double* __restrict__ part = part0 + z * 2 * (size_t)n;
    float* __restrict__ alpha = alpha0 + z;
    float* __restrict__ record = record0 ? record0 + z * alpha_pitch : nullptr;
    FDR_RA_ALPHA_FOLD(part, n, amax, alpha, record);
}

// y = max(u1 + alpha (u1 - u0), 0) on the window, alpha from the device scalar; the tiling of the direction kernel
#define FDR_RA_EXTRAPOLATE_TILE(u1, u1s, u0, u0s, alpha, y, ys, rows, cols) \
    do {                                                            \
        const int x = blockIdx.x * kRaCols + 4 * (int)threadIdx.x;  \
        if (x >= cols) return;                                      \
        const float al = *alpha;                                    \
        const int r0 = blockIdx.y * kRaRows;                        \
        for (int i = 0; i < kRaRows; ++i) {                         \
            const size_t r = (size_t)(r0 + i);                      \
            if (r0 + i >= rows) break;                              \
            const float4 a = ra_load4<VEC>(u1 + r * u1s, x, cols);  \
            const float4 b = ra_load4<VEC>(u0 + r * u0s, x, cols);  \
            float4 v;                                               \
            v.x = fmaxf(fmaf(al, a.x - b.x, a.x), 0.f);             \
            v.y = fmaxf(fmaf(al, a.y - b.y, a.y), 0.f);             \
            v.z = fmaxf(fmaf(al, a.z - b.z, a.z), 0.f);             \
            v.w = fmaxf(fmaf(al, a.w - b.w, a.w), 0.f);             \
            ra_store4<VEC>(y + r * ys, x, cols, v);                 \
        }                                                           \
    } while (0)
template <bool VEC>
__global__ __launch_bounds__(kRaThreads) void rlaccel_extrapolate_kernel(const float* __restrict__ u1, int u1s, const float* __restrict__ u0,
                                                                         int u0s, const float* __restrict__ alpha, float* __restrict__ y, int ys,
                                                                         int rows, int cols) {
    FDR_RA_EXTRAPOLATE_TILE(u1, u1s, u0, u0s, alpha, y, ys, rows, cols);
}
// the group form: image blockIdx.z on its planes, with alpha[z]
template <bool VEC>
__global__ __launch_bounds__(kRaThreads) void rlaccel_extrapolate_group_kernel(const RaPlanes pl, int u1s, int u0s, const float* __restrict__ alpha0,
                                                                               int ys, int rows, int cols) {
    const int z = blockIdx.z;
    const float* __restrict__ u1 = FDR_PICK_IMAGE(pl.u1, z);
    const float* __restrict__ u0 = FDR_PICK_IMAGE(pl.u0, z);
    float* __restrict__ y = FDR_PICK_IMAGE(pl.yw, z);
    const float* __restrict__ alpha = alpha0 + z;
    FDR_RA_EXTRAPOLATE_TILE(u1, u1s, u0, u0s, alpha, y, ys, rows, cols);
}

int rlaccel_partials(int rows, int cols) { return ((rows + kRaRows - 1) / kRaRows) * ((cols + kRaCols - 1) / kRaCols); }

namespace {
// 16-byte requests only when every row of every plane starts on a 16-byte boundary
bool ra_vec_ok(const void* a, int as, const void* b, int bs, const void* c, int cs) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0 && ((as | bs | cs) & 3) == 0;
}
dim3 ra_grid(int rows, int cols) { return dim3((unsigned)((cols + kRaCols - 1) / kRaCols), (unsigned)((rows + kRaRows - 1) / kRaRows)); }
}  // namespace

hipError_t launch_rlaccel_direction(const float* u1, int u1s, const float* y, int ys, float* g, int gs, int rows, int cols, double* part,
                                    hipStream_t s) {
    if (rows <= 0 || cols <= 0 || u1s < cols || ys < cols || gs < cols) return hipErrorInvalidValue;
    const bool vec = ra_vec_ok(u1, u1s, y, ys, g, gs);
    const int n = rlaccel_partials(rows, cols);
    const dim3 grid = ra_grid(rows, cols), block(kRaThreads);
    if (part) {
        if (vec) hipLaunchKernelGGL((rlaccel_direction_kernel<true, true>), grid, block, 0, s, u1, u1s, y, ys, g, gs, rows, cols, part, n);
        else hipLaunchKernelGGL((rlaccel_direction_kernel<false, true>), grid, block, 0, s, u1, u1s, y, ys, g, gs, rows, cols, part, n);
    } else {
        if (vec) hipLaunchKernelGGL((rlaccel_direction_kernel<true, false>), grid, block, 0, s, u1, u1s, y, ys, g, gs, rows, cols, part, n);
        else hipLaunchKernelGGL((rlaccel_direction_kernel<false, false>), grid, block, 0, s, u1, u1s, y, ys, g, gs, rows, cols, part, n);
    }
    return hipGetLastError();
}

hipError_t launch_rlaccel_alpha(const double* part, int n, float amax, float* alpha, float* record, hipStream_t s) {
    if (n <= 0 || !part || !alpha) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rlaccel_alpha_kernel, dim3(1), dim3(kRaThreads), 0, s, part, n, amax, alpha, record);
    return hipGetLastError();
}

hipError_t launch_rlaccel_extrapolate(const float* u1, int u1s, const float* u0, int u0s, const float* alpha, float* y, int ys, int rows,
                                      int cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0 || u1s < cols || u0s < cols || ys < cols || !alpha) return hipErrorInvalidValue;
    const dim3 grid = ra_grid(rows, cols), block(kRaThreads);
    if (ra_vec_ok(u1, u1s, u0, u0s, y, ys))
        hipLaunchKernelGGL((rlaccel_extrapolate_kernel<true>), grid, block, 0, s, u1, u1s, u0, u0s, alpha, y, ys, rows, cols);
    else
        hipLaunchKernelGGL((rlaccel_extrapolate_kernel<false>), grid, block, 0, s, u1, u1s, u0, u0s, alpha, y, ys, rows, cols);
    return hipGetLastError();
}

// ---- the group forms: nimg images per launch; one image is the single-image launch ----
namespace {
bool ra_vec_ok_n(int nimg, const float* const* a, int as, const float* const* b, int bs, const float* const* c, int cs) {
    for (int k = 0; k < nimg; ++k)
        if (!ra_vec_ok(a[k], as, b[k], bs, c[k], cs)) return false;
    return true;
}
}  // namespace

hipError_t launch_rlaccel_direction_n(int nimg, const float* const* u1, int u1s, const float* const* y, int ys, float* const* g, int gs, int rows,
                                      int cols, double* part, hipStream_t s) {
    if (nimg < 1 || nimg > kMaxGroup) return hipErrorInvalidValue;
    if (nimg == 1) return launch_rlaccel_direction(u1[0], u1s, y[0], ys, g[0], gs, rows, cols, part, s);
    if (rows <= 0 || cols <= 0 || u1s < cols || ys < cols || gs < cols) return hipErrorInvalidValue;
    RaPlanes pl{};
    for (int k = 0; k < nimg; ++k) { pl.u1[k] = u1[k]; pl.y[k] = y[k]; pl.g[k] = g[k]; }
    const bool vec = ra_vec_ok_n(nimg, u1, u1s, y, ys, g, gs);
    const int n = rlaccel_partials(rows, cols);
    dim3 grid = ra_grid(rows, cols);
    grid.z = (unsigned)nimg;
    const dim3 block(kRaThreads);
    if (part) {
        if (vec) hipLaunchKernelGGL((rlaccel_direction_group_kernel<true, true>), grid, block, 0, s, pl, u1s, ys, gs, rows, cols, part, n);
        else hipLaunchKernelGGL((rlaccel_direction_group_kernel<false, true>), grid, block, 0, s, pl, u1s, ys, gs, rows, cols, part, n);
    } else {
        if (vec) hipLaunchKernelGGL((rlaccel_direction_group_kernel<true, false>), grid, block, 0, s, pl, u1s, ys, gs, rows, cols, part, n);
        else hipLaunchKernelGGL((rlaccel_direction_group_kernel<false, false>), grid, block, 0, s, pl, u1s, ys, gs, rows, cols, part, n);
    }
    return hipGetLastError();
}

hipError_t launch_rlaccel_alpha_n(int nimg, const double* part, int n, float amax, float* alpha, float* record, size_t alpha_pitch, hipStream_t s) {
    if (nimg < 1 || nimg > kMaxGroup) return hipErrorInvalidValue;
    if (nimg == 1) return launch_rlaccel_alpha(part, n, amax, alpha, record, s);
    if (n <= 0 || !part || !alpha) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rlaccel_alpha_group_kernel, dim3(1, 1, (unsigned)nimg), dim3(kRaThreads), 0, s, part, n, amax, alpha, record, alpha_pitch);
    return hipGetLastError();
}

hipError_t launch_rlaccel_extrapolate_n(int nimg, const float* const* u1, int u1s, const float* const* u0, int u0s, const float* alpha,
                                        float* const* y, int ys, int rows, int cols, hipStream_t s) {
    if (nimg < 1 || nimg > kMaxGroup) return hipErrorInvalidValue;
    if (nimg == 1) return launch_rlaccel_extrapolate(u1[0], u1s, u0[0], u0s, alpha, y[0], ys, rows, cols, s);
    if (rows <= 0 || cols <= 0 || u1s < cols || u0s < cols || ys < cols || !alpha) return hipErrorInvalidValue;
    RaPlanes pl{};
    for (int k = 0; k < nimg; ++k) { pl.u1[k] = u1[k]; pl.u0[k] = u0[k]; pl.yw[k] = y[k]; }
    dim3 grid = ra_grid(rows, cols);
    grid.z = (unsigned)nimg;
    const dim3 block(kRaThreads);
    if (ra_vec_ok_n(nimg, u1, u1s, u0, u0s, y, ys))
        hipLaunchKernelGGL((rlaccel_extrapolate_group_kernel<true>), grid, block, 0, s, pl, u1s, u0s, alpha, ys, rows, cols);
    else
        hipLaunchKernelGGL((rlaccel_extrapolate_group_kernel<false>), grid, block, 0, s, pl, u1s, u0s, alpha, ys, rows, cols);
    return hipGetLastError();
}

}  // namespace fdr
