// fdr_tv.hip -- total-variation deconvolution by ADMM (fdr_tv_deconv_f32*; fast panel half-spectrum path), the kernels that are
// not transforms:
//
//     minimise  mu / 2 ||blur(x) - pad(d)||^2 + TV(x)  on the periodic M x N plan
//     n times:  g = D x + w;  z = shrink(g, 1 / rho);  w = g - z;  v = z - w;  rhs = mu b + rho D^T v;
//               x = IDFT2( DFT2(rhs) / (mu |H|^2 + rho L) )
//
// The solve is a blur with a third table (passes A, B' and C unchanged, fdr_api_tv.hip).  Here: the kernel that builds that table
// T = (1 / (M N)) / (mu |H|^2 + rho L) in the layout pass B' reads its filter from, the fused spatial kernel (differences,
// shrinkage, dual update and divergence in one launch), the start x = pad(d), w = 0, and the cropped / clamped output.  The start,
// the spatial kernel and the output have a group form for 2 .. kMaxGroup images per launch (fdr_tv_deconv_batch_f32*; blockIdx.z is
// the image, the per-image code is that of the single kernels), and the spatial kernel a coupled form for the channels of a colour
// picture (vectorial TV: one shrinkage by the joint gradient norm, tv_spatial_coupled_kernel).
#include "fdr_kernels.hpp"

namespace fdr {

// ---- the solve table (tv_quotient: fdr_kernels.hpp) ----
// One thread per row m of a panel p: the four columns 4 p .. 4 p + 3 (v < N/2) of op_h (H / (M N), row m at m * 4) -> T at the
// same place.  Column 0 of panel 0 is the packed DC / Nyquist column; its H slots (packed_column_operator_slot of fdr_rl.hip)
// hold H0[k] for 0 < k < M/2, HN[M - k] for M/2 < k < M and two real values at 0 and M/2, so |H0|^2 and |HN|^2 of the bin a T
// slot stands for come from the H slot at the same k: the pass stays pointwise.
__global__ __launch_bounds__(256) void tv_table_kernel(const float2* __restrict__ op_h, float2* __restrict__ T, const double* __restrict__ lap,
                                                       const int M, const int N, const size_t pstride, const int npanels, const double mu,
                                                       const double rho) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)npanels * M) return;
    const int p = (int)(idx / (size_t)M), m = (int)(idx - (size_t)p * M);
    const double mn = (double)M * (double)N, inv_mn = 1.0 / mn, mn2 = mn * mn;  // powers of two: exact
    const double* a = lap;
    const double* b = lap + M;
    const size_t at = (size_t)p * pstride + (size_t)m * 4;
    const float4 h01 = *reinterpret_cast<const float4*>(op_h + at), h23 = *reinterpret_cast<const float4*>(op_h + at + 2);
    const float2 h[4] = {make_float2(h01.x, h01.y), make_float2(h01.z, h01.w), make_float2(h23.x, h23.y), make_float2(h23.z, h23.w)};
    float2 t[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const double hx = h[l].x, hy = h[l].y;
        if (p == 0 && l == 0) {  // the packed column's slot S[m]
            if (m == 0 || m == M / 2)
                t[l] = make_float2(tv_quotient(hx * hx * mn2, a[m] + b[0], mu, rho, inv_mn), tv_quotient(hy * hy * mn2, a[m] + b[N / 2], mu, rho, inv_mn));
            else if (m < M / 2)
                t[l] = make_float2(tv_quotient((hx * hx + hy * hy) * mn2, a[m] + b[0], mu, rho, inv_mn), 0.f);
            else
                t[l] = make_float2(tv_quotient((hx * hx + hy * hy) * mn2, a[M - m] + b[N / 2], mu, rho, inv_mn), 0.f);
        } else {
            t[l] = make_float2(tv_quotient((hx * hx + hy * hy) * mn2, a[m] + b[4 * p + l], mu, rho, inv_mn), 0.f);
        }
    }
    *reinterpret_cast<float4*>(T + at) = make_float4(t[0].x, t[0].y, t[1].x, t[1].y);
    *reinterpret_cast<float4*>(T + at + 2) = make_float4(t[2].x, t[2].y, t[3].x, t[3].y);
}

hipError_t launch_tv_table(const float2* op_h, float2* T, const double* lap, int M, int N, size_t pstride, int npanels, double mu, double rho,
                           hipStream_t s) {
    if (!op_h || !T || !lap) return hipErrorInvalidValue;
    const size_t count = (size_t)npanels * M;
    hipLaunchKernelGGL(tv_table_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, op_h, T, lap, M, N, pstride, npanels, mu, rho);
    return hipGetLastError();
}

// ---- the start: x = pad(d) over the whole plan, wx = wy = 0 (four pixels of a row per thread) ----
__device__ __forceinline__ void tv_init_row(const float* __restrict__ d, const int rows, const int cols, const int stride, float* __restrict__ x,
                                            float* __restrict__ wx, float* __restrict__ wy, const int N) {
    const int j = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int i = blockIdx.y;
    if (j >= N) return;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < rows) {  // the window's rows have any stride and alignment: scalar loads
        const float* r = d + (size_t)i * stride;
        if (j < cols) v.x = r[j];
        if (j + 1 < cols) v.y = r[j + 1];
        if (j + 2 < cols) v.z = r[j + 2];
        if (j + 3 < cols) v.w = r[j + 3];
    }
    const size_t at = (size_t)i * N + j;
    *reinterpret_cast<float4*>(x + at) = v;
    *reinterpret_cast<float4*>(wx + at) = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(wy + at) = make_float4(0.f, 0.f, 0.f, 0.f);
}
__global__ __launch_bounds__(256) void tv_init_kernel(const float* __restrict__ d, const int rows, const int cols, const int stride,
                                                      float* __restrict__ x, float* __restrict__ wx, float* __restrict__ wy, const int N) {
    tv_init_row(d, rows, cols, stride, x, wx, wy, N);
}
// the group form: image blockIdx.z on its planes
struct TvInitPlanes {
    const float* d[kMaxGroup];
    float* x[kMaxGroup];
    float* wx[kMaxGroup];
    float* wy[kMaxGroup];
};
__global__ __launch_bounds__(256) void tv_init_group_kernel(const TvInitPlanes pl, const int rows, const int cols, const int stride, const int N) {
    const int z = blockIdx.z;
    tv_init_row(FDR_PICK_IMAGE(pl.d, z), rows, cols, stride, FDR_PICK_IMAGE(pl.x, z), FDR_PICK_IMAGE(pl.wx, z), FDR_PICK_IMAGE(pl.wy, z), N);
}

hipError_t launch_tv_init(const float* d, int rows, int cols, int stride, float* x, float* wx, float* wy, int M, int N, hipStream_t s) {
    const int tx = N / 4 < 256 ? N / 4 : 256;
    hipLaunchKernelGGL(tv_init_kernel, dim3((unsigned)(N / 4 / tx), (unsigned)M), dim3(tx), 0, s, d, rows, cols, stride, x, wx, wy, N);
    return hipGetLastError();
}

hipError_t launch_tv_init_n(int nimg, const float* const* d, int rows, int cols, int stride, float* const* x, float* const* wx, float* const* wy,
                            int M, int N, hipStream_t s) {
    if (nimg < 1 || nimg > kMaxGroup) return hipErrorInvalidValue;
    if (nimg == 1) return launch_tv_init(d[0], rows, cols, stride, x[0], wx[0], wy[0], M, N, s);
    TvInitPlanes pl;
    for (int k = 0; k < kMaxGroup; ++k) {
        const int q = k < nimg ? k : 0;
        pl.d[k] = d[q]; pl.x[k] = x[q]; pl.wx[k] = wx[q]; pl.wy[k] = wy[q];
    }
    const int tx = N / 4 < 256 ? N / 4 : 256;
    hipLaunchKernelGGL(tv_init_group_kernel, dim3((unsigned)(N / 4 / tx), (unsigned)M, (unsigned)nimg), dim3(tx), 0, s, pl, rows, cols, stride, N);
    return hipGetLastError();
}

// ---- the output: the window of x (row stride N) to `out`, max(x, 0) with nonneg ----
__device__ __forceinline__ void tv_output_pixel(const float* __restrict__ x, const int N, float* __restrict__ out, const int cols,
                                                const int out_stride, const int nonneg) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = blockIdx.y;
    if (j >= cols) return;
    const float v = x[i * N + j];
    out[i * out_stride + j] = nonneg ? fmaxf(v, 0.f) : v;
}
__global__ __launch_bounds__(256) void tv_output_kernel(const float* __restrict__ x, const int N, float* __restrict__ out, const int cols,
                                                        const int out_stride, const int nonneg) {
    tv_output_pixel(x, N, out, cols, out_stride, nonneg);
}
// the group form: image blockIdx.z
struct TvOutPlanes {
    const float* x[kMaxGroup];
    float* out[kMaxGroup];
};
__global__ __launch_bounds__(256) void tv_output_group_kernel(const TvOutPlanes pl, const int N, const int cols, const int out_stride, const int nonneg) {
    const int z = blockIdx.z;
    tv_output_pixel(FDR_PICK_IMAGE(pl.x, z), N, FDR_PICK_IMAGE(pl.out, z), cols, out_stride, nonneg);
}

hipError_t launch_tv_output(const float* x, int N, float* out, int rows, int cols, int out_stride, int nonneg, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(tv_output_kernel, dim3((unsigned)((cols + 255) / 256), (unsigned)rows), dim3(256), 0, s, x, N, out, cols, out_stride, nonneg);
    return hipGetLastError();
}

hipError_t launch_tv_output_n(int nimg, const float* const* x, int N, float* const* out, int rows, int cols, int out_stride, int nonneg,
                              hipStream_t s) {
    if (nimg < 1 || nimg > kMaxGroup) return hipErrorInvalidValue;
    if (nimg == 1) return launch_tv_output(x[0], N, out[0], rows, cols, out_stride, nonneg, s);
    if (rows <= 0 || cols <= 0) return hipSuccess;
    TvOutPlanes pl;
    for (int k = 0; k < kMaxGroup; ++k) { pl.x[k] = x[k < nimg ? k : 0]; pl.out[k] = out[k < nimg ? k : 0]; }
    hipLaunchKernelGGL(tv_output_group_kernel, dim3((unsigned)((cols + 255) / 256), (unsigned)rows, (unsigned)nimg), dim3(256), 0, s, pl, N, cols,
                       out_stride, nonneg);
    return hipGetLastError();
}

// ---- the fused spatial kernel ----
// The shrinkage of a kernel: isotropic and anisotropic TV of one image, or the joint one of vectorial TV, whose scale
// s = max(1 - t / m, 0), m^2 = the sum over the channels of gx^2 + gy^2, the coupled kernel has computed before it shrinks.
enum TvKind { TV_ISO = 0, TV_ANISO = 1, TV_JOINT = 2 };
// m^2 of one channel at one pixel, and the scale from m^2: the isotropic shrinkage is tv_scale(tv_norm2(gx, gy), t)
__device__ __forceinline__ float tv_norm2(float gx, float gy) { return gx * gx + gy * gy; }
__device__ __forceinline__ float tv_scale(float m2, float t) {
    const float m = sqrtf(m2);
    return m > t ? 1.f - t / m : 0.f;
}
// v = z - w_new = 2 z - g of one pixel from its g = D x + w; the new dual w_new = g - z goes to (nwx, nwy).  `joint` is the scale of
// TV_JOINT; the other kinds do not read it.
template <int KIND>
__device__ __forceinline__ void tv_shrink(float gx, float gy, float t, float joint, float& vx, float& vy, float& nwx, float& nwy) {
    float zx, zy;
    if (KIND == TV_ANISO) {
        zx = copysignf(fmaxf(fabsf(gx) - t, 0.f), gx);
        zy = copysignf(fmaxf(fabsf(gy) - t, 0.f), gy);
    } else {
        const float sc = KIND == TV_JOINT ? joint : tv_scale(tv_norm2(gx, gy), t);
        zx = sc * gx;
        zy = sc * gy;
    }
    nwx = gx - zx; nwy = gy - zy;
    vx = zx - nwx; vy = zy - nwy;
}

// A workgroup of TX x TY threads owns a tile of 4 TY rows x 4 TX columns of the plan (M, N, TX and TY are powers of two and the
// tile divides the plan, so no thread is idle and the periodic wrap is a mask); a thread owns 4 x 4 pixels.
//   x: the thread's 16 values stay in registers and go to LDS together with the tile's halo (one row above, one below, one column
//      left, one right), so every neighbour of x is an LDS read.
//   v: computed for the thread's 16 pixels from its own float4 loads of wx, wy.  The divergence needs vx one pixel to the left and
//      vy one pixel up: inside the 4 x 4 block they are registers, across threads they pass through LDS (the right column and the
//      bottom row of each block), and across tiles the first thread column / row recomputes them from the halo (w read once more
//      there).  The new duals go to the other half of a ping-pong pair, so that halo reads of a neighbouring tile never see a
//      value this launch has written.
// Two barriers, no atomics.  LDS: xs (4 TY + 2) rows of 4 TX + 8 floats (the interior starts at column 4: 16-byte aligned),
// vxr 4 TY x TX, vyb TY x 4 TX.
constexpr int kTvThreads = 256;
constexpr int kTvXsFloats = 5200;  // the largest (4 TY + 2) (4 TX + 8) over TX TY <= 256, TX >= 8: TX = 8, TY = 32

// where a thread stands: its tile (origin i0, j0; th x tw pixels; LDS row stride xst) and its block (rows i .. i + 3, columns
// j .. j + 3), and the masks of the periodic wrap
struct TvTile {
    int TX, TY, tx, ty, tw, th, xst, j0, i0, j, i, mM, mN;
};
__device__ __forceinline__ TvTile tv_tile(const int M, const int N, const int logtx) {
    TvTile g;
    g.TX = 1 << logtx; g.TY = blockDim.x >> logtx;
    g.tx = threadIdx.x & (g.TX - 1); g.ty = threadIdx.x >> logtx;
    g.tw = 4 * g.TX; g.th = 4 * g.TY; g.xst = g.tw + 8;
    g.j0 = blockIdx.x * g.tw; g.i0 = blockIdx.y * g.th;
    g.j = g.j0 + 4 * g.tx; g.i = g.i0 + 4 * g.ty;
    g.mM = M - 1; g.mN = N - 1;
    return g;
}

// x: own block to registers and LDS (LDS row r holds plan row i0 - 1 + r, LDS column c plan column j0 - 4 + c), the halo to LDS;
// xr is [row][col], row 4 = the row below, column 4 = the column to the right, both filled by tv_fetch_x after the barrier
__device__ __forceinline__ void tv_stage_x(const TvTile& g, const float* __restrict__ x, const int N, float* xs, float (&xr)[5][5]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4 q = *reinterpret_cast<const float4*>(x + (size_t)(g.i + r) * N + g.j);
        xr[r][0] = q.x; xr[r][1] = q.y; xr[r][2] = q.z; xr[r][3] = q.w;
        *reinterpret_cast<float4*>(xs + (4 * g.ty + r + 1) * g.xst + 4 + 4 * g.tx) = q;
    }
    if (g.ty == 0) *reinterpret_cast<float4*>(xs + 4 + 4 * g.tx) = *reinterpret_cast<const float4*>(x + (size_t)((g.i0 - 1) & g.mM) * N + g.j);
    if (g.ty == g.TY - 1)
        *reinterpret_cast<float4*>(xs + (g.th + 1) * g.xst + 4 + 4 * g.tx) =
            *reinterpret_cast<const float4*>(x + (size_t)((g.i0 + g.th) & g.mM) * N + g.j);
    for (int r = threadIdx.x; r < 2 * (g.th + 2); r += blockDim.x) {  // the two halo columns, rows i0 - 1 .. i0 + th
        const int rr = r >> 1, right = r & 1;
        const int col = right ? ((g.j0 + g.tw) & g.mN) : ((g.j0 - 1) & g.mN);
        xs[rr * g.xst + (right ? 4 + g.tw : 3)] = x[(size_t)((g.i0 - 1 + rr) & g.mM) * N + col];
    }
}
__device__ __forceinline__ void tv_fetch_x(const TvTile& g, const float* xs, float (&xr)[5][5]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) xr[r][4] = xs[(4 * g.ty + r + 1) * g.xst + 8 + 4 * g.tx];
    const float4 q = *reinterpret_cast<const float4*>(xs + (4 * g.ty + 5) * g.xst + 4 + 4 * g.tx);
    xr[4][0] = q.x; xr[4][1] = q.y; xr[4][2] = q.z; xr[4][3] = q.w;
}
// the duals of the own block
__device__ __forceinline__ void tv_load_w(const TvTile& g, const float* __restrict__ wx, const float* __restrict__ wy, const int N,
                                          float (&wxr)[4][4], float (&wyr)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4 qx = *reinterpret_cast<const float4*>(wx + (size_t)(g.i + r) * N + g.j);
        const float4 qy = *reinterpret_cast<const float4*>(wy + (size_t)(g.i + r) * N + g.j);
        wxr[r][0] = qx.x; wxr[r][1] = qx.y; wxr[r][2] = qx.z; wxr[r][3] = qx.w;
        wyr[r][0] = qy.x; wyr[r][1] = qy.y; wyr[r][2] = qy.z; wyr[r][3] = qy.w;
    }
}
// g = D x + w of the four pixels left of the block (the halo column j0 - 1, rows i .. i + 3): for the tile's first thread column
__device__ __forceinline__ void tv_g_left(const TvTile& g, const float* xs, const float (&xr)[5][5], const float* __restrict__ wx,
                                          const float* __restrict__ wy, const int N, float (&gx)[4], float (&gy)[4]) {
    const int col = (g.j0 - 1) & g.mN;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float xc = xs[(4 * g.ty + r + 1) * g.xst + 3], xd = xs[(4 * g.ty + r + 2) * g.xst + 3];
        const size_t at = (size_t)(g.i + r) * N + col;
        gx[r] = xr[r][0] - xc + wx[at];
        gy[r] = xd - xc + wy[at];
    }
}
// g of the four pixels above the block (the halo row i0 - 1, columns j .. j + 3): for the tile's first thread row
__device__ __forceinline__ void tv_g_up(const TvTile& g, const float* xs, const float (&xr)[5][5], const float* __restrict__ wx,
                                        const float* __restrict__ wy, const int N, float (&gx)[4], float (&gy)[4]) {
    const size_t at = (size_t)((g.i0 - 1) & g.mM) * N + g.j;
    const float4 qx = *reinterpret_cast<const float4*>(wx + at), qy = *reinterpret_cast<const float4*>(wy + at);
    const float4 xu = *reinterpret_cast<const float4*>(xs + 4 + 4 * g.tx);
    const float xur = xs[8 + 4 * g.tx];
    const float xa[5] = {xu.x, xu.y, xu.z, xu.w, xur}, ax[4] = {qx.x, qx.y, qx.z, qx.w}, ay[4] = {qy.x, qy.y, qy.z, qy.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        gx[c] = xa[c + 1] - xa[c] + ax[c];
        gy[c] = xr[0][c] - xa[c] + ay[c];
    }
}

// One image's tile: the body of every spatial kernel.  js, jl, ju: the joint scales of TV_JOINT at the own block, at the four
// pixels to its left (tx == 0) and at the four above it (ty == 0); the other kinds do not read them.  LDS is free again after the
// last barrier inside, except for the reads of vxr / vyb that follow it: a caller that goes on to another image puts a barrier
// between them.
template <int KIND>
__device__ __forceinline__ void tv_spatial_tile(const TvTile& g, float* xs, float* vxr, float* vyb, const float* __restrict__ x,
                                                const float* __restrict__ wx, const float* __restrict__ wy, const float* __restrict__ b,
                                                float* __restrict__ nwx, float* __restrict__ nwy, float* __restrict__ rhs, const int N,
                                                const float mu, const float rho, const float t, const float (&js)[4][4], const float (&jl)[4],
                                                const float (&ju)[4]) {
    float xr[5][5];
    tv_stage_x(g, x, N, xs, xr);
    float wxr[4][4], wyr[4][4];
    tv_load_w(g, wx, wy, N, wxr, wyr);
    __syncthreads();
    tv_fetch_x(g, xs, xr);
    // v on the own block; the new duals leave at once
    float vx[4][4], vy[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float ox[4], oy[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            tv_shrink<KIND>(xr[r][c + 1] - xr[r][c] + wxr[r][c], xr[r + 1][c] - xr[r][c] + wyr[r][c], t, js[r][c], vx[r][c], vy[r][c], ox[c], oy[c]);
        *reinterpret_cast<float4*>(nwx + (size_t)(g.i + r) * N + g.j) = make_float4(ox[0], ox[1], ox[2], ox[3]);
        *reinterpret_cast<float4*>(nwy + (size_t)(g.i + r) * N + g.j) = make_float4(oy[0], oy[1], oy[2], oy[3]);
        vxr[(4 * g.ty + r) * g.TX + g.tx] = vx[r][3];
    }
    *reinterpret_cast<float4*>(vyb + g.ty * g.tw + 4 * g.tx) = make_float4(vy[3][0], vy[3][1], vy[3][2], vy[3][3]);
    // vx one column to the left of the block, vy one row above it
    float vxl[4], vyu[4];
    if (g.tx == 0) {  // across the tile's left edge: from the halo column j0 - 1
        float hx[4], hy[4];
        tv_g_left(g, xs, xr, wx, wy, N, hx, hy);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float uy, ox, oy;
            tv_shrink<KIND>(hx[r], hy[r], t, jl[r], vxl[r], uy, ox, oy);
        }
    }
    if (g.ty == 0) {  // across the tile's top edge: from the halo row i0 - 1
        float hx[4], hy[4];
        tv_g_up(g, xs, xr, wx, wy, N, hx, hy);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float ux, ox, oy;
            tv_shrink<KIND>(hx[c], hy[c], t, ju[c], ux, vyu[c], ox, oy);
        }
    }
    __syncthreads();
    if (g.tx != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) vxl[r] = vxr[(4 * g.ty + r) * g.TX + g.tx - 1];
    }
    if (g.ty != 0) {
        const float4 q = *reinterpret_cast<const float4*>(vyb + (g.ty - 1) * g.tw + 4 * g.tx);
        vyu[0] = q.x; vyu[1] = q.y; vyu[2] = q.z; vyu[3] = q.w;
    }
    // rhs = mu b + rho (Dx^T vx + Dy^T vy),  Dx^T v[i, j] = v[i, j - 1] - v[i, j]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4 q = *reinterpret_cast<const float4*>(b + (size_t)(g.i + r) * N + g.j);
        const float bb[4] = {q.x, q.y, q.z, q.w};
        float o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float left = c == 0 ? vxl[r] : vx[r][c - 1];
            const float up = r == 0 ? vyu[c] : vy[r - 1][c];
            o[c] = mu * bb[c] + rho * ((left - vx[r][c]) + (up - vy[r][c]));
        }
        *reinterpret_cast<float4*>(rhs + (size_t)(g.i + r) * N + g.j) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

template <bool ANISO>
__global__ __launch_bounds__(kTvThreads) void tv_spatial_kernel(const float* __restrict__ x, const float* __restrict__ wx, const float* __restrict__ wy,
                                                                const float* __restrict__ b, float* __restrict__ nwx, float* __restrict__ nwy,
                                                                float* __restrict__ rhs, const int M, const int N, const int logtx, const float mu,
                                                                const float rho, const float t) {
    __shared__ __attribute__((aligned(16))) float xs[kTvXsFloats];
    __shared__ __attribute__((aligned(16))) float vxr[1024];
    __shared__ __attribute__((aligned(16))) float vyb[1024];
    const float no44[4][4] = {}, no4[4] = {};
    tv_spatial_tile<ANISO ? TV_ANISO : TV_ISO>(tv_tile(M, N, logtx), xs, vxr, vyb, x, wx, wy, b, nwx, nwy, rhs, N, mu, rho, t, no44, no4, no4);
}

// the planes of a group: x, the duals and b (read) and the new duals (written) of image k lie k * stride floats behind those of image
// 0 (the TV workspace of the plan), its rhs (written) is rhs[k].  One short pointer array: seven of them do not fit the scalar registers.
struct TvPlanes {
    const float* x;
    const float* wx;
    const float* wy;
    const float* b;
    float* nwx;
    float* nwy;
    size_t stride;
    float* rhs[kMaxGroup];
};

// the group form: image blockIdx.z on its planes, the single kernel's tile on each
template <bool ANISO>
__global__ __launch_bounds__(kTvThreads) void tv_spatial_group_kernel(const TvPlanes pl, const int M, const int N, const int logtx, const float mu,
                                                                      const float rho, const float t) {
    __shared__ __attribute__((aligned(16))) float xs[kTvXsFloats];
    __shared__ __attribute__((aligned(16))) float vxr[1024];
    __shared__ __attribute__((aligned(16))) float vyb[1024];
    const int z = blockIdx.z;
    const float no44[4][4] = {}, no4[4] = {};
    const size_t at = (size_t)z * pl.stride;
    tv_spatial_tile<ANISO ? TV_ANISO : TV_ISO>(tv_tile(M, N, logtx), xs, vxr, vyb, pl.x + at, pl.wx + at, pl.wy + at, pl.b + at, pl.nwx + at,
                                               pl.nwy + at, FDR_PICK_IMAGE(pl.rhs, z), N, mu, rho, t, no44, no4, no4);
}

// Vectorial TV: the nimg images are the channels of one picture and share one shrinkage, z_c = s g_c with s = max(1 - t / m, 0) and
// m^2 = sum over c of gx_c^2 + gy_c^2, added in the order c = 0, 1, ..  A workgroup owns its tile in every channel.  Sweep 1 stages
// each channel's x tile as the single kernel does and adds up m^2 in registers: for the thread's 16 pixels, and, as the single
// kernel recomputes v there, for the 4 pixels left of the tile (tx == 0) and the 4 above it (ty == 0) -- with the same expressions
// for g, so a pixel gets the same m^2 in every workgroup that looks at it.  Sweep 2 is the single kernel's tile per channel with
// the joint scale in place of its own; x and the duals are read a second time (the tile was in cache a moment ago) rather than
// kept: one form for any number of channels, and the LDS of the single kernel.  The new duals go to the other half of each
// channel's ping-pong pair, so no halo read sees a value of this launch.  No atomics; the order of every sum is fixed.
__global__ __launch_bounds__(kTvThreads) void tv_spatial_coupled_kernel(const TvPlanes pl, const int nimg, const int M, const int N,
                                                                        const int logtx, const float mu, const float rho, const float t) {
    __shared__ __attribute__((aligned(16))) float xs[kTvXsFloats];
    __shared__ __attribute__((aligned(16))) float vxr[1024];
    __shared__ __attribute__((aligned(16))) float vyb[1024];
    const TvTile g = tv_tile(M, N, logtx);
    float js[4][4] = {}, jl[4] = {}, ju[4] = {};
    for (int c = 0; c < nimg; ++c) {  // sweep 1: m^2
        const float* x = pl.x + (size_t)c * pl.stride;
        const float* wx = pl.wx + (size_t)c * pl.stride;
        const float* wy = pl.wy + (size_t)c * pl.stride;
        float xr[5][5];
        tv_stage_x(g, x, N, xs, xr);
        float wxr[4][4], wyr[4][4];
        tv_load_w(g, wx, wy, N, wxr, wyr);
        __syncthreads();
        tv_fetch_x(g, xs, xr);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float q = tv_norm2(xr[r][k + 1] - xr[r][k] + wxr[r][k], xr[r + 1][k] - xr[r][k] + wyr[r][k]);
                js[r][k] = c == 0 ? q : js[r][k] + q;
            }
        if (g.tx == 0) {
            float hx[4], hy[4];
            tv_g_left(g, xs, xr, wx, wy, N, hx, hy);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float q = tv_norm2(hx[r], hy[r]);
                jl[r] = c == 0 ? q : jl[r] + q;
            }
        }
        if (g.ty == 0) {
            float hx[4], hy[4];
            tv_g_up(g, xs, xr, wx, wy, N, hx, hy);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float q = tv_norm2(hx[k], hy[k]);
                ju[k] = c == 0 ? q : ju[k] + q;
            }
        }
        __syncthreads();  // xs is read no more: the next channel may stage
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) js[r][k] = tv_scale(js[r][k], t);
        jl[r] = tv_scale(jl[r], t);
        ju[r] = tv_scale(ju[r], t);
    }
    for (int c = 0; c < nimg; ++c) {  // sweep 2: shrink, duals, divergence, rhs per channel
        const size_t at = (size_t)c * pl.stride;
        tv_spatial_tile<TV_JOINT>(g, xs, vxr, vyb, pl.x + at, pl.wx + at, pl.wy + at, pl.b + at, pl.nwx + at, pl.nwy + at, FDR_PICK_IMAGE(pl.rhs, c), N,
                                  mu, rho, t, js, jl, ju);
        __syncthreads();  // vxr and vyb are read no more
    }
}

// tile geometry of an M x N plan (M >= 8, N >= 32, powers of two): TX = min(64, N / 4) thread columns, TY = min(256 / TX, M / 4)
static bool tv_geometry(int M, int N, int* logtx, int* TX, int* TY) {
    if (M < 8 || N < 32 || (M & (M - 1)) || (N & (N - 1))) return false;
    *logtx = 6;
    while ((4 << *logtx) > N) --*logtx;
    *TX = 1 << *logtx;
    *TY = kTvThreads / *TX;
    if (*TY > M / 4) *TY = M / 4;
    return (4 * *TY + 2) * (4 * *TX + 8) <= kTvXsFloats && 4 * *TY * *TX <= 1024;
}

// a group of 1 <= nimg <= kMaxGroup images in one launch: the planes of image k lie k * stride floats behind those given.  Uncoupled: blockIdx.z = image, every image with the bits of the single
// launch (one image is that launch).  Coupled: the images are the channels of one picture (isotropic only), one workgroup per tile.
hipError_t launch_tv_spatial_n(int nimg, const float* x, const float* wx, const float* wy, const float* b, float* nwx, float* nwy, size_t stride,
                               float* const* rhs, int M, int N, float mu, float rho, int anisotropic, int coupled, hipStream_t s) {
    if (nimg < 1 || nimg > kMaxGroup || (coupled && anisotropic)) return hipErrorInvalidValue;
    if (nimg == 1 && !coupled) return launch_tv_spatial(x, wx, wy, b, nwx, nwy, rhs[0], M, N, mu, rho, anisotropic, s);
    int logtx, TX, TY;
    if (!tv_geometry(M, N, &logtx, &TX, &TY)) return hipErrorInvalidValue;
    TvPlanes pl = {x, wx, wy, b, nwx, nwy, stride, {}};
    for (int k = 0; k < kMaxGroup; ++k) pl.rhs[k] = rhs[k < nimg ? k : 0];
    const float t = 1.f / rho;
    const dim3 tiles((unsigned)(N / (4 * TX)), (unsigned)(M / (4 * TY)));
    const dim3 grid(tiles.x, tiles.y, (unsigned)nimg);
    if (coupled)
        hipLaunchKernelGGL(tv_spatial_coupled_kernel, tiles, dim3(TX * TY), 0, s, pl, nimg, M, N, logtx, mu, rho, t);
    else if (anisotropic)
        hipLaunchKernelGGL((tv_spatial_group_kernel<true>), grid, dim3(TX * TY), 0, s, pl, M, N, logtx, mu, rho, t);
    else
        hipLaunchKernelGGL((tv_spatial_group_kernel<false>), grid, dim3(TX * TY), 0, s, pl, M, N, logtx, mu, rho, t);
    return hipGetLastError();
}

hipError_t launch_tv_spatial(const float* x, const float* wx, const float* wy, const float* b, float* nwx, float* nwy, float* rhs, int M, int N,
                             float mu, float rho, int anisotropic, hipStream_t s) {
    int logtx, TX, TY;
    if (!tv_geometry(M, N, &logtx, &TX, &TY)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(N / (4 * TX)), (unsigned)(M / (4 * TY)));
    const float t = 1.f / rho;
    if (anisotropic)
        hipLaunchKernelGGL((tv_spatial_kernel<true>), grid, dim3(TX * TY), 0, s, x, wx, wy, b, nwx, nwy, rhs, M, N, logtx, mu, rho, t);
    else
        hipLaunchKernelGGL((tv_spatial_kernel<false>), grid, dim3(TX * TY), 0, s, x, wx, wy, b, nwx, nwy, rhs, M, N, logtx, mu, rho, t);
    return hipGetLastError();
}

}  // namespace fdr
