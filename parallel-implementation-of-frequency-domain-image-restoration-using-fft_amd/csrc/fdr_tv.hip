// fdr_tv.hip -- total-variation deconvolution by ADMM (fdr_tv_deconv_f32*; fast panel half-spectrum path), the kernels that are
// not transforms:
//
//     minimise  mu / 2 ||blur(x) - pad(d)||^2 + TV(x)  on the periodic M x N plan
//     n times:  g = D x + w;  z = shrink(g, 1 / rho);  w = g - z;  v = z - w;  rhs = mu b + rho D^T v;
//               x = IDFT2( DFT2(rhs) / (mu |H|^2 + rho L) )
//
// The solve is a blur with a third table (passes A, B' and C unchanged, fdr_api_tv.hip).  Here: the kernel that builds that table
// T = (1 / (M N)) / (mu |H|^2 + rho L) in the layout pass B' reads its filter from, the fused spatial kernel (differences,
// shrinkage, dual update and divergence in one launch), the start x = pad(d), w = 0, and the cropped / clamped output.
#include "fdr_kernels.hpp"

namespace fdr {

// ---- the solve table ----
// (1 / (M N)) / (mu h2 + rho lap) in double, rounded once; a zero (or negative) denominator gives 0, as the CLS filter does
__device__ __forceinline__ float tv_quotient(double h2, double lap, double mu, double rho, double inv_mn) {
    const double den = mu * h2 + rho * lap;
    return den > 0.0 ? (float)(inv_mn / den) : 0.f;
}

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
__global__ __launch_bounds__(256) void tv_init_kernel(const float* __restrict__ d, const int rows, const int cols, const int stride,
                                                      float* __restrict__ x, float* __restrict__ wx, float* __restrict__ wy, const int N) {
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

hipError_t launch_tv_init(const float* d, int rows, int cols, int stride, float* x, float* wx, float* wy, int M, int N, hipStream_t s) {
    const int tx = N / 4 < 256 ? N / 4 : 256;
    hipLaunchKernelGGL(tv_init_kernel, dim3((unsigned)(N / 4 / tx), (unsigned)M), dim3(tx), 0, s, d, rows, cols, stride, x, wx, wy, N);
    return hipGetLastError();
}

// ---- the output: the window of x (row stride N) to `out`, max(x, 0) with nonneg ----
__global__ __launch_bounds__(256) void tv_output_kernel(const float* __restrict__ x, const int N, float* __restrict__ out, const int cols,
                                                        const int out_stride, const int nonneg) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = blockIdx.y;
    if (j >= cols) return;
    const float v = x[i * N + j];
    out[i * out_stride + j] = nonneg ? fmaxf(v, 0.f) : v;
}

hipError_t launch_tv_output(const float* x, int N, float* out, int rows, int cols, int out_stride, int nonneg, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(tv_output_kernel, dim3((unsigned)((cols + 255) / 256), (unsigned)rows), dim3(256), 0, s, x, N, out, cols, out_stride, nonneg);
    return hipGetLastError();
}

// ---- the fused spatial kernel ----
// v = z - w_new = 2 z - g of one pixel from its g = D x + w; the new dual w_new = g - z goes to (nwx, nwy).
template <bool ANISO>
__device__ __forceinline__ void tv_shrink(float gx, float gy, float t, float& vx, float& vy, float& nwx, float& nwy) {
    float zx, zy;
    if (ANISO) {
        zx = copysignf(fmaxf(fabsf(gx) - t, 0.f), gx);
        zy = copysignf(fmaxf(fabsf(gy) - t, 0.f), gy);
    } else {
        const float m = sqrtf(gx * gx + gy * gy);
        const float sc = m > t ? 1.f - t / m : 0.f;
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

template <bool ANISO>
__global__ __launch_bounds__(kTvThreads) void tv_spatial_kernel(const float* __restrict__ x, const float* __restrict__ wx, const float* __restrict__ wy,
                                                                const float* __restrict__ b, float* __restrict__ nwx, float* __restrict__ nwy,
                                                                float* __restrict__ rhs, const int M, const int N, const int logtx, const float mu,
                                                                const float rho, const float t) {
    __shared__ __attribute__((aligned(16))) float xs[kTvXsFloats];
    __shared__ __attribute__((aligned(16))) float vxr[1024];
    __shared__ __attribute__((aligned(16))) float vyb[1024];
    const int TX = 1 << logtx, TY = blockDim.x >> logtx;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> logtx;
    const int tw = 4 * TX, th = 4 * TY, xst = tw + 8;
    const int j0 = blockIdx.x * tw, i0 = blockIdx.y * th;
    const int j = j0 + 4 * tx, i = i0 + 4 * ty;  // the thread's block: rows i .. i + 3, columns j .. j + 3
    const int mM = M - 1, mN = N - 1;

    // x: own block to registers and LDS (LDS row r holds plan row i0 - 1 + r, LDS column c plan column j0 - 4 + c)
    float xr[5][5];  // [row][col], row 4 = the row below, column 4 = the column to the right
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4 q = *reinterpret_cast<const float4*>(x + (size_t)(i + r) * N + j);
        xr[r][0] = q.x; xr[r][1] = q.y; xr[r][2] = q.z; xr[r][3] = q.w;
        *reinterpret_cast<float4*>(xs + (4 * ty + r + 1) * xst + 4 + 4 * tx) = q;
    }
    if (ty == 0) *reinterpret_cast<float4*>(xs + 4 + 4 * tx) = *reinterpret_cast<const float4*>(x + (size_t)((i0 - 1) & mM) * N + j);
    if (ty == TY - 1)
        *reinterpret_cast<float4*>(xs + (th + 1) * xst + 4 + 4 * tx) = *reinterpret_cast<const float4*>(x + (size_t)((i0 + th) & mM) * N + j);
    for (int r = threadIdx.x; r < 2 * (th + 2); r += blockDim.x) {  // the two halo columns, rows i0 - 1 .. i0 + th
        const int rr = r >> 1, right = r & 1;
        const int col = right ? ((j0 + tw) & mN) : ((j0 - 1) & mN);
        xs[rr * xst + (right ? 4 + tw : 3)] = x[(size_t)((i0 - 1 + rr) & mM) * N + col];
    }
    // the duals of the own block
    float wxr[4][4], wyr[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4 qx = *reinterpret_cast<const float4*>(wx + (size_t)(i + r) * N + j);
        const float4 qy = *reinterpret_cast<const float4*>(wy + (size_t)(i + r) * N + j);
        wxr[r][0] = qx.x; wxr[r][1] = qx.y; wxr[r][2] = qx.z; wxr[r][3] = qx.w;
        wyr[r][0] = qy.x; wyr[r][1] = qy.y; wyr[r][2] = qy.z; wyr[r][3] = qy.w;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) xr[r][4] = xs[(4 * ty + r + 1) * xst + 8 + 4 * tx];
    {
        const float4 q = *reinterpret_cast<const float4*>(xs + (4 * ty + 5) * xst + 4 + 4 * tx);
        xr[4][0] = q.x; xr[4][1] = q.y; xr[4][2] = q.z; xr[4][3] = q.w;
    }
    // v on the own block; the new duals leave at once
    float vx[4][4], vy[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float ox[4], oy[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            tv_shrink<ANISO>(xr[r][c + 1] - xr[r][c] + wxr[r][c], xr[r + 1][c] - xr[r][c] + wyr[r][c], t, vx[r][c], vy[r][c], ox[c], oy[c]);
        *reinterpret_cast<float4*>(nwx + (size_t)(i + r) * N + j) = make_float4(ox[0], ox[1], ox[2], ox[3]);
        *reinterpret_cast<float4*>(nwy + (size_t)(i + r) * N + j) = make_float4(oy[0], oy[1], oy[2], oy[3]);
        vxr[(4 * ty + r) * TX + tx] = vx[r][3];
    }
    *reinterpret_cast<float4*>(vyb + ty * tw + 4 * tx) = make_float4(vy[3][0], vy[3][1], vy[3][2], vy[3][3]);
    // vx one column to the left of the block, vy one row above it
    float vxl[4], vyu[4];
    if (tx == 0) {  // across the tile's left edge: from the halo column j0 - 1
        const int col = (j0 - 1) & mN;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float xc = xs[(4 * ty + r + 1) * xst + 3], xd = xs[(4 * ty + r + 2) * xst + 3];
            const size_t at = (size_t)(i + r) * N + col;
            float uy, ox, oy;
            tv_shrink<ANISO>(xr[r][0] - xc + wx[at], xd - xc + wy[at], t, vxl[r], uy, ox, oy);
        }
    }
    if (ty == 0) {  // across the tile's top edge: from the halo row i0 - 1
        const size_t at = (size_t)((i0 - 1) & mM) * N + j;
        const float4 qx = *reinterpret_cast<const float4*>(wx + at), qy = *reinterpret_cast<const float4*>(wy + at);
        const float4 xu = *reinterpret_cast<const float4*>(xs + 4 + 4 * tx);
        const float xur = xs[8 + 4 * tx];
        const float xa[5] = {xu.x, xu.y, xu.z, xu.w, xur}, ax[4] = {qx.x, qx.y, qx.z, qx.w}, ay[4] = {qy.x, qy.y, qy.z, qy.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float ux, ox, oy;
            tv_shrink<ANISO>(xa[c + 1] - xa[c] + ax[c], xr[0][c] - xa[c] + ay[c], t, ux, vyu[c], ox, oy);
        }
    }
    __syncthreads();
    if (tx != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) vxl[r] = vxr[(4 * ty + r) * TX + tx - 1];
    }
    if (ty != 0) {
        const float4 q = *reinterpret_cast<const float4*>(vyb + (ty - 1) * tw + 4 * tx);
        vyu[0] = q.x; vyu[1] = q.y; vyu[2] = q.z; vyu[3] = q.w;
    }
    // rhs = mu b + rho (Dx^T vx + Dy^T vy),  Dx^T v[i, j] = v[i, j - 1] - v[i, j]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4 q = *reinterpret_cast<const float4*>(b + (size_t)(i + r) * N + j);
        const float bb[4] = {q.x, q.y, q.z, q.w};
        float o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float left = c == 0 ? vxl[r] : vx[r][c - 1];
            const float up = r == 0 ? vyu[c] : vy[r - 1][c];
            o[c] = mu * bb[c] + rho * ((left - vx[r][c]) + (up - vy[r][c]));
        }
        *reinterpret_cast<float4*>(rhs + (size_t)(i + r) * N + j) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// tile geometry of an M x N plan (M >= 8, N >= 32, powers of two): TX = min(64, N / 4) thread columns, TY = min(256 / TX, M / 4)
hipError_t launch_tv_spatial(const float* x, const float* wx, const float* wy, const float* b, float* nwx, float* nwy, float* rhs, int M, int N,
                             float mu, float rho, int anisotropic, hipStream_t s) {
    if (M < 8 || N < 32 || (M & (M - 1)) || (N & (N - 1))) return hipErrorInvalidValue;
    int logtx = 6;
    while ((4 << logtx) > N) --logtx;
    const int TX = 1 << logtx;
    int TY = kTvThreads / TX;
    if (TY > M / 4) TY = M / 4;
    if ((4 * TY + 2) * (4 * TX + 8) > kTvXsFloats || 4 * TY * TX > 1024) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(N / (4 * TX)), (unsigned)(M / (4 * TY)));
    const float t = 1.f / rho;
    if (anisotropic)
        hipLaunchKernelGGL((tv_spatial_kernel<true>), grid, dim3(TX * TY), 0, s, x, wx, wy, b, nwx, nwy, rhs, M, N, logtx, mu, rho, t);
    else
        hipLaunchKernelGGL((tv_spatial_kernel<false>), grid, dim3(TX * TY), 0, s, x, wx, wy, b, nwx, nwy, rhs, M, N, logtx, mu, rho, t);
    return hipGetLastError();
}

}  // namespace fdr
