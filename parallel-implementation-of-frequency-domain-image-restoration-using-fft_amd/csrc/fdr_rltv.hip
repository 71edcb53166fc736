// fdr_rltv.hip -- Richardson-Lucy with a total-variation prior (fdr_richardson_lucy_tv_f32*, fdr_rl_tv_factor_f32_dev; Dey et al.
// 2006, the RLTV of DeconvolutionLab2), the one kernel that is not a transform: the factor the multiplicative update is divided by.
// On the R x C domain of the estimate u (the window in the plain form, the whole plan in the free-boundary form), with forward
// differences that replicate at the far edges:
//
//     gx[i, j] = j < C-1 ? u[i, j+1] - u[i, j] : 0
//     gy[i, j] = i < R-1 ? u[i+1, j] - u[i, j] : 0
//     m  = sqrt(gx^2 + gy^2 + eps^2);  px = gx / m;  py = gy / m
//     div[i, j] = (px[i, j] - (j > 0 ? px[i, j-1] : 0)) + (py[i, j] - (i > 0 ? py[i-1, j] : 0))            (div = -D^T)
//     g = 1 - lambda div;  factor = w / g           (w = 1 for a null pointer; a zero of w stays zero)
//
// |div| <= 2 + sqrt(2), so lambda <= FDR_RLTV_MAX_LAMBDA = 0.125 keeps g >= 0.57: no clamp, no negative denominator.  The weighted
// update pass (ROW_OUT_RL_UPDATE_W of fdr_panel_rows.hip) multiplies by the factor, so no transform pass changes (fdr_api_rltv.hip).
//
// A group of 1 .. kMaxGroup planes, `pitch` floats apart, takes one launch (fdr_richardson_lucy_tv_batch_f32*,
// fdr_rl_tv_factor_group_f32_dev): uncoupled, blockIdx.z is the plane and every plane gets the code, and so the bits, of the launch
// on it alone.  Coupled, the planes are the channels of one picture and share the norm (vectorial TV):
//
//     m^2 = eps^2 + sum_c (gx_c^2 + gy_c^2)   (added in the order c = 0, 1, ..);  p_c = grad u_c / m;  g_c = 1 - lambda div p_c
//
// m is no smaller than a channel's own, so |div p_c| <= 2 + sqrt(2) and g >= 0.57 hold as before.
#include "fdr_kernels.hpp"

#include <cfloat>

namespace fdr {

// A workgroup of 16 x 16 threads owns a tile of 64 x 64 pixels, a thread 4 x 4 of them (the layout of tv_spatial_kernel).
//   u: the thread's 16 values go to registers and, with the tile's one-pixel halo, to LDS; every neighbour of u is an LDS read.  A row
//      of four moves as one 16-byte request where the pointer, the stride and the width allow it, as four guarded scalars where not
//      (the last thread column of an odd width, a loose stride, a pointer off by one float).  Every row and column index is clamped to the
//      domain, so beyond the far edges the last row / column repeats: the differences there are the 0 the edge rule asks for, with
//      no test per pixel, and no address leaves the planes.
//   p: computed for the thread's 16 pixels.  The divergence needs px one pixel to the left and py one pixel up: inside the block they
//      are registers, across threads they pass through LDS (the right column and the bottom row of each block), and across tiles the
//      first two waves recompute them from the halo, one value per lane -- never from another workgroup's output.
// Two barriers, no atomics.  Traffic: 4 bytes in and 4 out per pixel, 4 more with w.  LDS: xs 66 rows of 72 floats (the interior
// starts at column 4: 16-byte aligned), pxr 64 x 16, pyb 16 x 64, the halo's pxh 64 and pyh 64.
constexpr int kRltvTX = 16, kRltvTY = 16;
constexpr int kRltvTileW = 4 * kRltvTX, kRltvTileH = 4 * kRltvTY;  // 64 x 64
constexpr int kRltvXst = kRltvTileW + 8;

// four floats of the row at `row` from column j on: one request when `vec` (row + j is 16-byte aligned) and all four lie in the
// row, else four scalars whose columns are clamped to the row (beyond its end the last value repeats)
__device__ __forceinline__ float4 rltv_load4(const float* __restrict__ row, const int j, const int C, const bool vec) {
    if (vec && j + 3 < C) return *reinterpret_cast<const float4*>(row + j);
    const int last = C - 1;
    return make_float4(row[min(j, last)], row[min(j + 1, last)], row[min(j + 2, last)], row[min(j + 3, last)]);
}

// p = grad u / m through the reciprocal square root (one instruction, 1 ulp) and two products: with the correctly rounded sqrtf
// and two divisions the kernel is bound by its arithmetic, not by memory.  eps2 is a normal float (the launcher sees to it), so
// the root's argument is, and a zero difference gives an exact 0.
__device__ __forceinline__ void rltv_p(const float gx, const float gy, const float eps2, float& px, float& py) {
    const float rm = rsqrtf(gx * gx + gy * gy + eps2);
    px = gx * rm;
    py = gy * rm;
}

// The loads of one plane's tile: the thread's 16 values to xr[0 .. 3][0 .. 3] and, with the tile's one-pixel halo, to xs (LDS row r
// holds row i0 - 1 + r, LDS column c column j0 - 4 + c).  A barrier, then rltv_neighbours.
__device__ __forceinline__ void rltv_stage(const float* __restrict__ u, const int R, const int C, const int stride, const bool vec_u,
                                           float* __restrict__ xs, float (&xr)[5][5], const int tx, const int ty, const int i0, const int j0) {
    const int j = j0 + 4 * tx, i = i0 + 4 * ty;  // the thread's block: rows i .. i + 3, columns j .. j + 3
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4 q = rltv_load4(u + (size_t)min(i + r, R - 1) * stride, j, C, vec_u);
        xr[r][0] = q.x; xr[r][1] = q.y; xr[r][2] = q.z; xr[r][3] = q.w;
        *reinterpret_cast<float4*>(xs + (4 * ty + r + 1) * kRltvXst + 4 + 4 * tx) = q;
    }
    if (ty == 0)
        *reinterpret_cast<float4*>(xs + 4 + 4 * tx) = rltv_load4(u + (size_t)max(i0 - 1, 0) * stride, j, C, vec_u);
    if (ty == kRltvTY - 1)
        *reinterpret_cast<float4*>(xs + (kRltvTileH + 1) * kRltvXst + 4 + 4 * tx) =
            rltv_load4(u + (size_t)min(i0 + kRltvTileH, R - 1) * stride, j, C, vec_u);
    for (int r = threadIdx.x; r < 2 * (kRltvTileH + 2); r += blockDim.x) {  // the two halo columns, rows i0 - 1 .. i0 + 64
        const int rr = r >> 1, right = r & 1;
        const int gi = min(max(i0 - 1 + rr, 0), R - 1), gj = right ? min(j0 + kRltvTileW, C - 1) : max(j0 - 1, 0);
        xs[rr * kRltvXst + (right ? 4 + kRltvTileW : 3)] = u[(size_t)gi * stride + gj];
    }
}
// xr[r][4], the column to the right of the thread's block, and xr[4][c], the row below it, from the staged tile
__device__ __forceinline__ void rltv_neighbours(const float* __restrict__ xs, float (&xr)[5][5], const int tx, const int ty) {
#pragma unroll
    for (int r = 0; r < 4; ++r) xr[r][4] = xs[(4 * ty + r + 1) * kRltvXst + 8 + 4 * tx];
    const float4 q = *reinterpret_cast<const float4*>(xs + (4 * ty + 5) * kRltvXst + 4 + 4 * tx);
    xr[4][0] = q.x; xr[4][1] = q.y; xr[4][2] = q.z; xr[4][3] = q.w;
}
// the thread's 16 weights (HAS_W), loaded as the estimate is
template <bool HAS_W>
__device__ __forceinline__ void rltv_load_w(const float* __restrict__ w, const int R, const int C, const int stride, const bool vec_w,
                                            float (&wr)[4][4], const int i, const int j) {
    if (HAS_W) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4 q = rltv_load4(w + (size_t)min(i + r, R - 1) * stride, j, C, vec_w);
            wr[r][0] = q.x; wr[r][1] = q.y; wr[r][2] = q.z; wr[r][3] = q.w;
        }
    }
}
// From the staged tile of one plane (rltv_stage, a barrier, rltv_neighbours) to its factor: p on the thread's block and on the halo,
// the divergence, the quotient, the store.  JOINT: p = grad u times the given reciprocal roots (rm for the thread's 16 pixels, rmh for
// the lane's halo pixel) instead of the plane's own.  One barrier.
template <bool HAS_W, bool JOINT>
__device__ __forceinline__ void rltv_finish(const float* __restrict__ xs, float* __restrict__ pxr, float* __restrict__ pyb,
                                            float* __restrict__ pxh, float* __restrict__ pyh, const float (&xr)[5][5],
                                            const float (&wr)[4][4], const float (&rm)[4][4], const float rmh, const float eps2,
                                            const float lambda, const int R, const int C, float* __restrict__ out, const int out_stride,
                                            const int vec_out, const int tx, const int ty, const int i0, const int j0) {
    const int j = j0 + 4 * tx, i = i0 + 4 * ty;
    // p on the own block
    float px[4][4], py[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float gx = xr[r][c + 1] - xr[r][c], gy = xr[r + 1][c] - xr[r][c];
            if (JOINT) {
                px[r][c] = gx * rm[r][c];
                py[r][c] = gy * rm[r][c];
            } else {
                rltv_p(gx, gy, eps2, px[r][c], py[r][c]);
            }
        }
        pxr[(4 * ty + r) * kRltvTX + tx] = px[r][3];
    }
    *reinterpret_cast<float4*>(pyb + ty * kRltvTileW + 4 * tx) = make_float4(py[3][0], py[3][1], py[3][2], py[3][3]);
    // px one column to the left of the tile and py one row above it, from the halo: one value per lane of the first two waves; 0
    // across the domain's near edges
    if (threadIdx.x < kRltvTileH) {
        const int t = threadIdx.x;
        float v = 0.f, unused;
        if (j0 > 0) {
            const float xc = xs[(t + 1) * kRltvXst + 3];
            const float gx = xs[(t + 1) * kRltvXst + 4] - xc, gy = xs[(t + 2) * kRltvXst + 3] - xc;
            if (JOINT) v = gx * rmh;
            else rltv_p(gx, gy, eps2, v, unused);
        }
        pxh[t] = v;
    } else if (threadIdx.x < kRltvTileH + kRltvTileW) {
        const int t = threadIdx.x - kRltvTileH;
        float v = 0.f, unused;
        if (i0 > 0) {
            const float xa = xs[4 + t];
            const float gx = xs[5 + t] - xa, gy = xs[kRltvXst + 4 + t] - xa;
            if (JOINT) v = gy * rmh;
            else rltv_p(gx, gy, eps2, unused, v);
        }
        pyh[t] = v;
    }
    __syncthreads();
    float pxl[4], pyu[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pxl[r] = tx == 0 ? pxh[4 * ty + r] : pxr[(4 * ty + r) * kRltvTX + tx - 1];
    {
        const float4 q = *reinterpret_cast<const float4*>(ty == 0 ? pyh + 4 * tx : pyb + (ty - 1) * kRltvTileW + 4 * tx);
        pyu[0] = q.x; pyu[1] = q.y; pyu[2] = q.z; pyu[3] = q.w;
    }
    // factor = w / (1 - lambda div)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (i + r >= R) break;
        float o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float left = c == 0 ? pxl[r] : px[r][c - 1];
            const float up = r == 0 ? pyu[c] : py[r - 1][c];
            const float g = 1.f - lambda * ((px[r][c] - left) + (py[r][c] - up));
            o[c] = (HAS_W ? wr[r][c] : 1.f) / g;
        }
        float* dst = out + (size_t)(i + r) * out_stride + j;
        if (vec_out && j + 3 < C) {
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (j + c < C) dst[c] = o[c];
        }
    }
}

#define FDR_RLTV_LDS                                                                \
    __shared__ __attribute__((aligned(16))) float xs[(kRltvTileH + 2) * kRltvXst];  \
    __shared__ __attribute__((aligned(16))) float pxr[kRltvTileH * kRltvTX];        \
    __shared__ __attribute__((aligned(16))) float pyb[kRltvTY * kRltvTileW];        \
    __shared__ __attribute__((aligned(16))) float pxh[kRltvTileH];                  \
    __shared__ __attribute__((aligned(16))) float pyh[kRltvTileW]

// blockIdx.z = the plane: plane k's u and out lie k u_pitch and k out_pitch floats behind those given, w is the group's.  One plane
// is the single launch.
template <bool HAS_W>
__global__ __launch_bounds__(kRltvTX* kRltvTY) void rltv_factor_kernel(const float* __restrict__ u, const size_t u_pitch,
                                                                        const float* __restrict__ w, const int R, const int C, const int stride,
                                                                        const float lambda, const float eps2, float* __restrict__ out,
                                                                        const size_t out_pitch, const int out_stride, const int vec_u,
                                                                        const int vec_w, const int vec_out) {
    FDR_RLTV_LDS;
    const int tx = threadIdx.x & (kRltvTX - 1), ty = threadIdx.x / kRltvTX;
    const int j0 = blockIdx.x * kRltvTileW, i0 = blockIdx.y * kRltvTileH;
    u += (size_t)blockIdx.z * u_pitch;
    out += (size_t)blockIdx.z * out_pitch;
    float xr[5][5];  // [row][col], row 4 = the row below, column 4 = the column to the right
    float wr[4][4], rm[4][4];  // (rm: the coupled kernel's)
    rltv_stage(u, R, C, stride, vec_u, xs, xr, tx, ty, i0, j0);
    rltv_load_w<HAS_W>(w, R, C, stride, vec_w, wr, i0 + 4 * ty, j0 + 4 * tx);
    __syncthreads();
    rltv_neighbours(xs, xr, tx, ty);
    rltv_finish<HAS_W, false>(xs, pxr, pyb, pxh, pyh, xr, wr, rm, 0.f, eps2, lambda, R, C, out, out_stride, vec_out, tx, ty, i0, j0);
}

// The planes are the nch channels of one picture, and one workgroup owns its tile in every channel.  Sweep 1 stages each channel's
// tile in turn and adds gx^2 + gy^2 to m^2 in registers, in channel order from eps^2: for the thread's 16 pixels and, in the first
// two waves, for the lane's halo pixel (left of or above the tile), whose p the divergence needs.  The expressions are those of the
// tile that owns the pixel, on the same clamped loads, so a pixel has the same m in every workgroup that looks at it.  Sweep 2 is
// the single kernel's tile per channel (read again: 4 more bytes per pixel, mostly from L2) with the joint reciprocal root in the
// place of its own.  The LDS is the single kernel's, not a tile per channel; no atomics; no workgroup reads another's output.  With
// one channel m^2 = eps^2 + (gx^2 + gy^2), the sum of the single kernel with its two operands exchanged: the same bits.
template <bool HAS_W>
__global__ __launch_bounds__(kRltvTX* kRltvTY) void rltv_factor_coupled_kernel(const float* __restrict__ u, const size_t u_pitch, const int nch,
                                                                                const float* __restrict__ w, const int R, const int C,
                                                                                const int stride, const float lambda, const float eps2,
                                                                                float* __restrict__ out, const size_t out_pitch,
                                                                                const int out_stride, const int vec_u, const int vec_w,
                                                                                const int vec_out) {
    FDR_RLTV_LDS;
    const int tx = threadIdx.x & (kRltvTX - 1), ty = threadIdx.x / kRltvTX;
    const int j0 = blockIdx.x * kRltvTileW, i0 = blockIdx.y * kRltvTileH;
    float xr[5][5];
    float wr[4][4], rm[4][4];
    float mh = eps2;  // the lane's halo pixel: lanes 0 .. 63 (j0 - 1, i0 + lane), lanes 64 .. 127 (j0 + lane - 64, i0 - 1)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) rm[r][c] = eps2;
    rltv_load_w<HAS_W>(w, R, C, stride, vec_w, wr, i0 + 4 * ty, j0 + 4 * tx);
    for (int ch = 0; ch < nch; ++ch) {  // sweep 1: m^2
        if (ch > 0) __syncthreads();    // the last channel's tile has been read
        rltv_stage(u + (size_t)ch * u_pitch, R, C, stride, vec_u, xs, xr, tx, ty, i0, j0);
        __syncthreads();
        rltv_neighbours(xs, xr, tx, ty);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float gx = xr[r][c + 1] - xr[r][c], gy = xr[r + 1][c] - xr[r][c];
                rm[r][c] = rm[r][c] + (gx * gx + gy * gy);
            }
        if (threadIdx.x < kRltvTileH) {
            const int t = threadIdx.x;
            if (j0 > 0) {
                const float xc = xs[(t + 1) * kRltvXst + 3];
                const float gx = xs[(t + 1) * kRltvXst + 4] - xc, gy = xs[(t + 2) * kRltvXst + 3] - xc;
                mh = mh + (gx * gx + gy * gy);
            }
        } else if (threadIdx.x < kRltvTileH + kRltvTileW) {
            const int t = threadIdx.x - kRltvTileH;
            if (i0 > 0) {
                const float xa = xs[4 + t];
                const float gx = xs[5 + t] - xa, gy = xs[kRltvXst + 4 + t] - xa;
                mh = mh + (gx * gx + gy * gy);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) rm[r][c] = rsqrtf(rm[r][c]);
    const float rmh = rsqrtf(mh);
    for (int ch = 0; ch < nch; ++ch) {  // sweep 2: the factor of every channel
        // (sweep 1 has read its last tile; within this sweep the barrier of rltv_finish stands between a tile's reads and the next stage)
        if (ch == 0) __syncthreads();
        rltv_stage(u + (size_t)ch * u_pitch, R, C, stride, vec_u, xs, xr, tx, ty, i0, j0);
        __syncthreads();
        rltv_neighbours(xs, xr, tx, ty);
        rltv_finish<HAS_W, true>(xs, pxr, pyb, pxh, pyh, xr, wr, rm, rmh, eps2, lambda, R, C, out + (size_t)ch * out_pitch, out_stride, vec_out,
                                 tx, ty, i0, j0);
    }
}

// rows of `p` with row stride `stride` floats can move as 16-byte requests from every column that is a multiple of four, in every
// one of `count` planes `pitch` floats apart
static bool rltv_vec_ok(const float* p, int stride, int count = 1, size_t pitch = 0) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (stride & 3) == 0 && (count == 1 || (pitch & 3) == 0);
}

hipError_t launch_rltv_factor_group(const float* u, size_t u_pitch, int count, int rows, int cols, int stride, const float* w, float lambda,
                                    float eps, float* out, size_t out_pitch, int out_stride, bool coupled, hipStream_t s) {
    if (!u || !out || count < 1 || count > kMaxGroup || rows <= 0 || cols <= 0 || stride < cols || out_stride < cols) return hipErrorInvalidValue;
    const unsigned gx = (unsigned)((cols + kRltvTileW - 1) / kRltvTileW), gy = (unsigned)((rows + kRltvTileH - 1) / kRltvTileH);
    if (gy > 65535u) return hipErrorInvalidValue;
    const dim3 grid(gx, gy, coupled ? 1u : (unsigned)count), block(kRltvTX * kRltvTY);
    const float eps2 = fmaxf(eps * eps, FLT_MIN);  // an eps below 1e-19 would leave the root of a flat pixel at 0: 0 / 0
    const int vu = rltv_vec_ok(u, stride, count, u_pitch), vw = w && rltv_vec_ok(w, stride), vo = rltv_vec_ok(out, out_stride, count, out_pitch);
    if (coupled) {
        if (w)
            hipLaunchKernelGGL((rltv_factor_coupled_kernel<true>), grid, block, 0, s, u, u_pitch, count, w, rows, cols, stride, lambda, eps2, out,
                               out_pitch, out_stride, vu, vw, vo);
        else
            hipLaunchKernelGGL((rltv_factor_coupled_kernel<false>), grid, block, 0, s, u, u_pitch, count, w, rows, cols, stride, lambda, eps2, out,
                               out_pitch, out_stride, vu, vw, vo);
    } else if (w) {
        hipLaunchKernelGGL((rltv_factor_kernel<true>), grid, block, 0, s, u, u_pitch, w, rows, cols, stride, lambda, eps2, out, out_pitch,
                           out_stride, vu, vw, vo);
    } else {
        hipLaunchKernelGGL((rltv_factor_kernel<false>), grid, block, 0, s, u, u_pitch, w, rows, cols, stride, lambda, eps2, out, out_pitch,
                           out_stride, vu, vw, vo);
    }
    return hipGetLastError();
}

hipError_t launch_rltv_factor(const float* u, int rows, int cols, int stride, const float* w, float lambda, float eps, float* out,
                              int out_stride, hipStream_t s) {
    return launch_rltv_factor_group(u, 0, 1, rows, cols, stride, w, lambda, eps, out, 0, out_stride, false, s);
}

}  // namespace fdr
