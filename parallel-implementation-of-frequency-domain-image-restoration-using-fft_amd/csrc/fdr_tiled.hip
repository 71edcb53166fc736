// fdr_tiled.hip -- sectioned restoration (fdr_restore_tiled_f32*; driver in fdr_api_tiled.hip): the two kernels the tiles' own
// iterations do not have.
//
//   tiled_blend_kernel       the partition-of-unity blend of the staged tile windows into the caller's picture,
//                                out[y, x] = sum_a sum_b (Wy_a(y) Wx_b(x)) o_ab[y - y_a, x - x_b]
//                            over the tiles that cover the pixel (at most three per axis), a outer and b inner, ascending, every product
//                            and sum rounded on its own from +0: a float32 model on the host repeats it bit for bit.  A gather over
//                            the output: no atomics, every pixel written once.
//   tiled_psf_centre_kernel  a PSF rolled into an M x N plane so that its centre (prows / 2, pcols / 2) lies at the origin.
//
// The blend is memory-bound: 4 bytes read per covering tile and 4 written per pixel, and for whole runs of rows and columns exactly
// one tile covers a pixel.  The weights come from two host-built tables, one entry per picture row and per picture column.
#include "fdr_kernels.hpp"

namespace fdr {

namespace {

struct TiledBlendArgs {
    TiledAxis ar, ac;
    int rows, cols, out_stride;
    int ovec;  // 16-byte stores: the out pointer and its stride keep every group of four aligned
};

}  // namespace

// A thread owns the four consecutive pixels x .. x + 3 of a row and walks down the picture in steps of the grid's height; its four
// column entries are read once, and the entry of its next row is read one row ahead.  Where one tile covers all four pixels in
// both axes (`cone` and a row entry of one tile) the staged values are one run of four floats: a 16-byte load when the run is
// aligned, and always coalesced over the wave.  Elsewhere -- in the seams -- every pixel gathers its up to 3 x 3 values; the loops
// are unrolled with constant indices so that nothing goes to scratch.
__global__ __launch_bounds__(256) void tiled_blend_kernel(const float* __restrict__ stage, const TiledCover* __restrict__ rtab,
                                                          const TiledCover* __restrict__ ctab, float* __restrict__ out, const TiledBlendArgs g) {
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (x >= g.cols) return;
    TiledCover c[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) c[l] = ctab[x + l];  // (the table is padded to a multiple of four entries)
    const bool cone = c[0].count == 1 && c[1].count == 1 && c[2].count == 1 && c[3].count == 1 && c[0].first == c[3].first;
    const bool whole = x + 3 < g.cols;
    const size_t tile_px = (size_t)g.ar.win * g.ac.win;
    const int ystep = gridDim.y * blockDim.y;
    int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (y >= g.rows) return;
    TiledCover rnext = rtab[y];
    for (;; y += ystep) {
        const TiledCover r = rnext;
        const bool more = ystep < g.rows - y;  // (written so that y + ystep cannot overflow)
        if (more) rnext = rtab[y + ystep];  // the next row's entry is on its way while this row's values are fetched
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (cone && r.count == 1) {
            const int a = r.first, b = c[0].first;
            const float* src = stage + ((size_t)a * g.ac.n + b) * tile_px + (size_t)(y - tiled_origin(g.ar, a)) * g.ac.win + (x - tiled_origin(g.ac, b));
            float v[4];
            if (((uintptr_t)src & 15) == 0) {
                const float4 q = *reinterpret_cast<const float4*>(src);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int l = 0; l < 4; ++l) v[l] = src[l];
            }
#pragma unroll
            for (int l = 0; l < 4; ++l) acc[l] = __fadd_rn(acc[l], __fmul_rn(__fmul_rn(r.w[0], c[l].w[0]), v[l]));
        } else {
#pragma unroll
            for (int i = 0; i < kTiledMaxCover; ++i) {
                if (i < r.count) {
                    const int a = r.first + i;
                    const float wy = r.w[i];
                    const float* trow = stage + (size_t)a * g.ac.n * tile_px + (size_t)(y - tiled_origin(g.ar, a)) * g.ac.win;
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
#pragma unroll
                        for (int j = 0; j < kTiledMaxCover; ++j) {
                            if (j < c[l].count) {
                                const int b = c[l].first + j;
                                const float v = trow[(size_t)b * tile_px + (x + l - tiled_origin(g.ac, b))];
                                acc[l] = __fadd_rn(acc[l], __fmul_rn(__fmul_rn(wy, c[l].w[j]), v));
                            }
                        }
                    }
                }
            }
        }
        float* dst = out + (size_t)y * g.out_stride + x;
        if (whole && g.ovec) {
            *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (x + l < g.cols) dst[l] = acc[l];
        }
        if (!more) break;
    }
}

// plane[u, v] = psf[(u + prows / 2) mod M, (v + pcols / 2) mod N] where that lies in the PSF, 0 elsewhere: every element of the plane
// is written, so the plane needs no clearing
__global__ __launch_bounds__(256) void tiled_psf_centre_kernel(const float* __restrict__ psf, const int prows, const int pcols, const int pstride,
                                                               float* __restrict__ plane, const int M, const int N) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int u = blockIdx.y * blockDim.y + threadIdx.y;
    if (u >= M || v >= N) return;
    int i = u + prows / 2, j = v + pcols / 2;
    if (i >= M) i -= M;
    if (j >= N) j -= N;
    plane[(size_t)u * N + v] = (i < prows && j < pcols) ? psf[(size_t)i * pstride + j] : 0.f;
}

hipError_t launch_tiled_blend(const float* stage, const TiledCover* rtab, const TiledCover* ctab, TiledAxis ar, TiledAxis ac, float* out, int rows,
                              int cols, int out_stride, hipStream_t s) {
    if (!stage || !rtab || !ctab || !out || rows < 1 || cols < 1 || out_stride < cols || ar.n < 1 || ac.n < 1 || ar.win < 1 || ac.win < 1 ||
        ar.win > rows || ac.win > cols || ar.last != rows - ar.win || ac.last != cols - ac.win)
        return hipErrorInvalidValue;
    const int groups = (cols + 3) / 4;
    const int tx = groups <= 64 ? 64 : groups <= 128 ? 128 : 256, ty = 256 / tx;
    const unsigned gx = (unsigned)((groups + tx - 1) / tx);
    // about two thousand workgroups, the rest of the rows by the grid-stride loop: a thread reads 128 bytes of column entries once,
    // so the more rows it walks the less they weigh beside the 32 bytes it moves per row
    unsigned gy = (unsigned)((rows + ty - 1) / ty);
    const unsigned cap = gx >= 2048 ? 1u : 2048u / gx;
    if (gy > cap) gy = cap;
    const TiledBlendArgs g = {ar, ac, rows, cols, out_stride, ((uintptr_t)out & 15) == 0 && (out_stride & 3) == 0};
    hipLaunchKernelGGL(tiled_blend_kernel, dim3(gx, gy), dim3(tx, ty), 0, s, stage, rtab, ctab, out, g);
    return hipGetLastError();
}

hipError_t launch_tiled_psf_centre(const float* psf, int prows, int pcols, int pstride, float* plane, int M, int N, hipStream_t s) {
    if (!psf || !plane || prows < 1 || pcols < 1 || pstride < pcols || prows > M || pcols > N) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((M + 3) / 4));
    hipLaunchKernelGGL(tiled_psf_centre_kernel, grid, dim3(64, 4), 0, s, psf, prows, pcols, pstride, plane, M, N);
    return hipGetLastError();
}

}  // namespace fdr
