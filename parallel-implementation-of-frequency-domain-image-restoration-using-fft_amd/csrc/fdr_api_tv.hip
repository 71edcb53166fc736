// fdr_api_tv.hip -- total-variation deconvolution by ADMM (fdr_tv_deconv_f32*; kernels in fdr_tv.hip): the workspace, the solve
// table, the driver (on a group of n >= 1 images: the batch of fdr_api_tvbatch.hip runs it too) and the two entry points.  The
// linear solve of an iteration is a blur with the table T in place of H: passes A, B' and C of fdr_api_operator.hip, unchanged.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassTvTable = "TV table: 1/(mu|H|^2+rho L)/MN";
const char* const kPassTvInit = "TV init: x = pad(d), w = 0";
const char* const kPassTvSpatial = "TV spatial: shrink+dual+div";
const char* const kPassTvSpatialJoint = "TV spatial: joint shrink+dual+div";  // the coupled kernel, all channels of a tile
const char* const kPassTvSolve ="B' op cols: FFT*T*IFFT (TV solve)";
const char* const kPassTvX = "C op rows: IFFT (TV x)";
const char* const kPassTvOut = "TV out: crop+clamp";
const char* const kPassTvNorm = "E TV minmax+normalize";

}  // namespace

namespace fdr {

// The first TV call of a plan, or the first on a larger group: T (ws_elems float2, zeroed once: the padding between panels is never
// written) and six M x N planes per image of the group -- x, b and the two pairs of duals of image 0, then those of image 1, ..  For
// one image this is the block the single-image calls have always had.  The new block is had before the old one is let go (nothing
// it holds outlives a call but T, which the next call builds again).
int ensure_tv_workspace(fdr_plan* p, const char* fn, int group) {
    if (p->tv_block && p->tv_group >= group) return FDR_OK;
    const size_t P = (size_t)p->M * p->N;
    const size_t t_bytes = (p->ws_elems * sizeof(float2) + 255) & ~(size_t)255;
    char* blk = nullptr;
    if (hipMalloc((void**)&blk, t_bytes + (size_t)group * 6 * P * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FDR_ERR_ALLOC, std::string(fn) + ": hipMalloc of the TV workspace failed");
    }
    const hipError_t e = hipMemset(blk, 0, t_bytes);
    if (e != hipSuccess) { (void)hipFree(blk); FDR_HIP(e); }
    if (p->tv_block) (void)hipFree(p->tv_block);  // (waits for the device: nothing queued still uses it)
    float* planes = reinterpret_cast<float*>(blk + t_bytes);
    p->tv_block = blk;
    p->tv_group = group;
    p->tv_T = reinterpret_cast<float2*>(blk);
    p->tv_x = planes;
    p->tv_b = planes + P;
    p->tv_w[0][0] = planes + 2 * P; p->tv_w[0][1] = planes + 3 * P;
    p->tv_w[1][0] = planes + 4 * P; p->tv_w[1][1] = planes + 5 * P;
    p->tv_gen = 0;
    return FDR_OK;
}

// everything a TV call refuses, before any device work
int tv_check(const fdr_plan* p, const char* fn, int rows, int cols, int stride, int out_stride, const fdr_tv_params* prm) {
    if (!prm) return null_arg(fn);
    const int rc = check_window(p, fn, NEED_OPERATOR_PSF, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    if (!std::isfinite(prm->mu) || !(prm->mu > 0.f)) return fail(FDR_ERR_ARG, std::string(fn) + ": mu must be finite and > 0");
    if (!std::isfinite(prm->rho) || !(prm->rho > 0.f)) return fail(FDR_ERR_ARG, std::string(fn) + ": rho must be finite and > 0");
    if (prm->iterations < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": iterations < 0");
    if (prm->norm_area != FDR_NORM_NONE && prm->norm_area != FDR_NORM_CROPPED && prm->norm_area != FDR_NORM_PADDED)
        return fail(FDR_ERR_ARG, std::string(fn) + ": unknown norm_area");
    return FDR_OK;
}

// workspace and Laplacian table (both synchronous, first call only)
int tv_prepare(fdr_plan* p, const char* fn, int group) {
    int rc = ensure_tv_workspace(p, fn, group);
    if (rc == FDR_OK) rc = ensure_lap_table(p);
    return rc;
}

// x, b, the duals and rhs (slot k's raw plane) are full M x N planes even for a cropped window: the solve is exact only on the
// periodic plan.  d is read by the first launches alone (b and the start), so for one image d_out may be d_img.
int tv_group_dev(fdr_plan* p, const char* fn, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                 float* const* d_outs, int out_stride, const fdr_tv_params& prm, bool coupled, hipStream_t s) {
    if (n < 1 || n > kMaxGroup || n > p->tv_group) return fail(FDR_ERR_STATE, std::string(fn) + ": the TV workspace does not hold the group");
    const int M = p->M, N = p->N, iters = prm.iterations;
    const size_t step = tv_image_stride(p);
    float *x[kMaxGroup], *b[kMaxGroup], *w0x[kMaxGroup], *w0y[kMaxGroup], *rhs[kMaxGroup];
    const float* xc[kMaxGroup];
    for (int k = 0; k < n; ++k) {
        x[k] = p->tv_x + k * step; b[k] = p->tv_b + k * step; w0x[k] = p->tv_w[0][0] + k * step; w0y[k] = p->tv_w[0][1] + k * step;
        xc[k] = x[k];
        rhs[k] = ws[k]->raw;
    }
    int rc = FDR_OK;
    if (iters > 0 && (p->tv_gen != p->op_gen || p->tv_mu != prm.mu || p->tv_rho != prm.rho)) {
        ScopedPass t(p, s, kPassTvTable);
        FDR_HIP(launch_tv_table(p->op_h, p->tv_T, p->lap, M, N, p->pstride, p->npanels, (double)prm.mu, (double)prm.rho, s));
        p->tv_gen = p->op_gen; p->tv_mu = prm.mu; p->tv_rho = prm.rho;
    }
    if (iters > 0) {  // b = blur^T(pad(d)) over the whole plan (mu is applied where b is read)
        rc = blur_window_dev_n(p, ws, n, d_imgs, rows, cols, stride, b, N, 1, s, M, N);
        if (rc != FDR_OK) return rc;
    }
    {
        ScopedPass t(p, s, kPassTvInit);
        FDR_HIP(launch_tv_init_n(n, d_imgs, rows, cols, stride, x, w0x, w0y, M, N, s));
    }
    for (int it = 0; it < iters && rc == FDR_OK; ++it) {
        float* const* w = p->tv_w[it & 1];
        float* const* nw = p->tv_w[(it + 1) & 1];
        {
            ScopedPass t(p, s, coupled ? kPassTvSpatialJoint : kPassTvSpatial);
            FDR_HIP(launch_tv_spatial_n(n, p->tv_x, w[0], w[1], p->tv_b, nw[0], nw[1], step, rhs, M, N, prm.mu, prm.rho, prm.anisotropic, coupled, s));
        }
        rc = op_rows_fwd_n(p, ws, n, rhs, M, N, N, s);
        if (rc == FDR_OK) rc = op_cols_table_n(p, ws, n, p->tv_T, kPassTvSolve, s);
        if (rc == FDR_OK) rc = op_rows_inv_n(p, ws, n, ROW_OUT_BLUR, kPassTvX, nullptr, 0, nullptr, x, N, M, N, s);
    }
    if (rc != FDR_OK) return rc;
    if (prm.norm_area == FDR_NORM_NONE) {
        ScopedPass t(p, s, kPassTvOut);
        FDR_HIP(launch_tv_output_n(n, xc, N, d_outs, rows, cols, out_stride, prm.nonneg, s));
        return FDR_OK;
    }
    const float* const* fin = xc;
    if (prm.nonneg) {  // the clamped planes go to rhs, free by now
        ScopedPass t(p, s, kPassTvOut);
        FDR_HIP(launch_tv_output_n(n, xc, N, rhs, rows, cols, N, 1, s));
        fin = rhs;
    }
    for (int k = 0; k < n && rc == FDR_OK; ++k) rc = normalize_window(p, fn, kPassTvNorm, fin[k], N, rows, cols, prm.norm_area, d_outs[k], out_stride, s);
    return rc;
}

int tv_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                const fdr_tv_params& prm, hipStream_t s) {
    fdr_plan::Slot* w = &p->slots[0];
    return tv_group_dev(p, fn, &w, 1, &d_img, rows, cols, stride, &d_out, out_stride, prm, false, s);
}

}  // namespace fdr

extern "C" {

int fdr_tv_deconv_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                          const fdr_tv_params* params, void* stream) {
    const char* fn = "fdr_tv_deconv_f32_dev";
    if (!p || !d_img || !d_out) return null_arg(fn);
    int rc = tv_check(p, fn, rows, cols, stride, out_stride, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = tv_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    return tv_dev_impl(p, fn, d_img, rows, cols, stride, d_out, out_stride, *params, (hipStream_t)stream);
}

int fdr_tv_deconv_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, float* out_host, int out_stride,
                      const fdr_tv_params* params) {
    const char* fn = "fdr_tv_deconv_f32";
    if (!p || !img_host || !out_host) return null_arg(fn);
    int rc = tv_check(p, fn, rows, cols, stride, out_stride, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = tv_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    return host_image_call(p, fn, img_host, rows, cols, stride, out_host, rows, cols, out_stride, [&](const float* d_in, float* d_out) {
        return tv_dev_impl(p, fn, d_in, rows, cols, cols, d_out, cols, *params, nullptr);
    });
}

}  // extern "C"
