// fdr_api_tv.hip -- total-variation deconvolution by ADMM (fdr_tv_deconv_f32*; kernels in fdr_tv.hip): the workspace, the solve
// table, the prior half-step and the output tail (the three stages the free-boundary driver of fdr_api_tvfree.hip shares), the
// driver (on a group of n >= 1 images: the batch of fdr_api_tvbatch.hip runs it too) and the two entry points.  The linear solve of
// an iteration is a blur with the table T in place of H: passes A, B' and C of fdr_api_operator.hip, unchanged.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassTvInit = "TV init: x = pad(d), w = 0";
const TvPassNames kTvPasses = {
    "TV table: 1/(mu|H|^2+rho L)/MN",
    "TV spatial: shrink+dual+div",
    "TV spatial: joint shrink+dual+div",  // the coupled kernel, all channels of a tile
    "B' op cols: FFT*T*IFFT (TV solve)",
    "C op rows: IFFT (TV x)",
    "TV out: crop+clamp",
    "E TV minmax+normalize",
};

}  // namespace

namespace fdr {

// The first TV call of a plan, or the first on a larger group.  T is zeroed once per block (the padding between panels is never
// written) and built again by the next call; for one image this is the block the single-image calls have always had.
int ensure_tv_workspace(fdr_plan* p, const char* fn, int group) {
    bool made = false;
    const int rc = ensure_workspace(p->tv.ws, fn, "TV workspace", group,
                                    [p](auto& c, int g) { layout(c, p->tv, (size_t)p->M * p->N, p->ws_elems, g); }, &made);
    if (rc != FDR_OK || !made) return rc;
    p->tv.gen = 0; p->tv.fr_gen = 0;
    const hipError_t e = hipMemset(p->tv.T, 0, p->ws_elems * sizeof(float2));
    if (e != hipSuccess) p->tv.ws.free_with(device_free);  // (no block rather than one whose padding was never cleared)
    FDR_HIP(e);
    return FDR_OK;
}

// everything a TV call refuses, before any device work
int tv_check(const fdr_plan* p, const char* fn, int rows, int cols, int stride, int out_stride, const fdr_tv_params* prm, PlanNeed need) {
    if (!prm) return null_arg(fn);
    const int rc = check_window(p, fn, need, rows, cols, stride, out_stride);
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

// ---- the stages the periodic driver below and the free-boundary driver (fdr_api_tvfree.hip) share, under the form's pass names ----

// T for the data weight `weight` (mu, or nu in the free forms) and rho, unless the plan holds it for this operator PSF already (a
// table of the frame set, which fdr_tv_deconv_frames_f32* left with tv.gen = 0, is never taken for it)
int tv_solve_table(fdr_plan* p, const TvPassNames& names, float weight, float rho, hipStream_t s) {
    if (p->tv.gen == p->op_gen && p->tv.fr_gen == 0 && p->tv.mu == weight && p->tv.rho == rho) return FDR_OK;
    ScopedPass t(p, s, names.table);
    FDR_HIP(launch_tv_table(p->op_h, p->tv.T, p->lap, p->M, p->N, p->pstride, p->npanels, (double)weight, (double)rho, s));
    p->tv.gen = p->op_gen; p->tv.fr_gen = 0; p->tv.mu = weight; p->tv.rho = rho;
    return FDR_OK;
}

// the prior half of iteration `it` on the group's planes: the spatial kernel (x, the duals of this iteration and b -> the duals of
// the next one and rhs, slot k's raw plane), then the solve of rhs into x: forward rows, the table columns, inverse rows
int tv_prior_half_step(fdr_plan* p, const TvPassNames& names, fdr_plan::Slot* const* ws, int n, int it, float weight, float rho, int anisotropic,
                       bool coupled, hipStream_t s) {
    const int M = p->M, N = p->N;
    const size_t step = tv_image_stride(p);
    float *x[kMaxGroup], *rhs[kMaxGroup];
    for (int k = 0; k < n; ++k) { x[k] = p->tv.x + k * step; rhs[k] = ws[k]->raw; }
    float* const* w = p->tv.w[it & 1];
    float* const* nw = p->tv.w[(it + 1) & 1];
    {
        ScopedPass t(p, s, coupled ? names.spatial_joint : names.spatial);
        FDR_HIP(launch_tv_spatial_n(n, p->tv.x, w[0], w[1], p->tv.b, nw[0], nw[1], step, rhs, M, N, weight, rho, anisotropic, coupled, s));
    }
    int rc = op_rows_fwd_n(p, ws, n, rhs, M, N, N, s);
    if (rc == FDR_OK) rc = op_cols_table_n(p, ws, n, p->tv.T, names.solve, s);
    if (rc == FDR_OK) rc = op_rows_inv_n(p, ws, n, ROW_OUT_BLUR, names.x, nullptr, 0, nullptr, x, N, M, N, s);
    return rc;
}

// the rows x cols window of every x to its output: cropped and clamped, or (clamped into rhs, free by now, and) normalised per image
int tv_output_tail(fdr_plan* p, const char* fn, const TvPassNames& names, fdr_plan::Slot* const* ws, int n, float* const* d_outs, int rows, int cols,
                   int out_stride, int nonneg, int norm_area, hipStream_t s) {
    const int N = p->N;
    const size_t step = tv_image_stride(p);
    const float* x[kMaxGroup];
    float* rhs[kMaxGroup];
    for (int k = 0; k < n; ++k) { x[k] = p->tv.x + k * step; rhs[k] = ws[k]->raw; }
    if (norm_area == FDR_NORM_NONE) {
        ScopedPass t(p, s, names.out);
        FDR_HIP(launch_tv_output_n(n, x, N, d_outs, rows, cols, out_stride, nonneg, s));
        return FDR_OK;
    }
    if (nonneg) {
        ScopedPass t(p, s, names.out);
        FDR_HIP(launch_tv_output_n(n, x, N, rhs, rows, cols, N, 1, s));
    }
    int rc = FDR_OK;
    for (int k = 0; k < n && rc == FDR_OK; ++k)
        rc = normalize_window(p, fn, names.norm, nonneg ? rhs[k] : x[k], N, rows, cols, norm_area, d_outs[k], out_stride, s);
    return rc;
}

// x, b, the duals and rhs (slot k's raw plane) are full M x N planes even for a cropped window: the solve is exact only on the
// periodic plan.  d is read by the first launches alone (b and the start), so for one image d_out may be d_img.
int tv_group_dev(fdr_plan* p, const char* fn, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                 float* const* d_outs, int out_stride, const fdr_tv_params& prm, bool coupled, hipStream_t s) {
    if (n < 1 || n > kMaxGroup || n > p->tv.ws.count) return fail(FDR_ERR_STATE, std::string(fn) + ": the TV workspace does not hold the group");
    const int M = p->M, N = p->N, iters = prm.iterations;
    const size_t step = tv_image_stride(p);
    float *x[kMaxGroup], *b[kMaxGroup], *w0x[kMaxGroup], *w0y[kMaxGroup];
    for (int k = 0; k < n; ++k) {
        x[k] = p->tv.x + k * step; b[k] = p->tv.b + k * step; w0x[k] = p->tv.w[0][0] + k * step; w0y[k] = p->tv.w[0][1] + k * step;
    }
    int rc = FDR_OK;
    if (iters > 0) {  // T, and b = blur^T(pad(d)) over the whole plan (mu is applied where b is read)
        rc = tv_solve_table(p, kTvPasses, prm.mu, prm.rho, s);
        if (rc == FDR_OK) rc = blur_window_dev_n(p, ws, n, d_imgs, rows, cols, stride, b, N, 1, s, M, N);
        if (rc != FDR_OK) return rc;
    }
    {
        ScopedPass t(p, s, kPassTvInit);
        FDR_HIP(launch_tv_init_n(n, d_imgs, rows, cols, stride, x, w0x, w0y, M, N, s));
    }
    for (int it = 0; it < iters && rc == FDR_OK; ++it) rc = tv_prior_half_step(p, kTvPasses, ws, n, it, prm.mu, prm.rho, prm.anisotropic, coupled, s);
    if (rc != FDR_OK) return rc;
    return tv_output_tail(p, fn, kTvPasses, ws, n, d_outs, rows, cols, out_stride, prm.nonneg, prm.norm_area, s);
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
