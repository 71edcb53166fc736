// fdr_api_rltv.hip -- Richardson-Lucy with a total-variation prior, plain and free-boundary (fdr_richardson_lucy_tv_f32*,
// fdr_rl_tv_factor_f32_dev; the kernel in fdr_rltv.hip): the workspace, the checks, one driver per form and the three entry points.
// A step is the step of the form (rl_step, rlfree_step) with the factor plane w / g in the place of the weighted update's second
// source, after one launch of the factor kernel on the estimate that enters the step.  lambda = 0 is the driver of the form itself.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

static_assert(FDR_RLTV_MAX_LAMBDA <= 0.125f, "g = 1 - lambda div >= 0.57 needs lambda <= 1 / 8 (|div| <= 2 + sqrt 2)");

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassRtFactor = "RLTV factor: w / (1 - lambda div)";

// two M x N planes, made by the first call with lambda > 0; the sticky HIP error is cleared and the plan intact when they cannot be had
int ensure_rltv_workspace(fdr_plan* p, const char* fn) {
    if (p->rt_block) return FDR_OK;
    const size_t P = (size_t)p->M * p->N;
    void* blk = nullptr;
    if (hipMalloc(&blk, 2 * P * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FDR_ERR_ALLOC, std::string(fn) + ": hipMalloc of the RLTV workspace failed");
    }
    p->rt_block = blk;
    p->rt_f = static_cast<float*>(blk);
    p->rt_u = p->rt_f + P;
    return FDR_OK;
}

int rltv_factor(fdr_plan* p, const float* u, int rows, int cols, int stride, const float* w, float lambda, float eps, hipStream_t s) {
    ScopedPass t(p, s, kPassRtFactor);
    FDR_HIP(launch_rltv_factor(u, rows, cols, stride, w, lambda, eps, p->rt_f, stride, s));
    return FDR_OK;
}

// lambda in [0, max] and eps finite and >= 0 (NaN fails both comparisons)
int prior_check(const char* fn, float lambda, float eps) {
    if (!(lambda >= 0.f && lambda <= FDR_RLTV_MAX_LAMBDA)) return fail(FDR_ERR_ARG, std::string(fn) + ": lambda must lie in [0, FDR_RLTV_MAX_LAMBDA]");
    if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(FDR_ERR_ARG, std::string(fn) + ": eps must be finite and >= 0");
    return FDR_OK;
}

fdr_rlfree_params free_params(const fdr_rl_tv_params& prm) {
    return fdr_rlfree_params{prm.iterations, prm.cov_sigma, prm.norm_area, prm.out_rows, prm.out_cols};
}

// everything the call refuses, before any device work: the prior's two numbers and what the underlying form refuses
int rltv_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
               const float* out, int out_stride, const fdr_rl_tv_params* prm) {
    if (!prm) return null_arg(fn);
    int rc = prior_check(fn, prm->lambda, prm->eps);
    if (rc != FDR_OK) return rc;
    if (prm->free_boundary) {
        const fdr_rlfree_params f = free_params(*prm);
        return rlfree_check(p, fn, img, rows, cols, stride, weights, wstride, out, out_stride, &f);
    }
    rc = rl_check(p, fn, img, rows, cols, stride, out, out_stride, prm->iterations, prm->norm_area);
    if (rc == FDR_OK)
        rc = plain_form_check(fn, weights, rows, cols, prm->out_rows, prm->out_cols, false,
                              ": the plain form's output window is the input's (out_rows, out_cols = 0 or rows, cols)");
    return rc;
}

// The plain form.  The weighted update reads the factor at the row stride of u, so u lives dense (row stride cols) in rt_u beside
// the factor in rt_f; the last update (or, for no iterations, the start) goes to the output, or under a normalisation to the raw
// plane, from where the normalise pass writes the output: the routing of rl_group_dev.
int rltv_plain_dev(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                   const fdr_rl_tv_params& prm, float eps, hipStream_t s) {
    fdr_plan::Slot* w = &p->slots[0];
    const int n = prm.iterations;
    const bool norm = prm.norm_area != FDR_NORM_NONE;
    float* fin = norm ? w->raw : d_out;
    const int fs = norm ? cols : out_stride;
    float* u = p->rt_u;
    const float* y = u;
    int rc = rl_init_estimate(p, d_img, rows, cols, stride, n == 0 ? fin : u, n == 0 ? fs : cols, s);
    for (int it = 0; it < n && rc == FDR_OK; ++it) {
        const bool last = it == n - 1;
        float* out = last ? fin : u;
        rc = rltv_factor(p, u, rows, cols, cols, nullptr, prm.lambda, eps, s);
        if (rc == FDR_OK) rc = rl_step(p, &w, 1, &d_img, stride, &y, cols, &out, last ? fs : cols, rows, cols, s, nullptr, nullptr, it, p->rt_f);
    }
    if (rc != FDR_OK || !norm) return rc;
    return rl_normalize(p, fn, fin, fs, rows, cols, prm.norm_area, d_out, out_stride, s);
}

// The free-boundary form: begin and finish of that form, the steps in place in rf_u with factor = wgt / g in the place of wgt.
int rltv_free_dev(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* d_out,
                  int out_stride, const fdr_rl_tv_params& prm, float eps, hipStream_t s) {
    fdr_plan::Slot* w = &p->slots[0];
    const fdr_rlfree_params f = free_params(prm);
    int rc = rlfree_begin(p, d_img, rows, cols, stride, d_w, wstride, f.sigma, nullptr, nullptr, s);
    float* u = p->rf_u;
    const float* y = u;
    const float* dw = p->rf_dw;
    for (int it = 0; it < prm.iterations && rc == FDR_OK; ++it) {
        rc = rltv_factor(p, u, p->M, p->N, p->N, p->rf_wgt, prm.lambda, eps, s);
        if (rc == FDR_OK) rc = rlfree_step(p, &w, 1, &y, &u, &dw, p->rt_f, rows, cols, s);
    }
    if (rc != FDR_OK) return rc;
    return rlfree_finish(p, fn, u, d_out, out_stride, f, s);
}

// one image on slot 0; lambda = 0: the driver of the form, nothing of this file
int rltv_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* d_out,
                  int out_stride, const fdr_rl_tv_params& prm, hipStream_t s) {
    const float eps = prm.eps == 0.f ? FDR_RLTV_EPS : prm.eps;
    if (prm.free_boundary) {
        if (prm.lambda == 0.f) return rlfree_batch_dev(p, fn, d_img, 0, 1, rows, cols, stride, d_w, wstride, d_out, 0, out_stride, free_params(prm), s);
        return rltv_free_dev(p, fn, d_img, rows, cols, stride, d_w, wstride, d_out, out_stride, prm, eps, s);
    }
    if (prm.lambda == 0.f) {
        fdr_plan::Slot* w = &p->slots[0];
        return rl_group_dev(p, fn, &w, 1, &d_img, rows, cols, stride, &d_out, out_stride, prm.iterations, prm.norm_area, s);
    }
    return rltv_plain_dev(p, fn, d_img, rows, cols, stride, d_out, out_stride, prm, eps, s);
}

int ensure_workspaces(fdr_plan* p, const char* fn, const fdr_rl_tv_params& prm) {
    int rc = prm.free_boundary ? ensure_rlfree_workspace(p, fn) : FDR_OK;
    if (rc == FDR_OK && prm.lambda != 0.f) rc = ensure_rltv_workspace(p, fn);
    return rc;
}

}  // namespace

extern "C" {

int fdr_richardson_lucy_tv_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                                   float* d_out, int out_stride, const fdr_rl_tv_params* params, void* stream) {
    const char* fn = "fdr_richardson_lucy_tv_f32_dev";
    if (!p || !d_img || !d_out) return null_arg(fn);
    int rc = rltv_check(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = ensure_workspaces(p, fn, *params);
    if (rc != FDR_OK) return rc;
    return rltv_dev_impl(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, *params, (hipStream_t)stream);
}

int fdr_richardson_lucy_tv_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                               float* out_host, int out_stride, const fdr_rl_tv_params* params) {
    const char* fn = "fdr_richardson_lucy_tv_f32";
    if (!p || !img_host || !out_host) return null_arg(fn);
    int rc = rltv_check(p, fn, img_host, rows, cols, stride, weights_host, wstride, out_host, out_stride, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const fdr_rl_tv_params prm = *params;
    rc = ensure_workspaces(p, fn, prm);
    if (rc != FDR_OK) return rc;
    const bool free_form = prm.free_boundary != 0;
    if (free_form && weights_host) rc = stage_weights(p, weights_host, rows, cols, wstride);
    if (rc != FDR_OK) return rc;
    const int orows = free_form ? prm.out_rows : rows, ocols = free_form ? prm.out_cols : cols;
    return host_image_call(p, fn, img_host, rows, cols, stride, out_host, orows, ocols, out_stride, [&](const float* d_in, float* d_out) {
        return rltv_dev_impl(p, fn, d_in, rows, cols, cols, free_form && weights_host ? p->rf_u : nullptr, cols, d_out, ocols, prm, nullptr);
    });
}

int fdr_rl_tv_factor_f32_dev(int device, const float* d_u, int rows, int cols, int stride, const float* d_w, float lambda, float eps,
                             float* d_out, int out_stride, void* stream) {
    const char* fn = "fdr_rl_tv_factor_f32_dev";
    if (!d_u || !d_out) return null_arg(fn);
    if (rows <= 0 || cols <= 0) return fail(FDR_ERR_ARG, std::string(fn) + ": rows and cols must be positive");
    if (stride < cols || out_stride < cols) return fail(FDR_ERR_ARG, std::string(fn) + ": a stride below cols");
    const int rc = prior_check(fn, lambda, eps);
    if (rc != FDR_OK) return rc;
    const ByteRange o = window_range(d_out, rows, cols, out_stride);
    if (ranges_overlap(window_range(d_u, rows, cols, stride), o) || (d_w && ranges_overlap(window_range(d_w, rows, cols, stride), o)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps an input");
    FDR_HIP(hipSetDevice(device));
    FDR_HIP(launch_rltv_factor(d_u, rows, cols, stride, d_w, lambda, eps == 0.f ? FDR_RLTV_EPS : eps, d_out, out_stride, (hipStream_t)stream));
    return FDR_OK;
}

}  // extern "C"
