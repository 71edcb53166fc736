// fdr_api_rlfree.hip -- free-boundary, weighted Richardson-Lucy, plain and accelerated (fdr_richardson_lucy_free_f32*, _free_accel_f32*;
// kernels in fdr_rlfree.hip and the weighted update kind of fdr_panel_rows.hip): the workspace, the checks, the one step and the one
// driver of the form, both on a group of n >= 1 images, and the four entry points.  The single call is a batch of one image; the
// batch (fdr_api_rlbatch.hip) and the blind call (fdr_api_blind.hip) run the same driver, which also runs the accelerated recursion
// (rl_accel_loop) on a launch group; the auto call (fdr_api_rlstop.hip) has its own loop around the same step.  Every transform is an operator pass of
// fdr_api_operator.hip: the estimate goes through pass A as a dense M x N plane, the ratio through the window.
#include "fdr_host.hpp"

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassRfSetup = "RLF setup: dw, W, sums";
const char* const kPassRfStart = "RLF start: wgt = 1/alpha, u";
const char* const kPassRfRatio = "C op rows: IFFT+RL ratio (free)";
const char* const kPassRfRatioFit = "C op rows: IFFT+RL ratio+fit (free)";
const char* const kPassRfUpdate = "C op rows: IFFT+RL update (weighted)";
const char* const kPassRfCrop = "RLF out: crop";
const char* const kPassRfNorm = "E RLF minmax+normalize";

}  // namespace

namespace fdr {

// The workspace of the free-boundary calls: the first call of a plan makes the three planes of one image; a batched call on groups
// of g images grows it to 1 + 2 g planes on its first use.
int ensure_rlfree_workspace(fdr_plan* p, const char* fn, int group) {
    return ensure_workspace(p->rlfree.ws, fn, "free-boundary workspace", group, [p](auto& c, int g) {
        layout(c, p->rlfree, (size_t)p->M * p->N, 2 * (size_t)rlfree_partials(p->M, p->N) + 2, g);
    });
}

}  // namespace fdr

namespace {

// image k of a group: its dense M x N estimate, its dw and the partials of its sums
float* rlfree_u_plane(const fdr_plan* p, int k) { return k == 0 ? p->rlfree.u : p->rlfree.u + (size_t)(1 + 2 * k) * p->M * p->N; }
float* rlfree_dw_plane(const fdr_plan* p, int k) { return k == 0 ? p->rlfree.dw : p->rlfree.u + (size_t)(2 + 2 * k) * p->M * p->N; }
double* rlfree_part(const fdr_plan* p, int k) { return p->rlfree.part + (size_t)k * (2 * (size_t)rlfree_partials(p->M, p->N) + 2); }

// setup: dw and W = pad(m) dense into `dw` and `W` (W also to keep_w when that is not null), the two sums behind the partials at
// `part`; *sums is where the device holds (sum dw, sum W).  d_w may be W's plane itself.
int rlfree_setup_image(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* dw, float* W,
                       double* part, float* keep_w, const double** sums, hipStream_t s) {
    ScopedPass t(p, s, kPassRfSetup);
    FDR_HIP(launch_rlfree_setup(d_img, stride, d_w, wstride, rows, cols, dw, W, part, s));
    if (keep_w) FDR_HIP(hipMemcpyAsync(keep_w, W, (size_t)rows * cols * sizeof(float), hipMemcpyDeviceToDevice, s));
    *sums = part + 2 * (size_t)rlfree_partials(rows, cols);
    return FDR_OK;
}
// start: the M x N plane `alpha` becomes alpha > sigma ? 1 / alpha : 0 and u = alpha > sigma ? sum dw / sum W : 0
int rlfree_start_image(fdr_plan* p, float* alpha, float* u, float sigma, const double* sums, hipStream_t s) {
    ScopedPass t(p, s, kPassRfStart);
    FDR_HIP(launch_rlfree_start(alpha, u, (size_t)p->M * p->N, sigma, sums, s));
    return FDR_OK;
}

}  // namespace

namespace fdr {

// everything a free-boundary call refuses, before any device work: what the Richardson-Lucy calls refuse, and sigma, the output
// window and an output that overlaps the weights
int rlfree_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
                 const float* out, int out_stride, const fdr_rlfree_params* prm, PlanNeed need) {
    if (!prm) return null_arg(fn);
    const int rc = check_window(p, fn, need, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    if (weights && wstride < cols) return fail(FDR_ERR_ARG, std::string(fn) + ": the weights' stride must be >= cols");
    if (prm->iterations < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": iterations < 0");
    if (!(prm->sigma > 0.f && prm->sigma < 1.f)) return fail(FDR_ERR_ARG, std::string(fn) + ": sigma must lie in (0, 1)");
    if (prm->norm_area != FDR_NORM_NONE && prm->norm_area != FDR_NORM_CROPPED && prm->norm_area != FDR_NORM_PADDED)
        return fail(FDR_ERR_ARG, std::string(fn) + ": unknown norm_area");
    if (prm->out_rows < rows || prm->out_rows > p->M || prm->out_cols < cols || prm->out_cols > p->N || out_stride < prm->out_cols)
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output window must lie in [rows .. M] x [cols .. N] and have a stride >= out_cols");
    const ByteRange o = window_range(out, prm->out_rows, prm->out_cols, out_stride);
    if (ranges_overlap(window_range(img, rows, cols, stride), o)) return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the input");
    if (weights && ranges_overlap(window_range(weights, rows, cols, wstride), o))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the weights");
    return FDR_OK;
}

int stage_weights(fdr_plan* p, const float* weights_host, int rows, int cols, int wstride) {
    FDR_HIP(hipMemcpy2D(p->rlfree.u, (size_t)cols * sizeof(float), weights_host, (size_t)wstride * sizeof(float), (size_t)cols * sizeof(float),
                        (size_t)rows, hipMemcpyHostToDevice));
    return FDR_OK;
}

int rlfree_step(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float* const* ys, float* const* outs, const float* const* datums,
                const float* wgt, int rows, int cols, hipStream_t s, const RlFit* fit, const RlHooks* hooks, int it, size_t wgt_pitch) {
    if (hooks && n > 1) return fail(FDR_ERR_STATE, "rlfree_step: the hooks take one image per step");
    const int M = p->M, N = p->N;
    float* r[kMaxGroup];
    for (int k = 0; k < n; ++k) r[k] = ws[k]->raw;
    int rc = op_rows_fwd_n(p, ws, n, ys, M, N, N, s);                                                // c = fullblur(y) ...
    if (rc == FDR_OK && hooks && hooks->after_fwd) rc = hooks->after_fwd(it);
    if (rc == FDR_OK) rc = op_cols_n(p, ws, n, false, s);
    if (rc == FDR_OK)                                                                                // ... r = dw / c
        rc = op_rows_inv_n(p, ws, n, fit ? ROW_OUT_RL_RATIO_STAT : ROW_OUT_RL_RATIO, fit ? kPassRfRatioFit : kPassRfRatio, datums, cols, nullptr, r,
                           cols, rows, cols, s, fit);
    if (rc == FDR_OK && hooks && hooks->after_ratio) rc = hooks->after_ratio(it);
    if (rc == FDR_OK) rc = op_rows_fwd_n(p, ws, n, r, rows, cols, cols, s);                          // g = fullblur^T(pad(r)) ...
    if (rc == FDR_OK) rc = op_cols_n(p, ws, n, true, s);
    if (rc == FDR_OK) rc = op_rows_inv_n(p, ws, n, ROW_OUT_RL_UPDATE_W, kPassRfUpdate, ys, N, wgt, outs, N, M, N, s, nullptr, wgt_pitch);  // ... out = max(y wgt g, 0)
    return rc;
}

// u and wgt are dense M x N planes of the workspace, dw and r (the slot's raw plane) dense rows x cols.  W = pad(m) lies in u's
// plane until alpha has been transformed out of it.
int rlfree_begin(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float sigma, float* keep_w,
                 const double** sums, hipStream_t s) {
    const double* sm = nullptr;
    int rc = rlfree_setup_image(p, d_img, rows, cols, stride, d_w, wstride, p->rlfree.dw, p->rlfree.u, p->rlfree.part, keep_w, &sm, s);
    if (rc == FDR_OK) rc = blur_window_dev(p, p->rlfree.u, rows, cols, cols, p->rlfree.wgt, p->N, p->M, p->N, 1, s);  // alpha over the whole plan
    if (rc == FDR_OK) rc = rlfree_start_image(p, p->rlfree.wgt, p->rlfree.u, sigma, sm, s);
    if (sums) *sums = sm;
    return rc;
}

int rlfree_finish(fdr_plan* p, const char* fn, const float* u, float* d_out, int out_stride, const fdr_rlfree_params& prm, hipStream_t s) {
    if (prm.norm_area == FDR_NORM_NONE) {
        ScopedPass t(p, s, kPassRfCrop);
        FDR_HIP(launch_rlfree_crop(u, p->N, d_out, prm.out_rows, prm.out_cols, out_stride, s));
        return FDR_OK;
    }
    return normalize_window(p, fn, kPassRfNorm, u, p->N, prm.out_rows, prm.out_cols, prm.norm_area, d_out, out_stride, s);
}

// The weights serve every image, so the coverage alpha = fullblur^T(W) and wgt = 1 / alpha are computed once per call, by the begin
// of image 0.  Every other image runs the same setup (its dw and its sums; W again, into its own u plane, which the start
// overwrites) and the same start kernel on a copy of wgt in its slot's raw plane with the threshold 0: wgt > 0 exactly where
// alpha > sigma (for a finite alpha), so u = sum dw / sum W there and 0 elsewhere, the bits of the single call.  With groups of one
// image that copy would replace the coverage passes of the single calls, so several images are the loop of batches of one.
int rlfree_batch_dev(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride, const float* d_w,
                     int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_rlfree_params& prm, hipStream_t s, const RlHooks* hooks,
                     float* keep_w, bool accel, float* d_alphas, size_t alpha_pitch, const RlTvPrior* tv) {
    if (accel && hooks) return fail(FDR_ERR_STATE, "rlfree_batch_dev: the accelerated recursion takes no hooks");
    const int group = launch_group(p, count);
    if (tv && (accel || hooks || group == 1 || p->rltv.ws.count < group))
        return fail(FDR_ERR_STATE, "rlfree_batch_dev: the prior takes launch groups of several images, plain steps and its workspace");
    const size_t P = (size_t)p->M * p->N;
    int rc = FDR_OK;
    if (group == 1 && count > 1) {  // the loop of the single-image calls, each with its own coverage
        for (int i = 0; i < count && rc == FDR_OK; ++i)
            rc = rlfree_batch_dev(p, fn, d_imgs + (size_t)i * img_pitch, 0, 1, rows, cols, stride, d_w, wstride, d_out + (size_t)i * out_pitch, 0,
                                  out_stride, prm, s, hooks, keep_w, accel, d_alphas ? d_alphas + (size_t)i * alpha_pitch : nullptr, 0);
        return rc;
    }
    rc = rlfree_begin(p, d_imgs, rows, cols, stride, d_w, wstride, prm.sigma, keep_w, nullptr, s);
    if (rc == FDR_OK && tv)  // the prior's estimates lie one pitch apart, in its own workspace: image 0's start goes there
        FDR_HIP(hipMemcpyAsync(p->rltv.u, p->rlfree.u, P * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const LaunchGroup g(p, i0, count, d_imgs, img_pitch, d_out, out_pitch);
        float* us[kMaxGroup];
        const float* dws[kMaxGroup];
        for (int k = 0; k < g.n && rc == FDR_OK; ++k) {
            us[k] = tv ? p->rltv.u + (size_t)k * P : rlfree_u_plane(p, k); dws[k] = rlfree_dw_plane(p, k);
            if (i0 + k == 0) continue;  // begun above
            const double* sums = nullptr;
            rc = rlfree_setup_image(p, g.ins[k], rows, cols, stride, d_w, wstride, rlfree_dw_plane(p, k), us[k], rlfree_part(p, k), nullptr, &sums, s);
            if (rc != FDR_OK) break;
            FDR_HIP(hipMemcpyAsync(g.ws[k]->raw, p->rlfree.wgt, (size_t)p->M * p->N * sizeof(float), hipMemcpyDeviceToDevice, s));
            rc = rlfree_start_image(p, g.ws[k]->raw, us[k], 0.f, sums, s);
        }
        float* fin[kMaxGroup];  // where u_n lies
        for (int k = 0; k < g.n; ++k) fin[k] = us[k];
        if (accel && rc == FDR_OK) {  // the estimate alternates between image k's u plane and its plane of the acceleration workspace
            float* U[kMaxGroup][2];
            for (int k = 0; k < g.n; ++k) { U[k][0] = us[k]; U[k][1] = rlaccel_u_plane(p, k); }
            const int strides[2] = {p->N, p->N};
            rc = rl_accel_loop(p, g.n, prm.iterations, p->M, p->N, U, strides, 0, nullptr, 0, d_alphas ? d_alphas + (size_t)i0 * alpha_pitch : nullptr,
                               alpha_pitch, s, [&](const float* const* ys, int, float* const* outs, int) {
                                   return rlfree_step(p, g.ws, g.n, ys, outs, dws, p->rlfree.wgt, rows, cols, s);
                               }, fin);
        }
        for (int it = 0; it < prm.iterations && rc == FDR_OK && !accel; ++it) {
            if (tv) rc = rltv_factor_group(p, g.n, p->M, p->N, p->N, p->rlfree.wgt, *tv, s);  // factor_k = wgt / g_k from the u_k that enter the step
            if (rc == FDR_OK) rc = rlfree_step(p, g.ws, g.n, us, us, dws, tv ? p->rltv.f : p->rlfree.wgt, rows, cols, s, nullptr, hooks, it, tv ? P : 0);
            if (rc == FDR_OK && hooks && hooks->after_step) rc = hooks->after_step(it);
        }
        for (int k = 0; k < g.n && rc == FDR_OK; ++k) rc = rlfree_finish(p, fn, fin[k], g.outs[k], out_stride, prm, s);
    }
    return rc;
}

}  // namespace fdr

namespace {

// One image: the driver on a batch of one, plain or accelerated
int rlfree_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride,
                    float* d_out, int out_stride, const fdr_rlfree_params& prm, bool accel, float* d_alphas, hipStream_t s) {
    return rlfree_batch_dev(p, fn, d_img, 0, 1, rows, cols, stride, d_w, wstride, d_out, 0, out_stride, prm, s, nullptr, nullptr, accel, d_alphas, 0);
}

// the checks, the device, the workspaces and the driver of the four entry points; the accelerated ones also refuse alphas that
// overlap a window
int rlfree_dev_entry(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                     float* d_out, int out_stride, const fdr_rlfree_params* params, bool accel, float* d_alphas, hipStream_t s) {
    if (!p || !d_img || !d_out) return null_arg(fn);
    int rc = rlfree_check(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, params);
    if (rc == FDR_OK && accel)
        rc = check_alphas(fn, d_alphas, params->iterations, d_out, out_stride, params->out_rows, params->out_cols, "output");
    if (rc == FDR_OK && accel) rc = check_alphas(fn, d_alphas, params->iterations, d_img, stride, rows, cols, "input");
    if (rc == FDR_OK && accel && d_weights) rc = check_alphas(fn, d_alphas, params->iterations, d_weights, wstride, rows, cols, "weights");
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = ensure_rlfree_workspace(p, fn);
    if (rc == FDR_OK && accel) rc = ensure_rlaccel_workspace(p, fn);
    if (rc != FDR_OK) return rc;
    return rlfree_dev_impl(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, *params, accel, d_alphas, s);
}

int rlfree_host_entry(fdr_plan* p, const char* fn, const float* img_host, int rows, int cols, int stride, const float* weights_host,
                      int wstride, float* out_host, int out_stride, const fdr_rlfree_params* params, bool accel, float* alphas_host) {
    if (!p || !img_host || !out_host) return null_arg(fn);
    int rc = rlfree_check(p, fn, img_host, rows, cols, stride, weights_host, wstride, out_host, out_stride, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = ensure_rlfree_workspace(p, fn);
    if (rc == FDR_OK && accel) rc = ensure_rlaccel_workspace(p, fn);
    if (rc != FDR_OK) return rc;
    const fdr_rlfree_params prm = *params;
    return with_host_alphas(fn, alphas_host, prm.iterations, [&](float* d_alphas) {
        int rc2 = weights_host ? stage_weights(p, weights_host, rows, cols, wstride) : FDR_OK;
        if (rc2 != FDR_OK) return rc2;
        return host_image_call(p, fn, img_host, rows, cols, stride, out_host, prm.out_rows, prm.out_cols, out_stride,
                               [&](const float* d_in, float* d_out) {
                                   return rlfree_dev_impl(p, fn, d_in, rows, cols, cols, weights_host ? p->rlfree.u : nullptr, cols, d_out, prm.out_cols,
                                                          prm, accel, d_alphas, nullptr);
                               });
    });
}

}  // namespace

extern "C" {

int fdr_richardson_lucy_free_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                                     float* d_out, int out_stride, const fdr_rlfree_params* params, void* stream) {
    return rlfree_dev_entry(p, "fdr_richardson_lucy_free_f32_dev", d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, params,
                            false, nullptr, (hipStream_t)stream);
}

int fdr_richardson_lucy_free_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                                 float* out_host, int out_stride, const fdr_rlfree_params* params) {
    return rlfree_host_entry(p, "fdr_richardson_lucy_free_f32", img_host, rows, cols, stride, weights_host, wstride, out_host, out_stride,
                             params, false, nullptr);
}

int fdr_richardson_lucy_free_accel_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_weights,
                                           int wstride, float* d_out, int out_stride, const fdr_rlfree_params* params, float* d_alphas,
                                           void* stream) {
    return rlfree_dev_entry(p, "fdr_richardson_lucy_free_accel_f32_dev", d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride,
                            params, true, d_alphas, (hipStream_t)stream);
}

int fdr_richardson_lucy_free_accel_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const float* weights_host,
                                       int wstride, float* out_host, int out_stride, const fdr_rlfree_params* params, float* alphas_host) {
    return rlfree_host_entry(p, "fdr_richardson_lucy_free_accel_f32", img_host, rows, cols, stride, weights_host, wstride, out_host,
                             out_stride, params, true, alphas_host);
}

}  // extern "C"
