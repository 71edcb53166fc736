// fdr_api_rltv.hip -- Richardson-Lucy with a total-variation prior, plain and free-boundary (fdr_richardson_lucy_tv_f32*,
// fdr_rl_tv_factor_f32_dev; the kernel in fdr_rltv.hip): the workspace, the checks, one driver per form and the three entry points.
// A step is the step of the form (rl_step, rlfree_step) with the factor plane w / g in the place of the weighted update's second
// source, after one launch of the factor kernel on the estimate that enters the step.  lambda = 0 is the driver of the form itself.
// The batch (fdr_richardson_lucy_tv_batch_f32*, fdr_rl_tv_factor_group_f32_dev) runs launch groups: one factor launch for the group,
// coupled over the channels or not, then the step of the form on the group with image k's factor plane as its second source.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

static_assert(FDR_RLTV_MAX_LAMBDA <= 0.125f, "g = 1 - lambda div >= 0.57 needs lambda <= 1 / 8 (|div| <= 2 + sqrt 2)");

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassRtFactor = "RLTV factor: w / (1 - lambda div)";
const char* const kPassRtFactorGroup = "RLTV factor (group): w / (1 - lambda div)";
const char* const kPassRtFactorCoupled = "RLTV factor (coupled): w / (1 - lambda div p_c)";

}  // namespace

namespace fdr {

// made by the first call with lambda > 0 for one image and grown by the first batched call on groups of g
int ensure_rltv_workspace(fdr_plan* p, const char* fn, int group) {
    return ensure_workspace(p->rltv.ws, fn, "RLTV workspace", group, [p](auto& c, int g) { layout(c, p->rltv, (size_t)p->M * p->N, g); });
}

int rltv_factor(fdr_plan* p, const float* u, int rows, int cols, int stride, const float* w, float lambda, float eps, hipStream_t s) {
    ScopedPass t(p, s, kPassRtFactor);
    FDR_HIP(launch_rltv_factor(u, rows, cols, stride, w, lambda, eps, p->rltv.f, stride, s));
    return FDR_OK;
}

// lambda in [0, max] and eps finite and >= 0 (NaN fails both comparisons)
int prior_check(const char* fn, float lambda, float eps) {
    if (!(lambda >= 0.f && lambda <= FDR_RLTV_MAX_LAMBDA)) return fail(FDR_ERR_ARG, std::string(fn) + ": lambda must lie in [0, FDR_RLTV_MAX_LAMBDA]");
    if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(FDR_ERR_ARG, std::string(fn) + ": eps must be finite and >= 0");
    return FDR_OK;
}

}  // namespace fdr

namespace {

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

// the plain form on a launch group of n > 1 images: image k's estimate dense in rltv.u + k M N beside its factor in rltv.f + k M N, the
// routing of rltv_plain_dev per image, one factor launch and one step for the group per iteration
int rltv_plain_group_dev(fdr_plan* p, const char* fn, const LaunchGroup& g, int rows, int cols, int stride, int out_stride,
                         const fdr_rl_tv_batch_params& prm, const RlTvPrior& tv, hipStream_t s) {
    const size_t P = (size_t)p->M * p->N;
    const int n = prm.iterations;
    const bool norm = prm.norm_area != FDR_NORM_NONE;
    const int fs = norm ? cols : out_stride;
    float *fin[kMaxGroup], *us[kMaxGroup];
    for (int k = 0; k < g.n; ++k) { fin[k] = norm ? g.ws[k]->raw : g.outs[k]; us[k] = p->rltv.u + (size_t)k * P; }
    int rc = FDR_OK;
    for (int k = 0; k < g.n && rc == FDR_OK; ++k) rc = rl_init_estimate(p, g.ins[k], rows, cols, stride, n == 0 ? fin[k] : us[k], n == 0 ? fs : cols, s);
    for (int it = 0; it < n && rc == FDR_OK; ++it) {
        const bool last = it == n - 1;
        rc = rltv_factor_group(p, g.n, rows, cols, cols, nullptr, tv, s);
        if (rc == FDR_OK)
            rc = rl_step(p, g.ws, g.n, g.ins, stride, us, cols, last ? fin : us, last ? fs : cols, rows, cols, s, nullptr, nullptr, it, p->rltv.f, P);
    }
    for (int k = 0; k < g.n && rc == FDR_OK && norm; ++k) rc = rl_normalize(p, fn, fin[k], fs, rows, cols, prm.norm_area, g.outs[k], out_stride, s);
    return rc;
}

// The plain form.  The weighted update reads the factor at the row stride of u, so u lives dense (row stride cols) in rltv.u beside
// the factor in rltv.f; the last update (or, for no iterations, the start) goes to the output, or under a normalisation to the raw
// plane, from where the normalise pass writes the output: the routing of rl_group_dev.
int rltv_plain_dev(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                   const fdr_rl_tv_params& prm, float eps, hipStream_t s) {
    fdr_plan::Slot* w = &p->slots[0];
    const int n = prm.iterations;
    const bool norm = prm.norm_area != FDR_NORM_NONE;
    float* fin = norm ? w->raw : d_out;
    const int fs = norm ? cols : out_stride;
    float* u = p->rltv.u;
    const float* y = u;
    int rc = rl_init_estimate(p, d_img, rows, cols, stride, n == 0 ? fin : u, n == 0 ? fs : cols, s);
    for (int it = 0; it < n && rc == FDR_OK; ++it) {
        const bool last = it == n - 1;
        float* out = last ? fin : u;
        rc = rltv_factor(p, u, rows, cols, cols, nullptr, prm.lambda, eps, s);
        if (rc == FDR_OK) rc = rl_step(p, &w, 1, &d_img, stride, &y, cols, &out, last ? fs : cols, rows, cols, s, nullptr, nullptr, it, p->rltv.f);
    }
    if (rc != FDR_OK || !norm) return rc;
    return rl_normalize(p, fn, fin, fs, rows, cols, prm.norm_area, d_out, out_stride, s);
}

// The free-boundary form: begin and finish of that form, the steps in place in rlfree.u with factor = wgt / g in the place of wgt.
int rltv_free_dev(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* d_out,
                  int out_stride, const fdr_rl_tv_params& prm, float eps, hipStream_t s) {
    fdr_plan::Slot* w = &p->slots[0];
    const fdr_rlfree_params f = free_params(prm);
    int rc = rlfree_begin(p, d_img, rows, cols, stride, d_w, wstride, f.sigma, nullptr, nullptr, s);
    float* u = p->rlfree.u;
    const float* y = u;
    const float* dw = p->rlfree.dw;
    for (int it = 0; it < prm.iterations && rc == FDR_OK; ++it) {
        rc = rltv_factor(p, u, p->M, p->N, p->N, p->rlfree.wgt, prm.lambda, eps, s);
        if (rc == FDR_OK) rc = rlfree_step(p, &w, 1, &y, &u, &dw, p->rltv.f, rows, cols, s);
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

fdr_rl_tv_params single_params(const fdr_rl_tv_batch_params& b) {
    return fdr_rl_tv_params{b.iterations, b.free_boundary, b.lambda, b.eps, b.norm_area, b.cov_sigma, b.out_rows, b.out_cols};
}
fdr_rl_batch_params plain_batch_params(const fdr_rl_tv_batch_params& b) {
    return fdr_rl_batch_params{b.iterations, b.norm_area, b.free_boundary, b.cov_sigma, b.out_rows, b.out_cols};
}

// what the batch refuses, before any device work: the prior's numbers, `couple`, what fdr_richardson_lucy_batch_f32* refuses and,
// coupled, a batch of more than one launch group
int rltv_batch_check(const fdr_plan* p, const char* fn, const float* imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                     const float* weights, int wstride, const float* out, size_t out_pitch, int out_stride, const fdr_rl_tv_batch_params& b,
                     fdr_rlfree_params* free_prm) {
    int rc = prior_check(fn, b.lambda, b.eps);
    if (rc != FDR_OK) return rc;
    if (b.couple != FDR_TV_COUPLE_NONE && b.couple != FDR_TV_COUPLE_CHANNELS) return fail(FDR_ERR_ARG, std::string(fn) + ": unknown couple");
    rc = rl_batch_check(p, fn, imgs, img_pitch, count, rows, cols, stride, weights, wstride, out, out_pitch, out_stride, plain_batch_params(b), free_prm);
    if (rc != FDR_OK) return rc;
    if (b.couple == FDR_TV_COUPLE_CHANNELS && count > p->group)
        return fail(FDR_ERR_ARG, std::string(fn) + ": coupled channels must form one launch group (count <= group of fdr_plan_set_batching)");
    return FDR_OK;
}

// checked arguments -> the workspaces -> the drivers, group by group.  lambda = 0: the batch without the prior; groups of one
// (uncoupled): the loop of the single calls
int rltv_batch_run(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride, const float* d_w,
                   int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_rl_tv_batch_params& b, const fdr_rlfree_params& free_prm,
                   hipStream_t s) {
    if (b.lambda == 0.f)
        return rl_batch_run(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_w, wstride, d_out, out_pitch, out_stride, plain_batch_params(b), free_prm, s);
    const int group = launch_group(p, count);
    const bool coupled = b.couple == FDR_TV_COUPLE_CHANNELS && count > 1;  // (one channel: its own norm, the single call)
    int rc = b.free_boundary ? ensure_rlfree_workspace(p, fn, group) : FDR_OK;
    if (rc == FDR_OK) rc = ensure_rltv_workspace(p, fn, group);
    if (rc != FDR_OK) return rc;
    const RlTvPrior tv{b.lambda, b.eps == 0.f ? FDR_RLTV_EPS : b.eps, coupled};
    if (group == 1) {
        const fdr_rl_tv_params one = single_params(b);
        for (int i = 0; i < count && rc == FDR_OK; ++i)
            rc = rltv_dev_impl(p, fn, d_imgs + (size_t)i * img_pitch, rows, cols, stride, d_w, wstride, d_out + (size_t)i * out_pitch, out_stride, one, s);
        return rc;
    }
    if (b.free_boundary)
        return rlfree_batch_dev(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_w, wstride, d_out, out_pitch, out_stride, free_prm, s, nullptr,
                                nullptr, false, nullptr, 0, &tv);
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const LaunchGroup g(p, i0, count, d_imgs, img_pitch, d_out, out_pitch);
        rc = rltv_plain_group_dev(p, fn, g, rows, cols, stride, out_stride, b, tv, s);
    }
    return rc;
}

int ensure_workspaces(fdr_plan* p, const char* fn, const fdr_rl_tv_params& prm) {
    int rc = prm.free_boundary ? ensure_rlfree_workspace(p, fn) : FDR_OK;
    if (rc == FDR_OK && prm.lambda != 0.f) rc = ensure_rltv_workspace(p, fn);
    return rc;
}

}  // namespace

namespace fdr {

int rltv_factor_group(fdr_plan* p, int n, int rows, int cols, int stride, const float* w, const RlTvPrior& tv, hipStream_t s) {
    const size_t P = (size_t)p->M * p->N;
    if (n < 1 || n > p->rltv.ws.count) return fail(FDR_ERR_STATE, "rltv_factor_group: the workspace does not hold the group");
    ScopedPass t(p, s, tv.coupled ? kPassRtFactorCoupled : kPassRtFactorGroup);
    FDR_HIP(launch_rltv_factor_group(p->rltv.u, P, n, rows, cols, stride, w, tv.lambda, tv.eps, p->rltv.f, P, stride, tv.coupled, s));
    return FDR_OK;
}

}  // namespace fdr

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
        return rltv_dev_impl(p, fn, d_in, rows, cols, cols, free_form && weights_host ? p->rlfree.u : nullptr, cols, d_out, ocols, prm, nullptr);
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

int fdr_richardson_lucy_tv_batch_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                         const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                         const fdr_rl_tv_batch_params* params, void* stream) {
    const char* fn = "fdr_richardson_lucy_tv_batch_f32_dev";
    if (!p || !params) return null_arg(fn);
    if (count < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": negative count");
    if (count == 0) return FDR_OK;
    if (!d_imgs || !d_out) return null_arg(fn);
    fdr_rlfree_params free_prm{};
    const int rc = rltv_batch_check(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, *params, &free_prm);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return rltv_batch_run(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, *params, free_prm,
                          (hipStream_t)stream);
}

// host pointers: every image in (dense), the batch on the null stream, every result back; one-shot device buffers
int fdr_richardson_lucy_tv_batch_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                     const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                     const fdr_rl_tv_batch_params* params) {
    const char* fn = "fdr_richardson_lucy_tv_batch_f32";
    if (!p || !params) return null_arg(fn);
    if (count < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": negative count");
    if (count == 0) return FDR_OK;
    if (!imgs_host || !out_host) return null_arg(fn);
    fdr_rlfree_params free_prm{};
    const fdr_rl_tv_batch_params b = *params;
    int rc = rltv_batch_check(p, fn, imgs_host, img_pitch, count, rows, cols, stride, weights_host, wstride, out_host, out_pitch, out_stride, b, &free_prm);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const int out_rows = b.free_boundary ? b.out_rows : rows, out_cols = b.free_boundary ? b.out_cols : cols;
    const size_t in_px = (size_t)rows * cols, out_px = (size_t)out_rows * out_cols;
    DeviceBuffer d_in, d_out, d_w;
    FDR_ALLOC(d_in, (size_t)count * in_px * sizeof(float), fn);
    FDR_ALLOC(d_out, (size_t)count * out_px * sizeof(float), fn);
    if (weights_host) FDR_ALLOC(d_w, in_px * sizeof(float), fn);
    {
        ScopedPhase phase(p, FDR_PHASE_H2D, nullptr);
        for (int i = 0; i < count; ++i)
            FDR_HIP(hipMemcpy2D(d_in.as<float>() + (size_t)i * in_px, (size_t)cols * sizeof(float), imgs_host + (size_t)i * img_pitch,
                                (size_t)stride * sizeof(float), (size_t)cols * sizeof(float), (size_t)rows, hipMemcpyHostToDevice));
        if (weights_host)
            FDR_HIP(hipMemcpy2D(d_w.ptr, (size_t)cols * sizeof(float), weights_host, (size_t)wstride * sizeof(float), (size_t)cols * sizeof(float),
                                (size_t)rows, hipMemcpyHostToDevice));
    }
    {
        ScopedPhase phase(p, FDR_PHASE_COMPUTE, nullptr);
        rc = rltv_batch_run(p, fn, d_in.as<float>(), in_px, count, rows, cols, cols, d_w.as<float>(), cols, d_out.as<float>(), out_px, out_cols, b,
                            free_prm, nullptr);
    }
    if (rc == FDR_OK) {
        ScopedPhase phase(p, FDR_PHASE_D2H, nullptr);
        for (int i = 0; i < count; ++i)
            FDR_HIP(hipMemcpy2D(out_host + (size_t)i * out_pitch, (size_t)out_stride * sizeof(float), d_out.as<float>() + (size_t)i * out_px,
                                (size_t)out_cols * sizeof(float), (size_t)out_cols * sizeof(float), (size_t)out_rows, hipMemcpyDeviceToHost));
    }
    (void)hipStreamSynchronize(nullptr);  // (also on an error: the one-shot buffers are freed on return)
    resolve_phases(p);
    return rc;
}

int fdr_rl_tv_factor_group_f32_dev(int device, const float* d_u, size_t u_pitch, int count, int rows, int cols, int stride, const float* d_w,
                                   float lambda, float eps, int couple, float* d_out, size_t out_pitch, int out_stride, void* stream) {
    const char* fn = "fdr_rl_tv_factor_group_f32_dev";
    if (!d_u || !d_out) return null_arg(fn);
    if (count < 1 || count > kMaxGroup) return fail(FDR_ERR_ARG, std::string(fn) + ": count must lie in 1 .. 8");
    if (rows <= 0 || cols <= 0) return fail(FDR_ERR_ARG, std::string(fn) + ": rows and cols must be positive");
    if (stride < cols || out_stride < cols) return fail(FDR_ERR_ARG, std::string(fn) + ": a stride below cols");
    if (couple != FDR_TV_COUPLE_NONE && couple != FDR_TV_COUPLE_CHANNELS) return fail(FDR_ERR_ARG, std::string(fn) + ": unknown couple");
    if (count > 1 && out_pitch < (size_t)(rows - 1) * out_stride + cols) return fail(FDR_ERR_ARG, std::string(fn) + ": the output planes overlap each other");
    const int rc = prior_check(fn, lambda, eps);
    if (rc != FDR_OK) return rc;
    const ByteRange o = window_range(d_out, rows, cols, out_stride, count, out_pitch);
    if (ranges_overlap(window_range(d_u, rows, cols, stride, count, u_pitch), o) || (d_w && ranges_overlap(window_range(d_w, rows, cols, stride), o)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the outputs overlap an input");
    FDR_HIP(hipSetDevice(device));
    FDR_HIP(launch_rltv_factor_group(d_u, u_pitch, count, rows, cols, stride, d_w, lambda, eps == 0.f ? FDR_RLTV_EPS : eps, d_out, out_pitch,
                                     out_stride, couple == FDR_TV_COUPLE_CHANNELS, (hipStream_t)stream));
    return FDR_OK;
}

}  // extern "C"
