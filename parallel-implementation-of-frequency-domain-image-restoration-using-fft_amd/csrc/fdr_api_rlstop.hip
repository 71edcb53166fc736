// fdr_api_rlstop.hip -- Richardson-Lucy that stops from the data (fdr_richardson_lucy_auto_f32*; kernels: the ratio kind
// ROW_OUT_RL_RATIO_STAT of fdr_panel_rows.hip and the fold of fdr_rlstop.hip): the workspace, the checks, the driver around the
// unchanged steps of the four forms (fdr_api_rl.hip, fdr_api_rlfree.hip, fdr_api_rlaccel.hip) and the two entry points.
//
// The final count is not known in advance, so nothing is routed by it: the estimate stays in its own plane(s) for every step, the
// accelerated forms start at parity 0, and what the stop leaves is brought to the output (or to the normalise pass) afterwards.
// The values of u_k do not depend on the plane they lie in, so the output has the bits of the call with that count.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassRsFold = "RLS fold: res, kl";
const char* const kPassRsNoise = "RLS noise: sum |d * n|";
const char* const kPassRsMove = "RLS out: move";

constexpr int kRsTraceSteps = 1024;  // steps of the internal trace the first call makes room for

// the checked arguments with their defaults
struct AutoArgs {
    int n, rule, every, norm_area;
    bool free_form, accel, estimate;
    double sigma, gain, tau;
    fdr_rlfree_params fp;  // free form
};

bool finite_nonneg(float v) { return std::isfinite(v) && v >= 0.f; }

// everything an auto call refuses, before any device work: what the underlying form refuses, then the rule's own arguments
int auto_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
               const float* out, int out_stride, const fdr_rl_auto_params* prm, const double* d_trace, AutoArgs* a) {
    a->n = prm->iterations; a->rule = prm->rule; a->norm_area = prm->norm_area;
    a->free_form = prm->free_boundary != 0; a->accel = prm->accelerate != 0;
    a->fp = fdr_rlfree_params{prm->iterations, prm->cov_sigma, prm->norm_area, prm->out_rows, prm->out_cols};
    int rc;
    if (a->free_form) {
        rc = rlfree_check(p, fn, img, rows, cols, stride, weights, wstride, out, out_stride, &a->fp);
    } else {
        rc = rl_check(p, fn, img, rows, cols, stride, out, out_stride, prm->iterations, prm->norm_area);
        if (rc == FDR_OK)
            rc = plain_form_check(fn, weights, rows, cols, prm->out_rows, prm->out_cols, true,
                                  ": the plain form's output window is the input's (out_rows, out_cols = 0 or rows, cols)");
        a->fp.out_rows = rows; a->fp.out_cols = cols;
    }
    if (rc != FDR_OK) return rc;
    if (prm->rule != FDR_RL_STOP_NONE && prm->rule != FDR_RL_STOP_RESIDUAL && prm->rule != FDR_RL_STOP_KL)
        return fail(FDR_ERR_ARG, std::string(fn) + ": unknown rule");
    if (prm->rule == FDR_RL_STOP_KL && !(std::isfinite(prm->gain) && prm->gain > 0.f))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the KL rule needs a finite gain > 0");
    if (!finite_nonneg(prm->sigma) || !finite_nonneg(prm->tau)) return fail(FDR_ERR_ARG, std::string(fn) + ": sigma and tau must be finite and >= 0");
    if (prm->check_every < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": check_every < 0");
    a->sigma = prm->sigma; a->gain = prm->gain;
    a->tau = prm->tau != 0.f ? (double)prm->tau : 1.0;
    a->every = prm->check_every ? prm->check_every : 1;
    a->estimate = prm->rule == FDR_RL_STOP_RESIDUAL && prm->sigma == 0.f;
    if (a->estimate) {
        rc = noise_window_check(fn, rows, cols, stride);
        if (rc != FDR_OK) return rc;
    }
    if (d_trace && a->n > 0) {
        const ByteRange t = byte_range(d_trace, (size_t)a->n * 2 * sizeof(double));
        if (ranges_overlap(t, window_range(img, rows, cols, stride))) return fail(FDR_ERR_ARG, std::string(fn) + ": the trace overlaps the input");
        if (ranges_overlap(t, window_range(out, a->fp.out_rows, a->fp.out_cols, out_stride)))
            return fail(FDR_ERR_ARG, std::string(fn) + ": the trace overlaps the output");
        if (weights && ranges_overlap(t, window_range(weights, rows, cols, wstride)))
            return fail(FDR_ERR_ARG, std::string(fn) + ": the trace overlaps the weights");
    }
    return FDR_OK;
}

// the partials (first call), the two planes of the weighted free form (its first call) and room for `steps` steps in the internal trace
int ensure_rlstop_workspace(fdr_plan* p, const char* fn, bool free_form, int steps) {
    if (!p->rlstop.ws.block) {
        const int n_part = rows4_minmax_partials(p->logN, p->M, 1, 1);
        if (n_part <= 0) return fail(FDR_ERR_STATE, std::string(fn) + ": no inverse row pass for this plan");
        const int rc = ensure_workspace(p->rlstop.ws, fn, "workspace", 1,
                                        [p, n_part](auto& c, int) { layout(c, p->rlstop, (size_t)n_part, (size_t)kRegMaxPartials + 1); });
        if (rc != FDR_OK) return rc;
        p->rlstop.n_part = n_part;
    }
    // a grown trace: only calls that wait for their own end use it, so nothing in flight reads the old one
    int rc = ensure_workspace(p->rlstop.trace_ws, fn, "trace", steps > kRsTraceSteps ? steps : kRsTraceSteps,
                              [p](auto& c, int n) { layout(c, p->rlstop.trace, 2 * (size_t)n, 8); });
    if (rc == FDR_OK && free_form)
        rc = ensure_workspace(p->rlstop.planes_ws, fn, "weight planes", 1, [p](auto& c, int) { layout(c, p->rlstop.planes, 2 * (size_t)p->M * p->N, 16); });
    return rc;
}

// The whole call on `s`.  tr: where the device writes the trace (the caller's, the internal one, or null for none).  With a rule
// the stream is waited for after every a.every steps and those entries are read back.
int auto_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* d_out,
                  int out_stride, const AutoArgs& a, double* tr, fdr_rl_auto_result* res, hipStream_t s) {
    const int M = p->M, N = p->N, n = a.n;
    *res = fdr_rl_auto_result{n, 0, a.sigma, 0.0, 0.0};
    double sigma = a.sigma;
    int rc = FDR_OK;
    if (a.estimate) {
        ScopedPass t(p, s, kPassRsNoise);
        rc = noise_sigma_dev(d_img, rows, cols, stride, p->rlstop.noise, &sigma, s);
        if (rc != FDR_OK) return rc;
    }
    // the start of the form; cur = the plane of u_k (row stride cs), U / us = the two planes of the accelerated estimate
    // free-boundary form with weights: the ratio pass reads d and W (dense copies) and forms dw itself.  Without weights W = 1 and
    // dw = d+: the pass reads the stored dw as its datum and nothing else (max(dw, 0) = dw, the same bits).
    const bool weighted = a.free_form && d_w != nullptr;
    float* W = weighted ? p->rlstop.planes : nullptr;
    const float* D = weighted ? p->rlstop.planes + (size_t)M * N : p->rlfree.dw;
    double S = (double)rows * (double)cols;
    float* cur;
    if (a.free_form) {
        const double* sums = nullptr;
        if (weighted)
            FDR_HIP(hipMemcpy2DAsync(p->rlstop.planes + (size_t)M * N, (size_t)cols * sizeof(float), d_img, (size_t)stride * sizeof(float),
                                     (size_t)cols * sizeof(float), (size_t)rows, hipMemcpyDeviceToDevice, s));
        rc = rlfree_begin(p, d_img, rows, cols, stride, d_w, wstride, a.fp.sigma, W, &sums, s);
        if (rc != FDR_OK) return rc;
        if (a.rule != FDR_RL_STOP_NONE) {
            FDR_HIP(hipMemcpyAsync(&S, sums + 1, sizeof(double), hipMemcpyDeviceToHost, s));
            FDR_HIP(hipStreamSynchronize(s));
        }
        cur = p->rlfree.u;
    } else {
        rc = rl_init_estimate(p, d_img, rows, cols, stride, d_out, out_stride, s);
        if (rc != FDR_OK) return rc;
        cur = d_out;
    }
    float* const U[1][2] = {{cur, a.accel ? p->rlaccel.u : cur}};  // a group of one image for rl_accel_steps
    const int us[2] = {a.free_form ? N : out_stride, a.free_form ? N : (a.accel ? cols : out_stride)};
    const int R = a.free_form ? M : rows, C = a.free_form ? N : cols;  // the window the estimate lives on

    const RlFit fit{W, p->rlstop.part};
    fdr_plan::Slot* w0 = &p->slots[0];
    int k = 0;  // the step about to run
    auto step = [&](const float* y, int ys, float* out, int os) {
        int rc2 = a.free_form ? rlfree_step(p, &w0, 1, &y, &out, &D, p->rlfree.wgt, rows, cols, s, &fit)
                              : rl_step(p, &w0, 1, &d_img, stride, &y, ys, &out, os, rows, cols, s, &fit);
        if (rc2 == FDR_OK && tr) {
            ScopedPass t(p, s, kPassRsFold);
            FDR_HIP(launch_rlstop_fold(p->rlstop.part, p->rlstop.n_part, tr + 2 * (size_t)k, s));
        }
        ++k;
        return rc2;
    };
    const double target = a.rule == FDR_RL_STOP_RESIDUAL ? a.tau * sigma * sigma * S : (a.rule == FDR_RL_STOP_KL ? a.tau : 0.0);
    std::vector<double> seen;
    int done = 0, stopped = 0;
    double statistic = 0.0;
    while (done < n && !stopped) {
        const int k1 = a.rule == FDR_RL_STOP_NONE ? n : (n - done < a.every ? n : done + a.every);
        if (a.accel) {
            rc = rl_accel_steps(p, 1, done, k1, n, R, C, U, us, 0, nullptr, 0, nullptr, 0, s,
                                [&](const float* const* ys, int ystride, float* const* outs, int os) { return step(ys[0], ystride, outs[0], os); }, &cur);
        } else {
            for (int i = done; i < k1 && rc == FDR_OK; ++i) rc = step(cur, us[0], cur, us[0]);
        }
        if (rc != FDR_OK) return rc;
        if (a.rule != FDR_RL_STOP_NONE) {
            seen.resize((size_t)(k1 - done) * 2);
            FDR_HIP(hipMemcpyAsync(seen.data(), tr + 2 * (size_t)done, seen.size() * sizeof(double), hipMemcpyDeviceToHost, s));
            FDR_HIP(hipStreamSynchronize(s));
            for (int i = 0; i < k1 - done && !stopped; ++i) {
                statistic = a.rule == FDR_RL_STOP_RESIDUAL ? seen[2 * i] : 2.0 * a.gain * seen[2 * i + 1] / S;
                stopped = statistic <= target;
            }
        }
        done = k1;
    }
    *res = fdr_rl_auto_result{done, stopped, sigma, target, statistic};

    // u_done lies in `cur`: to the output
    if (a.free_form) return rlfree_finish(p, fn, cur, d_out, out_stride, a.fp, s);
    const int cs = cur == d_out ? out_stride : cols;
    if (a.norm_area == FDR_NORM_NONE) {
        if (cur == d_out) return FDR_OK;
        ScopedPass t(p, s, kPassRsMove);
        FDR_HIP(hipMemcpy2DAsync(d_out, (size_t)out_stride * sizeof(float), cur, (size_t)cs * sizeof(float), (size_t)cols * sizeof(float),
                                 (size_t)rows, hipMemcpyDeviceToDevice, s));
        return FDR_OK;
    }
    if (cur == d_out) {  // the normalise pass reads one plane and writes another: through the raw plane, free once the last step is done
        ScopedPass t(p, s, kPassRsMove);
        float* raw = p->slots[0].raw;
        FDR_HIP(hipMemcpy2DAsync(raw, (size_t)cols * sizeof(float), d_out, (size_t)out_stride * sizeof(float), (size_t)cols * sizeof(float),
                                 (size_t)rows, hipMemcpyDeviceToDevice, s));
        cur = raw;
    }
    return rl_normalize(p, fn, cur, cols, rows, cols, a.norm_area, d_out, out_stride, s);
}

// the workspaces of the form and of the trace
int auto_prepare(fdr_plan* p, const char* fn, const AutoArgs& a, bool weighted, bool internal_trace) {
    int rc = FDR_OK;
    if (a.free_form) rc = ensure_rlfree_workspace(p, fn);
    if (rc == FDR_OK && a.accel) rc = ensure_rlaccel_workspace(p, fn);
    if (rc == FDR_OK) rc = ensure_rlstop_workspace(p, fn, a.free_form && weighted, internal_trace ? a.n : 0);
    return rc;
}

}  // namespace

extern "C" {

int fdr_richardson_lucy_auto_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                                     float* d_out, int out_stride, const fdr_rl_auto_params* params, fdr_rl_auto_result* result,
                                     double* d_trace, void* stream) {
    const char* fn = "fdr_richardson_lucy_auto_f32_dev";
    if (!p || !d_img || !d_out || !params || !result) return null_arg(fn);
    AutoArgs a{};
    int rc = auto_check(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, params, d_trace, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const bool internal = !d_trace && a.rule != FDR_RL_STOP_NONE;
    rc = auto_prepare(p, fn, a, d_weights != nullptr, internal);
    if (rc != FDR_OK) return rc;
    return auto_dev_impl(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, a, d_trace ? d_trace : (internal ? p->rlstop.trace : nullptr),
                         result, (hipStream_t)stream);
}

int fdr_richardson_lucy_auto_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                                 float* out_host, int out_stride, const fdr_rl_auto_params* params, fdr_rl_auto_result* result,
                                 double* trace_host) {
    const char* fn = "fdr_richardson_lucy_auto_f32";
    if (!p || !img_host || !out_host || !params || !result) return null_arg(fn);
    AutoArgs a{};
    int rc = auto_check(p, fn, img_host, rows, cols, stride, weights_host, wstride, out_host, out_stride, params, nullptr, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const bool internal = trace_host || a.rule != FDR_RL_STOP_NONE;
    rc = auto_prepare(p, fn, a, weights_host != nullptr, internal);
    if (rc != FDR_OK) return rc;
    if (a.free_form && weights_host) rc = stage_weights(p, weights_host, rows, cols, wstride);
    if (rc != FDR_OK) return rc;
    rc = host_image_call(p, fn, img_host, rows, cols, stride, out_host, a.fp.out_rows, a.fp.out_cols, out_stride,
                         [&](const float* d_in, float* d_out) {
                             return auto_dev_impl(p, fn, d_in, rows, cols, cols, a.free_form && weights_host ? p->rlfree.u : nullptr, cols, d_out,
                                                  a.fp.out_cols, a, internal ? p->rlstop.trace : nullptr, result, nullptr);
                         });
    if (rc == FDR_OK && trace_host && result->iterations_done > 0)
        FDR_HIP(hipMemcpy(trace_host, p->rlstop.trace, (size_t)result->iterations_done * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return rc;
}

}  // extern "C"
