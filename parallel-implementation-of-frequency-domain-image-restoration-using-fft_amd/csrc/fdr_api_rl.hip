// fdr_api_rl.hip -- Richardson-Lucy, the plain form (fdr_richardson_lucy_f32*, fdr_richardson_lucy_accel_f32*; kernels in fdr_rl.hip
// and the RL kinds of fdr_panel_rows.hip): the checks, the one step and the one driver of the form, both on a group of n >= 1 images,
// and the four entry points.  Every transform is an operator pass of fdr_api_operator.hip.  The batch (fdr_api_rlbatch.hip) and the
// blind call (fdr_api_blind.hip) run the drivers (rl_group_dev, accelerated: rl_group_accel_dev); the auto call (fdr_api_rlstop.hip)
// routes its planes itself, around the same step.
#include "fdr_host.hpp"

using namespace fdr;

static_assert(kRlTau == FDR_RL_TAU, "the ratio guard of the kernels is FDR_RL_TAU");

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassRlInit = "RL init: u = max(d, 0)";
const char* const kPassRlRatio = "C op rows: IFFT+RL ratio";
const char* const kPassRlRatioFit = "C op rows: IFFT+RL ratio+fit";
const char* const kPassRlUpdate = "C op rows: IFFT+RL update";
const char* const kPassRlUpdateF = "C op rows: IFFT+RL update (factor)";
const char* const kPassRlNorm = "E RL minmax+normalize";

}  // namespace

namespace fdr {

// everything a Richardson-Lucy call refuses: plan, operator PSF and window, the iteration count, the normalisation, an output
// that overlaps the input (the input is read on every iteration)
int rl_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* out, int out_stride,
             int iterations, int norm_area, PlanNeed need) {
    const int rc = check_window(p, fn, need, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    if (iterations < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": iterations < 0");
    if (norm_area != FDR_NORM_NONE && norm_area != FDR_NORM_CROPPED && norm_area != FDR_NORM_PADDED)
        return fail(FDR_ERR_ARG, std::string(fn) + ": unknown norm_area");
    if (ranges_overlap(window_range(img, rows, cols, stride), window_range(out, rows, cols, out_stride)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the input (the input is read on every iteration)");
    return FDR_OK;
}

int plain_form_check(const char* fn, const float* weights, int rows, int cols, int out_rows, int out_cols, bool each_alone, const char* window_msg) {
    if (weights) return fail(FDR_ERR_ARG, std::string(fn) + ": the plain form takes no weights");
    const bool r0 = out_rows == 0, c0 = out_cols == 0, r1 = out_rows == rows, c1 = out_cols == cols;
    if (each_alone ? !((r0 || r1) && (c0 || c1)) : !((r0 && c0) || (r1 && c1))) return fail(FDR_ERR_ARG, std::string(fn) + window_msg);
    return FDR_OK;
}

int rl_step(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int stride, const float* const* ys, int ystride,
            float* const* outs, int os, int rows, int cols, hipStream_t s, const RlFit* fit, const RlHooks* hooks, int it, const float* factor,
            size_t factor_pitch) {
    if (hooks && n > 1) return fail(FDR_ERR_STATE, "rl_step: the hooks take one image per step");
    float* r[kMaxGroup];
    for (int k = 0; k < n; ++k) r[k] = ws[k]->raw;
    const int rs = cols;
    int rc = op_rows_fwd_n(p, ws, n, ys, rows, cols, ystride, s);                                        // c = blur(y) ...
    if (rc == FDR_OK && hooks && hooks->after_fwd) rc = hooks->after_fwd(it);
    if (rc == FDR_OK) rc = op_cols_n(p, ws, n, false, s);
    if (rc == FDR_OK)                                                                                    // ... r = d+ / c
        rc = op_rows_inv_n(p, ws, n, fit ? ROW_OUT_RL_RATIO_STAT : ROW_OUT_RL_RATIO, fit ? kPassRlRatioFit : kPassRlRatio, d_imgs, stride, nullptr,
                           r, rs, rows, cols, s, fit);
    if (rc == FDR_OK && hooks && hooks->after_ratio) rc = hooks->after_ratio(it);
    if (rc == FDR_OK) rc = op_rows_fwd_n(p, ws, n, r, rows, cols, rs, s);                                // g = blur^T(r) ...
    if (rc == FDR_OK) rc = op_cols_n(p, ws, n, true, s);
    if (rc == FDR_OK && factor)                                                                          // ... out = max(y factor g, 0)
        return op_rows_inv_n(p, ws, n, ROW_OUT_RL_UPDATE_W, kPassRlUpdateF, ys, ystride, factor, outs, os, rows, cols, s, nullptr, factor_pitch);
    if (rc == FDR_OK) rc = op_rows_inv_n(p, ws, n, ROW_OUT_RL_UPDATE, kPassRlUpdate, ys, ystride, nullptr, outs, os, rows, cols, s);  // ... out = max(y g, 0)
    return rc;
}

int rl_init_estimate(fdr_plan* p, const float* d_img, int rows, int cols, int stride, float* u, int us, hipStream_t s) {
    ScopedPass t(p, s, kPassRlInit);
    FDR_HIP(launch_rl_init(d_img, rows, cols, stride, u, us, s));
    return FDR_OK;
}
int rl_normalize(fdr_plan* p, const char* fn, const float* fin, int fs, int rows, int cols, int norm_area, float* d_out, int out_stride,
                 hipStream_t s) {
    return normalize_window(p, fn, kPassRlNorm, fin, fs, rows, cols, norm_area, d_out, out_stride, s);
}

// u_k lives in image k's output window, r_k in slot k's raw plane, the spectrum in slot k's work; with a normalisation the last
// update (or, for no iterations, the start) goes to the raw plane instead and the normalise pass writes the output from there
int rl_group_dev(fdr_plan* p, const char* fn, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                 float* const* d_outs, int out_stride, int iterations, int norm_area, hipStream_t s, const RlHooks* hooks) {
    const bool norm = norm_area != FDR_NORM_NONE;
    float* fin[kMaxGroup];
    for (int k = 0; k < n; ++k) fin[k] = norm ? ws[k]->raw : d_outs[k];
    const int fs = norm ? cols : out_stride;
    int rc = FDR_OK;
    for (int k = 0; k < n && rc == FDR_OK; ++k)
        rc = rl_init_estimate(p, d_imgs[k], rows, cols, stride, iterations == 0 ? fin[k] : d_outs[k], iterations == 0 ? fs : out_stride, s);
    for (int it = 0; it < iterations && rc == FDR_OK; ++it) {
        const bool last = it == iterations - 1;
        rc = rl_step(p, ws, n, d_imgs, stride, d_outs, out_stride, last ? fin : d_outs, last ? fs : out_stride, rows, cols, s, nullptr, hooks, it);
        if (rc == FDR_OK && hooks && hooks->after_step) rc = hooks->after_step(it);
    }
    for (int k = 0; k < n && rc == FDR_OK && norm; ++k) rc = rl_normalize(p, fn, fin[k], fs, rows, cols, norm_area, d_outs[k], out_stride, s);
    return rc;
}

// Accelerated (rl_accel_loop): image k's estimate alternates between its output window and its plane of the acceleration workspace,
// starting where u_n comes to lie in the output window (`first`, common to the group), and the last update goes to slot k's raw plane
// under a normalisation.
int rl_group_accel_dev(fdr_plan* p, const char* fn, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                       float* const* d_outs, int out_stride, int iterations, int norm_area, float* d_alphas, size_t alpha_pitch, hipStream_t s) {
    const bool norm = norm_area != FDR_NORM_NONE;
    float* fin[kMaxGroup];
    float* U[kMaxGroup][2];
    for (int k = 0; k < n; ++k) {
        fin[k] = norm ? ws[k]->raw : d_outs[k];
        U[k][0] = d_outs[k];
        U[k][1] = rlaccel_u_plane(p, k);
    }
    const int fs = norm ? cols : out_stride;
    const int us[2] = {out_stride, cols};
    const int first = iterations & 1;
    int rc = FDR_OK;
    for (int k = 0; k < n && rc == FDR_OK; ++k)
        rc = rl_init_estimate(p, d_imgs[k], rows, cols, stride, iterations == 0 ? fin[k] : U[k][first], iterations == 0 ? fs : us[first], s);
    if (rc != FDR_OK) return rc;
    rc = rl_accel_loop(p, n, iterations, rows, cols, U, us, first, fin, fs, d_alphas, alpha_pitch, s,
                       [&](const float* const* ys, int ystride, float* const* outs, int os) {
                           return rl_step(p, ws, n, d_imgs, stride, ys, ystride, outs, os, rows, cols, s);
                       }, nullptr);
    for (int k = 0; k < n && rc == FDR_OK && norm; ++k) rc = rl_normalize(p, fn, fin[k], fs, rows, cols, norm_area, d_outs[k], out_stride, s);
    return rc;
}

}  // namespace fdr

namespace {

// One image on slot 0: the driver of the form, plain or accelerated, on a group of one
int rl_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride, int iterations,
                int norm_area, bool accel, float* d_alphas, hipStream_t s) {
    fdr_plan::Slot* w = &p->slots[0];
    if (!accel) return rl_group_dev(p, fn, &w, 1, &d_img, rows, cols, stride, &d_out, out_stride, iterations, norm_area, s);
    return rl_group_accel_dev(p, fn, &w, 1, &d_img, rows, cols, stride, &d_out, out_stride, iterations, norm_area, d_alphas, 0, s);
}

// the checks, the device and the driver of the four entry points; the accelerated ones also refuse alphas that overlap a window and
// make sure of their workspace
int rl_dev_entry(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride, int iterations,
                 int norm_area, bool accel, float* d_alphas, hipStream_t s) {
    if (!p || !d_img || !d_out) return null_arg(fn);
    int rc = rl_check(p, fn, d_img, rows, cols, stride, d_out, out_stride, iterations, norm_area);
    if (rc == FDR_OK && accel) rc = check_alphas(fn, d_alphas, iterations, d_out, out_stride, rows, cols, "output");
    if (rc == FDR_OK && accel) rc = check_alphas(fn, d_alphas, iterations, d_img, stride, rows, cols, "input");
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    if (accel) rc = ensure_rlaccel_workspace(p, fn);
    if (rc != FDR_OK) return rc;
    return rl_dev_impl(p, fn, d_img, rows, cols, stride, d_out, out_stride, iterations, norm_area, accel, d_alphas, s);
}

int rl_host_entry(fdr_plan* p, const char* fn, const float* img_host, int rows, int cols, int stride, float* out_host, int out_stride,
                  int iterations, int norm_area, bool accel, float* alphas_host) {
    if (!p || !img_host || !out_host) return null_arg(fn);
    int rc = rl_check(p, fn, img_host, rows, cols, stride, out_host, out_stride, iterations, norm_area);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    if (accel) rc = ensure_rlaccel_workspace(p, fn);
    if (rc != FDR_OK) return rc;
    return with_host_alphas(fn, alphas_host, iterations, [&](float* d_alphas) {
        return host_image_call(p, fn, img_host, rows, cols, stride, out_host, rows, cols, out_stride, [&](const float* d_in, float* d_out) {
            return rl_dev_impl(p, fn, d_in, rows, cols, cols, d_out, cols, iterations, norm_area, accel, d_alphas, nullptr);
        });
    });
}

}  // namespace

extern "C" {

int fdr_richardson_lucy_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride, int iterations,
                                int norm_area, void* stream) {
    return rl_dev_entry(p, "fdr_richardson_lucy_f32_dev", d_img, rows, cols, stride, d_out, out_stride, iterations, norm_area, false, nullptr,
                        (hipStream_t)stream);
}

int fdr_richardson_lucy_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, float* out_host, int out_stride,
                            int iterations, int norm_area) {
    return rl_host_entry(p, "fdr_richardson_lucy_f32", img_host, rows, cols, stride, out_host, out_stride, iterations, norm_area, false,
                         nullptr);
}

int fdr_richardson_lucy_accel_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                                      int iterations, int norm_area, float* d_alphas, void* stream) {
    return rl_dev_entry(p, "fdr_richardson_lucy_accel_f32_dev", d_img, rows, cols, stride, d_out, out_stride, iterations, norm_area, true,
                        d_alphas, (hipStream_t)stream);
}

int fdr_richardson_lucy_accel_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, float* out_host, int out_stride,
                                  int iterations, int norm_area, float* alphas_host) {
    return rl_host_entry(p, "fdr_richardson_lucy_accel_f32", img_host, rows, cols, stride, out_host, out_stride, iterations, norm_area, true,
                         alphas_host);
}

}  // extern "C"
