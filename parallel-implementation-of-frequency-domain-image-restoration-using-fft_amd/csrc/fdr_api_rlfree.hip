// fdr_api_rlfree.hip -- free-boundary, weighted Richardson-Lucy, plain and accelerated (fdr_richardson_lucy_free_f32*, _free_accel_f32*; kernels in fdr_rlfree.hip and the
// weighted update kind of fdr_panel_rows.hip): the workspace, the checks, the driver and the two entry points.  Every transform is an
// operator pass of fdr_api_operator.hip: the estimate goes through pass A as a dense M x N plane, the ratio through the window.
#include "fdr_host.hpp"

#include <cstdint>

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

// The workspace of the free-boundary calls: 1 + 2 g planes of M x N floats (wgt; u and dw of g images) and the double partials of
// the two sums, once per image.  The first call of a plan makes the three planes of one image; a batched call on groups of g images
// grows it to 1 + 2 g planes on its first use.  The new block is had before the old one is let go: on FDR_ERR_ALLOC the plan and the
// workspace it had stay as they were.  Plane order: u_0, wgt, dw_0, then u_k, dw_k for k = 1 .. g - 1.
int ensure_rlfree_workspace(fdr_plan* p, const char* fn, int group) {
    if (p->rf_block && p->rf_group >= group) return FDR_OK;
    const size_t P = (size_t)p->M * p->N;
    const size_t n_part = 2 * (size_t)rlfree_partials(p->M, p->N) + 2;
    const size_t planes = 1 + 2 * (size_t)group;
    char* blk = nullptr;
    if (hipMalloc((void**)&blk, planes * P * sizeof(float) + (size_t)group * n_part * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FDR_ERR_ALLOC, std::string(fn) + ": hipMalloc of the free-boundary workspace failed");
    }
    if (p->rf_block) (void)hipFree(p->rf_block);  // (waits for the device: nothing queued still uses it)
    float* base = reinterpret_cast<float*>(blk);
    p->rf_block = blk;
    p->rf_group = group;
    p->rf_u = base;
    p->rf_wgt = base + P;
    p->rf_dw = base + 2 * P;
    p->rf_part = reinterpret_cast<double*>(base + planes * P);  // a multiple of 8 bytes in (P >= 256)
    return FDR_OK;
}
float* rlfree_u_plane(const fdr_plan* p, int k) { return k == 0 ? p->rf_u : p->rf_u + (size_t)(1 + 2 * k) * p->M * p->N; }
float* rlfree_dw_plane(const fdr_plan* p, int k) { return k == 0 ? p->rf_dw : p->rf_u + (size_t)(2 + 2 * k) * p->M * p->N; }
double* rlfree_part(const fdr_plan* p, int k) { return p->rf_part + (size_t)k * (2 * (size_t)rlfree_partials(p->M, p->N) + 2); }

bool spans_overlap(const float* a, int a_stride, int a_rows, int a_cols, const float* b, int b_stride, int b_rows, int b_cols) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + ((size_t)(a_rows - 1) * a_stride + a_cols) * sizeof(float);
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + ((size_t)(b_rows - 1) * b_stride + b_cols) * sizeof(float);
    return a0 < b1 && b0 < a1;
}

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
    if (spans_overlap(img, stride, rows, cols, out, out_stride, prm->out_rows, prm->out_cols))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the input");
    if (weights && spans_overlap(weights, wstride, rows, cols, out, out_stride, prm->out_rows, prm->out_cols))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the weights");
    return FDR_OK;
}

// one iteration on the whole plan: c = window(fullblur(y)), r = dw / c into the plan's raw plane, out = max(y wgt fullblur^T(pad(r)), 0);
// y and out are dense M x N planes, and `out` may be y itself.  With `fit` (weights and d dense, row stride cols) the ratio pass forms
// dw = w d+ itself, the product of the setup pass, and leaves the fit partials of c beside the same r.
int rlfree_step(fdr_plan* p, const float* y, float* out, int rows, int cols, hipStream_t s, const RlFit* fit, const float* d_dense,
                const RlHooks* hooks) {
    const int M = p->M, N = p->N;
    float* r = p->slots[0].raw;
    int rc = op_rows_fwd(p, y, M, N, N, s);                                                         // c = fullblur(y) ...
    if (rc == FDR_OK && hooks) rc = hooks->after_fwd();
    if (rc == FDR_OK) rc = op_cols(p, false, s);
    if (rc == FDR_OK && fit) rc = op_rows_inv(p, ROW_OUT_RL_RATIO_STAT, kPassRfRatioFit, d_dense, cols, r, cols, rows, cols, s, fit);
    else if (rc == FDR_OK) rc = op_rows_inv(p, ROW_OUT_RL_RATIO, kPassRfRatio, p->rf_dw, cols, r, cols, rows, cols, s);  // ... r = dw / c
    if (rc == FDR_OK && hooks) rc = hooks->after_ratio();
    if (rc == FDR_OK) rc = op_rows_fwd(p, r, rows, cols, cols, s);                                  // g = fullblur^T(pad(r)) ...
    if (rc == FDR_OK) rc = op_cols(p, true, s);
    if (rc != FDR_OK) return rc;
    ScopedPass t(p, s, kPassRfUpdate);                                                              // ... out = max(y wgt g, 0)
    RowArgs a = panel_row_args(p);
    a.src_c = p->slots[0].work;
    a.src_real = y; a.src_real2 = p->rf_wgt; a.src_stride = N;
    a.out = out; a.out_rows = M; a.out_cols = N; a.out_stride = N;
    FDR_HIP(launch_rows4(p->logN, ROW_IN_COMPLEX, ROW_OUT_RL_UPDATE_W, a, p->tw_row_f, s));
    return FDR_OK;
}

// u and wgt are dense M x N planes of the workspace, dw and r (the plan's raw plane) dense rows x cols.  W = pad(m) lies in u's
// plane until alpha has been transformed out of it; d_w may be that plane itself (the host form stages the weights there).
// begin: the setup, the coverage and the start; the dense W (rows x cols) is copied to keep_w first when that is not null, and
// *sums is where the device holds (sum dw, sum W).
int rlfree_begin(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float sigma, float* keep_w,
                 const double** sums, hipStream_t s) {
    const int M = p->M, N = p->N;
    float *u = p->rf_u, *wgt = p->rf_wgt, *dw = p->rf_dw;
    const int n_part = rlfree_partials(rows, cols);
    {
        ScopedPass t(p, s, kPassRfSetup);
        FDR_HIP(launch_rlfree_setup(d_img, stride, d_w, wstride, rows, cols, dw, u, p->rf_part, s));
        if (keep_w) FDR_HIP(hipMemcpyAsync(keep_w, u, (size_t)rows * cols * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    const int rc = blur_window_dev(p, u, rows, cols, cols, wgt, N, M, N, 1, s);  // alpha = fullblur^T(W) over the whole plan
    if (rc != FDR_OK) return rc;
    ScopedPass t(p, s, kPassRfStart);
    FDR_HIP(launch_rlfree_start(wgt, u, (size_t)M * N, sigma, p->rf_part + 2 * (size_t)n_part, s));
    if (sums) *sums = p->rf_part + 2 * (size_t)n_part;
    return FDR_OK;
}

// The pieces of rlfree_begin for a batch, which computes the coverage once and starts every image from it.  setup: dw and W = pad(m)
// dense into `dw` and `W`, the two sums behind the partials at `part`; returns where the device holds (sum dw, sum W).
int rlfree_setup_image(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* dw, float* W,
                       double* part, const double** sums, hipStream_t s) {
    ScopedPass t(p, s, kPassRfSetup);
    FDR_HIP(launch_rlfree_setup(d_img, stride, d_w, wstride, rows, cols, dw, W, part, s));
    *sums = part + 2 * (size_t)rlfree_partials(rows, cols);
    return FDR_OK;
}
// start: the M x N plane `alpha` becomes alpha > sigma ? 1 / alpha : 0 and u = alpha > sigma ? sum dw / sum W : 0
int rlfree_start_image(fdr_plan* p, float* alpha, float* u, float sigma, const double* sums, hipStream_t s) {
    ScopedPass t(p, s, kPassRfStart);
    FDR_HIP(launch_rlfree_start(alpha, u, (size_t)p->M * p->N, sigma, sums, s));
    return FDR_OK;
}

// rlfree_step for a group of n images on the slots ws[0 .. n), in place on the dense M x N estimates us[k]; dws[k] dense rows x cols;
// wgt is the one plane of the call
int rlfree_step_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, float* const* us, const float* const* dws, int rows, int cols, hipStream_t s) {
    const int M = p->M, N = p->N;
    float* r[kMaxGroup];
    for (int k = 0; k < n; ++k) r[k] = ws[k]->raw;
    int rc = op_rows_fwd_n(p, ws, n, us, M, N, N, s);
    if (rc == FDR_OK) rc = op_cols_n(p, ws, n, false, s);
    if (rc == FDR_OK) rc = op_rows_inv_n(p, ws, n, ROW_OUT_RL_RATIO, kPassRfRatio, dws, cols, nullptr, r, cols, rows, cols, s);
    if (rc == FDR_OK) rc = op_rows_fwd_n(p, ws, n, r, rows, cols, cols, s);
    if (rc == FDR_OK) rc = op_cols_n(p, ws, n, true, s);
    if (rc == FDR_OK) rc = op_rows_inv_n(p, ws, n, ROW_OUT_RL_UPDATE_W, kPassRfUpdate, us, N, p->rf_wgt, us, N, M, N, s);
    return rc;
}

// finish: the output window of the dense M x N estimate u, cropped or normalised, into d_out
int rlfree_finish(fdr_plan* p, const char* fn, const float* u, float* d_out, int out_stride, const fdr_rlfree_params& prm, hipStream_t s) {
    if (prm.norm_area == FDR_NORM_NONE) {
        ScopedPass t(p, s, kPassRfCrop);
        FDR_HIP(launch_rlfree_crop(u, p->N, d_out, prm.out_rows, prm.out_cols, out_stride, s));
        return FDR_OK;
    }
    return normalize_window(p, fn, kPassRfNorm, u, p->N, prm.out_rows, prm.out_cols, prm.norm_area, d_out, out_stride, s);
}

}  // namespace fdr

namespace {

// Accelerated (rl_accel_loop), the estimate alternates between u's plane and one of the acceleration workspace.
int rlfree_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride,
                    float* d_out, int out_stride, const fdr_rlfree_params& prm, bool accel, float* d_alphas, hipStream_t s) {
    const int M = p->M, N = p->N;
    float* u = p->rf_u;
    int rc = rlfree_begin(p, d_img, rows, cols, stride, d_w, wstride, prm.sigma, nullptr, nullptr, s);
    if (rc != FDR_OK) return rc;
    if (accel) {
        float* const U[2] = {u, p->ra_u};
        const int us[2] = {N, N};
        rc = rl_accel_loop(p, prm.iterations, M, N, U, us, 0, nullptr, 0, d_alphas, s,
                           [&](const float* y, int, float* out, int) { return rlfree_step(p, y, out, rows, cols, s); }, &u);
    } else {
        for (int it = 0; it < prm.iterations && rc == FDR_OK; ++it) rc = rlfree_step(p, u, u, rows, cols, s);
    }
    if (rc != FDR_OK) return rc;
    return rlfree_finish(p, fn, u, d_out, out_stride, prm, s);
}

}  // namespace

namespace fdr {

// the driver of fdr_richardson_lucy_free_f32_dev on a checked call with its workspace (a batch with groups of one is the loop of these)
int rlfree_plain_dev(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* d_out,
                     int out_stride, const fdr_rlfree_params& prm, hipStream_t s) {
    return rlfree_dev_impl(p, fn, d_img, rows, cols, stride, d_w, wstride, d_out, out_stride, prm, false, nullptr, s);
}

}  // namespace fdr

namespace {

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
    DeviceBuffer d_alphas;
    if (accel && alphas_host && prm.iterations > 0) FDR_ALLOC(d_alphas, (size_t)prm.iterations * sizeof(float), fn);
    if (weights_host)  // staged dense into u's plane, where the setup pass leaves W anyway
        FDR_HIP(hipMemcpy2D(p->rf_u, (size_t)cols * sizeof(float), weights_host, (size_t)wstride * sizeof(float), (size_t)cols * sizeof(float),
                            (size_t)rows, hipMemcpyHostToDevice));
    rc = host_image_call(p, fn, img_host, rows, cols, stride, out_host, prm.out_rows, prm.out_cols, out_stride,
                         [&](const float* d_in, float* d_out) {
                             return rlfree_dev_impl(p, fn, d_in, rows, cols, cols, weights_host ? p->rf_u : nullptr, cols, d_out, prm.out_cols,
                                                    prm, accel, d_alphas.as<float>(), nullptr);
                         });
    if (rc == FDR_OK && d_alphas.ptr)
        FDR_HIP(hipMemcpy(alphas_host, d_alphas.ptr, (size_t)prm.iterations * sizeof(float), hipMemcpyDeviceToHost));
    return rc;
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
