// fdr_api_rlbatch.hip -- the blur operator and Richardson-Lucy, both forms, on several images per launch (fdr_blur_batch_f32_dev,
// fdr_richardson_lucy_batch_f32*): `count` images with one operator PSF (and, free-boundary form, one weights plane) are cut into
// launch groups of plan->group images, and every pass of a group is ONE launch over its images (the group forms of the operator
// passes in fdr_api_operator.hip, the steps rl_step_n / rlfree_step_n).  A group runs to completion on the caller's stream, on the
// slots 0 .. g - 1, before the next one starts; the internal streams and FDR_OPT_BATCH_GRAPH are not used.  Every image comes out
// with the bits of its single-image call: the kernels of a group share the step plan and the epilogue of the single-image ones.
#include "fdr_host.hpp"

#include <cstdint>

using namespace fdr;

namespace {

// the bytes `count` windows rows x cols (row stride `stride`, `pitch` elements apart) span: [lo, hi)
struct Span { uintptr_t lo, hi; };
Span batch_span(const float* base, size_t pitch, int count, int rows, int cols, int stride) {
    const uintptr_t lo = (uintptr_t)base;
    return {lo, lo + ((size_t)(count - 1) * pitch + (size_t)(rows - 1) * stride + cols) * sizeof(float)};
}
bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

// what the two batched Richardson-Lucy calls refuse, before any device work: the single-image call of the form on image 0 (plan,
// operator PSF, window, strides, iteration count, normalisation, sigma, output window), weights in the plain form, and an output
// that overlaps the input or the weights anywhere in the span of the batch
int rl_batch_check(const fdr_plan* p, const char* fn, const float* imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                   const float* weights, int wstride, const float* out, size_t out_pitch, int out_stride, const fdr_rl_batch_params& b,
                   fdr_rlfree_params* free_prm) {
    int out_rows = rows, out_cols = cols;
    if (b.free_boundary) {
        *free_prm = fdr_rlfree_params{b.iterations, b.sigma, b.norm_area, b.out_rows, b.out_cols};
        const int rc = rlfree_check(p, fn, imgs, rows, cols, stride, weights, wstride, out, out_stride, free_prm);
        if (rc != FDR_OK) return rc;
        out_rows = b.out_rows; out_cols = b.out_cols;
    } else {
        if (weights) return fail(FDR_ERR_ARG, std::string(fn) + ": the plain form takes no weights");
        if (!((b.out_rows == 0 && b.out_cols == 0) || (b.out_rows == rows && b.out_cols == cols)))
            return fail(FDR_ERR_ARG, std::string(fn) + ": the plain form's output window is rows x cols (out_rows = out_cols = 0, or rows and cols)");
        const int rc = rl_check(p, fn, imgs, rows, cols, stride, out, out_stride, b.iterations, b.norm_area);
        if (rc != FDR_OK) return rc;
    }
    const Span so = batch_span(out, out_pitch, count, out_rows, out_cols, out_stride);
    if (overlap(so, batch_span(imgs, img_pitch, count, rows, cols, stride)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the outputs of the batch overlap its inputs (the input is read on every iteration)");
    if (weights && overlap(so, batch_span(weights, 0, 1, rows, cols, wstride)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the outputs of the batch overlap the weights");
    return FDR_OK;
}

// images of one launch group: the plan's group on the path of the operator, never more than the batch holds
int launch_group(const fdr_plan* p, int count) { return p->group < count ? p->group : count; }

// the plain form on a group of n >= 2 images: u_k lives in image k's output window, r_k in slot k's raw plane; with a normalisation
// the last update (or, for no iterations, the start) goes to the raw plane instead and the normalise pass writes the output
int rl_group_dev(fdr_plan* p, const char* fn, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                 float* const* d_outs, int out_stride, int iterations, int norm_area, hipStream_t s) {
    const bool norm = norm_area != FDR_NORM_NONE;
    float* fin[kMaxGroup];
    for (int k = 0; k < n; ++k) fin[k] = norm ? ws[k]->raw : d_outs[k];
    const int fs = norm ? cols : out_stride;
    int rc = FDR_OK;
    for (int k = 0; k < n && rc == FDR_OK; ++k)
        rc = rl_init_estimate(p, d_imgs[k], rows, cols, stride, iterations == 0 ? fin[k] : d_outs[k], iterations == 0 ? fs : out_stride, s);
    for (int it = 0; it < iterations && rc == FDR_OK; ++it) {
        const bool last = it == iterations - 1;
        rc = rl_step_n(p, ws, n, d_imgs, stride, d_outs, out_stride, last ? fin : d_outs, last ? fs : out_stride, rows, cols, s);
    }
    for (int k = 0; k < n && rc == FDR_OK && norm; ++k) rc = rl_normalize(p, fn, fin[k], fs, rows, cols, norm_area, d_outs[k], out_stride, s);
    return rc;
}

int rl_batch_dev_impl(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                      float* d_out, size_t out_pitch, int out_stride, int iterations, int norm_area, hipStream_t s) {
    const int group = launch_group(p, count);
    int rc = FDR_OK;
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const int n = count - i0 < group ? count - i0 : group;
        if (n == 1) {  // a group of one is the single-image call
            rc = rl_plain_dev(p, fn, d_imgs + (size_t)i0 * img_pitch, rows, cols, stride, d_out + (size_t)i0 * out_pitch, out_stride, iterations,
                              norm_area, s);
            continue;
        }
        fdr_plan::Slot* ws[kMaxGroup];
        const float* ins[kMaxGroup];
        float* outs[kMaxGroup];
        for (int k = 0; k < n; ++k) {
            ws[k] = &p->slots[k]; ins[k] = d_imgs + (size_t)(i0 + k) * img_pitch; outs[k] = d_out + (size_t)(i0 + k) * out_pitch;
        }
        rc = rl_group_dev(p, fn, ws, n, ins, rows, cols, stride, outs, out_stride, iterations, norm_area, s);
    }
    return rc;
}

// The free-boundary form.  The weights serve every image, so the coverage alpha = fullblur^T(W) and wgt = 1 / alpha are computed once
// per call, from the setup of image 0, and image 0 starts as in its single call.  Every other image runs the same setup (its dw and
// its sums; W again, into its own u plane, which the start overwrites) and the same start kernel on a copy of wgt in its slot's raw
// plane with the threshold 0: wgt > 0 exactly where alpha > sigma (for a finite alpha), so u = sum dw / sum W there and 0 elsewhere,
// the bits of the single call.
int rlfree_batch_dev_impl(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                          const float* d_w, int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_rlfree_params& prm,
                          hipStream_t s) {
    const int group = launch_group(p, count);
    int rc = FDR_OK;
    if (group == 1) {  // the loop of the single-image calls
        for (int i = 0; i < count && rc == FDR_OK; ++i)
            rc = rlfree_plain_dev(p, fn, d_imgs + (size_t)i * img_pitch, rows, cols, stride, d_w, wstride, d_out + (size_t)i * out_pitch,
                                  out_stride, prm, s);
        return rc;
    }
    const int M = p->M, N = p->N;
    const double* sums = nullptr;
    rc = rlfree_setup_image(p, d_imgs, rows, cols, stride, d_w, wstride, p->rf_dw, p->rf_u, rlfree_part(p, 0), &sums, s);
    if (rc == FDR_OK) rc = blur_window_dev(p, p->rf_u, rows, cols, cols, p->rf_wgt, N, M, N, 1, s);  // alpha over the whole plan
    if (rc == FDR_OK) rc = rlfree_start_image(p, p->rf_wgt, p->rf_u, prm.sigma, sums, s);
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const int n = count - i0 < group ? count - i0 : group;
        fdr_plan::Slot* ws[kMaxGroup];
        float* us[kMaxGroup];
        const float* dws[kMaxGroup];
        for (int k = 0; k < n && rc == FDR_OK; ++k) {
            ws[k] = &p->slots[k]; us[k] = rlfree_u_plane(p, k); dws[k] = rlfree_dw_plane(p, k);
            if (i0 + k == 0) continue;  // started above
            rc = rlfree_setup_image(p, d_imgs + (size_t)(i0 + k) * img_pitch, rows, cols, stride, d_w, wstride, rlfree_dw_plane(p, k), us[k],
                                    rlfree_part(p, k), &sums, s);
            if (rc != FDR_OK) break;
            FDR_HIP(hipMemcpyAsync(ws[k]->raw, p->rf_wgt, (size_t)M * N * sizeof(float), hipMemcpyDeviceToDevice, s));
            rc = rlfree_start_image(p, ws[k]->raw, us[k], 0.f, sums, s);
        }
        for (int it = 0; it < prm.iterations && rc == FDR_OK; ++it) rc = rlfree_step_n(p, ws, n, us, dws, rows, cols, s);
        for (int k = 0; k < n && rc == FDR_OK; ++k) rc = rlfree_finish(p, fn, us[k], d_out + (size_t)(i0 + k) * out_pitch, out_stride, prm, s);
    }
    return rc;
}

// checked arguments -> the workspace of the form -> its driver
int rl_batch_run(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                 const float* d_w, int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_rl_batch_params& b,
                 const fdr_rlfree_params& free_prm, hipStream_t s) {
    if (!b.free_boundary)
        return rl_batch_dev_impl(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, b.iterations, b.norm_area, s);
    const int rc = ensure_rlfree_workspace(p, fn, launch_group(p, count));
    if (rc != FDR_OK) return rc;
    return rlfree_batch_dev_impl(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_w, wstride, d_out, out_pitch, out_stride, free_prm, s);
}

}  // namespace

extern "C" {

int fdr_blur_batch_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride, float* d_out,
                           size_t out_pitch, int out_stride, int adjoint, void* stream) {
    const char* fn = "fdr_blur_batch_f32_dev";
    if (!p) return null_arg(fn);
    if (count < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": negative count");
    if (count == 0) return FDR_OK;
    if (!d_imgs || !d_out) return null_arg(fn);
    int rc = check_window(p, fn, NEED_OPERATOR_PSF, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    const int group = launch_group(p, count);
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const int n = count - i0 < group ? count - i0 : group;
        fdr_plan::Slot* ws[kMaxGroup];
        const float* ins[kMaxGroup];
        float* outs[kMaxGroup];
        for (int k = 0; k < n; ++k) {
            ws[k] = &p->slots[k]; ins[k] = d_imgs + (size_t)(i0 + k) * img_pitch; outs[k] = d_out + (size_t)(i0 + k) * out_pitch;
        }
        rc = blur_window_dev_n(p, ws, n, ins, rows, cols, stride, outs, out_stride, adjoint, s);
    }
    return rc;
}

int fdr_richardson_lucy_batch_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                      const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                      const fdr_rl_batch_params* params, void* stream) {
    const char* fn = "fdr_richardson_lucy_batch_f32_dev";
    if (!p || !params) return null_arg(fn);
    if (count < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": negative count");
    if (count == 0) return FDR_OK;
    if (!d_imgs || !d_out) return null_arg(fn);
    fdr_rlfree_params free_prm{};
    const int rc = rl_batch_check(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, *params,
                                  &free_prm);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return rl_batch_run(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, *params, free_prm,
                        (hipStream_t)stream);
}

// host pointers: every image in (dense), the batch on the null stream, every result back; one-shot device buffers
int fdr_richardson_lucy_batch_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                  const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                  const fdr_rl_batch_params* params) {
    const char* fn = "fdr_richardson_lucy_batch_f32";
    if (!p || !params) return null_arg(fn);
    if (count < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": negative count");
    if (count == 0) return FDR_OK;
    if (!imgs_host || !out_host) return null_arg(fn);
    fdr_rlfree_params free_prm{};
    int rc = rl_batch_check(p, fn, imgs_host, img_pitch, count, rows, cols, stride, weights_host, wstride, out_host, out_pitch, out_stride, *params,
                            &free_prm);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const int out_rows = params->free_boundary ? params->out_rows : rows, out_cols = params->free_boundary ? params->out_cols : cols;
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
        fdr_rl_batch_params b = *params;
        rc = rl_batch_run(p, fn, d_in.as<float>(), in_px, count, rows, cols, cols, d_w.as<float>(), cols, d_out.as<float>(), out_px, out_cols, b,
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

}  // extern "C"
