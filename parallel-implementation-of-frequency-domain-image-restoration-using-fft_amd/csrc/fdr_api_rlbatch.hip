// fdr_api_rlbatch.hip -- the blur operator and Richardson-Lucy, both forms, on several images per launch (fdr_blur_batch_f32_dev,
// fdr_richardson_lucy_batch_f32*, fdr_richardson_lucy_batch_accel_f32*): `count` images with one operator PSF (and, free-boundary form, one weights plane) are cut into
// launch groups of plan->group images, and every pass of a group is ONE launch over its images (the group forms of the operator
// passes in fdr_api_operator.hip, the drivers rl_group_dev of fdr_api_rl.hip and rlfree_batch_dev of fdr_api_rlfree.hip).  A group
// runs to completion on the caller's stream, on the slots 0 .. g - 1, before the next one starts; the internal streams and
// FDR_OPT_BATCH_GRAPH are not used.  Every image comes out with the bits of its single-image call: the kernels of a group share the
// step plan and the epilogue of the single-image ones, and a group of one is the single-image call.  The accelerated batch runs the
// recursion of fdr_api_rlaccel.hip on the group (drivers rl_group_accel_dev, rlfree_batch_dev with `accel`): per iteration one
// extrapolation, one direction and one alpha launch for the group, every image with its own inner products and its own alpha.
#include "fdr_host.hpp"

using namespace fdr;

namespace fdr {

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
        int rc = plain_form_check(fn, weights, rows, cols, b.out_rows, b.out_cols, false,
                                  ": the plain form's output window is rows x cols (out_rows = out_cols = 0, or rows and cols)");
        if (rc == FDR_OK) rc = rl_check(p, fn, imgs, rows, cols, stride, out, out_stride, b.iterations, b.norm_area);
        if (rc != FDR_OK) return rc;
    }
    const ByteRange so = window_range(out, out_rows, out_cols, out_stride, count, out_pitch);
    if (ranges_overlap(so, window_range(imgs, rows, cols, stride, count, img_pitch)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the outputs of the batch overlap its inputs (the input is read on every iteration)");
    if (weights && ranges_overlap(so, window_range(weights, rows, cols, wstride)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the outputs of the batch overlap the weights");
    return FDR_OK;
}

// checked arguments -> the workspace of the form -> its driver, the plain form's group by group
// (`accel`: the accelerated recursion, image i's alphas to d_alphas + i alpha_pitch when d_alphas is not null; the acceleration
// workspace grows to the group before anything runs.  Groups of one are the loop of the single accelerated calls in either form.)
int rl_batch_run(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                 const float* d_w, int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_rl_batch_params& b,
                 const fdr_rlfree_params& free_prm, hipStream_t s, bool accel, float* d_alphas, size_t alpha_pitch) {
    const int group = launch_group(p, count);
    int rc = FDR_OK;
    if (b.free_boundary) rc = ensure_rlfree_workspace(p, fn, group);
    if (rc == FDR_OK && accel) rc = ensure_rlaccel_workspace(p, fn, group);
    if (rc != FDR_OK) return rc;
    if (b.free_boundary)
        return rlfree_batch_dev(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_w, wstride, d_out, out_pitch, out_stride, free_prm, s, nullptr,
                                nullptr, accel, d_alphas, alpha_pitch);
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const LaunchGroup g(p, i0, count, d_imgs, img_pitch, d_out, out_pitch);
        if (accel)
            rc = rl_group_accel_dev(p, fn, g.ws, g.n, g.ins, rows, cols, stride, g.outs, out_stride, b.iterations, b.norm_area,
                                    d_alphas ? d_alphas + (size_t)i0 * alpha_pitch : nullptr, alpha_pitch, s);
        else
            rc = rl_group_dev(p, fn, g.ws, g.n, g.ins, rows, cols, stride, g.outs, out_stride, b.iterations, b.norm_area, s);
    }
    return rc;
}

}  // namespace fdr

namespace {

// what the accelerated batch refuses on top of rl_batch_check: an alpha pitch below the iteration count, and alphas that overlap,
// anywhere in the span of the batch, the inputs, the outputs or the weights.  Null alphas or no iterations: nothing to check.
int rl_batch_alphas_check(const char* fn, const float* imgs, size_t img_pitch, int count, int rows, int cols, int stride, const float* weights,
                          int wstride, const float* out, size_t out_pitch, int out_stride, const fdr_rl_batch_params& b, const float* alphas,
                          size_t alpha_pitch) {
    if (!alphas || b.iterations <= 0) return FDR_OK;
    if (alpha_pitch < (size_t)b.iterations) return fail(FDR_ERR_ARG, std::string(fn) + ": alpha_pitch must be >= iterations");
    const ByteRange al = byte_range(alphas, ((size_t)(count - 1) * alpha_pitch + (size_t)b.iterations) * sizeof(float));
    const int out_rows = b.free_boundary ? b.out_rows : rows, out_cols = b.free_boundary ? b.out_cols : cols;
    if (ranges_overlap(al, window_range(out, out_rows, out_cols, out_stride, count, out_pitch)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the alphas overlap the outputs of the batch");
    if (ranges_overlap(al, window_range(imgs, rows, cols, stride, count, img_pitch)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the alphas overlap the inputs of the batch");
    if (weights && ranges_overlap(al, window_range(weights, rows, cols, wstride)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the alphas overlap the weights");
    return FDR_OK;
}

// the _dev entry of both batches
int rl_batch_dev_entry(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                       const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_rl_batch_params* params,
                       bool accel, float* d_alphas, size_t alpha_pitch, hipStream_t s) {
    if (!p || !params) return null_arg(fn);
    if (count < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": negative count");
    if (count == 0) return FDR_OK;
    if (!d_imgs || !d_out) return null_arg(fn);
    fdr_rlfree_params free_prm{};
    int rc = rl_batch_check(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, *params, &free_prm);
    if (rc == FDR_OK && accel)
        rc = rl_batch_alphas_check(fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, *params,
                                   d_alphas, alpha_pitch);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return rl_batch_run(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, *params, free_prm, s,
                        accel, d_alphas, alpha_pitch);
}

// host pointers: every image in (dense), the batch on the null stream, every result back; one-shot device buffers
// (accelerated: the alphas of image i dense on the device, `iterations` apart, back to alphas_host + i alpha_pitch)
int rl_batch_host_entry(fdr_plan* p, const char* fn, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                        const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                        const fdr_rl_batch_params* params, bool accel, float* alphas_host, size_t alpha_pitch) {
    if (!p || !params) return null_arg(fn);
    if (count < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": negative count");
    if (count == 0) return FDR_OK;
    if (!imgs_host || !out_host) return null_arg(fn);
    fdr_rlfree_params free_prm{};
    int rc = rl_batch_check(p, fn, imgs_host, img_pitch, count, rows, cols, stride, weights_host, wstride, out_host, out_pitch, out_stride, *params,
                            &free_prm);
    if (rc == FDR_OK && accel)
        rc = rl_batch_alphas_check(fn, imgs_host, img_pitch, count, rows, cols, stride, weights_host, wstride, out_host, out_pitch, out_stride,
                                   *params, alphas_host, alpha_pitch);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const int out_rows = params->free_boundary ? params->out_rows : rows, out_cols = params->free_boundary ? params->out_cols : cols;
    const size_t in_px = (size_t)rows * cols, out_px = (size_t)out_rows * out_cols;
    const size_t n_al = accel && alphas_host && params->iterations > 0 ? (size_t)params->iterations : 0;
    DeviceBuffer d_in, d_out, d_w, d_al;
    if (n_al) FDR_ALLOC(d_al, (size_t)count * n_al * sizeof(float), fn);
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
                          free_prm, nullptr, accel, n_al ? d_al.as<float>() : nullptr, n_al);
    }
    if (rc == FDR_OK) {
        ScopedPhase phase(p, FDR_PHASE_D2H, nullptr);
        for (int i = 0; i < count; ++i)
            FDR_HIP(hipMemcpy2D(out_host + (size_t)i * out_pitch, (size_t)out_stride * sizeof(float), d_out.as<float>() + (size_t)i * out_px,
                                (size_t)out_cols * sizeof(float), (size_t)out_cols * sizeof(float), (size_t)out_rows, hipMemcpyDeviceToHost));
        if (n_al)
            FDR_HIP(hipMemcpy2D(alphas_host, alpha_pitch * sizeof(float), d_al.ptr, n_al * sizeof(float), n_al * sizeof(float), (size_t)count,
                                hipMemcpyDeviceToHost));
    }
    (void)hipStreamSynchronize(nullptr);  // (also on an error: the one-shot buffers are freed on return)
    resolve_phases(p);
    return rc;
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
        const LaunchGroup g(p, i0, count, d_imgs, img_pitch, d_out, out_pitch);
        rc = blur_window_dev_n(p, g.ws, g.n, g.ins, rows, cols, stride, g.outs, out_stride, adjoint, s);
    }
    return rc;
}

int fdr_richardson_lucy_batch_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                      const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                      const fdr_rl_batch_params* params, void* stream) {
    return rl_batch_dev_entry(p, "fdr_richardson_lucy_batch_f32_dev", d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out,
                              out_pitch, out_stride, params, false, nullptr, 0, (hipStream_t)stream);
}

int fdr_richardson_lucy_batch_accel_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                            const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                            const fdr_rl_batch_params* params, float* d_alphas, size_t alpha_pitch, void* stream) {
    return rl_batch_dev_entry(p, "fdr_richardson_lucy_batch_accel_f32_dev", d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride,
                              d_out, out_pitch, out_stride, params, true, d_alphas, alpha_pitch, (hipStream_t)stream);
}

int fdr_richardson_lucy_batch_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                  const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                  const fdr_rl_batch_params* params) {
    return rl_batch_host_entry(p, "fdr_richardson_lucy_batch_f32", imgs_host, img_pitch, count, rows, cols, stride, weights_host, wstride, out_host,
                               out_pitch, out_stride, params, false, nullptr, 0);
}

int fdr_richardson_lucy_batch_accel_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                        const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                        const fdr_rl_batch_params* params, float* alphas_host, size_t alpha_pitch) {
    return rl_batch_host_entry(p, "fdr_richardson_lucy_batch_accel_f32", imgs_host, img_pitch, count, rows, cols, stride, weights_host, wstride,
                               out_host, out_pitch, out_stride, params, true, alphas_host, alpha_pitch);
}

}  // extern "C"
