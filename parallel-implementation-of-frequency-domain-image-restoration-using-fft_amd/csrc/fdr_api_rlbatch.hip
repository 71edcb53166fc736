// fdr_api_rlbatch.hip -- the blur operator and Richardson-Lucy, both forms, on several images per launch (fdr_blur_batch_f32_dev,
// fdr_richardson_lucy_batch_f32*): `count` images with one operator PSF (and, free-boundary form, one weights plane) are cut into
// launch groups of plan->group images, and every pass of a group is ONE launch over its images (the group forms of the operator
// passes in fdr_api_operator.hip, the drivers rl_group_dev of fdr_api_rl.hip and rlfree_batch_dev of fdr_api_rlfree.hip).  A group
// runs to completion on the caller's stream, on the slots 0 .. g - 1, before the next one starts; the internal streams and
// FDR_OPT_BATCH_GRAPH are not used.  Every image comes out with the bits of its single-image call: the kernels of a group share the
// step plan and the epilogue of the single-image ones, and a group of one is the single-image call.
#include "fdr_host.hpp"

using namespace fdr;

namespace {

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
int rl_batch_run(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                 const float* d_w, int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_rl_batch_params& b,
                 const fdr_rlfree_params& free_prm, hipStream_t s) {
    const int group = launch_group(p, count);
    int rc = FDR_OK;
    if (b.free_boundary) {
        rc = ensure_rlfree_workspace(p, fn, group);
        if (rc != FDR_OK) return rc;
        return rlfree_batch_dev(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_w, wstride, d_out, out_pitch, out_stride, free_prm, s);
    }
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const LaunchGroup g(p, i0, count, d_imgs, img_pitch, d_out, out_pitch);
        rc = rl_group_dev(p, fn, g.ws, g.n, g.ins, rows, cols, stride, g.outs, out_stride, b.iterations, b.norm_area, s);
    }
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
