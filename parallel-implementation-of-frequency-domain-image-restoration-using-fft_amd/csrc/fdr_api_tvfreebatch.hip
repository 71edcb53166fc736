// fdr_api_tvfreebatch.hip -- free-boundary and noise-constrained TV deconvolution on several images per launch
// (fdr_tv_deconv_free_batch_f32*, fdr_tv_deconv_auto_batch_f32*): `count` crops with one operator PSF and one weights window are cut
// into launch groups of plan->group images, and every pass of a group is ONE launch over its images (the driver tvfree_group_dev of
// fdr_api_tvfree.hip on the group forms of the operator passes, of the TV kernels and of the window kernels).  A group runs to
// completion on the caller's stream, on the slots and workspace planes 0 .. g - 1, before the next one starts.  FDR_TV_COUPLE_NONE:
// every image comes out with the bits of its single-image call, and a group of one is that call.  FDR_TV_COUPLE_CHANNELS: the images
// are the channels of one picture and share one shrinkage by their joint gradient norm, so they sit in one group; the data step, the
// duals and, in the auto form, the ball, the sums and mu_k stay per channel.  Here: the checks, the loop over the groups and the
// four entry points.
#include "fdr_host.hpp"

#include <cmath>
#include <vector>

using namespace fdr;

namespace fdr {

// what the batched forms (these and the Poisson one of fdr_api_tvpoisson.hip) refuse beyond the single call on image 0 (checked
// by the caller), before any device work: an unknown coupling, the coupled form with the anisotropic shrinkage or with more channels than the plan's launch group holds, and any output
// of the batch that overlaps any input or the weights (a later group still reads them after an earlier one has written its output)
int crop_batch_check(const fdr_plan* p, const char* fn, const float* imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                     const float* weights, int wstride, const float* out, size_t out_pitch, int out_stride, const fdr_tv_free_params& one,
                     int coupling) {
    if (coupling != FDR_TV_COUPLE_NONE && coupling != FDR_TV_COUPLE_CHANNELS) return fail(FDR_ERR_ARG, std::string(fn) + ": unknown coupling");
    if (coupling == FDR_TV_COUPLE_CHANNELS) {
        if (one.anisotropic) return fail(FDR_ERR_ARG, std::string(fn) + ": the coupled form has the isotropic shrinkage only");
        if (count > p->group)
            return fail(FDR_ERR_ARG, std::string(fn) + ": the coupled channels share one launch: count must not exceed the plan's group (fdr_plan_set_batching)");
    }
    const ByteRange o = window_range(out, one.out_rows, one.out_cols, out_stride, count, out_pitch);
    if (ranges_overlap(o, window_range(imgs, rows, cols, stride, count, img_pitch)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the outputs of the batch overlap its inputs");
    if (weights && ranges_overlap(o, window_range(weights, rows, cols, wstride)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the outputs of the batch overlap the weights");
    return FDR_OK;
}

}  // namespace fdr

namespace {

int free_batch_check(const fdr_plan* p, const char* fn, const float* imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                     const float* weights, int wstride, const float* out, size_t out_pitch, int out_stride, const fdr_tv_free_batch_params& b,
                     fdr_tv_free_params* one) {
    *one = fdr_tv_free_params{b.mu, b.rho, b.nu, b.iterations, b.anisotropic, b.nonneg, b.norm_area, b.out_rows, b.out_cols};
    const int rc = tvfree_check(p, fn, imgs, rows, cols, stride, weights, wstride, out, out_stride, one);
    if (rc != FDR_OK) return rc;
    return crop_batch_check(p, fn, imgs, img_pitch, count, rows, cols, stride, weights, wstride, out, out_pitch, out_stride, *one, b.coupling);
}

// the auto form: the single call on image 0 (sigma, tau, nu and the rest), then the batch, the noise levels and the traces.  `trace`
// is the device range of the traces or null (the host form keeps its traces in a buffer of its own); want_trace says whether the
// caller asked for one, which is what the pitch is checked for.
int auto_batch_check(const fdr_plan* p, const char* fn, const float* imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                     const float* weights, int wstride, const float* out, size_t out_pitch, int out_stride, const fdr_tv_auto_batch_params& b,
                     const double* sigmas, const double* trace, bool want_trace, size_t trace_pitch, TvAutoArgs* a) {
    if (!std::isfinite(b.sigma) || b.sigma < 0.f) return fail(FDR_ERR_ARG, std::string(fn) + ": sigma and tau must be finite and >= 0");
    // with sigmas the common level is not used: whether a level is estimated is asked of the entries below
    const fdr_tv_auto_params one = {sigmas ? 1.f : b.sigma, b.tau, b.rho, b.nu, b.iterations, b.anisotropic, b.nonneg, b.norm_area, b.out_rows, b.out_cols};
    int rc = tvauto_check(p, fn, imgs, rows, cols, stride, weights, wstride, out, out_stride, &one, nullptr, a);
    if (rc != FDR_OK) return rc;
    rc = crop_batch_check(p, fn, imgs, img_pitch, count, rows, cols, stride, weights, wstride, out, out_pitch, out_stride, a->fp, b.coupling);
    if (rc != FDR_OK) return rc;
    if (sigmas) {
        bool estimate = false;
        for (int i = 0; i < count; ++i) {
            if (!std::isfinite(sigmas[i]) || sigmas[i] < 0.0) return fail(FDR_ERR_ARG, std::string(fn) + ": every entry of sigmas must be finite and >= 0");
            estimate = estimate || sigmas[i] == 0.0;
        }
        if (estimate) {
            rc = noise_window_check(fn, rows, cols, stride);
            if (rc != FDR_OK) return rc;
        }
    }
    const size_t n3 = (size_t)a->fp.iterations * 3;
    if (want_trace && n3 > 0) {
        if (count > 1 && trace_pitch < n3) return fail(FDR_ERR_ARG, std::string(fn) + ": trace_pitch must be >= 3 iterations");
        if (trace) {
            const ByteRange t = byte_range(trace, ((size_t)(count - 1) * trace_pitch + n3) * sizeof(double));
            if (ranges_overlap(t, window_range(imgs, rows, cols, stride, count, img_pitch)))
                return fail(FDR_ERR_ARG, std::string(fn) + ": the traces overlap the inputs");
            if (ranges_overlap(t, window_range(out, a->fp.out_rows, a->fp.out_cols, out_stride, count, out_pitch)))
                return fail(FDR_ERR_ARG, std::string(fn) + ": the traces overlap the outputs");
            if (weights && ranges_overlap(t, window_range(weights, rows, cols, wstride)))
                return fail(FDR_ERR_ARG, std::string(fn) + ": the traces overlap the weights");
        }
    }
    return FDR_OK;
}

// checked arguments -> the workspaces for the group -> the driver, group by group
int free_batch_run(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride, const float* d_w,
                   int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_tv_free_params& one, bool coupled, hipStream_t s) {
    const int group = launch_group(p, count);
    int rc = tvfree_prepare(p, fn, group);
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const LaunchGroup g(p, i0, count, d_imgs, img_pitch, d_out, out_pitch);
        rc = tvfree_group_dev(p, fn, g.ws, g.n, g.ins, rows, cols, stride, d_w, wstride, g.outs, out_stride, one, coupled, s);
    }
    return rc;
}

// The same for the auto form.  Image i's noise level is sigmas[i], or a.sigma without sigmas; a level of 0 is estimated from the
// image before its group's first iteration (one wait on `s` each).  sigma_used and stats (host; null: not wanted) receive every
// image's level and the (res_c, res_e, mu_k, S) of its last step: the sums of a group are read back when the group has run, before
// the next one overwrites them, which only the host form asks for.
int auto_batch_run(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride, const float* d_w,
                   int wstride, float* d_out, size_t out_pitch, int out_stride, const TvAutoArgs& a, const double* sigmas, bool coupled,
                   double* d_trace, size_t trace_pitch, double* sigma_used, double* stats, hipStream_t s) {
    const int group = launch_group(p, count);
    const int iters = a.fp.iterations;
    int rc = tvauto_prepare(p, fn, group);
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const LaunchGroup g(p, i0, count, d_imgs, img_pitch, d_out, out_pitch);
        TvDataStep au = tv_data_auto(a.tau);
        for (int k = 0; k < g.n && rc == FDR_OK; ++k) {
            double sigma = sigmas ? sigmas[i0 + k] : a.sigma;
            if (sigma == 0.0 && iters > 0) rc = tvauto_noise_dev(p, g.ins[k], rows, cols, stride, &sigma, s);
            au.sigma[k] = sigma;
            au.trace[k] = d_trace ? d_trace + (size_t)(i0 + k) * trace_pitch : nullptr;
            if (sigma_used) sigma_used[i0 + k] = sigma;
        }
        if (rc != FDR_OK) break;
        rc = tvfree_group_dev(p, fn, g.ws, g.n, g.ins, rows, cols, stride, d_w, wstride, g.outs, out_stride, a.fp, coupled, s, au);
        if (rc == FDR_OK && stats && iters > 0) {
            FDR_HIP(hipMemcpyAsync(stats + 4 * (size_t)i0, p->tvauto.stat, 4 * (size_t)g.n * sizeof(double), hipMemcpyDeviceToHost, s));
            FDR_HIP(hipStreamSynchronize(s));
        }
    }
    return rc;
}

}  // namespace

extern "C" {

int fdr_tv_deconv_free_batch_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                     const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                     const fdr_tv_free_batch_params* params, void* stream) {
    const char* fn = "fdr_tv_deconv_free_batch_f32_dev";
    int rc;
    if (!tv_batch_begin(fn, p, params, count, d_imgs, d_out, &rc)) return rc;
    fdr_tv_free_params one{};
    rc = free_batch_check(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, *params, &one);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return free_batch_run(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, one,
                          params->coupling == FDR_TV_COUPLE_CHANNELS, (hipStream_t)stream);
}

int fdr_tv_deconv_free_batch_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                 const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                 const fdr_tv_free_batch_params* params) {
    const char* fn = "fdr_tv_deconv_free_batch_f32";
    int rc;
    if (!tv_batch_begin(fn, p, params, count, imgs_host, out_host, &rc)) return rc;
    fdr_tv_free_params one{};
    rc = free_batch_check(p, fn, imgs_host, img_pitch, count, rows, cols, stride, weights_host, wstride, out_host, out_pitch, out_stride, *params,
                              &one);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const bool coupled = params->coupling == FDR_TV_COUPLE_CHANNELS;
    DeviceBuffer d_w;
    rc = stage_crop_weights(fn, weights_host, rows, cols, wstride, &d_w);
    if (rc != FDR_OK) return rc;
    return host_batch_call(p, fn, imgs_host, img_pitch, count, rows, cols, stride, out_host, out_pitch, out_stride, one.out_rows, one.out_cols,
                           [&](const float* d_in, size_t px, float* d_out, size_t opx) {
                               return free_batch_run(p, fn, d_in, px, count, rows, cols, cols, d_w.as<float>(), cols, d_out, opx, one.out_cols, one,
                                                     coupled, nullptr);
                           });
}

int fdr_tv_deconv_auto_batch_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                     const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                     const fdr_tv_auto_batch_params* params, const double* sigmas, double* d_trace, size_t trace_pitch,
                                     void* stream) {
    const char* fn = "fdr_tv_deconv_auto_batch_f32_dev";
    int rc;
    if (!tv_batch_begin(fn, p, params, count, d_imgs, d_out, &rc)) return rc;
    TvAutoArgs a{};
    rc = auto_batch_check(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, *params,
                                    sigmas, d_trace, d_trace != nullptr, trace_pitch, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return auto_batch_run(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, a, sigmas,
                          params->coupling == FDR_TV_COUPLE_CHANNELS, d_trace, trace_pitch, nullptr, nullptr, (hipStream_t)stream);
}

int fdr_tv_deconv_auto_batch_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                 const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                 const fdr_tv_auto_batch_params* params, const double* sigmas, fdr_tv_auto_result* results, double* trace_host,
                                 size_t trace_pitch) {
    const char* fn = "fdr_tv_deconv_auto_batch_f32";
    int rc;
    if (!tv_batch_begin(fn, p, params, count, imgs_host, out_host, &rc)) return rc;
    TvAutoArgs a{};
    rc = auto_batch_check(p, fn, imgs_host, img_pitch, count, rows, cols, stride, weights_host, wstride, out_host, out_pitch, out_stride, *params,
                              sigmas, nullptr, trace_host != nullptr, trace_pitch, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const bool coupled = params->coupling == FDR_TV_COUPLE_CHANNELS;
    const size_t n3 = (size_t)a.fp.iterations * 3;
    DeviceBuffer d_w, d_tr;  // the dense weights and the traces (3 n doubles per image, dense), for this call alone
    rc = stage_crop_weights(fn, weights_host, rows, cols, wstride, &d_w);
    if (rc != FDR_OK) return rc;
    if (trace_host && n3 > 0) FDR_ALLOC(d_tr, (size_t)count * n3 * sizeof(double), fn);
    std::vector<double> sigma_used((size_t)count, 0.0), stats(4 * (size_t)count, 0.0);
    rc = host_batch_call(p, fn, imgs_host, img_pitch, count, rows, cols, stride, out_host, out_pitch, out_stride, a.fp.out_rows, a.fp.out_cols,
                         [&](const float* d_in, size_t px, float* d_out, size_t opx) {
                             return auto_batch_run(p, fn, d_in, px, count, rows, cols, cols, d_w.as<float>(), cols, d_out, opx, a.fp.out_cols, a,
                                                   sigmas, coupled, d_tr.as<double>(), n3, sigma_used.data(), results ? stats.data() : nullptr,
                                                   nullptr);
                         });
    if (rc != FDR_OK) return rc;
    if (trace_host && n3 > 0)  // (one image: its trace is 3 n doubles whatever the pitch says)
        FDR_HIP(hipMemcpy2D(trace_host, (count > 1 ? trace_pitch : n3) * sizeof(double), d_tr.ptr, n3 * sizeof(double), n3 * sizeof(double), (size_t)count,
                            hipMemcpyDeviceToHost));
    if (results)
        for (int i = 0; i < count; ++i) {
            const double* st = &stats[4 * (size_t)i];  // (res_c, res_e, mu_k, S) of the last step
            results[i] = fdr_tv_auto_result{sigma_used[i], a.tau * sigma_used[i] * sigma_used[i] * st[3], st[2], st[0], st[3]};
        }
    return FDR_OK;
}

}  // extern "C"
