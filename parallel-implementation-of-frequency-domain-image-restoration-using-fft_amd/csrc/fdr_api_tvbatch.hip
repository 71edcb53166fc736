// fdr_api_tvbatch.hip -- total-variation deconvolution on several images per launch (fdr_tv_deconv_batch_f32*): `count` images with
// one operator PSF are cut into launch groups of plan->group images, and every pass of a group -- b, the start, per iteration the
// spatial kernel, the forward rows, the solve columns and the x rows, the output -- is ONE launch over its images (the driver
// tv_group_dev of fdr_api_tv.hip on the group forms of the operator passes).  A group runs to completion on the caller's stream, on the
// slots and workspace planes 0 .. g - 1, before the next one starts.  FDR_TV_COUPLE_NONE: every image comes out with the bits of its
// single-image call, and a group of one is that call.  FDR_TV_COUPLE_CHANNELS: the images are the channels of one picture and share
// one shrinkage by their joint gradient norm (vectorial TV; tv_spatial_coupled_kernel of fdr_tv.hip), so they sit in one group.
#include "fdr_host.hpp"

using namespace fdr;

namespace {

// what the batched TV calls refuse, before any device work: the single-image call on image 0 (plan, operator PSF, window, strides,
// mu, rho, iterations, norm_area), an unknown coupling, the coupled form with the anisotropic shrinkage or with more channels than
// the plan's launch group holds, and an output that overlaps the input anywhere in the span of the batch (a later group still reads
// its input after an earlier one has written its output)
int tv_batch_check(const fdr_plan* p, const char* fn, const float* imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                   const float* out, size_t out_pitch, int out_stride, const fdr_tv_batch_params& b, fdr_tv_params* one) {
    *one = fdr_tv_params{b.mu, b.rho, b.iterations, b.anisotropic, b.nonneg, b.norm_area};
    const int rc = tv_check(p, fn, rows, cols, stride, out_stride, one);
    if (rc != FDR_OK) return rc;
    if (b.coupling != FDR_TV_COUPLE_NONE && b.coupling != FDR_TV_COUPLE_CHANNELS) return fail(FDR_ERR_ARG, std::string(fn) + ": unknown coupling");
    if (b.coupling == FDR_TV_COUPLE_CHANNELS) {
        if (b.anisotropic) return fail(FDR_ERR_ARG, std::string(fn) + ": the coupled form has the isotropic shrinkage only");
        if (count > p->group)
            return fail(FDR_ERR_ARG, std::string(fn) + ": the coupled channels share one launch: count must not exceed the plan's group (fdr_plan_set_batching)");
    }
    if (ranges_overlap(window_range(out, rows, cols, out_stride, count, out_pitch), window_range(imgs, rows, cols, stride, count, img_pitch)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the outputs of the batch overlap its inputs");
    return FDR_OK;
}

// checked arguments -> the workspace for the group -> the driver, group by group
int tv_batch_run(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride, float* d_out,
                 size_t out_pitch, int out_stride, const fdr_tv_params& one, bool coupled, hipStream_t s) {
    const int group = launch_group(p, count);
    int rc = tv_prepare(p, fn, group);
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const LaunchGroup g(p, i0, count, d_imgs, img_pitch, d_out, out_pitch);
        rc = tv_group_dev(p, fn, g.ws, g.n, g.ins, rows, cols, stride, g.outs, out_stride, one, coupled, s);
    }
    return rc;
}

}  // namespace

extern "C" {

int fdr_tv_deconv_batch_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride, float* d_out,
                                size_t out_pitch, int out_stride, const fdr_tv_batch_params* params, void* stream) {
    const char* fn = "fdr_tv_deconv_batch_f32_dev";
    int rc;
    if (!tv_batch_begin(fn, p, params, count, d_imgs, d_out, &rc)) return rc;
    fdr_tv_params one{};
    rc = tv_batch_check(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, *params, &one);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return tv_batch_run(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, one,
                        params->coupling == FDR_TV_COUPLE_CHANNELS, (hipStream_t)stream);
}

int fdr_tv_deconv_batch_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride, float* out_host,
                            size_t out_pitch, int out_stride, const fdr_tv_batch_params* params) {
    const char* fn = "fdr_tv_deconv_batch_f32";
    int rc;
    if (!tv_batch_begin(fn, p, params, count, imgs_host, out_host, &rc)) return rc;
    fdr_tv_params one{};
    rc = tv_batch_check(p, fn, imgs_host, img_pitch, count, rows, cols, stride, out_host, out_pitch, out_stride, *params, &one);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const bool coupled = params->coupling == FDR_TV_COUPLE_CHANNELS;
    return host_batch_call(p, fn, imgs_host, img_pitch, count, rows, cols, stride, out_host, out_pitch, out_stride, rows, cols,
                           [&](const float* d_in, size_t px, float* d_out, size_t opx) {
                               return tv_batch_run(p, fn, d_in, px, count, rows, cols, cols, d_out, opx, cols, one, coupled, nullptr);
                           });
}

}  // extern "C"
