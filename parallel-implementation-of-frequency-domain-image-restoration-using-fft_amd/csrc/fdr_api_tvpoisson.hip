// fdr_api_tvpoisson.hip -- Poisson-likelihood TV deconvolution (fdr_tv_deconv_poisson_f32*, its batches and the data step alone;
// kernel in fdr_tvfree.hip): the free-boundary iteration of fdr_api_tvfree.hip with the least-squares data step replaced by that
// of the Poisson term mu m [(blur(x) + b) - d+ log(blur(x) + b)].  Here: the checks and the entry points.  The driver is the free
// call's (tvfree_group_dev with the POISSON data step), on its workspaces and on the shared solve table built for nu; nothing is allocated
// that the free call does not allocate.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

namespace {

fdr_tv_free_params free_params(const fdr_tv_poisson_params& q) {
    return fdr_tv_free_params{q.mu, q.rho, q.nu, q.iterations, q.anisotropic, q.nonneg, q.norm_area, q.out_rows, q.out_cols};
}

int background_check(const char* fn, float background) {
    if (!std::isfinite(background) || background < 0.f) return fail(FDR_ERR_ARG, std::string(fn) + ": background must be finite and >= 0");
    return FDR_OK;
}

// everything a Poisson call refuses for one image, before any device work: what the free call refuses, and the background
int poisson_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
                  const float* out, int out_stride, const fdr_tv_poisson_params* prm, fdr_tv_free_params* fp) {
    if (!prm) return null_arg(fn);
    *fp = free_params(*prm);
    const int rc = tvfree_check(p, fn, img, rows, cols, stride, weights, wstride, out, out_stride, fp);
    if (rc != FDR_OK) return rc;
    return background_check(fn, prm->background);
}

int poisson_batch_check(const fdr_plan* p, const char* fn, const float* imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                        const float* weights, int wstride, const float* out, size_t out_pitch, int out_stride,
                        const fdr_tv_poisson_batch_params& b, fdr_tv_free_params* fp) {
    const fdr_tv_poisson_params one = {b.mu, b.rho, b.nu, b.background, b.iterations, b.anisotropic, b.nonneg, b.norm_area, b.out_rows, b.out_cols};
    const int rc = poisson_check(p, fn, imgs, rows, cols, stride, weights, wstride, out, out_stride, &one, fp);
    if (rc != FDR_OK) return rc;
    return crop_batch_check(p, fn, imgs, img_pitch, count, rows, cols, stride, weights, wstride, out, out_pitch, out_stride, *fp, b.coupling);
}

// checked arguments -> the free call's workspaces for the group -> the driver, group by group
int poisson_batch_run(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                      const float* d_w, int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_tv_free_params& fp,
                      float background, bool coupled, hipStream_t s) {
    const int group = launch_group(p, count);
    const TvDataStep po = tv_data_poisson(background);
    int rc = tvfree_prepare(p, fn, group);
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const LaunchGroup g(p, i0, count, d_imgs, img_pitch, d_out, out_pitch);
        rc = tvfree_group_dev(p, fn, g.ws, g.n, g.ins, rows, cols, stride, d_w, wstride, g.outs, out_stride, fp, coupled, s, po);
    }
    return rc;
}

// what the step alone refuses: a plan whose planes the kernel cannot take, a window outside them, the strides, the three scalars,
// planes that are not 16-byte aligned
int step_check(const fdr_plan* p, const char* fn, int rows, int cols, int stride, const float* d_w, int wstride, float mu, float nu,
               float background) {
    if (p->M < 1 || p->N < 4 || (p->N & 3)) return fail(FDR_ERR_ARG, std::string(fn) + ": the plan's N must be a multiple of 4");
    if (rows < 1 || cols < 1 || rows > p->M || cols > p->N) return fail(FDR_ERR_ARG, std::string(fn) + ": the window must lie within the plan");
    if (stride < cols) return fail(FDR_ERR_ARG, std::string(fn) + ": stride must be >= cols");
    if (d_w && wstride < cols) return fail(FDR_ERR_ARG, std::string(fn) + ": the weights' stride must be >= cols");
    if (!std::isfinite(mu) || !(mu > 0.f)) return fail(FDR_ERR_ARG, std::string(fn) + ": mu must be finite and > 0");
    if (!std::isfinite(nu) || !(nu > 0.f)) return fail(FDR_ERR_ARG, std::string(fn) + ": nu must be finite and > 0");
    return background_check(fn, background);
}

}  // namespace

extern "C" {

int fdr_tv_deconv_poisson_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                                  float* d_out, int out_stride, const fdr_tv_poisson_params* params, void* stream) {
    const char* fn = "fdr_tv_deconv_poisson_f32_dev";
    if (!p || !d_img || !d_out) return null_arg(fn);
    fdr_tv_free_params fp{};
    int rc = poisson_check(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, params, &fp);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = tvfree_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    return tvfree_dev_impl(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, fp, (hipStream_t)stream,
                           tv_data_poisson(params->background));
}

int fdr_tv_deconv_poisson_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                              float* out_host, int out_stride, const fdr_tv_poisson_params* params) {
    const char* fn = "fdr_tv_deconv_poisson_f32";
    if (!p || !img_host || !out_host) return null_arg(fn);
    fdr_tv_free_params fp{};
    int rc = poisson_check(p, fn, img_host, rows, cols, stride, weights_host, wstride, out_host, out_stride, params, &fp);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = tvfree_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    const TvDataStep po = tv_data_poisson(params->background);
    DeviceBuffer d_w;  // the weights, dense, for this call alone
    rc = stage_crop_weights(fn, weights_host, rows, cols, wstride, &d_w);
    if (rc != FDR_OK) return rc;
    return host_image_call(p, fn, img_host, rows, cols, stride, out_host, fp.out_rows, fp.out_cols, out_stride,
                           [&](const float* d_in, float* d_out) {
                               return tvfree_dev_impl(p, fn, d_in, rows, cols, cols, d_w.as<float>(), cols, d_out, fp.out_cols, fp, nullptr, po);
                           });
}

int fdr_tv_deconv_poisson_batch_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                        const float* d_weights, int wstride, float* d_out, size_t out_pitch, int out_stride,
                                        const fdr_tv_poisson_batch_params* params, void* stream) {
    const char* fn = "fdr_tv_deconv_poisson_batch_f32_dev";
    int rc;
    if (!tv_batch_begin(fn, p, params, count, d_imgs, d_out, &rc)) return rc;
    fdr_tv_free_params fp{};
    rc = poisson_batch_check(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, *params, &fp);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return poisson_batch_run(p, fn, d_imgs, img_pitch, count, rows, cols, stride, d_weights, wstride, d_out, out_pitch, out_stride, fp,
                             params->background, params->coupling == FDR_TV_COUPLE_CHANNELS, (hipStream_t)stream);
}

int fdr_tv_deconv_poisson_batch_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                    const float* weights_host, int wstride, float* out_host, size_t out_pitch, int out_stride,
                                    const fdr_tv_poisson_batch_params* params) {
    const char* fn = "fdr_tv_deconv_poisson_batch_f32";
    int rc;
    if (!tv_batch_begin(fn, p, params, count, imgs_host, out_host, &rc)) return rc;
    fdr_tv_free_params fp{};
    rc = poisson_batch_check(p, fn, imgs_host, img_pitch, count, rows, cols, stride, weights_host, wstride, out_host, out_pitch, out_stride, *params,
                                 &fp);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const bool coupled = params->coupling == FDR_TV_COUPLE_CHANNELS;
    const float background = params->background;
    DeviceBuffer d_w;
    rc = stage_crop_weights(fn, weights_host, rows, cols, wstride, &d_w);
    if (rc != FDR_OK) return rc;
    return host_batch_call(p, fn, imgs_host, img_pitch, count, rows, cols, stride, out_host, out_pitch, out_stride, fp.out_rows, fp.out_cols,
                           [&](const float* d_in, size_t px, float* d_out, size_t opx) {
                               return poisson_batch_run(p, fn, d_in, px, count, rows, cols, cols, d_w.as<float>(), cols, d_out, opx, fp.out_cols, fp,
                                                        background, coupled, nullptr);
                           });
}

int fdr_tv_poisson_step_f32_dev(fdr_plan* p, float* d_c, float* d_q, const float* d_img, int rows, int cols, int stride, const float* d_weights,
                                int wstride, float mu, float nu, float background, void* stream) {
    const char* fn = "fdr_tv_poisson_step_f32_dev";
    if (!p || !d_c || !d_q || !d_img) return null_arg(fn);
    const int rc = step_check(p, fn, rows, cols, stride, d_weights, wstride, mu, nu, background);
    if (rc != FDR_OK) return rc;
    if (((uintptr_t)d_c & 15) || ((uintptr_t)d_q & 15)) return fail(FDR_ERR_ARG, std::string(fn) + ": the planes c and q must be 16-byte aligned");
    const ByteRange c = window_range(d_c, p->M, p->N, p->N), q = window_range(d_q, p->M, p->N, p->N);
    const ByteRange d = window_range(d_img, rows, cols, stride);
    if (ranges_overlap(c, q) || ranges_overlap(c, d) || ranges_overlap(q, d) ||
        (d_weights && (ranges_overlap(c, window_range(d_weights, rows, cols, wstride)) || ranges_overlap(q, window_range(d_weights, rows, cols, wstride)))))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the planes c and q overlap each other, the data or the weights");
    FDR_HIP(hipSetDevice(p->device));
    FDR_HIP(launch_tvpoisson_data_n(1, &d_c, &d_q, &d_img, stride, d_weights, wstride, rows, cols, p->M, p->N, mu, nu, background, (hipStream_t)stream));
    return FDR_OK;
}

int fdr_tv_poisson_step_group_f32_dev(fdr_plan* p, float* d_c, size_t c_pitch, float* d_q, size_t q_pitch, const float* d_imgs, size_t img_pitch,
                                      int count, int rows, int cols, int stride, const float* d_weights, int wstride, float mu, float nu,
                                      float background, void* stream) {
    const char* fn = "fdr_tv_poisson_step_group_f32_dev";
    if (!p || !d_c || !d_q || !d_imgs) return null_arg(fn);
    if (count < 1 || count > kMaxGroup) return fail(FDR_ERR_ARG, std::string(fn) + ": count must lie in 1 .. 8");
    const int rc = step_check(p, fn, rows, cols, stride, d_weights, wstride, mu, nu, background);
    if (rc != FDR_OK) return rc;
    const size_t P = (size_t)p->M * p->N;
    if (((uintptr_t)d_c & 15) || ((uintptr_t)d_q & 15) || (count > 1 && ((c_pitch & 3) || (q_pitch & 3))))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the planes c and q must be 16-byte aligned");
    if (count > 1 && (c_pitch < P || q_pitch < P)) return fail(FDR_ERR_ARG, std::string(fn) + ": the planes of the group overlap each other");
    const ByteRange c = window_range(d_c, p->M, p->N, p->N, count, c_pitch), q = window_range(d_q, p->M, p->N, p->N, count, q_pitch);
    const ByteRange d = window_range(d_imgs, rows, cols, stride, count, img_pitch);
    if (ranges_overlap(c, q) || ranges_overlap(c, d) || ranges_overlap(q, d) ||
        (d_weights && (ranges_overlap(c, window_range(d_weights, rows, cols, wstride)) || ranges_overlap(q, window_range(d_weights, rows, cols, wstride)))))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the planes c and q overlap each other, the data or the weights");
    float *cs[kMaxGroup], *qs[kMaxGroup];
    const float* ds[kMaxGroup];
    for (int k = 0; k < count; ++k) { cs[k] = d_c + k * c_pitch; qs[k] = d_q + k * q_pitch; ds[k] = d_imgs + k * img_pitch; }
    FDR_HIP(hipSetDevice(p->device));
    FDR_HIP(launch_tvpoisson_data_n(count, cs, qs, ds, stride, d_weights, wstride, rows, cols, p->M, p->N, mu, nu, background, (hipStream_t)stream));
    return FDR_OK;
}

}  // extern "C"
