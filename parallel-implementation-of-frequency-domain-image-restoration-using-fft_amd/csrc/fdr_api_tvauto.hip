// fdr_api_tvauto.hip -- noise-constrained TV deconvolution (fdr_tv_deconv_auto_f32*; kernels in fdr_tvauto.hip): the free-boundary
// iteration of fdr_api_tvfree.hip with the weight of every data step taken from the discrepancy of that step.  Here: the small block
// it adds to the workspaces of the free call (per image of a launch group), the checks and the two entry points.  The driver is the
// free call's (tvfree_group_dev with the AUTO data step), on the shared solve table built for nu; the batched entry points are in
// fdr_api_tvfreebatch.hip.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassTaNoise = "TVA noise: sum |d * n|";

bool finite_nonneg(float v) { return std::isfinite(v) && v >= 0.f; }

}  // namespace

namespace fdr {

// everything an auto call refuses, before any device work: what the free call refuses, then its own arguments
int tvauto_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
                 const float* out, int out_stride, const fdr_tv_auto_params* prm, const double* d_trace, TvAutoArgs* a) {
    if (!prm) return null_arg(fn);
    if (!finite_nonneg(prm->sigma) || !finite_nonneg(prm->tau)) return fail(FDR_ERR_ARG, std::string(fn) + ": sigma and tau must be finite and >= 0");
    // nu = 0 selects the ratio; a rho the free check refuses gives a nu it refuses too, or is refused itself
    const float nu = prm->nu != 0.f ? prm->nu : FDR_TV_AUTO_NU_RATIO * prm->rho;
    a->fp = fdr_tv_free_params{1.f, prm->rho, nu, prm->iterations, prm->anisotropic, prm->nonneg, prm->norm_area, prm->out_rows, prm->out_cols};
    int rc = tvfree_check(p, fn, img, rows, cols, stride, weights, wstride, out, out_stride, &a->fp);
    if (rc != FDR_OK) return rc;
    if (!(a->fp.nu > 0.f)) return fail(FDR_ERR_ARG, std::string(fn) + ": nu must be finite and >= 0");
    a->sigma = prm->sigma;
    a->tau = prm->tau != 0.f ? (double)prm->tau : 1.0;
    a->estimate = prm->sigma == 0.f;
    if (a->estimate) {
        rc = noise_window_check(fn, rows, cols, stride);
        if (rc != FDR_OK) return rc;
    }
    if (d_trace && prm->iterations > 0) {
        const ByteRange t = byte_range(d_trace, (size_t)prm->iterations * 3 * sizeof(double));
        if (ranges_overlap(t, window_range(img, rows, cols, stride))) return fail(FDR_ERR_ARG, std::string(fn) + ": the trace overlaps the input");
        if (ranges_overlap(t, window_range(out, prm->out_rows, prm->out_cols, out_stride)))
            return fail(FDR_ERR_ARG, std::string(fn) + ": the trace overlaps the output");
        if (weights && ranges_overlap(t, window_range(weights, rows, cols, wstride)))
            return fail(FDR_ERR_ARG, std::string(fn) + ": the trace overlaps the weights");
    }
    return FDR_OK;
}

// the first auto call of a plan, or the first on a larger group
int ensure_tvauto_workspace(fdr_plan* p, const char* fn, int group) {
    return ensure_workspace(p->tvauto.ws, fn, "noise-constrained TV workspace", group, [p](auto& c, int g) {
        layout(c, p->tvauto, (size_t)tvauto_max_partials(p->M, p->N), (size_t)kRegMaxPartials + 1, g);
    });
}

// the free call's workspaces first, then the block of this call
int tvauto_prepare(fdr_plan* p, const char* fn, int group) {
    int rc = tvfree_prepare(p, fn, group);
    if (rc == FDR_OK) rc = ensure_tvauto_workspace(p, fn, group);
    return rc;
}

// the noise level of one window, as fdr_noise_sigma_f32 estimates it: one launch and one read-back (waits for `s`)
int tvauto_noise_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, double* sigma, hipStream_t s) {
    ScopedPass t(p, s, kPassTaNoise);
    return noise_sigma_dev(d_img, rows, cols, stride, p->tvauto.noise, sigma, s);
}

}  // namespace fdr

namespace {

// The whole call on `s`: the noise estimate when sigma is not given (one read-back), then the iteration.  *sigma_used, when not
// null, receives the noise level of the ball.
int tvauto_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* d_out,
                    int out_stride, const TvAutoArgs& a, double* d_trace, double* sigma_used, hipStream_t s) {
    double sigma = a.sigma;
    if (a.estimate && a.fp.iterations > 0) {
        const int rc = tvauto_noise_dev(p, d_img, rows, cols, stride, &sigma, s);
        if (rc != FDR_OK) return rc;
    }
    if (sigma_used) *sigma_used = sigma;
    TvDataStep au = tv_data_auto(a.tau);
    au.sigma[0] = sigma;
    au.trace[0] = d_trace;
    return tvfree_dev_impl(p, fn, d_img, rows, cols, stride, d_w, wstride, d_out, out_stride, a.fp, s, au);
}

}  // namespace

extern "C" {

int fdr_tv_deconv_auto_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                               float* d_out, int out_stride, const fdr_tv_auto_params* params, double* d_trace, void* stream) {
    const char* fn = "fdr_tv_deconv_auto_f32_dev";
    if (!p || !d_img || !d_out) return null_arg(fn);
    TvAutoArgs a{};
    int rc = tvauto_check(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, params, d_trace, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = tvauto_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    return tvauto_dev_impl(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, a, d_trace, nullptr, (hipStream_t)stream);
}

int fdr_tv_deconv_auto_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                           float* out_host, int out_stride, const fdr_tv_auto_params* params, fdr_tv_auto_result* result, double* trace_host) {
    const char* fn = "fdr_tv_deconv_auto_f32";
    if (!p || !img_host || !out_host) return null_arg(fn);
    TvAutoArgs a{};
    int rc = tvauto_check(p, fn, img_host, rows, cols, stride, weights_host, wstride, out_host, out_stride, params, nullptr, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = tvauto_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    const int n = a.fp.iterations;
    DeviceBuffer d_w, d_tr;  // the dense weights and the trace, for this call alone
    rc = stage_crop_weights(fn, weights_host, rows, cols, wstride, &d_w);
    if (rc != FDR_OK) return rc;
    if (trace_host && n > 0) FDR_ALLOC(d_tr, (size_t)n * 3 * sizeof(double), fn);
    double sigma = a.sigma;
    rc = host_image_call(p, fn, img_host, rows, cols, stride, out_host, a.fp.out_rows, a.fp.out_cols, out_stride,
                         [&](const float* d_in, float* d_out) {
                             return tvauto_dev_impl(p, fn, d_in, rows, cols, cols, d_w.as<float>(), cols, d_out, a.fp.out_cols, a,
                                                    d_tr.as<double>(), &sigma, nullptr);
                         });
    if (rc != FDR_OK) return rc;
    if (trace_host && n > 0) FDR_HIP(hipMemcpy(trace_host, d_tr.ptr, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (result) {
        double st[4] = {0.0, 0.0, 0.0, 0.0};  // (res_c, res_e, mu_k, S) of the last step
        if (n > 0) FDR_HIP(hipMemcpy(st, p->tvauto.stat, sizeof st, hipMemcpyDeviceToHost));
        *result = fdr_tv_auto_result{sigma, a.tau * sigma * sigma * st[3], st[2], st[0], st[3]};
    }
    return FDR_OK;
}

}  // extern "C"
