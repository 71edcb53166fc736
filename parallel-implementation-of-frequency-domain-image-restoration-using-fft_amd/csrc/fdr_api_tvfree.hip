// fdr_api_tvfree.hip -- free-boundary, weighted TV deconvolution by ADMM with two splittings (fdr_tv_deconv_free_f32*; the data step
// in fdr_tvfree.hip): the two planes per image it adds to the TV workspace, the checks, the driver (on a group of n >= 1 images: the
// batches of fdr_api_tvfreebatch.hip run it too, and the noise-constrained and Poisson forms with their own data step, chosen by a
// TvDataStep) and the two entry points.  Everything but the data step is the periodic call's: the start of fdr_tv.hip, the table,
// the prior half-step and the output tail of fdr_api_tv.hip with nu in the place of mu, and the blur chain of fdr_api_operator.hip
// on full planes.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassTaNorm = "TVA norm+mu: res_e, res_c, S -> mu_k";
const char* const kPassTaData = "TVA data: s, q, r = 2s-e (mu_k)";

}  // namespace

namespace fdr {

// (shared with the multi-frame form of fdr_api_tvframes.hip, which runs these passes)
const char* const kPassTfInit = "TVF init: x = pad(d), w = q = 0";
const char* const kPassTfData = "TVF data: s, q, r = 2s-e (window)";
const char* const kPassTpData = "TVP data: Poisson s, q, r = 2s-e (window)";
const TvPassNames kTfPasses = {
    "TV table: 1/(nu|H|^2+rho L)/MN (free)",
    "TV spatial: shrink+dual+div (free)",
    "TV spatial: joint shrink+dual+div (free)",  // the coupled kernel, all channels of a tile
    "B' op cols: FFT*T*IFFT (TVF solve)",
    "C op rows: IFFT (TVF x)",
    "TVF out: crop+clamp",
    "E TVF minmax+normalize",
};

// everything a free-boundary TV call refuses, before any device work: what the periodic call refuses, and nu, the weights' stride,
// the output window and an output that overlaps the input or the weights (both are read in every iteration)
int tvfree_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
                 const float* out, int out_stride, const fdr_tv_free_params* prm, PlanNeed need) {
    if (!prm) return null_arg(fn);
    const fdr_tv_params periodic = {prm->mu, prm->rho, prm->iterations, prm->anisotropic, prm->nonneg, prm->norm_area};
    const int rc = tv_check(p, fn, rows, cols, stride, out_stride, &periodic, need);
    if (rc != FDR_OK) return rc;
    if (!std::isfinite(prm->nu) || prm->nu < 0.f) return fail(FDR_ERR_ARG, std::string(fn) + ": nu must be finite and >= 0");
    if (weights && wstride < cols) return fail(FDR_ERR_ARG, std::string(fn) + ": the weights' stride must be >= cols");
    if (prm->out_rows < rows || prm->out_rows > p->M || prm->out_cols < cols || prm->out_cols > p->N || out_stride < prm->out_cols)
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output window must lie in [rows .. M] x [cols .. N] and have a stride >= out_cols");
    const ByteRange o = window_range(out, prm->out_rows, prm->out_cols, out_stride);
    if (ranges_overlap(window_range(img, rows, cols, stride), o)) return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the input");
    if (weights && ranges_overlap(window_range(weights, rows, cols, wstride), o))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the weights");
    return FDR_OK;
}

// the new block first (nothing old is let go before it is had), then the periodic call's workspace for the group and the Laplacian table
int tvfree_prepare(fdr_plan* p, const char* fn, int group) {
    int rc = ensure_tvfree_workspace(p, fn, group);
    if (rc == FDR_OK) rc = tv_prepare(p, fn, group);
    return rc;
}

// x, b, the duals, q, c / r and rhs (slot k's raw plane) are full M x N planes; d and the weights are read from the caller's
// windows by every data step
int tvfree_group_dev(fdr_plan* p, const char* fn, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                     const float* d_w, int wstride, float* const* d_outs, int out_stride, const fdr_tv_free_params& prm, bool coupled, hipStream_t s,
                     const TvDataStep& data) {
    if (n < 1 || n > kMaxGroup || n > p->tv.ws.count || n > p->tvfree.ws.count || (data.kind == TvDataStep::AUTO && n > p->tvauto.ws.count))
        return fail(FDR_ERR_STATE, std::string(fn) + ": the free-boundary TV workspaces do not hold the group");
    const int M = p->M, N = p->N, iters = prm.iterations;
    const size_t P = (size_t)M * N, step = tv_image_stride(p);
    const float nu = prm.nu > 0.f ? prm.nu : prm.rho;
    float *x[kMaxGroup], *b[kMaxGroup], *w0x[kMaxGroup], *w0y[kMaxGroup], *q[kMaxGroup], *c[kMaxGroup];
    const float *xc[kMaxGroup], *cc[kMaxGroup], *qc[kMaxGroup];
    for (int k = 0; k < n; ++k) {
        x[k] = p->tv.x + k * step; b[k] = p->tv.b + k * step; w0x[k] = p->tv.w[0][0] + k * step; w0y[k] = p->tv.w[0][1] + k * step;
        q[k] = p->tvfree.q + k * P; c[k] = p->tvfree.c + k * P;
        xc[k] = x[k]; cc[k] = c[k]; qc[k] = q[k];
    }
    int rc = FDR_OK;
    // T is the periodic call's table for mu = nu: the cache says so, and a periodic call with another mu builds its own again
    if (iters > 0) rc = tv_solve_table(p, kTfPasses, nu, prm.rho, s);
    if (rc != FDR_OK) return rc;
    {
        ScopedPass t(p, s, kPassTfInit);
        FDR_HIP(launch_tv_init_n(n, d_imgs, rows, cols, stride, x, w0x, w0y, M, N, s));
        if (iters > 0) FDR_HIP(hipMemsetAsync(p->tvfree.q, 0, (size_t)n * P * sizeof(float), s));  // the group's q planes lie together
    }
    for (int it = 0; it < iters && rc == FDR_OK; ++it) {
        rc = blur_window_dev_n(p, ws, n, xc, M, N, N, c, N, 0, s, M, N);  // c = blur(x)
        if (rc != FDR_OK) break;
        switch (data.kind) {  // the data step: c becomes r
        case TvDataStep::AUTO: {  // the weight of this step from the discrepancy of e = c + q, image by image, then the step with it
            {
                ScopedPass t(p, s, kPassTaNorm);
                double* tr[kMaxGroup];
                for (int k = 0; k < n; ++k) tr[k] = data.trace[k] ? data.trace[k] + 3 * (size_t)it : nullptr;
                FDR_HIP(launch_tvauto_norm_n(n, cc, qc, d_imgs, stride, d_w, wstride, rows, cols, M, N, p->tvauto.part, s));
                FDR_HIP(launch_tvauto_mu_n(n, p->tvauto.part, tvauto_partials(rows, cols), data.sigma, data.tau, nu, p->tvauto.mu, p->tvauto.stat, tr, s));
            }
            ScopedPass t(p, s, kPassTaData);
            FDR_HIP(launch_tvauto_data_n(n, c, q, d_imgs, stride, d_w, wstride, rows, cols, M, N, p->tvauto.mu, nu, s));
            break;
        }
        case TvDataStep::POISSON: {  // the Poisson likelihood: another step on the same window, planes and bytes
            ScopedPass t(p, s, kPassTpData);
            FDR_HIP(launch_tvpoisson_data_n(n, c, q, d_imgs, stride, d_w, wstride, rows, cols, M, N, prm.mu, nu, data.background, s));
            break;
        }
        case TvDataStep::LEAST_SQUARES: {
            ScopedPass t(p, s, kPassTfData);
            FDR_HIP(launch_tvfree_data_n(n, c, q, d_imgs, stride, d_w, wstride, rows, cols, M, N, prm.mu, nu, s));
            break;
        }
        }
        rc = blur_window_dev_n(p, ws, n, cc, M, N, N, b, N, 1, s, M, N);  // b = blur^T(r)
        if (rc == FDR_OK) rc = tv_prior_half_step(p, kTfPasses, ws, n, it, nu, prm.rho, prm.anisotropic, coupled, s);
    }
    if (rc != FDR_OK) return rc;
    return tv_output_tail(p, fn, kTfPasses, ws, n, d_outs, prm.out_rows, prm.out_cols, out_stride, prm.nonneg, prm.norm_area, s);
}

int tvfree_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* d_out,
                    int out_stride, const fdr_tv_free_params& prm, hipStream_t s, const TvDataStep& data) {
    fdr_plan::Slot* w = &p->slots[0];
    return tvfree_group_dev(p, fn, &w, 1, &d_img, rows, cols, stride, d_w, wstride, &d_out, out_stride, prm, false, s, data);
}

// the first free-boundary TV call of a plan, or the first on a larger group
int ensure_tvfree_workspace(fdr_plan* p, const char* fn, int group) {
    return ensure_workspace(p->tvfree.ws, fn, "free-boundary TV workspace", group,
                            [p](auto& c, int g) { layout(c, p->tvfree, (size_t)p->M * p->N, g); });
}

}  // namespace fdr

extern "C" {

int fdr_tv_deconv_free_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                               float* d_out, int out_stride, const fdr_tv_free_params* params, void* stream) {
    const char* fn = "fdr_tv_deconv_free_f32_dev";
    if (!p || !d_img || !d_out) return null_arg(fn);
    int rc = tvfree_check(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = tvfree_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    return tvfree_dev_impl(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_out, out_stride, *params, (hipStream_t)stream);
}

int fdr_tv_deconv_free_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                           float* out_host, int out_stride, const fdr_tv_free_params* params) {
    const char* fn = "fdr_tv_deconv_free_f32";
    if (!p || !img_host || !out_host) return null_arg(fn);
    int rc = tvfree_check(p, fn, img_host, rows, cols, stride, weights_host, wstride, out_host, out_stride, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = tvfree_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    const fdr_tv_free_params prm = *params;
    DeviceBuffer d_w;  // the weights, dense, for this call alone
    rc = stage_crop_weights(fn, weights_host, rows, cols, wstride, &d_w);
    if (rc != FDR_OK) return rc;
    return host_image_call(p, fn, img_host, rows, cols, stride, out_host, prm.out_rows, prm.out_cols, out_stride,
                           [&](const float* d_in, float* d_out) {
                               return tvfree_dev_impl(p, fn, d_in, rows, cols, cols, d_w.as<float>(), cols, d_out, prm.out_cols, prm, nullptr);
                           });
}

}  // extern "C"
