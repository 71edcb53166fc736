// fdr_api_tvframes.hip -- multi-frame TV deconvolution (fdr_tv_deconv_frames_f32*; the table kernel in fdr_tvframes.hip, the
// per-image weights mode of the data step in fdr_tvfree.hip): the K exposures of fdr_set_frame_psfs* under one TV prior, by the
// free-boundary ADMM iteration of fdr_api_tvfree.hip with one splitting s_k = blur_k(x) per frame.  Everything is an existing stage:
// the frames run in launch groups of the plan's `group` as in fdr_api_frames.hip -- pass A and pass C on the group, pass B' frame
// by frame on H_k, the data step of the group's windows in one launch, then pass A, pass B' on conj(H_k) and the sum kernel, which
// adds the frames' spectra into ONE accumulator so that one inverse row pass gives b = sum_k blur_k^T(r_k) -- and the prior half-step
// and the output tail of fdr_api_tv.hip run once, on the one x and the one pair of duals of the TV workspace.  New are the table
// T = (1 / (M N)) / (nu sum_k |H_k|^2 + rho L) and the workspace of K planes q, K planes c / r and the accumulator.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id; every other pass runs under the name it has elsewhere
const char* const kPassTmTable = "TV table: 1/(nu sum|H_k|^2+rho L)/MN (frames)";

struct TvFramesArgs {
    const float* imgs; size_t img_pitch; int count, rows, cols, stride;
    const float* weights; size_t weight_pitch; int wstride;
    float* out; int out_stride;
};

fdr_tv_free_params free_params(const fdr_tv_frames_params& q) {
    return fdr_tv_free_params{q.mu, q.rho, q.nu, q.iterations, q.anisotropic, q.nonneg, q.norm_area, q.out_rows, q.out_cols};
}

// everything the call refuses, before any device work
int tvframes_check(const fdr_plan* p, const char* fn, const TvFramesArgs& a, const fdr_tv_frames_params* prm) {
    if (!p || !a.imgs || !a.out || !prm) return null_arg(fn);
    if (a.count < 1 || a.count > FDR_MAX_FRAMES) return fail(FDR_ERR_ARG, std::string(fn) + ": count must lie in 1 .. FDR_MAX_FRAMES");
    const fdr_tv_free_params f = free_params(*prm);
    const int rc = tvfree_check(p, fn, a.imgs, a.rows, a.cols, a.stride, a.weights, a.wstride, a.out, a.out_stride, &f, NEED_OPERATOR);
    if (rc != FDR_OK) return rc;
    if (prm->data_term != FDR_TV_FRAMES_LEAST_SQUARES && prm->data_term != FDR_TV_FRAMES_POISSON)
        return fail(FDR_ERR_ARG, std::string(fn) + ": unknown data_term");
    if (!std::isfinite(prm->background) || prm->background < 0.f) return fail(FDR_ERR_ARG, std::string(fn) + ": background must be finite and >= 0");
    if (prm->data_term == FDR_TV_FRAMES_LEAST_SQUARES && prm->background != 0.f)
        return fail(FDR_ERR_ARG, std::string(fn) + ": background must be 0 with the least-squares data term");
    if (p->frames.count == 0) return fail(FDR_ERR_STATE, std::string(fn) + ": no frame PSFs set on this plan (call fdr_set_frame_psfs* first)");
    if (a.count != p->frames.count) return fail(FDR_ERR_ARG, std::string(fn) + ": count is not the number of frame PSFs set (fdr_frame_count)");
    if (a.count > 1 && a.img_pitch < window_span(a.rows, a.cols, a.stride)) return fail(FDR_ERR_ARG, std::string(fn) + ": the frames overlap each other (img_pitch)");
    if (a.weights && a.weight_pitch != 0 && a.weight_pitch < window_span(a.rows, a.cols, a.wstride))
        return fail(FDR_ERR_ARG, std::string(fn) + ": weight_pitch must be 0 (one plane for all frames) or at least a window's span");
    const ByteRange o = window_range(a.out, prm->out_rows, prm->out_cols, a.out_stride);
    if (ranges_overlap(window_range(a.imgs, a.rows, a.cols, a.stride, a.count, a.img_pitch), o))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps a frame");
    if (a.weights && ranges_overlap(window_range(a.weights, a.rows, a.cols, a.wstride, a.weight_pitch ? a.count : 1, a.weight_pitch), o))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the weights");
    return FDR_OK;
}

// the workspace for `count` frames
int ensure_tvframes_workspace(fdr_plan* p, const char* fn, int count) {
    return ensure_workspace(p->tvframes.ws, fn, "multi-frame TV workspace", count,
                            [p](auto& c, int n) { layout(c, p->tvframes, (size_t)p->M * p->N, p->ws_elems, n); });
}

// the new block first (nothing old is let go before it is had), then the TV workspace of one image and the Laplacian table
int tvframes_prepare(fdr_plan* p, const char* fn, int count) {
    int rc = ensure_tvframes_workspace(p, fn, count);
    if (rc == FDR_OK) rc = tv_prepare(p, fn, 1);
    return rc;
}

// T from the K frame tables for nu and rho, unless the plan holds it for this frame set already
int tvframes_table(fdr_plan* p, int count, float nu, float rho, hipStream_t s) {
    if (p->tv.fr_gen != 0 && p->tv.fr_gen == p->frames.gen && p->tv.mu == nu && p->tv.rho == rho) return FDR_OK;
    ScopedPass t(p, s, kPassTmTable);
    FrameTables tabs{};
    for (int k = 0; k < count; ++k) tabs.p[k] = frame_table(p, k, false);
    FDR_HIP(launch_tv_frames_table(tabs, count, p->tv.T, p->lap, p->M, p->N, p->pstride, p->npanels, (double)nu, (double)rho, s));
    p->tv.gen = 0; p->tv.fr_gen = p->frames.gen; p->tv.mu = nu; p->tv.rho = rho;  // (tv.gen 0: the operator's calls build theirs again)
    return FDR_OK;
}

// The restoration on checked device arguments with its workspaces.  x, b, the duals and rhs (slot 0's raw plane) are the TV
// workspace's planes of image 0; q_k and c_k / r_k are full M x N planes of the frames' workspace; every d_k and weights window is
// read from the caller's windows by every data step.
int tvframes_dev(fdr_plan* p, const char* fn, const TvFramesArgs& a, const fdr_tv_frames_params& prm, hipStream_t s) {
    const int M = p->M, N = p->N, rows = a.rows, cols = a.cols, count = a.count, iters = prm.iterations;
    const size_t P = (size_t)M * N;
    const float nu = prm.nu > 0.f ? prm.nu : prm.rho;
    if (count > p->tvframes.ws.count || p->tv.ws.count < 1) return fail(FDR_ERR_STATE, std::string(fn) + ": the multi-frame TV workspaces do not hold the frames");
    TvPassNames names = kTfPasses;
    names.table = kPassTmTable;
    fdr_plan::Slot* w0 = &p->slots[0];
    int rc = FDR_OK;
    if (iters > 0) rc = tvframes_table(p, count, nu, prm.rho, s);
    if (rc != FDR_OK) return rc;
    {
        ScopedPass t(p, s, kPassTfInit);
        const float* d0 = a.imgs;
        FDR_HIP(launch_tv_init_n(1, &d0, rows, cols, a.stride, &p->tv.x, &p->tv.w[0][0], &p->tv.w[0][1], M, N, s));
        if (iters > 0) FDR_HIP(hipMemsetAsync(p->tvframes.q, 0, (size_t)count * P * sizeof(float), s));  // the frames' q planes lie together
    }
    const int group = launch_group(p, count);
    for (int it = 0; it < iters && rc == FDR_OK; ++it) {
        for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
            const int n = group < count - i0 ? group : count - i0;
            fdr_plan::Slot* ws[kMaxGroup];
            const float *xs[kMaxGroup], *ds[kMaxGroup], *cc[kMaxGroup], *wk[kMaxGroup];
            float *c[kMaxGroup], *q[kMaxGroup];
            for (int k = 0; k < n; ++k) {
                ws[k] = &p->slots[k]; xs[k] = p->tv.x; ds[k] = a.imgs + (size_t)(i0 + k) * a.img_pitch;
                c[k] = p->tvframes.c + (size_t)(i0 + k) * P; q[k] = p->tvframes.q + (size_t)(i0 + k) * P; cc[k] = c[k];
                wk[k] = a.weights ? a.weights + (size_t)(i0 + k) * a.weight_pitch : nullptr;
            }
            rc = op_rows_fwd_n(p, ws, n, xs, M, N, N, s);                                         // c_k = blur_k(x) ...
            if (rc == FDR_OK) rc = frames_cols(p, ws, n, i0, false, s);
            if (rc == FDR_OK) rc = op_rows_inv_n(p, ws, n, ROW_OUT_BLUR, kPassFrBlur, nullptr, 0, nullptr, c, N, M, N, s);
            if (rc != FDR_OK) break;
            {   // ... the data step of the group's windows: c_k becomes r_k
                const bool poisson = prm.data_term == FDR_TV_FRAMES_POISSON;
                const bool own = a.weights && a.weight_pitch != 0;  // a weights window per frame
                ScopedPass t(p, s, poisson ? kPassTpData : kPassTfData);
                if (poisson && own)
                    FDR_HIP(launch_tvpoisson_data_weights_n(n, c, q, ds, a.stride, wk, a.wstride, rows, cols, M, N, prm.mu, nu, prm.background, s));
                else if (poisson)
                    FDR_HIP(launch_tvpoisson_data_n(n, c, q, ds, a.stride, a.weights, a.wstride, rows, cols, M, N, prm.mu, nu, prm.background, s));
                else if (own)
                    FDR_HIP(launch_tvfree_data_weights_n(n, c, q, ds, a.stride, wk, a.wstride, rows, cols, M, N, prm.mu, nu, s));
                else
                    FDR_HIP(launch_tvfree_data_n(n, c, q, ds, a.stride, a.weights, a.wstride, rows, cols, M, N, prm.mu, nu, s));
            }
            rc = op_rows_fwd_n(p, ws, n, cc, M, N, N, s);                                         // ... b = sum_k blur_k^T(r_k)
            if (rc == FDR_OK) rc = frames_cols(p, ws, n, i0, true, s);
            if (rc == FDR_OK) rc = frames_sum(p, p->tvframes.acc, ws, n, i0 == 0, s);
        }
        if (rc == FDR_OK) rc = frames_rows_inv(p, p->tvframes.acc, ROW_OUT_BLUR, kPassFrBlur, nullptr, 0, nullptr, p->tv.b, N, M, N, s);
        if (rc == FDR_OK) rc = tv_prior_half_step(p, names, &w0, 1, it, nu, prm.rho, prm.anisotropic, false, s);
    }
    if (rc != FDR_OK) return rc;
    float* out = a.out;
    return tv_output_tail(p, fn, names, &w0, 1, &out, prm.out_rows, prm.out_cols, a.out_stride, prm.nonneg, prm.norm_area, s);
}

}  // namespace

extern "C" {

int fdr_tv_deconv_frames_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                 const float* d_weights, size_t weight_pitch, int wstride, float* d_out, int out_stride,
                                 const fdr_tv_frames_params* params) {
    const char* fn = "fdr_tv_deconv_frames_f32_dev";
    const TvFramesArgs a{d_imgs, img_pitch, count, rows, cols, stride, d_weights, weight_pitch, wstride, d_out, out_stride};
    int rc = tvframes_check(p, fn, a, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = tvframes_prepare(p, fn, count);
    if (rc != FDR_OK) return rc;
    return tvframes_dev(p, fn, a, *params, (hipStream_t)params->stream);
}

// host pointers: every frame and weights plane in (dense), the call on the null stream, the result back; one-shot device buffers
int fdr_tv_deconv_frames_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                             const float* weights_host, size_t weight_pitch, int wstride, float* out_host, int out_stride,
                             const fdr_tv_frames_params* params) {
    const char* fn = "fdr_tv_deconv_frames_f32";
    const TvFramesArgs h{imgs_host, img_pitch, count, rows, cols, stride, weights_host, weight_pitch, wstride, out_host, out_stride};
    int rc = tvframes_check(p, fn, h, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const fdr_tv_frames_params prm = *params;
    rc = tvframes_prepare(p, fn, count);
    if (rc != FDR_OK) return rc;
    const size_t in_px = (size_t)rows * cols, out_px = (size_t)prm.out_rows * prm.out_cols;
    const int nw = !weights_host ? 0 : weight_pitch ? count : 1;
    DeviceBuffer d_in, d_out, d_w;
    FDR_ALLOC(d_in, (size_t)count * in_px * sizeof(float), fn);
    FDR_ALLOC(d_out, out_px * sizeof(float), fn);
    if (nw) FDR_ALLOC(d_w, (size_t)nw * in_px * sizeof(float), fn);
    {
        ScopedPhase phase(p, FDR_PHASE_H2D, nullptr);
        for (int k = 0; k < count; ++k)
            FDR_HIP(hipMemcpy2D(d_in.as<float>() + (size_t)k * in_px, (size_t)cols * sizeof(float), imgs_host + (size_t)k * img_pitch,
                                (size_t)stride * sizeof(float), (size_t)cols * sizeof(float), (size_t)rows, hipMemcpyHostToDevice));
        for (int k = 0; k < nw; ++k)
            FDR_HIP(hipMemcpy2D(d_w.as<float>() + (size_t)k * in_px, (size_t)cols * sizeof(float), weights_host + (size_t)k * weight_pitch,
                                (size_t)wstride * sizeof(float), (size_t)cols * sizeof(float), (size_t)rows, hipMemcpyHostToDevice));
    }
    {
        ScopedPhase phase(p, FDR_PHASE_COMPUTE, nullptr);
        const TvFramesArgs a{d_in.as<float>(), in_px, count, rows, cols, cols, d_w.as<float>(), nw > 1 ? in_px : 0, cols, d_out.as<float>(), prm.out_cols};
        rc = tvframes_dev(p, fn, a, prm, nullptr);
    }
    if (rc == FDR_OK) {
        ScopedPhase phase(p, FDR_PHASE_D2H, nullptr);
        FDR_HIP(hipMemcpy2D(out_host, (size_t)out_stride * sizeof(float), d_out.as<float>(), (size_t)prm.out_cols * sizeof(float),
                            (size_t)prm.out_cols * sizeof(float), (size_t)prm.out_rows, hipMemcpyDeviceToHost));
    }
    (void)hipStreamSynchronize(nullptr);  // (also on an error: the one-shot buffers are freed on return)
    resolve_phases(p);
    return rc;
}

}  // extern "C"
