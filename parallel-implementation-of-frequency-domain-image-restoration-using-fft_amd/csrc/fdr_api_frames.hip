// fdr_api_frames.hip -- multi-frame Richardson-Lucy (fdr_set_frame_psfs*, fdr_frame_count, fdr_spectrum_sum_f32_dev,
// fdr_blur_frames_f32_dev, fdr_richardson_lucy_frames_f32*; the kernels in fdr_frames.hip): K exposures of one scene, one PSF each,
// restored jointly on the free-boundary, weighted form.  The frame tables are a plan member of their own; every transform is an
// operator pass of fdr_api_operator.hip, run on launch groups of the plan's `group` frames: pass A and pass C on the group, pass B'
// frame by frame (each frame has its own table), and on the adjoint side the sum kernel, which adds the frames' spectra into ONE
// accumulator spectrum so that one inverse row pass serves all K.  The setup, start, crop and normalisation are the free form's, the
// prior's factor is fdr_api_rltv.hip's.
#include "fdr_host.hpp"

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassFrSetup = "RLM setup: dw_k, W_k, sums";
const char* const kPassFrStart = "RLM start: fold, wgt = 1/alpha, u";
const char* const kPassFrColsH = "B' op cols: FFT*H_k*IFFT (frame)";
const char* const kPassFrColsConj = "B' op cols: FFT*conj(H_k)*IFFT (frame)";
const char* const kPassFrSum = "S frames: sum of spectra";
const char* const kPassFrRatio = "C op rows: IFFT+RL ratio (frames)";
const char* const kPassFrUpdate = "C op rows: IFFT+RL update (frames)";

size_t frames_part_set(const fdr_plan* p) { return 2 * (size_t)rlfree_partials(p->M, p->N) + 2; }

// the workspace for `count` frames
int ensure_frames_workspace(fdr_plan* p, const char* fn, int count) {
    return ensure_workspace(p->frames.ws, fn, "frames workspace", count,
                            [p](auto& c, int n) { layout(c, p->frames, (size_t)p->M * p->N, p->ws_elems, frames_part_set(p), n); });
}

}  // namespace

namespace fdr {

const char* const kPassFrBlur = "C op rows: IFFT+crop (frames)";

const float2* frame_table(const fdr_plan* p, int k, bool adjoint) { return p->frames.tables + (2 * (size_t)k + (adjoint ? 1 : 0)) * p->ws_elems; }

// the frames i0 .. i0 + n - 1 on the slots ws[0 .. n): pass B' of each on its own table, then their spectra into the accumulator
// (`first`: stored, else added to what it holds)
int frames_cols(fdr_plan* p, fdr_plan::Slot* const* ws, int n, int i0, bool adjoint, hipStream_t s) {
    int rc = FDR_OK;
    for (int k = 0; k < n && rc == FDR_OK; ++k)
        rc = op_cols_table_n(p, &ws[k], 1, frame_table(p, i0 + k, adjoint), adjoint ? kPassFrColsConj : kPassFrColsH, s);
    return rc;
}
int frames_sum(fdr_plan* p, float2* acc, fdr_plan::Slot* const* ws, int n, bool first, hipStream_t s) {
    ScopedPass t(p, s, kPassFrSum);
    FrameSrcs srcs{};
    for (int k = 0; k < n; ++k) srcs.p[k] = reinterpret_cast<const float*>(ws[k]->work);
    FDR_HIP(launch_frames_sum(reinterpret_cast<float*>(acc), srcs, n, 2 * p->ws_elems, !first, s));
    return FDR_OK;
}
// pass C of the accumulator: a Slot value whose spectrum is `acc`
int frames_rows_inv(fdr_plan* p, float2* acc, RowOut kind, const char* name, const float* src, int src_stride, const float* src2, float* out,
                    int out_stride, int rows, int cols, hipStream_t s) {
    fdr_plan::Slot a = p->slots[0];
    a.work = acc;
    fdr_plan::Slot* w = &a;
    return op_rows_inv_n(p, &w, 1, kind, name, &src, src_stride, src2, &out, out_stride, rows, cols, s);
}

}  // namespace fdr

namespace {

// sum_k blur_k^T(y_k) of `count` windows (rows x cols, row stride `stride`, frame k's at ys + k pitch) -> the window out_rows x
// out_cols at d_out.  `prepare(k, slot)`, when set, produces frame k's window dense in the slot's raw plane first (the setup of the
// restoration); the windows are then read there.
int frames_adjoint(fdr_plan* p, const float* ys, size_t pitch, int count, int rows, int cols, int stride, float* d_out, int out_stride, int out_rows,
                   int out_cols, hipStream_t s, const std::function<int(int, fdr_plan::Slot*)>& prepare = nullptr) {
    const int group = launch_group(p, count);
    int rc = FDR_OK;
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const int n = group < count - i0 ? group : count - i0;
        fdr_plan::Slot* ws[kMaxGroup];
        const float* xs[kMaxGroup];
        for (int k = 0; k < n && rc == FDR_OK; ++k) {
            ws[k] = &p->slots[k];
            if (prepare) { rc = prepare(i0 + k, ws[k]); xs[k] = ws[k]->raw; }
            else xs[k] = ys + (size_t)(i0 + k) * pitch;
        }
        if (rc == FDR_OK) rc = op_rows_fwd_n(p, ws, n, xs, rows, cols, prepare ? cols : stride, s);
        if (rc == FDR_OK) rc = frames_cols(p, ws, n, i0, true, s);
        if (rc == FDR_OK) rc = frames_sum(p, p->frames.acc, ws, n, i0 == 0, s);
    }
    if (rc == FDR_OK) rc = frames_rows_inv(p, p->frames.acc, ROW_OUT_BLUR, kPassFrBlur, nullptr, 0, nullptr, d_out, out_stride, out_rows, out_cols, s);
    return rc;
}

struct FramesArgs {
    const float* imgs; size_t img_pitch; int count, rows, cols, stride;
    const float* weights; size_t weight_pitch; int wstride;
    float* out; int out_stride;
};

fdr_rlfree_params free_params(const fdr_rl_frames_params& prm) {
    return fdr_rlfree_params{prm.iterations, prm.sigma, prm.norm_area, prm.out_rows, prm.out_cols};
}

// everything the restoration refuses, before any device work
int frames_check(const fdr_plan* p, const char* fn, const FramesArgs& a, const fdr_rl_frames_params* prm) {
    if (!p || !a.imgs || !a.out || !prm) return null_arg(fn);
    if (a.count < 1 || a.count > FDR_MAX_FRAMES) return fail(FDR_ERR_ARG, std::string(fn) + ": count must lie in 1 .. FDR_MAX_FRAMES");
    const fdr_rlfree_params f = free_params(*prm);
    int rc = rlfree_check(p, fn, a.imgs, a.rows, a.cols, a.stride, a.weights, a.wstride, a.out, a.out_stride, &f, NEED_OPERATOR);
    if (rc != FDR_OK) return rc;
    if (p->frames.count == 0) return fail(FDR_ERR_STATE, std::string(fn) + ": no frame PSFs set on this plan (call fdr_set_frame_psfs* first)");
    if (a.count != p->frames.count) return fail(FDR_ERR_ARG, std::string(fn) + ": count is not the number of frame PSFs set (fdr_frame_count)");
    rc = prior_check(fn, prm->tv_lambda, prm->tv_eps);
    if (rc != FDR_OK) return rc;
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

int ensure_frames_call(fdr_plan* p, const char* fn, int count, const fdr_rl_frames_params& prm) {
    int rc = ensure_frames_workspace(p, fn, count);
    if (rc == FDR_OK && prm.tv_lambda != 0.f) rc = ensure_rltv_workspace(p, fn);
    return rc;
}

// The restoration on checked device arguments with its workspaces.  u, wgt dense M x N; dw_k dense rows x cols; r_k in slot k's raw
// plane; W_k = pad(m_k) passes through slot k's raw plane on its way into alpha.
int frames_rl_dev(fdr_plan* p, const char* fn, const FramesArgs& a, const fdr_rl_frames_params& prm, hipStream_t s) {
    const int M = p->M, N = p->N, rows = a.rows, cols = a.cols, count = a.count;
    const size_t P = (size_t)M * N;
    const size_t set = frames_part_set(p);
    // dw_k, W_k and their sums per frame, alpha = sum_k fullblur_k^T(W_k) over the whole plan
    int rc = frames_adjoint(p, nullptr, 0, count, rows, cols, cols, p->frames.wgt, N, M, N, s, [&](int k, fdr_plan::Slot* w) {
        ScopedPass t(p, s, kPassFrSetup);
        const float* m = a.weights ? a.weights + (size_t)k * a.weight_pitch : nullptr;
        FDR_HIP(launch_rlfree_setup(a.imgs + (size_t)k * a.img_pitch, a.stride, m, a.wstride, rows, cols, p->frames.dw + (size_t)k * P, w->raw,
                                    p->frames.part + (size_t)k * set, s));
        return FDR_OK;
    });
    if (rc != FDR_OK) return rc;
    {   // the K pairs (sum dw_k, sum W_k) folded in ascending k on the device, then the start of the free form on the folded pair
        ScopedPass t(p, s, kPassFrStart);
        FDR_HIP(launch_frames_fold(p->frames.part + 2 * (size_t)rlfree_partials(rows, cols), set, count, p->frames.sums, s));
        FDR_HIP(launch_rlfree_start(p->frames.wgt, p->frames.u, P, prm.sigma * (float)count, p->frames.sums, s));
    }
    const float eps = prm.tv_eps == 0.f ? FDR_RLTV_EPS : prm.tv_eps;
    const int group = launch_group(p, count);
    for (int it = 0; it < prm.iterations && rc == FDR_OK; ++it) {
        const float* wgt = p->frames.wgt;
        if (prm.tv_lambda != 0.f) {  // factor = wgt / g from the u that enters the step, in wgt's place
            rc = rltv_factor(p, p->frames.u, M, N, N, p->frames.wgt, prm.tv_lambda, eps, s);
            wgt = p->rltv.f;
        }
        for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
            const int n = group < count - i0 ? group : count - i0;
            fdr_plan::Slot* ws[kMaxGroup];
            const float *us[kMaxGroup], *dws[kMaxGroup];
            float* r[kMaxGroup];
            for (int k = 0; k < n; ++k) { ws[k] = &p->slots[k]; us[k] = p->frames.u; dws[k] = p->frames.dw + (size_t)(i0 + k) * P; r[k] = ws[k]->raw; }
            rc = op_rows_fwd_n(p, ws, n, us, M, N, N, s);                                        // c_k = window(fullblur_k(u)) ...
            if (rc == FDR_OK) rc = frames_cols(p, ws, n, i0, false, s);
            if (rc == FDR_OK)                                                                    // ... r_k = dw_k / c_k
                rc = op_rows_inv_n(p, ws, n, ROW_OUT_RL_RATIO, kPassFrRatio, dws, cols, nullptr, r, cols, rows, cols, s);
            if (rc == FDR_OK) rc = op_rows_fwd_n(p, ws, n, r, rows, cols, cols, s);               // sum_k fullblur_k^T(pad(r_k)) ...
            if (rc == FDR_OK) rc = frames_cols(p, ws, n, i0, true, s);
            if (rc == FDR_OK) rc = frames_sum(p, p->frames.acc, ws, n, i0 == 0, s);
        }
        if (rc == FDR_OK)                                                                        // ... u = max(u wgt g, 0)
            rc = frames_rows_inv(p, p->frames.acc, ROW_OUT_RL_UPDATE_W, kPassFrUpdate, p->frames.u, N, wgt, p->frames.u, N, M, N, s);
    }
    if (rc != FDR_OK) return rc;
    return rlfree_finish(p, fn, p->frames.u, a.out, a.out_stride, free_params(prm), s);
}

int set_frame_psfs_impl(fdr_plan* p, const char* fn, const float* d_psfs, size_t pitch, int count, int prows, int pcols, int pstride, hipStream_t s) {
    const int rc_tables = ensure_workspace(p->frames.tables_ws, fn, "frame tables", count,
                                           [p](auto& c, int n) { layout(c, p->frames.tables, 2 * (size_t)n * p->ws_elems, 16); });
    if (rc_tables != FDR_OK) return rc_tables;
    p->frames.count = 0;  // (a HIP error below leaves no half-built set behind)
    ++p->frames.gen;      // (the solve table of fdr_tv_deconv_frames_f32*, if tv.T holds it, is of the old set)
    for (int k = 0; k < count; ++k) {
        float2* h = p->frames.tables + 2 * (size_t)k * p->ws_elems;
        const int rc = build_operator_tables(p, d_psfs + (size_t)k * pitch, prows, pcols, pstride, h, h + p->ws_elems, s);
        if (rc != FDR_OK) return rc;
    }
    p->frames.count = count;
    return FDR_OK;
}

// what both setters refuse: the operator setter's checks, the count and the pitch
int frame_psfs_check(const fdr_plan* p, const char* fn, const float* psfs, size_t pitch, int count, int prows, int pcols, int pstride) {
    if (!p || !psfs) return null_arg(fn);
    const int rc = check_plan(p, fn, NEED_OPERATOR);
    if (rc != FDR_OK) return rc;
    if (count < 1 || count > FDR_MAX_FRAMES) return fail(FDR_ERR_ARG, std::string(fn) + ": count must lie in 1 .. FDR_MAX_FRAMES");
    if (prows <= 0 || pcols <= 0 || pstride < pcols) return fail(FDR_ERR_ARG, std::string(fn) + ": bad PSF shape");
    if (prows > p->M || pcols > p->N) return fail(FDR_ERR_ARG, std::string(fn) + ": PSF larger than the plan");
    if (count > 1 && pitch < window_span(prows, pcols, pstride)) return fail(FDR_ERR_ARG, std::string(fn) + ": the PSFs overlap each other (psf_pitch)");
    return FDR_OK;
}

}  // namespace

extern "C" {

int fdr_set_frame_psfs_dev(fdr_plan* p, const float* d_psfs, size_t psf_pitch, int count, int prows, int pcols, int pstride, void* stream) {
    const char* fn = "fdr_set_frame_psfs_dev";
    const int rc = frame_psfs_check(p, fn, d_psfs, psf_pitch, count, prows, pcols, pstride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return set_frame_psfs_impl(p, fn, d_psfs, psf_pitch, count, prows, pcols, pstride, (hipStream_t)stream);
}

// host pointers: the PSFs dense into a one-shot device buffer, the tables on the null stream; ready when the call returns
int fdr_set_frame_psfs(fdr_plan* p, const float* psfs_host, size_t psf_pitch, int count, int prows, int pcols, int pstride) {
    const char* fn = "fdr_set_frame_psfs";
    int rc = frame_psfs_check(p, fn, psfs_host, psf_pitch, count, prows, pcols, pstride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const size_t px = (size_t)prows * pcols;
    DeviceBuffer d;
    FDR_ALLOC(d, (size_t)count * px * sizeof(float), fn);
    {
        ScopedPhase ph(p, FDR_PHASE_H2D, nullptr);
        for (int k = 0; k < count; ++k)
            FDR_HIP(hipMemcpy2D(d.as<float>() + (size_t)k * px, (size_t)pcols * sizeof(float), psfs_host + (size_t)k * psf_pitch,
                                (size_t)pstride * sizeof(float), (size_t)pcols * sizeof(float), (size_t)prows, hipMemcpyHostToDevice));
    }
    rc = set_frame_psfs_impl(p, fn, d.as<float>(), px, count, prows, pcols, pcols, nullptr);
    (void)hipStreamSynchronize(nullptr);  // (also on an error: the one-shot buffer is freed on return)
    resolve_phases(p);
    return rc;
}

int fdr_frame_count(fdr_plan* p, int* count) {
    if (!p || !count) return null_arg("fdr_frame_count");
    *count = p->frames.count;
    return FDR_OK;
}

int fdr_spectrum_sum_f32_dev(int device, float* d_dst, const float* const* d_srcs, int n, size_t n_floats, int accumulate, void* stream) {
    const char* fn = "fdr_spectrum_sum_f32_dev";
    if (!d_dst || !d_srcs) return null_arg(fn);
    if (n < 1 || n > kMaxGroup) return fail(FDR_ERR_ARG, std::string(fn) + ": n must lie in 1 .. 8");
    if (n_floats < 2 || (n_floats & 1) != 0) return fail(FDR_ERR_ARG, std::string(fn) + ": n_floats must be even and >= 2");
    if (((uintptr_t)d_dst & 15) != 0) return fail(FDR_ERR_ARG, std::string(fn) + ": every pointer must be 16-byte aligned");
    const ByteRange o = byte_range(d_dst, n_floats * sizeof(float));
    FrameSrcs srcs{};
    for (int k = 0; k < n; ++k) {
        if (!d_srcs[k]) return null_arg(fn);
        if (((uintptr_t)d_srcs[k] & 15) != 0) return fail(FDR_ERR_ARG, std::string(fn) + ": every pointer must be 16-byte aligned");
        if (d_srcs[k] != d_dst && ranges_overlap(byte_range(d_srcs[k], n_floats * sizeof(float)), o))
            return fail(FDR_ERR_ARG, std::string(fn) + ": dst overlaps a source that is not dst itself");
        srcs.p[k] = d_srcs[k];
    }
    FDR_HIP(hipSetDevice(device));
    FDR_HIP(launch_frames_sum(d_dst, srcs, n, n_floats, accumulate != 0, (hipStream_t)stream));
    return FDR_OK;
}

int fdr_blur_frames_f32_dev(fdr_plan* p, const float* d_in, size_t in_pitch, int rows, int cols, int stride, float* d_out, size_t out_pitch,
                            int out_stride, int count, int adjoint, void* stream) {
    const char* fn = "fdr_blur_frames_f32_dev";
    if (!p || !d_in || !d_out) return null_arg(fn);
    int rc = check_window(p, fn, NEED_OPERATOR, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    if (p->frames.count == 0) return fail(FDR_ERR_STATE, std::string(fn) + ": no frame PSFs set on this plan (call fdr_set_frame_psfs* first)");
    if (count != p->frames.count) return fail(FDR_ERR_ARG, std::string(fn) + ": count is not the number of frame PSFs set (fdr_frame_count)");
    if (count > 1 && (adjoint ? in_pitch < window_span(rows, cols, stride) : out_pitch < window_span(rows, cols, out_stride)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the frames' windows overlap each other (pitch)");
    if (ranges_overlap(window_range(d_in, rows, cols, stride, adjoint ? count : 1, in_pitch),
                       window_range(d_out, rows, cols, out_stride, adjoint ? 1 : count, out_pitch)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the input");  // (a later launch group still reads what an earlier one wrote)
    FDR_HIP(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    if (adjoint) {
        rc = ensure_frames_workspace(p, fn, 1);
        if (rc != FDR_OK) return rc;
        return frames_adjoint(p, d_in, in_pitch, count, rows, cols, stride, d_out, out_stride, rows, cols, s);
    }
    const int group = launch_group(p, count);
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const int n = group < count - i0 ? group : count - i0;
        fdr_plan::Slot* ws[kMaxGroup];
        const float* xs[kMaxGroup];
        float* outs[kMaxGroup];
        for (int k = 0; k < n; ++k) { ws[k] = &p->slots[k]; xs[k] = d_in; outs[k] = d_out + (size_t)(i0 + k) * out_pitch; }
        rc = op_rows_fwd_n(p, ws, n, xs, rows, cols, stride, s);
        if (rc == FDR_OK) rc = frames_cols(p, ws, n, i0, false, s);
        if (rc == FDR_OK) rc = op_rows_inv_n(p, ws, n, ROW_OUT_BLUR, kPassFrBlur, nullptr, 0, nullptr, outs, out_stride, rows, cols, s);
    }
    return rc;
}

int fdr_richardson_lucy_frames_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                       const float* d_weights, size_t weight_pitch, int wstride, float* d_out, int out_stride,
                                       const fdr_rl_frames_params* params, void* stream) {
    const char* fn = "fdr_richardson_lucy_frames_f32_dev";
    const FramesArgs a{d_imgs, img_pitch, count, rows, cols, stride, d_weights, weight_pitch, wstride, d_out, out_stride};
    int rc = frames_check(p, fn, a, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = ensure_frames_call(p, fn, count, *params);
    if (rc != FDR_OK) return rc;
    return frames_rl_dev(p, fn, a, *params, (hipStream_t)stream);
}

// host pointers: every frame and weights plane in (dense), the call on the null stream, the result back; one-shot device buffers
int fdr_richardson_lucy_frames_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                                   const float* weights_host, size_t weight_pitch, int wstride, float* out_host, int out_stride,
                                   const fdr_rl_frames_params* params) {
    const char* fn = "fdr_richardson_lucy_frames_f32";
    const FramesArgs h{imgs_host, img_pitch, count, rows, cols, stride, weights_host, weight_pitch, wstride, out_host, out_stride};
    int rc = frames_check(p, fn, h, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const fdr_rl_frames_params prm = *params;
    rc = ensure_frames_call(p, fn, count, prm);
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
        const FramesArgs a{d_in.as<float>(), in_px, count, rows, cols, cols, d_w.as<float>(), nw > 1 ? in_px : 0, cols, d_out.as<float>(), prm.out_cols};
        rc = frames_rl_dev(p, fn, a, prm, nullptr);
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
