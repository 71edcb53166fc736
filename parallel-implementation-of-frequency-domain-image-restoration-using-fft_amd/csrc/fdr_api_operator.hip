// fdr_api_operator.hip -- the blur operator: passes A, B' and C of the fast half-spectrum path with the operator tables in place of
// W and the operator kinds of the inverse row pass, for a group of images; the PSF setters, the min-max normalisation of a window
// and the entry points of the blur.  Richardson-Lucy on these passes: fdr_api_rl.hip (plain form), fdr_api_rlfree.hip.
#include "fdr_host.hpp"

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassOpRowsPsf = "O rows: PSF pad+FFT (operator)";
const char* const kPassOpCols = "O cols: FFT -> H/MN, conj(H)/MN";
const char* const kPassOpRowsFwd = "A op rows: pad+FFT (blur / RL)";
const char* const kPassOpRowsFwdN = "A op rows: pad+FFT (blur / RL), group";
const char* const kPassOpColsH = "B' op cols: FFT*H*IFFT";
const char* const kPassOpColsConj = "B' op cols: FFT*conj(H)*IFFT";
const char* const kPassOpRowsBlur = "C op rows: IFFT+crop (blur)";

}  // namespace

namespace fdr {

// the PSF top-left in the M x N plane -> its row spectra (the rows it reaches) -> H / (M N) into h, conj(H) / (M N) into c
int build_operator_tables(fdr_plan* p, const float* d_psf, int prows, int pcols, int pstride, float2* h, float2* c, hipStream_t s) {
    ScopedPhase phase(p, FDR_PHASE_PRE, s);
    const int nvalid = (prows + 3) & ~3;  // <= M (M is a multiple of 8 on this path)
    {
        ScopedPass t(p, s, kPassOpRowsPsf);
        RowArgs ra = panel_row_args(p);
        ra.src_real = d_psf; ra.src_rows = prows; ra.src_cols = pcols; ra.src_stride = pstride;
        ra.dst_c = h; ra.M = nvalid;
        FDR_HIP(launch_rows4(p->logN, ROW_IN_REAL, ROW_OUT_COMPLEX, ra, p->tw_row_f, s));
    }
    {
        ScopedPass t(p, s, kPassOpCols);
        ColArgs ca = panel_col_args(p);
        ca.data = h; ca.nvalid = nvalid;
        FDR_HIP(launch_cols_panel_operator(p->logM, ca, c, p->tw_col_f, s));
    }
    return FDR_OK;
}

// the operator setter: the tables on op_h / op_c, made by the first call
int set_operator_psf_impl(fdr_plan* p, const float* d_psf, int prows, int pcols, int pstride, hipStream_t s) {
    if (!p->op_h) {
        float2* t = nullptr;
        if (hipMalloc((void**)&t, 2 * p->ws_elems * sizeof(float2)) != hipSuccess)
            return fail(FDR_ERR_ALLOC, "fdr_set_operator_psf: hipMalloc of the operator tables failed");
        p->op_h = t;
        p->op_c = t + p->ws_elems;
    }
    const int rc = build_operator_tables(p, d_psf, prows, pcols, pstride, p->op_h, p->op_c, s);
    if (rc != FDR_OK) return rc;
    p->have_op = true;
    ++p->op_gen;
    return FDR_OK;
}

// The three operator passes for a group of n >= 1 images on the slots ws[0 .. n), shaped as the panel stages of fdr_api_wiener.hip:
// one image goes by the single-image fields alone (batch.nimg 0: the launchers then pick the split kernels of small images), a
// group of 2 .. kMaxGroup images adds the batch block (blockIdx.y = image).
// pass A: the window of xs[k] (zero elsewhere, whatever the plan's pad mode) -> the half spectrum of slot k
int op_rows_fwd_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float* const* xs, int rows, int cols, int stride, hipStream_t s) {
    ScopedPass t(p, s, n > 1 ? kPassOpRowsFwdN : kPassOpRowsFwd);
    RowArgs a = panel_row_args(p);  // (pad_mode stays FDR_PAD_ZERO)
    a.src_real = xs[0]; a.src_rows = rows; a.src_cols = cols; a.src_stride = stride;
    a.dst_c = ws[0]->work;
    if (n > 1) {
        a.batch.nimg = n;
        for (int k = 0; k < kMaxGroup; ++k) { a.batch.src_real[k] = xs[k < n ? k : 0]; a.batch.spec[k] = ws[k < n ? k : 0]->work; }
    }
    FDR_HIP(launch_rows4(p->logN, ROW_IN_REAL, ROW_OUT_COMPLEX, a, p->tw_row_f, s));
    return FDR_OK;
}
// pass B', unchanged, with `table` as its filter: read once for the group
int op_cols_table_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float2* table, const char* name, hipStream_t s) {
    ScopedPass t(p, s, name);
    ColArgs c = panel_col_args(p);
    c.data = ws[0]->work; c.filt = table;
    c.batch.nimg = n;
    for (int k = 0; k < n; ++k) c.batch.data[k] = ws[k]->work;
    FDR_HIP(launch_cols_panel(p->logM, COL_FUSED, c, p->tw_col_f, s));
    return FDR_OK;
}
// pass C with an operator kind: the window rows x cols of the inverse transform of slot k through the kind's epilogue into outs[k];
// srcs[k] the kind's real source (null for ROW_OUT_BLUR), src2 the second source of ROW_OUT_RL_UPDATE_W: one plane for the group, or
// with src2_pitch image k's own at src2 + k src2_pitch
int op_rows_inv_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, RowOut kind, const char* name, const float* const* srcs, int src_stride,
                  const float* src2, float* const* outs, int out_stride, int rows, int cols, hipStream_t s, const RlFit* fit, size_t src2_pitch) {
    if (fit && n > 1) return fail(FDR_ERR_STATE, "op_rows_inv: the fit sums take one image per launch");
    ScopedPass t(p, s, name);
    RowArgs a = panel_row_args(p);
    a.src_c = ws[0]->work;
    a.src_real = srcs ? srcs[0] : nullptr; a.src_stride = src_stride;
    a.src_real2 = src2;
    a.src2_pitch = n > 1 ? (int)src2_pitch : 0;
    if (fit) {  // ROW_OUT_RL_RATIO_STAT: the weights beside the datum, the (res, kl) partials in the slot of the min/max ones
        a.src_real2 = fit->weights;
        a.mm_part = reinterpret_cast<float2*>(fit->part);
    }
    a.out = outs[0]; a.out_rows = rows; a.out_cols = cols; a.out_stride = out_stride;
    if (n > 1) {
        a.batch.nimg = n;
        for (int k = 0; k < kMaxGroup; ++k) {
            const int j = k < n ? k : 0;
            a.batch.spec[k] = ws[j]->work; a.batch.src_real[k] = srcs ? srcs[j] : nullptr; a.batch.out[k] = outs[j];
        }
    }
    FDR_HIP(launch_rows4(p->logN, ROW_IN_COMPLEX, kind, a, p->tw_row_f, s));
    return FDR_OK;
}

// the single-image forms: a group of one on slot 0
int op_rows_fwd(fdr_plan* p, const float* x, int rows, int cols, int stride, hipStream_t s) {
    fdr_plan::Slot* w = &p->slots[0];
    return op_rows_fwd_n(p, &w, 1, &x, rows, cols, stride, s);
}
int op_cols_table(fdr_plan* p, const float2* table, const char* name, hipStream_t s) {
    fdr_plan::Slot* w = &p->slots[0];
    return op_cols_table_n(p, &w, 1, table, name, s);
}
int op_rows_inv(fdr_plan* p, RowOut kind, const char* name, const float* src, int src_stride, float* out, int out_stride, int rows,
                int cols, hipStream_t s) {
    fdr_plan::Slot* w = &p->slots[0];
    return op_rows_inv_n(p, &w, 1, kind, name, &src, src_stride, nullptr, &out, out_stride, rows, cols, s);
}

// min-max to [0, 1] over the window; FDR_NORM_PADDED also counts the zeros outside it (one extra (0, 0) partial)
int normalize_window(fdr_plan* p, const char* fn, const char* name, const float* fin, int fs, int rows, int cols, int norm_area, float* d_out,
                     int out_stride, hipStream_t s) {
    ScopedPass t(p, s, name);
    const fdr_plan::Slot& w = p->slots[0];
    int n_part = 0;
    FDR_HIP(launch_minmax_real(fin, rows, fs, rows, cols, w.mm_part, &n_part, s));
    if (norm_area == FDR_NORM_PADDED && (rows < p->M || cols < p->N)) {
        if (n_part + 1 > p->mm_part_cap) return fail(FDR_ERR_STATE, std::string(fn) + ": min/max partial count out of range");
        FDR_HIP(hipMemsetAsync(w.mm_part + n_part, 0, sizeof(float2), s));  // (0.f, 0.f)
        ++n_part;
    }
    if (n_part <= 0 || n_part > p->mm_part_cap) return fail(FDR_ERR_STATE, std::string(fn) + ": min/max partial count out of range");
    FDR_HIP(launch_reduce_minmax(w.mm_part, n_part, w.mm, s));
    FDR_HIP(launch_normalize(fin, fs, nullptr, 0, w.mm, d_out, rows, cols, out_stride, s));
    return FDR_OK;
}

// pass B' on one of the operator tables
int op_cols_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, bool adjoint, hipStream_t s) {
    return op_cols_table_n(p, ws, n, adjoint ? p->op_c : p->op_h, adjoint ? kPassOpColsConj : kPassOpColsH, s);
}

// blur (or blur^T) of the window rows x cols of d_img, the window out_rows x out_cols of the result into d_out
int blur_window_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride, int out_rows, int out_cols,
                    int adjoint, hipStream_t s) {
    int rc = op_rows_fwd(p, d_img, rows, cols, stride, s);
    fdr_plan::Slot* w = &p->slots[0];
    if (rc == FDR_OK) rc = op_cols_n(p, &w, 1, adjoint != 0, s);
    if (rc == FDR_OK) rc = op_rows_inv(p, ROW_OUT_BLUR, kPassOpRowsBlur, nullptr, 0, d_out, out_stride, out_rows, out_cols, s);
    return rc;
}

// the same for a group of n images on the slots ws[0 .. n): six launches whatever n (out_rows = out_cols = 0: the window of the input)
int blur_window_dev_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                      float* const* d_outs, int out_stride, int adjoint, hipStream_t s, int out_rows, int out_cols) {
    int rc = op_rows_fwd_n(p, ws, n, d_imgs, rows, cols, stride, s);
    if (rc == FDR_OK) rc = op_cols_n(p, ws, n, adjoint != 0, s);
    if (rc == FDR_OK)
        rc = op_rows_inv_n(p, ws, n, ROW_OUT_BLUR, kPassOpRowsBlur, nullptr, 0, nullptr, d_outs, out_stride, out_rows ? out_rows : rows,
                           out_cols ? out_cols : cols, s);
    return rc;
}

}  // namespace fdr

extern "C" {

int fdr_set_operator_psf_dev(fdr_plan* p, const float* d_psf, int prows, int pcols, int pstride, void* stream) {
    return set_psf(p, "fdr_set_operator_psf_dev", {PSF_DEV, d_psf, prows, pcols, pstride, 0.0}, true, 0.f, 0.f, (hipStream_t)stream);
}

int fdr_set_operator_psf(fdr_plan* p, const float* psf_host, int prows, int pcols, int pstride) {
    return set_psf(p, "fdr_set_operator_psf", {PSF_HOST, psf_host, prows, pcols, pstride, 0.0}, true, 0.f, 0.f, nullptr);
}

int fdr_set_operator_psf_motion(fdr_plan* p, int size, double angle_deg, void* stream) {
    return set_psf(p, "fdr_set_operator_psf_motion", {PSF_MOTION, nullptr, size, size, size, angle_deg}, true, 0.f, 0.f, (hipStream_t)stream);
}

int fdr_blur_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride, int adjoint, void* stream) {
    const char* fn = "fdr_blur_f32_dev";
    if (!p || !d_img || !d_out) return null_arg(fn);
    const int rc = check_window(p, fn, NEED_OPERATOR_PSF, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return blur_window_dev(p, d_img, rows, cols, stride, d_out, out_stride, rows, cols, adjoint, (hipStream_t)stream);
}

int fdr_blur_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, float* out_host, int out_stride, int adjoint) {
    const char* fn = "fdr_blur_f32";
    if (!p || !img_host || !out_host) return null_arg(fn);
    const int rc = check_window(p, fn, NEED_OPERATOR_PSF, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return host_image_call(p, fn, img_host, rows, cols, stride, out_host, rows, cols, out_stride, [&](const float* d_in, float* d_out) {
        return blur_window_dev(p, d_in, rows, cols, cols, d_out, cols, rows, cols, adjoint, nullptr);
    });
}

}  // extern "C"
