// fdr_api_wiener.hip -- the Wiener / CLS restoration: the filter setters, filter export / import, the single-image operator on
// every path, the panel stages of a group of images, batches on the device (with graph replay) and the host-pointer batch pipeline.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassRowsFwd = "A rows: pad+FFT (real->complex)";
const char* const kPassColsWiener = "B cols: FFT+Wiener";
const char* const kPassRowsInv = "C rows: IFFT (complex)";
const char* const kPassColsInvReal = "D cols: IFFT+real+minmax";
const char* const kPassColsFused = "B' cols: FFT*W*IFFT";
const char* const kPassRowsInvReal = "C' rows: IFFT+real+minmax";
const char* const kPassNormalize = "E normalize+crop";
const char* const kPassRowsMinmax = "C1 rows: IFFT+minmax";
const char* const kPassRowsNorm = "C2 rows: IFFT+normalize+crop";
const char* const kPassSimple = "simple path (reference-shaped)";
const char* const kPassMixedRows = "A mixed rows: pad+FFT (real pairs)";
const char* const kPassMixedCols = "B mixed cols: FFT*W*IFFT";
const char* const kPassMixedRowsInv = "C mixed rows: IFFT+real+minmax";
const char* const kPassMixedNorm = "E mixed normalize+crop";

// the name of a pass over a group of n images: "<base> [n images]", or the base name itself for one image; made once, so that
// the pointers stay the same for the life of the process
struct GroupedName {
    const char* base;
    std::string group[kMaxGroup + 1];
    explicit GroupedName(const char* b) : base(b) {
        for (int n = 2; n <= kMaxGroup; ++n) group[n] = std::string(b) + " [" + std::to_string(n) + " images]";
    }
    const char* operator[](int n) const { return n == 1 ? base : group[n].c_str(); }
};
const GroupedName kPassRowsFwdN(kPassRowsFwd), kPassColsFusedN(kPassColsFused), kPassRowsInvRealN(kPassRowsInvReal),
    kPassNormalizeN(kPassNormalize), kPassRowsMinmaxN(kPassRowsMinmax), kPassRowsNormN(kPassRowsNorm);

}  // namespace

namespace fdr {

// The Laplacian table of the CLS filters and of the TV solve, built in double on the host and uploaded on the first fdr_set_psf_cls* or
// fdr_tv_deconv_f32* call of a plan (synchronous, outside the PRE phase); freed with the plan.  sin^2, not 2 - 2 cos: no cancellation at small frequencies.
int ensure_lap_table(fdr_plan* p) {
    if (p->lap) return FDR_OK;
    std::vector<double> t((size_t)p->M + p->N);
    const double pi = 3.14159265358979323846;
    for (int u = 0; u < p->M; ++u) { const double sn = std::sin(pi * u / p->M); t[u] = 4.0 * sn * sn; }
    for (int v = 0; v < p->N; ++v) { const double sn = std::sin(pi * v / p->N); t[(size_t)p->M + v] = 4.0 * sn * sn; }
    double* d = nullptr;
    FDR_HIP(hipMalloc((void**)&d, t.size() * sizeof(double)));
    const hipError_t e = hipMemcpy(d, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); FDR_HIP(e); }
    p->lap = d;
    return FDR_OK;
}

// gamma > 0: the constrained least-squares filter W = conj(H) / (|H|^2 + K + gamma L^2) (fast mode only); gamma == 0: the Wiener filter
int set_psf_dev_impl(fdr_plan* p, const float* d_psf, int prows, int pcols, int pstride, float K, hipStream_t s, double gamma) {
    const bool cls = gamma > 0.0;
    if (cls) {
        const int rc = ensure_lap_table(p);
        if (rc != FDR_OK) return rc;
    }
    ScopedPhase phase(p, FDR_PHASE_PRE, s);
    // pad top-left + forward 2-D FFT (fft/fft_serial.cpp:166-171,182)
    switch (p->path) {
        case PATH_MIXED: {
            // rows of the PSF only (the rows below are zero and not read by the column pass), which turns H into W on its way out
            MixRowArgs ra = mixed_row_args(p);
            ra.src_real = d_psf; ra.src_rows = prows; ra.src_cols = pcols; ra.src_stride = pstride; ra.dst_c = p->filt;
            FDR_HIP(launch_mixed_rows(MIX_ROWS_FWD_REAL, ra, (prows + 2 * p->mix_B - 1) / (2 * p->mix_B), s));
            MixColArgs ca = mixed_col_args(p);
            ca.src = p->filt; ca.dst = p->filt; ca.K = K; ca.rows_in = prows;
            ca.lap = p->lap; ca.gamma = gamma;
            FDR_HIP(launch_mixed_cols(cls ? MIX_COLS_FILTER_CLS : MIX_COLS_FILTER, ca, p->npanels, s));
            break;
        }
        case PATH_SIMPLE: {
            FDR_HIP(launch_pad_real_to_complex(d_psf, prows, pcols, pstride, p->filt, p->M, p->N, s));
            const int rc = dft2d_dev(p, p->filt, p->slots[0].work2, false, s);
            if (rc != FDR_OK) return rc;
            if (p->mode != FDR_MODE_FAST) break;  // parity keeps H; the column passes of the other fast paths write W themselves
            if (cls) FDR_HIP(launch_make_filter_cls(p->filt, p->filt, p->M, p->N, K, p->lap, gamma, s));
            else FDR_HIP(launch_make_filter_fast(p->filt, p->filt, (size_t)p->M * p->N, K, s));
            break;
        }
        case PATH_FAST_FULL:
        case PATH_FAST_HALF: {
            // the PSF reaches only the first `prows` rows of the padded field: the row pass transforms just those row groups,
            // the column pass takes every row below as zero (unread) and turns the spectrum into W on its way out
            const int nvalid = (prows + 3) & ~3;  // <= M (M is a multiple of 8 on this path)
            RowArgs ra = panel_row_args(p);
            ra.src_real = d_psf; ra.src_rows = prows; ra.src_cols = pcols; ra.src_stride = pstride;
            ra.dst_c = p->filt; ra.M = nvalid;
            FDR_HIP(launch_rows4(p->logN, ROW_IN_REAL, ROW_OUT_COMPLEX, ra, p->tw_row_f, s));
            ColArgs ca = panel_col_args(p);
            ca.data = p->filt; ca.nvalid = nvalid; ca.K = K;
            if (cls) FDR_HIP(launch_cols_panel_cls(p->logM, ca, p->lap, gamma, p->tw_col_f, s));
            else FDR_HIP(launch_cols_panel(p->logM, COL_FWD_FILTER, ca, p->tw_col_f, s));
            break;
        }
        case PATH_PARITY_PANEL: {
            RowArgs ra{};
            ra.src_real = d_psf; ra.src_rows = prows; ra.src_cols = pcols; ra.src_stride = pstride;
            ra.dst_c = p->filt; ra.M = p->M; ra.panel_c = 1; ra.pstride = p->pstride;
            FDR_HIP(launch_rows(p->logN, p->mode, ROW_IN_REAL, ROW_OUT_COMPLEX, false, ra, p->tw_row_f, s));
            ColArgs ca{};
            ca.data = p->filt; ca.N = p->N; ca.panel_c = 1; ca.pstride = p->pstride;
            FDR_HIP(launch_cols(p->logM, p->mode, COL_FWD, ca, p->tw_col_f, p->tw_col_i, s));
            break;
        }
    }
    p->K = K;
    p->have_psf = true;
    return FDR_OK;
}

}  // namespace fdr

namespace {

// ---- the fast panel paths in three stages, each for a group of n >= 1 images on the slots ws[0 .. n) ----
// One image goes by the single-image fields alone (batch.nimg 0: the launchers then pick the split kernels of small images); a
// group of 2 .. kMaxGroup images adds the batch block (blockIdx.y = image), which the row passes have on the half-spectrum path only.
int panel_stage_A(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride, hipStream_t s) {
    ScopedPass t(p, s, kPassRowsFwdN[n]);   // A: 4 rows per thread group, real -> panel-major (half) spectrum
    RowArgs a = panel_row_args(p);
    a.src_real = d_imgs[0]; a.src_rows = rows; a.src_cols = cols; a.src_stride = stride;
    a.dst_c = ws[0]->work; a.pad_mode = p->pad_mode;
    if (n > 1) {
        a.batch.nimg = n;
        for (int k = 0; k < kMaxGroup; ++k) { a.batch.src_real[k] = d_imgs[k < n ? k : 0]; a.batch.spec[k] = ws[k < n ? k : 0]->work; }
    }
    FDR_HIP(launch_rows4(p->logN, ROW_IN_REAL, ROW_OUT_COMPLEX, a, p->tw_row_f, s));
    return FDR_OK;
}
int panel_stage_B(fdr_plan* p, fdr_plan::Slot* const* ws, int n, hipStream_t s) {
    ScopedPass t(p, s, kPassColsFusedN[n]);  // B': per panel, columns forward * W * inverse
    ColArgs c = panel_col_args(p);
    c.data = ws[0]->work; c.filt = p->filt; c.K = p->K;
    c.batch.nimg = n;
    for (int k = 0; k < n; ++k) c.batch.data[k] = ws[k]->work;
    FDR_HIP(launch_cols_panel(p->logM, COL_FUSED, c, p->tw_col_f, s));
    return FDR_OK;
}
int panel_stage_CE(fdr_plan* p, fdr_plan::Slot* const* ws, int n, int rows, int cols, float* const* d_outs, int out_stride, int mm_rows,
                   int mm_cols, hipStream_t s) {
    const bool two_sweep = p->two_sweep && p->path == PATH_FAST_HALF;
    RowArgs a = panel_row_args(p);
    a.src_c = ws[0]->work; a.mm_part = ws[0]->mm_part; a.mm_rows = mm_rows; a.mm_cols = mm_cols;
    const int n_part = rows4_minmax_partials(p->logN, p->M, n, a.half);
    if (n_part <= 0 || n_part > p->mm_part_cap || (!two_sweep && n_part > 4096))
        return fail(FDR_ERR_STATE, "fdr_wiener: min/max partial count out of range");
    if (n > 1) {
        a.batch.nimg = n;
        for (int k = 0; k < kMaxGroup; ++k) {
            const fdr_plan::Slot* w = ws[k < n ? k : 0];
            a.batch.spec[k] = w->work; a.batch.mm_part[k] = w->mm_part;
            if (two_sweep) a.batch.out[k] = d_outs[k < n ? k : 0];
            else a.batch.raw[k] = w->raw;
        }
    }
    if (two_sweep) {
        // C1 + C2: the inverse row transform runs twice -- once for the min/max alone, once more with the normalisation
        // applied on store -- so the raw real plane never exists: 4 + 8 bytes per pixel instead of 8 + 8
        a.out = d_outs[0]; a.out_rows = rows; a.out_cols = cols; a.out_stride = out_stride; a.n_part = n_part;
        {
            ScopedPass t(p, s, kPassRowsMinmaxN[n]);
            FDR_HIP(launch_rows4(p->logN, ROW_IN_COMPLEX, ROW_OUT_MINMAX_ONLY, a, p->tw_row_f, s));
        }
        {
            ScopedPass t(p, s, kPassRowsNormN[n]);
            FDR_HIP(launch_rows4(p->logN, ROW_IN_COMPLEX, ROW_OUT_NORMALIZED, a, p->tw_row_f, s));
        }
        return FDR_OK;
    }
    {   // C': 4 rows rebuilt from the panels, inverse, real plane, min/max partials
        ScopedPass t(p, s, kPassRowsInvRealN[n]);
        a.dst_real = ws[0]->raw;
        FDR_HIP(launch_rows4(p->logN, ROW_IN_COMPLEX, ROW_OUT_REAL_MINMAX, a, p->tw_row_f, s));
    }
    {   // E: normalise to [0,1] and crop
        ScopedPass t(p, s, kPassNormalizeN[n]);
        NormBatch nb{};
        nb.nimg = n;
        for (int k = 0; k < kMaxGroup; ++k) {
            const fdr_plan::Slot* w = ws[k < n ? k : 0];
            nb.raw[k] = w->raw; nb.part[k] = w->mm_part; nb.out[k] = d_outs[k < n ? k : 0];
        }
        FDR_HIP(launch_normalize(ws[0]->raw, p->N, ws[0]->mm_part, n_part, nullptr, d_outs[0], rows, cols, out_stride, s, n > 1 ? &nb : nullptr));
    }
    return FDR_OK;
}

// A, B' and C + E for a group of n images.  Pass B' takes the group in one launch on both panel paths; the row passes do on the
// half-spectrum path (A once; C + E `chunk` images at a time) and run image by image on the full spectrum.
int panel_group(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride, float* const* d_outs,
                int out_stride, int mm_rows, int mm_cols, int chunk, hipStream_t s) {
    const int na = p->path == PATH_FAST_HALF ? n : 1, nc = na < chunk ? na : chunk;
    int rc = FDR_OK;
    for (int k = 0; k < n && rc == FDR_OK; k += na) rc = panel_stage_A(p, ws + k, na, d_imgs + k, rows, cols, stride, s);
    if (rc == FDR_OK) rc = panel_stage_B(p, ws, n, s);
    for (int k = 0; k < n && rc == FDR_OK; k += nc)
        rc = panel_stage_CE(p, ws + k, n - k < nc ? n - k : nc, rows, cols, d_outs + k, out_stride, mm_rows, mm_cols, s);
    return rc;
}

// the mixed-radix operator: A (image rows -> spectrum), B (columns . W . inverse columns, only the rows C reads), C (inverse rows,
// real parts of the cropped rows to the raw plane, min/max over the window), E (normalise + crop)
int mixed_wiener_dev(fdr_plan* p, fdr_plan::Slot& w, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                     int mm_rows, int mm_cols, hipStream_t s) {
    const int B = p->mix_B, need = rows > mm_rows ? rows : mm_rows;  // spectrum rows pass C transforms
    {
        ScopedPass t(p, s, kPassMixedRows);
        MixRowArgs a = mixed_row_args(p);
        a.src_real = d_img; a.src_rows = rows; a.src_cols = cols; a.src_stride = stride; a.dst_c = w.work;
        FDR_HIP(launch_mixed_rows(MIX_ROWS_FWD_REAL, a, (rows + 2 * B - 1) / (2 * B), s));
    }
    {
        ScopedPass t(p, s, kPassMixedCols);
        MixColArgs c = mixed_col_args(p);
        c.src = w.work; c.dst = w.work; c.filt = p->filt; c.rows_in = rows; c.rows_out = need;
        FDR_HIP(launch_mixed_cols(MIX_COLS_FUSED, c, p->npanels, s));
    }
    // raw plane of the cropped rows x cols, row stride rs (a multiple of 4 where it fits: vector normalisation)
    const int rs = ((cols + 3) & ~3) <= p->N ? ((cols + 3) & ~3) : cols;
    const int n_part = (need + 2 * B - 1) / (2 * B);
    if (n_part > p->mm_part_cap) return fail(FDR_ERR_STATE, "fdr_wiener: min/max partial count out of range");
    {
        ScopedPass t(p, s, kPassMixedRowsInv);
        MixRowArgs a = mixed_row_args(p);
        a.src_c = w.work; a.rows_in = need; a.dst_real = w.raw; a.dst_stride = rs; a.out_rows = rows; a.out_cols = cols;
        a.mm_rows = mm_rows; a.mm_cols = mm_cols; a.mm_part = w.mm_part; a.scale = (float)(1.0 / ((double)p->M * p->N));
        FDR_HIP(launch_mixed_rows(MIX_ROWS_INV_REAL, a, n_part, s));
    }
    {
        ScopedPass t(p, s, kPassMixedNorm);
        FDR_HIP(launch_normalize(w.raw, rs, w.mm_part, n_part, nullptr, d_out, rows, cols, out_stride, s));
    }
    return FDR_OK;
}

// one image on slot w; the entry points have checked plan and window
int wiener_dev_impl(fdr_plan* p, fdr_plan::Slot& w, const float* d_img, int rows, int cols, int stride, float* d_out,
                    int out_stride, int norm_area, hipStream_t s) {
    const int mm_rows = norm_area == FDR_NORM_PADDED ? p->M : rows;
    const int mm_cols = norm_area == FDR_NORM_PADDED ? p->N : cols;
    int n_part = 0;

    switch (p->path) {
        case PATH_MIXED:
            return mixed_wiener_dev(p, w, d_img, rows, cols, stride, d_out, out_stride, mm_rows, mm_cols, s);
        case PATH_FAST_FULL:
        case PATH_FAST_HALF: {  // a group of one
            fdr_plan::Slot* one = &w;
            return panel_group(p, &one, 1, &d_img, rows, cols, stride, &d_out, out_stride, mm_rows, mm_cols, 1, s);
        }
        case PATH_SIMPLE: {
            ScopedPass t(p, s, kPassSimple);
            FDR_HIP(launch_pad_real_to_complex(d_img, rows, cols, stride, w.work, p->M, p->N, s));
            int rc = dft2d_dev(p, w.work, w.work2, false, s);
            if (rc != FDR_OK) return rc;
            FDR_HIP(launch_wiener_pointwise(w.work, p->filt, (size_t)p->M * p->N, p->K, p->mode, s));
            rc = dft2d_dev(p, w.work, w.work2, true, s);
            if (rc != FDR_OK) return rc;
            FDR_HIP(launch_real_minmax(w.work, w.raw, p->M, p->N, mm_rows, mm_cols, w.mm_part, &n_part, s));
            break;
        }
        case PATH_PARITY_PANEL: {
            {   // A: rows, real -> complex (fft/fft_serial.cpp:157-165,176 first half)
                ScopedPass t(p, s, kPassRowsFwd);
                RowArgs a{};
                a.src_real = d_img; a.src_rows = rows; a.src_cols = cols; a.src_stride = stride;
                a.dst_c = w.work; a.M = p->M; a.panel_c = 1; a.pstride = p->pstride;
                FDR_HIP(launch_rows(p->logN, p->mode, ROW_IN_REAL, ROW_OUT_COMPLEX, false, a, p->tw_row_f, s));
            }
            {   // B: columns forward + Wiener quotient (:176 second half, :186-224)
                ScopedPass t(p, s, kPassColsWiener);
                ColArgs c{};
                c.data = w.work; c.filt = p->filt; c.K = p->K; c.N = p->N; c.panel_c = 1; c.pstride = p->pstride;
                FDR_HIP(launch_cols(p->logM, p->mode, COL_FWD_WIENER, c, p->tw_col_f, p->tw_col_i, s));
            }
            {   // C: rows inverse (:229 first half)
                ScopedPass t(p, s, kPassRowsInv);
                RowArgs a{};
                a.src_c = w.work; a.dst_c = w.work; a.M = p->M; a.panel_c = 1; a.pstride = p->pstride;
                FDR_HIP(launch_rows(p->logN, p->mode, ROW_IN_COMPLEX, ROW_OUT_COMPLEX, true, a, p->tw_row_i, s));
            }
            {   // D: columns inverse, real plane, min/max (:229 second half, :236-240, minMaxIdx of :246)
                ScopedPass t(p, s, kPassColsInvReal);
                ColArgs c{};
                c.data = w.work; c.dst_real = w.raw; c.mm_part = w.mm_part; c.mm_rows = mm_rows; c.mm_cols = mm_cols; c.N = p->N;
                c.panel_c = 1; c.pstride = p->pstride;
                FDR_HIP(launch_cols(p->logM, p->mode, COL_INV_REAL, c, p->tw_col_f, p->tw_col_i, s));
                n_part = cols_minmax_partials(p->logM, p->N);
            }
            break;
        }
    }
    {   // E: normalise to [0,1] and crop (fft/fft_serial.cpp:246, serial.cpp:38)
        ScopedPass t(p, s, kPassNormalize);
        if (n_part <= 0 || n_part > p->mm_part_cap) return fail(FDR_ERR_STATE, "fdr_wiener: min/max partial count out of range");
        const bool pp = p->path == PATH_PARITY_PANEL;  // the raw plane is panel-major then
        if (n_part <= 4096) {
            if (pp) FDR_HIP(launch_normalize_panels(w.raw, p->M, w.mm_part, n_part, nullptr, d_out, rows, cols, out_stride, s));
            else FDR_HIP(launch_normalize(w.raw, p->N, w.mm_part, n_part, nullptr, d_out, rows, cols, out_stride, s));
        } else {  // many partials (reference-shaped path): fold them once in a separate launch
            FDR_HIP(launch_reduce_minmax(w.mm_part, n_part, w.mm, s));
            if (pp) FDR_HIP(launch_normalize_panels(w.raw, p->M, nullptr, 0, w.mm, d_out, rows, cols, out_stride, s));
            else FDR_HIP(launch_normalize(w.raw, p->N, nullptr, 0, w.mm, d_out, rows, cols, out_stride, s));
        }
    }
    return FDR_OK;
}

// fork, every pass of every group, join -- all relative to `us` (the caller's stream, or the capturing stream)
int batch_enqueue(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride, float* d_out,
                  size_t out_pitch, int out_stride, int norm_area, hipStream_t us) {
    int rc = FDR_OK;
    const int mm_rows = norm_area == FDR_NORM_PADDED ? p->M : rows;
    const int mm_cols = norm_area == FDR_NORM_PADDED ? p->N : cols;
    const int group = on_panel_path(p) ? p->group : 1;
    // per-kernel profiling wants un-overlapped durations: keep everything on the caller's stream then
    const int ns = (p->timer.enabled || count <= group) ? 1 : p->nstreams;
    if (ns > 1) {  // fork: internal streams wait for everything queued so far on the caller's stream
        FDR_HIP(hipEventRecord(p->fork, us));
        for (int k = 0; k < ns; ++k) FDR_HIP(hipStreamWaitEvent(p->slots[k * group].stream, p->fork, 0));
    }
    int chunk = 0;
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group, ++chunk) {
        const int n = count - i0 < group ? count - i0 : group;
        const int sidx = chunk % ns;
        fdr_plan::Slot* ws[fdr_plan::kMaxSlots];
        for (int k = 0; k < n; ++k) ws[k] = &p->slots[sidx * group + k];
        hipStream_t s = ns > 1 ? p->slots[sidx * group].stream : us;
        if (!on_panel_path(p)) {
            rc = wiener_dev_impl(p, *ws[0], d_imgs + (size_t)i0 * img_pitch, rows, cols, stride, d_out + (size_t)i0 * out_pitch,
                                 out_stride, norm_area, s);
            continue;
        }
        const float* ins[kMaxGroup]; float* outs[kMaxGroup];
        for (int k = 0; k < n; ++k) { ins[k] = d_imgs + (size_t)(i0 + k) * img_pitch; outs[k] = d_out + (size_t)(i0 + k) * out_pitch; }
        // The two inverse row passes (C1: extremes; C2: the same transform again, normalised) go in CHUNKS of the group
        // when the batch alternates over two or more streams: C1 is the pass with exposed compute, and in launches of half
        // the size it interleaves better with the memory-bound passes of the other stream's group.  With ONE stream the
        // chunks only make the launches smaller, and passes A / B' lose in chunks (LAB_NOTES "inverse row chunks").
        // Hence: >= 2 streams, and a chunk holds at least ce_chunk_bytes of spectrum (FDR_OPT_CE_CHUNK_MB, default
        // 160 MiB: pairs at 4096^2, the whole group below, no split where one image alone is larger).
        int ce_chunk = n;
        if (ns > 1) {
            const size_t spec_bytes = p->ws_elems * sizeof(float2);
            if (p->ce_chunk_bytes > 0 && spec_bytes <= p->ce_chunk_bytes) {
                const size_t c = p->ce_chunk_bytes / spec_bytes;
                if (c < (size_t)n) ce_chunk = (int)c;
            }
        }
        rc = panel_group(p, ws, n, ins, rows, cols, stride, outs, out_stride, mm_rows, mm_cols, ce_chunk, s);
    }
    if (ns > 1) {  // join -- also after an error: the caller's stream continues only after every internal stream has
                   // drained, so work already queued there cannot still be writing d_out when the caller goes on
        const std::string first_error = g_last_error;
        for (int k = 0; k < ns; ++k) {
            hipError_t e = hipEventRecord(p->slots[k * group].done, p->slots[k * group].stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(us, p->slots[k * group].done, 0);
            if (e != hipSuccess) {  // cannot order the streams: drain them on the host instead
                (void)hipStreamSynchronize(p->slots[k * group].stream);
                if (rc == FDR_OK) rc = fail(FDR_ERR_HIP, std::string("fdr_wiener_batch_f32_dev: join failed: ") + hipGetErrorString(e));
            }
        }
        if (rc != FDR_OK && !first_error.empty() && first_error != g_last_error && rc != FDR_ERR_HIP) g_last_error = first_error;
    }
    return rc;
}

}  // namespace

extern "C" {

int fdr_set_psf_dev(fdr_plan* p, const float* d_psf, int prows, int pcols, int pstride, float K, void* stream) {
    return set_psf(p, "fdr_set_psf_dev", {PSF_DEV, d_psf, prows, pcols, pstride, 0.0}, false, K, 0.f, (hipStream_t)stream);
}

int fdr_set_psf(fdr_plan* p, const float* psf_host, int prows, int pcols, int pstride, float K) {
    return set_psf(p, "fdr_set_psf", {PSF_HOST, psf_host, prows, pcols, pstride, 0.0}, false, K, 0.f, nullptr);
}

int fdr_set_psf_motion(fdr_plan* p, int size, double angle_deg, float K, void* stream) {
    return set_psf(p, "fdr_set_psf_motion", {PSF_MOTION, nullptr, size, size, size, angle_deg}, false, K, 0.f, (hipStream_t)stream);
}

int fdr_set_psf_cls_dev(fdr_plan* p, const float* d_psf, int prows, int pcols, int pstride, float K, float gamma, void* stream) {
    return set_psf(p, "fdr_set_psf_cls_dev", {PSF_DEV, d_psf, prows, pcols, pstride, 0.0}, false, K, gamma, (hipStream_t)stream);
}

int fdr_set_psf_cls(fdr_plan* p, const float* psf_host, int prows, int pcols, int pstride, float K, float gamma) {
    return set_psf(p, "fdr_set_psf_cls", {PSF_HOST, psf_host, prows, pcols, pstride, 0.0}, false, K, gamma, nullptr);
}

int fdr_set_psf_motion_cls(fdr_plan* p, int size, double angle_deg, float K, float gamma, void* stream) {
    return set_psf(p, "fdr_set_psf_motion_cls", {PSF_MOTION, nullptr, size, size, size, angle_deg}, false, K, gamma, (hipStream_t)stream);
}

int fdr_plan_filter_bytes(const fdr_plan* p, size_t* bytes) {
    if (!p || !bytes) return null_arg("fdr_plan_filter_bytes");
    const int rc = check_plan(p, "fdr_plan_filter_bytes", NEED_PLAN);
    if (rc != FDR_OK) return rc;
    *bytes = p->ws_elems * sizeof(float2);
    return FDR_OK;
}

int fdr_plan_export_filter_dev(fdr_plan* p, void* d_dst, size_t bytes, void* stream) {
    const char* fn = "fdr_plan_export_filter_dev";
    if (!p || !d_dst) return null_arg(fn);
    const int rc = check_plan(p, fn, NEED_FILTER);
    if (rc != FDR_OK) return rc;
    if (bytes != p->ws_elems * sizeof(float2)) return fail(FDR_ERR_ARG, std::string(fn) + ": size differs from fdr_plan_filter_bytes");
    FDR_HIP(hipSetDevice(p->device));
    FDR_HIP(hipMemcpyAsync(d_dst, p->filt, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return FDR_OK;
}

int fdr_plan_import_filter_dev(fdr_plan* p, const void* d_src, size_t bytes, float K, void* stream) {
    const char* fn = "fdr_plan_import_filter_dev";
    if (!p || !d_src) return null_arg(fn);
    const int rc = check_plan(p, fn, NEED_PLAN);
    if (rc != FDR_OK) return rc;
    if (bytes != p->ws_elems * sizeof(float2)) return fail(FDR_ERR_ARG, std::string(fn) + ": size differs from fdr_plan_filter_bytes");
    FDR_HIP(hipSetDevice(p->device));
    ScopedPhase phase(p, FDR_PHASE_PRE, (hipStream_t)stream);
    FDR_HIP(hipMemcpyAsync(p->filt, d_src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    p->K = K;
    p->have_psf = true;
    return FDR_OK;
}

int fdr_wiener_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                       int norm_area, void* stream) {
    const char* fn = "fdr_wiener_f32_dev";
    if (!p || !d_img || !d_out) return null_arg(fn);
    const int rc = check_window(p, fn, NEED_FILTER, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return wiener_dev_impl(p, p->slots[0], d_img, rows, cols, stride, d_out, out_stride, norm_area, (hipStream_t)stream);
}

int fdr_wiener_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, float* out_host, int out_stride,
                   int norm_area) {
    const char* fn = "fdr_wiener_f32";
    if (!p || !img_host || !out_host) return null_arg(fn);
    const int rc = check_window(p, fn, NEED_FILTER, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return host_image_call(p, fn, img_host, rows, cols, stride, out_host, rows, cols, out_stride, [&](const float* d_in, float* d_out) {
        return wiener_dev_impl(p, p->slots[0], d_in, rows, cols, cols, d_out, cols, norm_area, nullptr);
    });
}

int fdr_wiener_batch_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                             float* d_out, size_t out_pitch, int out_stride, int norm_area, void* stream) {
    const char* fn = "fdr_wiener_batch_f32_dev";
    if (!p) return null_arg(fn);
    if (count < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": negative count");
    if (count == 0) return FDR_OK;
    if (!d_imgs || !d_out) return null_arg(fn);
    int rc = check_window(p, fn, NEED_FILTER, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    hipStream_t us = (hipStream_t)stream;
    // graph replay: launch-bound batches (small images) pay one graph launch instead of 4 kernel launches per group.
    // Not with per-kernel profiling (host-side event pairs).
    if (p->batch_graph && on_panel_path(p) && !p->timer.enabled) {
        const fdr_plan::GraphKey key{d_imgs, d_out, img_pitch, out_pitch, count, rows, cols, stride, out_stride, norm_area, p->nstreams, p->group,
                                     p->two_sweep, p->K, p->ce_chunk_bytes, p->pad_mode};
        if (!(p->graph_exec && key == p->graph_key)) {
            if (p->graph_exec) { (void)hipGraphExecDestroy(p->graph_exec); p->graph_exec = nullptr; }
            if (!p->cap_stream) FDR_HIP(hipStreamCreateWithFlags(&p->cap_stream, hipStreamNonBlocking));
            FDR_HIP(hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeThreadLocal));
            rc = batch_enqueue(p, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, norm_area, p->cap_stream);
            hipGraph_t g = nullptr;
            const hipError_t e = hipStreamEndCapture(p->cap_stream, &g);  // (always: the stream has to leave capture mode)
            if (rc != FDR_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
            FDR_HIP(e);
            const hipError_t ei = hipGraphInstantiate(&p->graph_exec, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ei != hipSuccess) { p->graph_exec = nullptr; FDR_HIP(ei); }
            p->graph_key = key;
        }
        FDR_HIP(hipGraphLaunch(p->graph_exec, us));
        return FDR_OK;
    }
    return batch_enqueue(p, d_imgs, img_pitch, count, rows, cols, stride, d_out, out_pitch, out_stride, norm_area, us);
}

// ---- host-pointer batch: H2D, restore, D2H of consecutive images overlap on three streams ----------------------
// (the pipeline fft/fft_gpu.cu:306-350,372-385 sets out to build with pinned staging buffers and cudaMemcpyAsync)
int fdr_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return fail(FDR_ERR_ARG, "fdr_host_alloc: bad argument");
    FDR_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return FDR_OK;
}
int fdr_host_free(void* p) {
    if (p) FDR_HIP(hipHostFree(p));
    return FDR_OK;
}

int fdr_wiener_batch_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                         float* out_host, size_t out_pitch, int out_stride, int norm_area) {
    if (!p || !imgs_host || !out_host) return null_arg("fdr_wiener_batch_f32");
    if (count < 0) return fail(FDR_ERR_ARG, "fdr_wiener_batch_f32: negative count");
    if (count == 0) return FDR_OK;
    std::vector<const float*> ins((size_t)count);
    std::vector<float*> outs((size_t)count);
    for (int i = 0; i < count; ++i) { ins[i] = imgs_host + (size_t)i * img_pitch; outs[i] = out_host + (size_t)i * out_pitch; }
    return fdr_wiener_batch_ptrs_f32(p, ins.data(), outs.data(), count, rows, cols, stride, out_stride, norm_area);
}

int fdr_wiener_batch_ptrs_f32(fdr_plan* p, const float* const* imgs_host, float* const* outs_host, int count, int rows, int cols,
                              int stride, int out_stride, int norm_area) {
    const char* fn = "fdr_wiener_batch_ptrs_f32";
    if (!p || !imgs_host || !outs_host) return null_arg(fn);
    if (count < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": negative count");
    if (count == 0) return FDR_OK;
    for (int i = 0; i < count; ++i)
        if (!imgs_host[i] || !outs_host[i]) return null_arg(fn);
    int rc = check_window(p, fn, NEED_FILTER, rows, cols, stride, out_stride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    // Three images in flight: one arriving, one being restored, one leaving, each on its own stream.  Pinned buffers
    // (fdr_host_alloc) are read / written by DMA and all three stages overlap; with pageable buffers the runtime stages
    // every copy itself and the copy calls block, which leaves the synchronous rate (LAB_NOTES "host-pointer calls").
    constexpr int D = 3;
    const size_t bytes = (size_t)rows * cols * sizeof(float), rowb = (size_t)cols * sizeof(float);
    // streams, events and device staging live in the plan (created on first use, sized for the plan's M x N)
    fdr_plan::HostPipe& hp = p->pipe;
    if (!hp.ready) {  // built into locals and committed only when every stream and event exists (failure-atomic)
        hipStream_t st[3] = {nullptr, nullptr, nullptr};
        hipEvent_t ev[3 * D] = {};
        hipError_t ce = hipSuccess;
        for (int k = 0; k < 3 && ce == hipSuccess; ++k) ce = hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking);
        for (int k = 0; k < 3 * D && ce == hipSuccess; ++k) ce = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
        if (ce != hipSuccess) {
            for (int k = 0; k < 3; ++k) if (st[k]) (void)hipStreamDestroy(st[k]);
            for (int k = 0; k < 3 * D; ++k) if (ev[k]) (void)hipEventDestroy(ev[k]);
            FDR_HIP(ce);
        }
        hp.s_in = st[0]; hp.s_cmp = st[1]; hp.s_out = st[2];
        for (int k = 0; k < D; ++k) { hp.e_in[k] = ev[3 * k]; hp.e_cmp[k] = ev[3 * k + 1]; hp.e_out[k] = ev[3 * k + 2]; }
        hp.ready = true;
    }
    if (hp.cap < bytes) {
        const size_t cap = (size_t)p->M * p->N * sizeof(float);
        for (int k = 0; k < D; ++k) { (void)hipFree(hp.d_in[k]); (void)hipFree(hp.d_out[k]); hp.d_in[k] = hp.d_out[k] = nullptr; }
        hp.cap = 0;
        for (int k = 0; k < D; ++k)
            if (hipMalloc((void**)&hp.d_in[k], cap) != hipSuccess || hipMalloc((void**)&hp.d_out[k], cap) != hipSuccess)
                return fail(FDR_ERR_ALLOC, "fdr_wiener_batch_f32: hipMalloc of the staging buffers failed");
        hp.cap = cap;
    }
    float* const* d_in = hp.d_in;
    float* const* d_out = hp.d_out;
    hipStream_t s_in = hp.s_in, s_cmp = hp.s_cmp, s_out = hp.s_out;
    hipEvent_t *e_in = hp.e_in, *e_cmp = hp.e_cmp, *e_out = hp.e_out;
    hipError_t e = hipSuccess;
    auto bad = [&](hipError_t err) { e = err; return err != hipSuccess; };
    for (int i = 0; i < count; ++i) {
        const int k = i % D;
        const float* src = imgs_host[i];
        float* dst = outs_host[i];
        // slot k is free again once image i-D has left the device (its D2H read d_out[k], its kernels read d_in[k])
        if (i >= D && bad(hipStreamWaitEvent(s_in, e_out[k], 0))) break;
        {
            ScopedPhase ph(p, FDR_PHASE_H2D, s_in);
            if (bad(stride == cols ? hipMemcpyAsync(d_in[k], src, bytes, hipMemcpyHostToDevice, s_in)
                                   : hipMemcpy2DAsync(d_in[k], rowb, src, (size_t)stride * sizeof(float), rowb, rows, hipMemcpyHostToDevice, s_in))) break;
        }
        if (bad(hipEventRecord(e_in[k], s_in)) || bad(hipStreamWaitEvent(s_cmp, e_in[k], 0))) break;
        {
            ScopedPhase ph(p, FDR_PHASE_COMPUTE, s_cmp);
            rc = wiener_dev_impl(p, p->slots[0], d_in[k], rows, cols, cols, d_out[k], cols, norm_area, s_cmp);
        }
        if (rc != FDR_OK) break;
        if (bad(hipEventRecord(e_cmp[k], s_cmp)) || bad(hipStreamWaitEvent(s_out, e_cmp[k], 0))) break;
        {
            ScopedPhase ph(p, FDR_PHASE_D2H, s_out);
            if (bad(out_stride == cols ? hipMemcpyAsync(dst, d_out[k], bytes, hipMemcpyDeviceToHost, s_out)
                                       : hipMemcpy2DAsync(dst, (size_t)out_stride * sizeof(float), d_out[k], rowb, rowb, rows, hipMemcpyDeviceToHost, s_out))) break;
        }
        if (bad(hipEventRecord(e_out[k], s_out))) break;
    }
    // everything queued must have left the device before the call returns (also on the error paths: the buffers are reused)
    (void)hipStreamSynchronize(s_in);
    (void)hipStreamSynchronize(s_cmp);
    { hipError_t es = hipStreamSynchronize(s_out); if (e == hipSuccess) e = es; }
    resolve_phases(p);
    if (rc != FDR_OK) return rc;
    FDR_HIP(e);
    return FDR_OK;
}

}  // extern "C"
