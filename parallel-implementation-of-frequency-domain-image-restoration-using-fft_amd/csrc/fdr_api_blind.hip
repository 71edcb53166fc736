// fdr_api_blind.hip -- blind Richardson-Lucy, both forms (fdr_richardson_lucy_blind_f32*; kernels in fdr_blind.hip), and the
// Gaussian PSF: the workspace, the checks, the hooks and the entry points.  The image iterations are the form's own driver
// (rl_group_dev, rlfree_batch_dev, one image); the PSF step hangs on its three hooks (RlHooks), from iteration psf_hold on: the
// table conj(U_k) / (M N) from the row spectra of u_k, then, from the same r, corr_(u_k) through pass A, pass B' on that table and
// pass C cropped to the PSF; after the step the projection, the operator tables of p_(k+1) and (free form) its coverage.
#include "fdr_host.hpp"

#include <cmath>
#include <vector>

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id; four of them, so that the sixteen names of a plan still hold
// every pass of a free-boundary call beside them
const char* const kPassBlTable = "BL cols: FFT -> conj(U)/MN";
const char* const kPassBlCorr = "B' op cols: FFT*conj(U)*IFFT";
const char* const kPassBlCrop = "C op rows: IFFT+crop (PSF)";
const char* const kPassBlPsf = "BL PSF: start / project / wgt";

static_assert(FDR_BLIND_MAX_PSF == kBlindMaxPsf, "the PSF limit of the header is the one-workgroup kernels'");

int ensure_blind_workspace(fdr_plan* p, const char* fn, bool free_form) {
    int rc = ensure_workspace(p->blind.ws, fn, "blind workspace", 1, [p](auto& c, int) { layout(c, p->blind, p->ws_elems, (size_t)kBlindMaxPsf); });
    if (rc == FDR_OK && free_form)
        rc = ensure_workspace(p->blind.w_ws, fn, "blind workspace", 1, [p](auto& c, int) { layout(c, p->blind.w, (size_t)p->M * p->N, 16); });
    return rc;
}

fdr_rlfree_params free_params(const fdr_blind_params& b) {
    fdr_rlfree_params f{};
    f.iterations = b.iterations; f.sigma = b.cov_sigma; f.norm_area = b.norm_area; f.out_rows = b.out_rows; f.out_cols = b.out_cols;
    return f;
}

// everything a blind call refuses, before any device work: what the underlying form refuses (an operator PSF need not be set), and
// the PSF's shape and overlaps
int blind_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
                const float* psf, int prows, int pcols, int pstride, const float* out, int out_stride, const fdr_blind_params* prm) {
    if (!prm || !psf) return null_arg(fn);
    int rc = FDR_OK;
    int orows = rows, ocols = cols;
    if (prm->free_boundary) {
        const fdr_rlfree_params f = free_params(*prm);
        rc = rlfree_check(p, fn, img, rows, cols, stride, weights, wstride, out, out_stride, &f, NEED_OPERATOR);
        orows = prm->out_rows; ocols = prm->out_cols;
    } else {
        rc = rl_check(p, fn, img, rows, cols, stride, out, out_stride, prm->iterations, prm->norm_area, NEED_OPERATOR);
        if (rc == FDR_OK)
            rc = plain_form_check(fn, weights, rows, cols, prm->out_rows, prm->out_cols, false,
                                  ": the plain form's output window is the input's (out_rows, out_cols = 0 or rows, cols)");
    }
    if (rc != FDR_OK) return rc;
    if (prm->psf_hold < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": psf_hold < 0");
    if (prows <= 0 || pcols <= 0 || pstride < pcols) return fail(FDR_ERR_ARG, std::string(fn) + ": bad PSF shape");
    if (prows > p->M || pcols > p->N) return fail(FDR_ERR_ARG, std::string(fn) + ": PSF larger than the padded image");
    if ((size_t)prows * pcols > (size_t)kBlindMaxPsf) return fail(FDR_ERR_ARG, std::string(fn) + ": a PSF of more than 65536 entries");
    // den = corr_u(W) of a tap sums u over the window shifted by the tap.  Under a window smaller than the PSF that shifted window can
    // lie wholly where the coverage is below sigma, u = 0 there, and den is 0 up to the transform's rounding: its sign, and with it the
    // tap, would be noise.  A window of the PSF's size always reaches covered pixels.
    if (prm->free_boundary && (rows < prows || cols < pcols))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the free-boundary form needs a window of at least the PSF's size, prows x pcols");
    const ByteRange f = window_range(psf, prows, pcols, pstride);
    if (ranges_overlap(f, window_range(img, rows, cols, stride))) return fail(FDR_ERR_ARG, std::string(fn) + ": the PSF overlaps the input");
    if (weights && ranges_overlap(f, window_range(weights, rows, cols, wstride))) return fail(FDR_ERR_ARG, std::string(fn) + ": the PSF overlaps the weights");
    if (ranges_overlap(f, window_range(out, orows, ocols, out_stride))) return fail(FDR_ERR_ARG, std::string(fn) + ": the PSF overlaps the output");
    return FDR_OK;
}

// the PSF step's share of an iteration: what the three hooks run
struct BlindStep {
    fdr_plan* p; int rows, cols, prows, pcols; bool free_form; float sigma; hipStream_t s;
    // the table of the image: slot 0 holds the row spectra of u_k (`nrows` of them are not zero); they are only read
    int table(int nrows) const {
        ScopedPass t(p, s, kPassBlTable);
        ColArgs ca = panel_col_args(p);
        ca.data = p->slots[0].work; ca.nvalid = (nrows + 3) & ~3;  // <= M (M is a multiple of 8 on this path)
        FDR_HIP(launch_cols_panel_conj(p->logM, ca, p->blind.table, p->tw_col_f, s));
        return FDR_OK;
    }
    // corr_(u_k) of the window rows x cols of x (dense) into the PSF plane dst
    int corr(const float* x, float* dst) const {
        int rc = op_rows_fwd(p, x, rows, cols, cols, s);
        if (rc == FDR_OK) rc = op_cols_table(p, p->blind.table, kPassBlCorr, s);
        if (rc == FDR_OK) rc = op_rows_inv(p, ROW_OUT_BLUR, kPassBlCrop, nullptr, 0, dst, pcols, prows, pcols, s);
        return rc;
    }
    int after_ratio() const {
        int rc = corr(p->slots[0].raw, p->blind.num);
        if (rc == FDR_OK && free_form) rc = corr(p->blind.w, p->blind.den);
        return rc;
    }
    // p_(k+1) and its operator tables; after the last step the PSF also to `out` (row stride ostride), before it (free form) the
    // coverage of p_(k+1)
    int after_step(bool last, float* out, int ostride) const {
        {
            ScopedPass t(p, s, kPassBlPsf);
            FDR_HIP(launch_blind_psf_project(p->blind.p, p->blind.num, free_form ? p->blind.den : nullptr, prows, pcols, p->blind.status, last ? out : nullptr,
                                             ostride, s));
        }
        int rc = set_operator_psf_impl(p, p->blind.p, prows, pcols, pcols, s);
        if (rc != FDR_OK || last || !free_form) return rc;
        rc = blur_window_dev(p, p->blind.w, rows, cols, cols, p->rlfree.wgt, p->N, p->M, p->N, 1, s);
        if (rc != FDR_OK) return rc;
        ScopedPass t(p, s, kPassBlPsf);
        FDR_HIP(launch_blind_wgt(p->rlfree.wgt, (size_t)p->M * p->N, sigma, s));
        return FDR_OK;
    }
};

// the start PSF and its operator tables, the hooks, the form's driver on one image
int blind_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* d_psf,
                   int prows, int pcols, int pstride, float* d_out, int out_stride, const fdr_blind_params& prm, hipStream_t s) {
    const int n = prm.iterations, hold = prm.psf_hold;
    const bool free_form = prm.free_boundary != 0;
    const BlindStep bs{p, rows, cols, prows, pcols, free_form, prm.cov_sigma, s};
    {
        ScopedPass t(p, s, kPassBlPsf);
        FDR_HIP(launch_blind_psf_start(d_psf, prows, pcols, pstride, p->blind.p, p->blind.status, s));
    }
    const int rc = set_operator_psf_impl(p, p->blind.p, prows, pcols, pcols, s);
    if (rc != FDR_OK) return rc;
    RlHooks hooks;
    hooks.after_fwd = [&](int it) { return it < hold ? FDR_OK : bs.table(free_form ? p->M : rows); };
    hooks.after_ratio = [&](int it) { return it < hold ? FDR_OK : bs.after_ratio(); };
    hooks.after_step = [&](int it) { return it < hold ? FDR_OK : bs.after_step(it == n - 1, d_psf, pstride); };
    if (free_form)
        return rlfree_batch_dev(p, fn, d_img, 0, 1, rows, cols, stride, d_w, wstride, d_out, 0, out_stride, free_params(prm), s, &hooks, p->blind.w);
    fdr_plan::Slot* w = &p->slots[0];
    return rl_group_dev(p, fn, &w, 1, &d_img, rows, cols, stride, &d_out, out_stride, n, prm.norm_area, s, &hooks);
}

// the start PSF of the host form, as fdr.h states it: no negative entry, a finite sum > 0
int host_psf_check(const char* fn, const float* psf, int prows, int pcols, int pstride) {
    double sum = 0.0;
    for (int i = 0; i < prows; ++i)
        for (int j = 0; j < pcols; ++j) {
            const float v = psf[(size_t)i * pstride + j];
            if (v < 0.f) return fail(FDR_ERR_ARG, std::string(fn) + ": the start PSF has a negative entry");
            sum += (double)v;
        }
    if (!(sum > 0.0) || !std::isfinite(sum)) return fail(FDR_ERR_ARG, std::string(fn) + ": the start PSF's sum must be finite and > 0");
    return FDR_OK;
}

int ensure_form_workspaces(fdr_plan* p, const char* fn, bool free_form) {
    int rc = free_form ? ensure_rlfree_workspace(p, fn) : FDR_OK;
    if (rc == FDR_OK) rc = ensure_blind_workspace(p, fn, free_form);
    return rc;
}

}  // namespace

extern "C" {

int fdr_richardson_lucy_blind_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                                      float* d_psf, int prows, int pcols, int pstride, float* d_out, int out_stride,
                                      const fdr_blind_params* params, void* stream) {
    const char* fn = "fdr_richardson_lucy_blind_f32_dev";
    if (!p || !d_img || !d_out) return null_arg(fn);
    int rc = blind_check(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_psf, prows, pcols, pstride, d_out, out_stride, params);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = ensure_form_workspaces(p, fn, params->free_boundary != 0);
    if (rc != FDR_OK) return rc;
    return blind_dev_impl(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_psf, prows, pcols, pstride, d_out, out_stride, *params,
                          (hipStream_t)stream);
}

int fdr_richardson_lucy_blind_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                                  float* psf_host, int prows, int pcols, int pstride, float* out_host, int out_stride,
                                  const fdr_blind_params* params) {
    const char* fn = "fdr_richardson_lucy_blind_f32";
    if (!p || !img_host || !out_host) return null_arg(fn);
    int rc = blind_check(p, fn, img_host, rows, cols, stride, weights_host, wstride, psf_host, prows, pcols, pstride, out_host, out_stride, params);
    if (rc == FDR_OK) rc = host_psf_check(fn, psf_host, prows, pcols, pstride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    const fdr_blind_params prm = *params;
    const bool free_form = prm.free_boundary != 0;
    rc = ensure_form_workspaces(p, fn, free_form);
    if (rc != FDR_OK) return rc;
    const size_t pw = (size_t)pcols * sizeof(float);
    FDR_HIP(hipMemcpy2D(p->blind.stage, pw, psf_host, (size_t)pstride * sizeof(float), pw, (size_t)prows, hipMemcpyHostToDevice));
    if (free_form && weights_host) rc = stage_weights(p, weights_host, rows, cols, wstride);
    if (rc != FDR_OK) return rc;
    const int orows = free_form ? prm.out_rows : rows, ocols = free_form ? prm.out_cols : cols;
    rc = host_image_call(p, fn, img_host, rows, cols, stride, out_host, orows, ocols, out_stride, [&](const float* d_in, float* d_out) {
        return blind_dev_impl(p, fn, d_in, rows, cols, cols, free_form && weights_host ? p->rlfree.u : nullptr, cols, p->blind.stage, prows, pcols,
                              pcols, d_out, ocols, prm, nullptr);
    });
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipMemcpy2D(psf_host, (size_t)pstride * sizeof(float), p->blind.stage, pw, pw, (size_t)prows, hipMemcpyDeviceToHost));
    return FDR_OK;
}

int fdr_richardson_lucy_blind_status(fdr_plan* p, int* status) {
    const char* fn = "fdr_richardson_lucy_blind_status";
    if (!p || !status) return null_arg(fn);
    if (!p->blind.ws.block) return fail(FDR_ERR_STATE, std::string(fn) + ": no blind call has run on this plan");
    FDR_HIP(hipSetDevice(p->device));
    FDR_HIP(hipDeviceSynchronize());
    FDR_HIP(hipMemcpy(status, p->blind.status, sizeof(int), hipMemcpyDeviceToHost));
    return FDR_OK;
}

static int gaussian_check(const char* fn, int size, double* sigma, const float* out) {
    if (!out) return null_arg(fn);
    if (size <= 0 || (size_t)size * size > (size_t)kBlindMaxPsf) return fail(FDR_ERR_ARG, std::string(fn) + ": size must lie in 1 .. 256");
    if (*sigma == 0.0) *sigma = size / 4.0;
    if (!(*sigma > 0.0) || !std::isfinite(*sigma)) return fail(FDR_ERR_ARG, std::string(fn) + ": sigma must be finite and >= 0");
    return FDR_OK;
}

int fdr_psf_gaussian(int size, double sigma, float* out_host) {
    const int rc = gaussian_check("fdr_psf_gaussian", size, &sigma, out_host);
    if (rc != FDR_OK) return rc;
    const int c = size / 2;
    std::vector<double> g((size_t)size * size);
    double sum = 0.0;
    for (int i = 0; i < size; ++i)
        for (int j = 0; j < size; ++j) {
            const double y = i - c, x = j - c;
            sum += g[(size_t)i * size + j] = std::exp(-(y * y + x * x) / (2.0 * sigma * sigma));
        }
    for (size_t k = 0; k < g.size(); ++k) out_host[k] = (float)(g[k] / sum);
    return FDR_OK;
}

int fdr_psf_gaussian_dev(int device, int size, double sigma, float* d_out, void* stream) {
    const int rc = gaussian_check("fdr_psf_gaussian_dev", size, &sigma, d_out);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(device));
    FDR_HIP(launch_psf_gaussian(size, sigma, d_out, (hipStream_t)stream));
    return FDR_OK;
}

}  // extern "C"
