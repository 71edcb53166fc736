// fdr_api_tiled.hip -- sectioned restoration (fdr_tiled_layout_get, fdr_tiled_tile_origin, fdr_restore_tiled_f32*; kernels in
// fdr_tiled.hip): a picture of any size cut into overlapping tiles of one size, every tile restored on ONE tile plan as a crop of a
// larger scene by the free-boundary iteration of the chosen method (the drivers rlfree_batch_dev of fdr_api_rlfree.hip and
// tvfree_group_dev of fdr_api_tvfree.hip, on its window of the caller's picture, in place), with one PSF for all tiles or one per
// tile, and the tiles blended with a partition of unity.  Here: the geometry and the weight tables (host, integers and doubles), the
// checks, the workspace layout, the driver and the four entry points.  The bits of a tile are those of its single _dev call, so the
// scheduling is free: with one PSF and no weights the tiles of a tile row at the uniform pitch T - O are a batch of the plan's launch
// groups (their windows overlap in the caller's picture: the drivers only read them); otherwise the tiles run one by one.
#include "fdr_host.hpp"

#include <cmath>

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id.  A tile's own passes take up to 14 of the FDR_MAX_PASSES names (TV
// in launch groups), so the blend and the normalisation are recorded and the PSF roll, a few microseconds beside the PSF's transforms, is not
const char* const kPassTlBlend = "T blend: tiles -> picture";
const char* const kPassTlNorm = "E tiled minmax+normalize";

// one axis: a picture no longer than the tile is one tile of its own extent; otherwise n = ceil((extent - O) / (T - O)) tiles of T
// pixels, T - O apart, the last moved back to end at the edge.  0 <= O <= T / 2 (checked by the caller) keeps T - O >= 1.
TiledAxis tiled_axis(int extent, int T, int O) {
    if (extent <= T) return {1, extent, 0, 0};
    const int step = T - O;
    return {(int)(((long long)extent - O + step - 1) / step), T, step, extent - T};
}

struct TiledGeom {
    TiledAxis ar, ac;
    size_t tiles, tile_px;
};

// the tiling of a rows x cols picture, or FDR_ERR_ARG for what no tiling exists for
int tiled_geom(const char* fn, int rows, int cols, const fdr_tiled_params* prm, TiledGeom* g) {
    if (!prm) return null_arg(fn);
    if (rows < 1 || cols < 1) return fail(FDR_ERR_ARG, std::string(fn) + ": the picture must be at least 1 x 1");
    if (prm->tile_rows < 1 || prm->tile_cols < 1) return fail(FDR_ERR_ARG, std::string(fn) + ": the tile window must be at least 1 x 1");
    if (prm->overlap_rows < 0 || prm->overlap_cols < 0 || prm->overlap_rows > prm->tile_rows / 2 || prm->overlap_cols > prm->tile_cols / 2)
        return fail(FDR_ERR_ARG, std::string(fn) + ": the overlap must lie in [0 .. T / 2]");
    g->ar = tiled_axis(rows, prm->tile_rows, prm->overlap_rows);
    g->ac = tiled_axis(cols, prm->tile_cols, prm->overlap_cols);
    g->tiles = (size_t)g->ar.n * g->ac.n;
    g->tile_px = (size_t)g->ar.win * g->ac.win;
    return FDR_OK;
}

// h(s) = 0.5 - 0.5 cos(pi s) below 1, 1 from there on
double tiled_ramp(double s) { return s < 1.0 ? 0.5 - 0.5 * std::cos(M_PI * s) : 1.0; }

// the raw weight of tile a at its local position t: the rise against the real overlap with tile a - 1, times the fall against
// the real overlap with tile a + 1
double tiled_raw_weight(const TiledAxis& ax, int a, int t) {
    double w = 1.0;
    if (a > 0) {
        const int o = tiled_origin(ax, a - 1) + ax.win - tiled_origin(ax, a);
        if (o > 0) w *= tiled_ramp((t + 0.5) / o);
    }
    if (a + 1 < ax.n) {
        const int o = tiled_origin(ax, a) + ax.win - tiled_origin(ax, a + 1);
        if (o > 0) w *= tiled_ramp((ax.win - 1 - t + 0.5) / o);
    }
    return w;
}

// the table of one axis: for every position its first covering tile, their count and their normalised weights (double, rounded
// once); `padded` - extent entries of count 0 follow.  False when more than kTiledMaxCover tiles cover a position or none does,
// which O <= T / 2 rules out.
bool tiled_cover_table(const TiledAxis& ax, int extent, TiledCover* tab, int padded) {
    int a0 = 0;  // the first tile that still reaches y
    for (int y = 0; y < extent; ++y) {
        while (a0 < ax.n && tiled_origin(ax, a0) + ax.win <= y) ++a0;
        double raw[kTiledMaxCover], sum = 0.0;
        int n = 0;
        for (int a = a0; a < ax.n && tiled_origin(ax, a) <= y; ++a) {
            if (n == kTiledMaxCover) return false;
            raw[n] = tiled_raw_weight(ax, a, y - tiled_origin(ax, a));
            sum += raw[n++];
        }
        if (n == 0) return false;
        TiledCover c = {a0, n, {0.f, 0.f, 0.f}, {0, 0, 0}};
        for (int k = 0; k < n; ++k) c.w[k] = (float)(raw[k] / sum);
        tab[y] = c;
    }
    for (int y = extent; y < padded; ++y) tab[y] = TiledCover{0, 0, {0.f, 0.f, 0.f}, {0, 0, 0}};
    return true;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// the caller's workspace: the staging of every tile's window, the PSF plane of the tile plan, the row table and the column table
struct TiledWork {
    size_t stage, psf, tab, total;  // byte offsets, each a multiple of 256
};
TiledWork tiled_work(const TiledGeom& g, int rows, int cols, size_t M, size_t N) {
    TiledWork w;
    w.stage = 0;
    w.psf = align256(g.tiles * g.tile_px * sizeof(float));
    w.tab = w.psf + align256(M * N * sizeof(float));
    w.total = w.tab + align256(((size_t)rows + (((size_t)cols + 3) & ~(size_t)3)) * sizeof(TiledCover));
    return w;
}

int plan_dim(int need, int lo) {
    const int n = need > 8192 ? 8192 : fdr_next_pow2(need);
    return n < lo ? lo : n;
}

// rows of one band of the min-max over a picture wider or taller than the tile plan's partials hold (0: not even one row fits)
int norm_band_rows(const fdr_plan* p, int rows, int ld) {
    const long long per_row = ((long long)ld + 255) / 256;
    long long b = ((long long)p->mm_part_cap - 1) / per_row;
    if (b > 65535) b = 65535;
    return (int)(b < rows ? b : rows);
}

// Everything a tiled call refuses, before any device work; *g receives the tiling.  `work` null: the host form, which has no
// workspace of the caller's.
int tiled_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
                const float* psfs, size_t psf_pitch, int psf_count, int prows, int pcols, int pstride, const float* out, int out_stride,
                const fdr_tiled_params* prm, const void* work, size_t work_bytes, TiledGeom* g) {
    int rc = tiled_geom(fn, rows, cols, prm, g);
    if (rc != FDR_OK) return rc;
    if (prm->method != FDR_TILED_RL_FREE && prm->method != FDR_TILED_TV_FREE) return fail(FDR_ERR_ARG, std::string(fn) + ": unknown method");
    if (prm->norm_area == FDR_NORM_PADDED)
        return fail(FDR_ERR_ARG, std::string(fn) + ": FDR_NORM_PADDED has no meaning here (there is no single plan); FDR_NORM_NONE or FDR_NORM_CROPPED");
    if (stride < cols || out_stride < cols || (weights && wstride < cols))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the strides of the picture, the weights and the output must be >= cols");
    if (prows < 1 || pcols < 1 || pstride < pcols) return fail(FDR_ERR_ARG, std::string(fn) + ": bad PSF shape");
    // the tile's single call on tile (0, 0), its output the tile's staging (dense): plan, window, iterations, sigma or mu, rho, nu, norm_area
    const float* tile_out = work ? static_cast<const float*>(work) : out;
    if (prm->method == FDR_TILED_RL_FREE) {
        const fdr_rlfree_params one = {prm->iterations, prm->sigma, prm->norm_area, g->ar.win, g->ac.win};
        rc = rlfree_check(p, fn, img, g->ar.win, g->ac.win, stride, nullptr, 0, tile_out, work ? g->ac.win : out_stride, &one, NEED_OPERATOR);
        if (rc != FDR_OK) return rc;
    } else {
        rc = check_window(p, fn, NEED_OPERATOR, g->ar.win, g->ac.win, stride, out_stride);
        if (rc != FDR_OK) return rc;
        if (!std::isfinite(prm->mu) || !(prm->mu > 0.f)) return fail(FDR_ERR_ARG, std::string(fn) + ": mu must be finite and > 0");
        if (!std::isfinite(prm->rho) || !(prm->rho > 0.f)) return fail(FDR_ERR_ARG, std::string(fn) + ": rho must be finite and > 0");
        if (!std::isfinite(prm->nu) || prm->nu < 0.f) return fail(FDR_ERR_ARG, std::string(fn) + ": nu must be finite and >= 0");
        if (prm->iterations < 0) return fail(FDR_ERR_ARG, std::string(fn) + ": iterations < 0");
        if (prm->norm_area != FDR_NORM_NONE && prm->norm_area != FDR_NORM_CROPPED) return fail(FDR_ERR_ARG, std::string(fn) + ": unknown norm_area");
    }
    if ((long long)p->M < (long long)g->ar.win + prows - 1 || (long long)p->N < (long long)g->ac.win + pcols - 1)
        return fail(FDR_ERR_ARG, std::string(fn) + ": the tile plan must be at least (win_rows + prows - 1) x (win_cols + pcols - 1)");
    if (psf_count != 1 && (size_t)psf_count != g->tiles)
        return fail(FDR_ERR_ARG, std::string(fn) + ": psf_count must be 1 or tiles_r tiles_c");
    const size_t psf_span = (size_t)(prows - 1) * pstride + pcols;
    if (psf_count > 1 && psf_pitch < psf_span) return fail(FDR_ERR_ARG, std::string(fn) + ": psf_pitch is below the span of one PSF");
    if (prm->norm_area == FDR_NORM_CROPPED && norm_band_rows(p, rows, out_stride) < 1)
        return fail(FDR_ERR_ARG, std::string(fn) + ": out_stride is too large for the min-max of FDR_NORM_CROPPED on this tile plan");
    const ByteRange o = window_range(out, rows, cols, out_stride);
    if (ranges_overlap(o, window_range(img, rows, cols, stride))) return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the input");
    if (weights && ranges_overlap(o, window_range(weights, rows, cols, wstride)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the weights");
    const ByteRange ps = byte_range(psfs, ((size_t)(psf_count - 1) * psf_pitch + psf_span) * sizeof(float));
    if (ranges_overlap(o, ps)) return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the PSFs");
    if (work) {
        const size_t need = tiled_work(*g, rows, cols, (size_t)p->M, (size_t)p->N).total;
        if (work_bytes < need)
            return fail(FDR_ERR_ARG, std::string(fn) + ": work_bytes is below the " + std::to_string(need) + " bytes this call needs on this tile plan");
        if ((uintptr_t)work & 255) return fail(FDR_ERR_ARG, std::string(fn) + ": d_work must be 256-byte aligned");
        const ByteRange wr = byte_range(work, need);
        if (ranges_overlap(o, wr)) return fail(FDR_ERR_ARG, std::string(fn) + ": the output overlaps the workspace");
        if (ranges_overlap(wr, window_range(img, rows, cols, stride)) || ranges_overlap(wr, ps) ||
            (weights && ranges_overlap(wr, window_range(weights, rows, cols, wstride))))
            return fail(FDR_ERR_ARG, std::string(fn) + ": the workspace overlaps the input, the weights or the PSFs");
    }
    return FDR_OK;
}

// min-max of the blended picture to [0, 1] in place.  What fits the partials of the tile plan goes through normalize_window as
// every other call's FDR_NORM_CROPPED does; a larger picture is swept in bands of rows, the (min, max) so far carried along as one
// more partial: min and max do not round, so the scale and the shift are the same.
int tiled_normalize(fdr_plan* p, const char* fn, float* d_out, int rows, int cols, int out_stride, hipStream_t s) {
    const int band = norm_band_rows(p, rows, out_stride);
    if (band >= rows) return normalize_window(p, fn, kPassTlNorm, d_out, out_stride, rows, cols, FDR_NORM_CROPPED, d_out, out_stride, s);
    ScopedPass t(p, s, kPassTlNorm);
    const fdr_plan::Slot& w = p->slots[0];
    for (int y0 = 0; y0 < rows; y0 += band) {
        const int nr = rows - y0 < band ? rows - y0 : band;
        int n_part = 0;
        FDR_HIP(launch_minmax_real(d_out + (size_t)y0 * out_stride, nr, out_stride, nr, cols, w.mm_part, &n_part, s));
        if (y0 > 0) {
            FDR_HIP(hipMemcpyAsync(w.mm_part + n_part, w.mm, sizeof(float2), hipMemcpyDeviceToDevice, s));
            ++n_part;
        }
        FDR_HIP(launch_reduce_minmax(w.mm_part, n_part, w.mm, s));
    }
    FDR_HIP(launch_normalize(d_out, out_stride, nullptr, 0, w.mm, d_out, rows, cols, out_stride, s));
    return FDR_OK;
}

// the PSF of tile k centred in the plane, and the operator tables from the plane as from an M x N PSF
int tiled_set_psf(fdr_plan* p, const float* d_psf, int prows, int pcols, int pstride, float* plane, hipStream_t s) {
    FDR_HIP(launch_tiled_psf_centre(d_psf, prows, pcols, pstride, plane, p->M, p->N, s));
    return set_operator_psf_impl(p, plane, p->M, p->N, p->N, s);
}

// `count` tiles of one tile row, `pitch` pixels apart in the picture, into consecutive staging windows: the free-boundary driver of
// the method on the plan's launch groups (one tile: the single call)
int tiled_run_tiles(fdr_plan* p, const char* fn, const fdr_tiled_params& prm, const TiledGeom& g, const float* d_in, size_t pitch, int count,
                    int stride, const float* d_w, int wstride, float* d_stage, hipStream_t s) {
    const int wr = g.ar.win, wc = g.ac.win;
    if (prm.method == FDR_TILED_RL_FREE) {
        const fdr_rlfree_params one = {prm.iterations, prm.sigma, FDR_NORM_NONE, wr, wc};
        return rlfree_batch_dev(p, fn, d_in, pitch, count, wr, wc, stride, d_w, wstride, d_stage, g.tile_px, wc, one, s);
    }
    const fdr_tv_free_params one = {prm.mu, prm.rho, prm.nu, prm.iterations, prm.anisotropic, prm.nonneg, FDR_NORM_NONE, wr, wc};
    const int group = launch_group(p, count);
    int rc = FDR_OK;
    for (int i0 = 0; i0 < count && rc == FDR_OK; i0 += group) {
        const LaunchGroup lg(p, i0, count, d_in, pitch, d_stage, g.tile_px);
        rc = tvfree_group_dev(p, fn, lg.ws, lg.n, lg.ins, wr, wc, stride, d_w, wstride, lg.outs, wc, one, false, s);
    }
    return rc;
}

// the checked call: tables, workspaces of the method for the largest launch group, the tiles row by row, the blend, the normalisation
int tiled_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride,
                   const float* d_psfs, size_t psf_pitch, int psf_count, int prows, int pcols, int pstride, float* d_out, int out_stride,
                   const fdr_tiled_params& prm, const TiledGeom& g, void* d_work, hipStream_t s) {
    const TiledWork lay = tiled_work(g, rows, cols, (size_t)p->M, (size_t)p->N);
    char* base = static_cast<char*>(d_work);
    float* stage = reinterpret_cast<float*>(base + lay.stage);
    float* plane = reinterpret_cast<float*>(base + lay.psf);
    TiledCover* rtab = reinterpret_cast<TiledCover*>(base + lay.tab);
    TiledCover* ctab = rtab + rows;
    const int cols4 = (cols + 3) & ~3;
    // the tables, kept on the host in the plan while the upload may still read them
    p->tl_tab_host.resize((size_t)rows + cols4);
    if (!tiled_cover_table(g.ar, rows, p->tl_tab_host.data(), rows) || !tiled_cover_table(g.ac, cols, p->tl_tab_host.data() + rows, cols4))
        return fail(FDR_ERR_STATE, std::string(fn) + ": more than three tiles cover a pixel along an axis");
    // tiles of a row at the uniform pitch: a batch when they share the PSF and have no weights
    const bool batched = psf_count == 1 && !d_w;
    int uniform = 1;
    while (uniform < g.ac.n && (long long)uniform * g.ac.step <= g.ac.last) ++uniform;
    const int group = batched ? launch_group(p, uniform) : 1;
    int rc = prm.method == FDR_TILED_RL_FREE ? ensure_rlfree_workspace(p, fn, group) : tvfree_prepare(p, fn, group);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipMemcpyAsync(rtab, p->tl_tab_host.data(), p->tl_tab_host.size() * sizeof(TiledCover), hipMemcpyHostToDevice, s));
    if (psf_count == 1) rc = tiled_set_psf(p, d_psfs, prows, pcols, pstride, plane, s);
    for (int a = 0; a < g.ar.n && rc == FDR_OK; ++a) {
        const int ya = tiled_origin(g.ar, a);
        const float* in_row = d_img + (size_t)ya * stride;
        float* st_row = stage + (size_t)a * g.ac.n * g.tile_px;
        if (batched) {
            rc = tiled_run_tiles(p, fn, prm, g, in_row, (size_t)g.ac.step, uniform, stride, nullptr, 0, st_row, s);
            if (rc == FDR_OK && uniform < g.ac.n)  // the last tile, moved back to end at the edge
                rc = tiled_run_tiles(p, fn, prm, g, in_row + g.ac.last, 0, 1, stride, nullptr, 0, st_row + (size_t)uniform * g.tile_px, s);
            continue;
        }
        for (int b = 0; b < g.ac.n && rc == FDR_OK; ++b) {
            const int xb = tiled_origin(g.ac, b);
            if (psf_count > 1) rc = tiled_set_psf(p, d_psfs + ((size_t)a * g.ac.n + b) * psf_pitch, prows, pcols, pstride, plane, s);
            if (rc == FDR_OK)
                rc = tiled_run_tiles(p, fn, prm, g, in_row + xb, 0, 1, stride, d_w ? d_w + (size_t)ya * wstride + xb : nullptr, wstride,
                                     st_row + (size_t)b * g.tile_px, s);
        }
    }
    if (rc != FDR_OK) return rc;
    {
        ScopedPass t(p, s, kPassTlBlend);
        FDR_HIP(launch_tiled_blend(stage, rtab, ctab, g.ar, g.ac, d_out, rows, cols, out_stride, s));
    }
    if (prm.norm_area == FDR_NORM_CROPPED) rc = tiled_normalize(p, fn, d_out, rows, cols, out_stride, s);
    return rc;
}

}  // namespace

extern "C" {

int fdr_tiled_layout_get(int rows, int cols, int prows, int pcols, const fdr_tiled_params* params, fdr_tiled_layout* layout) {
    const char* fn = "fdr_tiled_layout_get";
    if (!layout) return null_arg(fn);
    TiledGeom g;
    const int rc = tiled_geom(fn, rows, cols, params, &g);
    if (rc != FDR_OK) return rc;
    if (prows < 1 || pcols < 1) return fail(FDR_ERR_ARG, std::string(fn) + ": bad PSF shape");
    layout->tiles_r = g.ar.n; layout->tiles_c = g.ac.n;
    layout->win_rows = g.ar.win; layout->win_cols = g.ac.win;
    const long long need_m = (long long)g.ar.win + prows - 1, need_n = (long long)g.ac.win + pcols - 1;
    layout->min_M = plan_dim(need_m > 8192 ? 8192 : (int)need_m, 8);
    layout->min_N = plan_dim(need_n > 8192 ? 8192 : (int)need_n, 32);
    layout->work_bytes = tiled_work(g, rows, cols, (size_t)layout->min_M, (size_t)layout->min_N).total;
    return FDR_OK;
}

int fdr_tiled_tile_origin(int rows, int cols, const fdr_tiled_params* params, int a, int b, int* y, int* x) {
    const char* fn = "fdr_tiled_tile_origin";
    if (!y || !x) return null_arg(fn);
    TiledGeom g;
    const int rc = tiled_geom(fn, rows, cols, params, &g);
    if (rc != FDR_OK) return rc;
    if (a < 0 || a >= g.ar.n || b < 0 || b >= g.ac.n) return fail(FDR_ERR_ARG, std::string(fn) + ": no such tile");
    *y = tiled_origin(g.ar, a);
    *x = tiled_origin(g.ac, b);
    return FDR_OK;
}

int fdr_restore_tiled_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_weights, int wstride,
                              const float* d_psfs, size_t psf_pitch, int psf_count, int prows, int pcols, int pstride, float* d_out,
                              int out_stride, const fdr_tiled_params* params, void* d_work, size_t work_bytes, void* stream) {
    const char* fn = "fdr_restore_tiled_f32_dev";
    if (!p || !d_img || !d_psfs || !d_out || !d_work) return null_arg(fn);
    TiledGeom g;
    const int rc = tiled_check(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_psfs, psf_pitch, psf_count, prows, pcols, pstride, d_out,
                               out_stride, params, d_work, work_bytes, &g);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return tiled_dev_impl(p, fn, d_img, rows, cols, stride, d_weights, wstride, d_psfs, psf_pitch, psf_count, prows, pcols, pstride, d_out,
                          out_stride, *params, g, d_work, (hipStream_t)stream);
}

int fdr_restore_tiled_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const float* weights_host, int wstride,
                          const float* psfs_host, size_t psf_pitch, int psf_count, int prows, int pcols, int pstride, float* out_host,
                          int out_stride, const fdr_tiled_params* params) {
    const char* fn = "fdr_restore_tiled_f32";
    if (!p || !img_host || !psfs_host || !out_host) return null_arg(fn);
    TiledGeom g;
    int rc = tiled_check(p, fn, img_host, rows, cols, stride, weights_host, wstride, psfs_host, psf_pitch, psf_count, prows, pcols, pstride,
                         out_host, out_stride, params, nullptr, 0, &g);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    // everything dense on the device, for this call alone
    const size_t px = (size_t)rows * cols, ppx = (size_t)prows * pcols;
    const size_t row_bytes = (size_t)cols * sizeof(float);
    DeviceBuffer d_in, d_out, d_w, d_psf, d_work;
    FDR_ALLOC(d_in, px * sizeof(float), fn);
    FDR_ALLOC(d_out, px * sizeof(float), fn);
    if (weights_host) FDR_ALLOC(d_w, px * sizeof(float), fn);
    FDR_ALLOC(d_psf, (size_t)psf_count * ppx * sizeof(float), fn);
    FDR_ALLOC(d_work, tiled_work(g, rows, cols, (size_t)p->M, (size_t)p->N).total, fn);
    {
        ScopedPhase phase(p, FDR_PHASE_H2D, nullptr);
        FDR_HIP(hipMemcpy2D(d_in.ptr, row_bytes, img_host, (size_t)stride * sizeof(float), row_bytes, (size_t)rows, hipMemcpyHostToDevice));
        if (weights_host)
            FDR_HIP(hipMemcpy2D(d_w.ptr, row_bytes, weights_host, (size_t)wstride * sizeof(float), row_bytes, (size_t)rows, hipMemcpyHostToDevice));
        for (int k = 0; k < psf_count; ++k)
            FDR_HIP(hipMemcpy2D(d_psf.as<float>() + (size_t)k * ppx, (size_t)pcols * sizeof(float), psfs_host + (size_t)k * psf_pitch,
                                (size_t)pstride * sizeof(float), (size_t)pcols * sizeof(float), (size_t)prows, hipMemcpyHostToDevice));
    }
    {
        ScopedPhase phase(p, FDR_PHASE_COMPUTE, nullptr);
        rc = tiled_dev_impl(p, fn, d_in.as<float>(), rows, cols, cols, d_w.as<float>(), cols, d_psf.as<float>(), ppx, psf_count, prows, pcols, pcols,
                            d_out.as<float>(), cols, *params, g, d_work.ptr, nullptr);
    }
    if (rc == FDR_OK) {
        ScopedPhase phase(p, FDR_PHASE_D2H, nullptr);
        FDR_HIP(hipMemcpy2D(out_host, (size_t)out_stride * sizeof(float), d_out.ptr, row_bytes, row_bytes, (size_t)rows, hipMemcpyDeviceToHost));
    }
    (void)hipStreamSynchronize(nullptr);  // (also on an error: the one-shot buffers are freed on return)
    resolve_phases(p);
    return rc;
}

}  // extern "C"
