// fdr_api_plan.hip -- plans of libfdr.so: twiddle tables, create / destroy / dims / options / batching, profiling and phase
// times, and what the entry points share: the checks, the PSF path and the host-pointer forms of a single-image call and of a TV
// batch (with its first refusals and the staging of a crop call's weights).  The host files
// (fdr_api_*.hip) use only the HIP runtime -- no torch, no OpenCV -- and there is deliberately NO CPU fallback in them: every
// entry point either launches HIP kernels or fails.
#include "fdr_host.hpp"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

using namespace fdr;

namespace fdr {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int null_arg(const char* fn) { return fail(FDR_ERR_ARG, std::string(fn) + ": null argument"); }

int ilog2(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

// Per-stage twiddle table for transforms of length n: stage len = 2,4,..,n at offset len/2-1.
// parity: replay of fft/fft_serial.cpp:54-63 -- ang evaluated in double and rounded to float,
//         wlen = (cosf(ang), sinf(ang)), w advanced by the float recurrence w *= wlen.
// fast  : exp(-+2 pi i k / len) evaluated in double (as fft/fft_gpu.cu:206-212), rounded once.
void build_twiddles(int n, int mode, bool inverse, std::vector<float2>& out) {
    out.assign(n > 1 ? (size_t)n - 1 : 1, make_float2(1.f, 0.f));
    const double PI = 3.1415926535897932384626433832795;  // CV_PI
    for (int len = 2; len <= n; len <<= 1) {
        float2* t = out.data() + (len / 2 - 1);
        if (mode == FDR_MODE_PARITY) {
            const float ang = (float)((double)2.0f * PI / (double)len * (double)(inverse ? 1.0f : -1.0f));
            const float wlr = cosf(ang), wli = sinf(ang);
            float wr = 1.0f, wi = 0.0f;
            for (int k = 0; k < len / 2; ++k) {
                t[k] = make_float2(wr, wi);
                const float ac = wr * wlr, bd = wi * wli, ad = wr * wli, bc = wi * wlr;
                wr = ac - bd;
                wi = ad + bc;
            }
        } else {
            for (int k = 0; k < len / 2; ++k) {
                const double a = (inverse ? 2.0 : -2.0) * PI * (double)k / (double)len;
                t[k] = make_float2((float)cos(a), (float)sin(a));
            }
        }
    }
}

// n x n twiddle table of fft_serial::dft_naive_inplace (fft/fft_serial.cpp:71-87), forward direction, laid out
// [t][k] so that adjacent threads (adjacent k) read adjacent entries: ang = 2.0f * CV_PI * k * t / n * sign evaluated left
// to right in double, rounded to float, then the C library's cosf / sinf -- the calls the serial path makes.
void build_naive_table(int n, std::vector<float2>& out) {
    out.resize((size_t)n * n);
    const double PI = 3.1415926535897932384626433832795;
    for (int k = 0; k < n; ++k)
        for (int t = 0; t < n; ++t) {
            const float ang = (float)((double)2.0f * PI * (double)k * (double)t / (double)n * (double)-1.0f);
            out[(size_t)t * n + k] = make_float2(cosf(ang), sinf(ang));
        }
}

void resolve_finished_phases(fdr_plan* p) {
    size_t keep = 0;
    for (auto& r : p->phase_pending) {
        float ms = 0.f;
        if (hipEventQuery(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            p->phase_ms[r.phase] += ms;
            p->timer.pool.push_back(r.a); p->timer.pool.push_back(r.b);
        } else {
            p->phase_pending[keep++] = r;
        }
    }
    p->phase_pending.resize(keep);
}

void resolve_phases(fdr_plan* p) {
    for (auto& r : p->phase_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) p->phase_ms[r.phase] += ms;
        p->timer.pool.push_back(r.a); p->timer.pool.push_back(r.b);
    }
    p->phase_pending.clear();
}

int check_plan(const fdr_plan* p, const char* fn, PlanNeed need) {
    if (p->tables_only) return fail(FDR_ERR_STATE, std::string(fn) + ": plan was created with FDR_FLAG_TABLES_ONLY (slab primitives only)");
    if (need == NEED_FILTER && !p->have_psf) return fail(FDR_ERR_STATE, std::string(fn) + ": no PSF set on this plan (call fdr_set_psf* first)");
    // (layout_radix2 gives PATH_FAST_HALF only to fast mode with 8 <= M, N <= 8192, both powers of two, and N >= 32: the
    // ranges of the message follow from the path)
    if ((need == NEED_OPERATOR || need == NEED_OPERATOR_PSF) && p->path != PATH_FAST_HALF)
        return fail(FDR_ERR_ARG, std::string(fn) + ": needs a FDR_MODE_FAST plan on the half-spectrum panel path (M, N powers of two, "
                                                   "8 <= M <= 8192, 32 <= N <= 8192, neither FDR_FLAG_SIMPLE_PATH nor FDR_FLAG_FULL_SPECTRUM)");
    if (need == NEED_OPERATOR_PSF && !p->have_op)
        return fail(FDR_ERR_STATE, std::string(fn) + ": no operator PSF set on this plan (call fdr_set_operator_psf* first)");
    if (need == NEED_MOTION && (p->mode != FDR_MODE_FAST || p->generic || p->M < 32 || p->N < 32 || p->M > kMixMaxLen || p->N > kMixMaxLen ||
                                !(p->path == PATH_MIXED || (fdr_is_pow2(p->M) && fdr_is_pow2(p->N)))))
        return fail(FDR_ERR_ARG, std::string(fn) + ": needs a FDR_MODE_FAST plan, M and N powers of two (or 2^a 3^b 5^c with "
                                                   "FDR_FLAG_MIXED_RADIX), 32 <= M, N <= 8192");
    return FDR_OK;
}

int check_window(const fdr_plan* p, const char* fn, PlanNeed need, int rows, int cols, int stride, int out_stride, int min) {
    const int rc = check_plan(p, fn, need);
    if (rc != FDR_OK) return rc;
    if (rows < min || cols < min || rows > p->M || cols > p->N || stride < cols || out_stride < cols)
        return fail(FDR_ERR_ARG, std::string(fn) + ": the image window must be at least " + std::to_string(min) + " x " + std::to_string(min) +
                                     ", fit the plan and have strides >= cols");
    return FDR_OK;
}

}  // namespace fdr

namespace {

std::atomic<bool> g_process_exiting{false};  // set by an atexit handler that runs before the HIP runtime's own (fdr_plan_destroy)

static_assert(sizeof(MixTwiddle) == sizeof(float2) && sizeof(MixStage) == sizeof(int4), "fdr_mixed_plan.hpp: the kernels read float2 / int4");

int upload(float2** dst, const std::vector<float2>& v) {
    FDR_HIP(hipMalloc((void**)dst, v.size() * sizeof(float2)));
    FDR_HIP(hipMemcpy(*dst, v.data(), v.size() * sizeof(float2), hipMemcpyHostToDevice));
    return FDR_OK;
}

// the buffers of one workspace slot: work and raw (and work2 on the simple path) unless the plan is tables-only, then the min/max
// pair and partials -- mm_part last, so a slot that has it has all its buffers
int alloc_slot(const fdr_plan* p, fdr_plan::Slot& w) {
    const bool ws = !p->tables_only;
    if ((ws && hipMalloc((void**)&w.work, p->ws_elems * sizeof(float2)) != hipSuccess) ||
        (ws && hipMalloc((void**)&w.raw, (size_t)p->M * p->N * sizeof(float)) != hipSuccess) ||
        (ws && p->path == PATH_SIMPLE && hipMalloc((void**)&w.work2, p->ws_elems * sizeof(float2)) != hipSuccess) ||
        hipMalloc((void**)&w.mm, 2 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&w.mm_part, (size_t)p->mm_part_cap * sizeof(float2)) != hipSuccess)
        return FDR_ERR_ALLOC;
    return FDR_OK;
}

void release_slot(fdr_plan::Slot& w) {
    (void)hipFree(w.work); (void)hipFree(w.work2); (void)hipFree(w.raw); (void)hipFree(w.mm); (void)hipFree(w.mm_part);
    if (w.stream) (void)hipStreamDestroy(w.stream);
    if (w.done) (void)hipEventDestroy(w.done);
}

// power-of-two plans (and FDR_FLAG_ANY_SIZE ones): the path, the layout of the intermediate spectrum, the naive-DFT tables
int layout_radix2(fdr_plan* p, std::vector<float2>& t) {
    const int M = p->M, N = p->N;
    // dimensions above 8192 (one row no longer fits the LDS): the reference-shaped sequence rows / transpose / rows / transpose
    // with the long row pass (fdr_simple.hip, long_gather_kernel) -- as the serial path, correct at any power of two and slower
    const bool simple = p->generic || (p->flags & FDR_FLAG_SIMPLE_PATH) != 0 || M < 8 || N < 8 || M > (1 << kMaxLdsLog) || N > (1 << kMaxLdsLog);
    const bool half = N >= 32 && (p->flags & FDR_FLAG_FULL_SPECTRUM) == 0;
    p->path = simple ? PATH_SIMPLE : p->mode == FDR_MODE_PARITY ? PATH_PARITY_PANEL : half ? PATH_FAST_HALF : PATH_FAST_FULL;
    p->big = (fdr_is_pow2(M) && M > (1 << kMaxLdsLog)) || (fdr_is_pow2(N) && N > (1 << kMaxLdsLog));
    if (simple) {
        p->ws_elems = (size_t)M * N;
    } else {
        // panel-major buffers: panels of 4 columns, PS elements apart (not a power of two: channel skew).
        // The bit-identical mode keeps the reference's pass order and full complex spectrum, but its intermediate is panel-major
        // too (all N/4 panels): the column passes B and D read and write contiguous M x 32-byte tiles instead of 32 bytes of
        // every row; A and C reach their 32-byte pieces through an XCD-aware workgroup order (fdr_rows.hip); the raw real plane
        // is panel-major as well and normalize_panels_kernel turns it back (LAB_NOTES "parity mode layout").  Same
        // butterflies, same tables, same bits (every parity test compares with ==).
        p->pstride = (size_t)M * 4 + 16;
        p->npanels = p->path == PATH_FAST_HALF ? N / 8 : N / 4;
        p->ws_elems = (size_t)p->npanels * p->pstride;
    }
    int rc = FDR_OK;
    if (!fdr_is_pow2(N)) {
        build_naive_table(N, t);
        if ((rc = upload(&p->naive_row, t)) != FDR_OK) return rc;
    }
    if (fdr_is_pow2(M)) return FDR_OK;
    if (M == N) {
        p->naive_col = p->naive_row;
        return FDR_OK;
    }
    build_naive_table(M, t);
    return upload(&p->naive_col, t);
}

// FDR_FLAG_MIXED_RADIX: both lengths' tables, panel width P and row-pass transforms per workgroup B (fdr_mixed_plan.hpp)
int layout_mixed(fdr_plan* p, std::vector<float2>& t) {
    const int M = p->M, N = p->N;
    p->path = PATH_MIXED;
    std::vector<MixTwiddle> tw;
    std::vector<MixStage> st;
    for (int d = 0; d < 2; ++d) {
        const int L = d == 0 ? N : M;
        MixLen& ml = d == 0 ? p->mix_row : p->mix_col;
        if (d == 1 && M == N) { ml = p->mix_row; break; }
        build_mixed_tables(L, tw, st);
        t.resize(tw.size());
        std::memcpy(t.data(), tw.data(), tw.size() * sizeof(float2));
        const int rc = upload(const_cast<float2**>(&ml.tw), t);
        if (rc != FDR_OK) return rc;
        int4* dst = nullptr;
        FDR_HIP(hipMalloc((void**)&dst, (st.empty() ? 1 : st.size()) * sizeof(int4)));
        ml.st = dst;
        if (!st.empty()) FDR_HIP(hipMemcpy(dst, st.data(), st.size() * sizeof(int4), hipMemcpyHostToDevice));
        ml.L = L; ml.nst = (int)st.size(); ml.nt = mixed_threads(L);
    }
    const MixLayout lay = mixed_layout(M, N);
    p->mix_logP = lay.logP;
    p->mix_P = 1 << lay.logP;
    p->mix_B = lay.B;
    p->pstride = (size_t)M * p->mix_P;
    p->npanels = N / p->mix_P;
    p->ws_elems = (size_t)p->npanels * p->pstride;
    return FDR_OK;
}

int plan_create_impl(fdr_plan* p, int device, int M, int N, int mode, unsigned flags) {
    const bool pow2 = fdr_is_pow2(M) && fdr_is_pow2(N);
    p->device = device; p->M = M; p->N = N; p->flags = flags;
    const bool mixed = !pow2 && mode == FDR_MODE_FAST && (flags & FDR_FLAG_MIXED_RADIX) != 0;
    p->generic = !pow2 && !mixed;  // only reachable with FDR_FLAG_ANY_SIZE: reference-shaped passes, parity arithmetic
    p->mode = p->generic ? FDR_MODE_PARITY : mode;
    p->tables_only = (flags & FDR_FLAG_TABLES_ONLY) != 0;
    p->logM = fdr_is_pow2(M) ? ilog2(M) : -1;
    p->logN = fdr_is_pow2(N) ? ilog2(N) : -1;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) p->num_cu = cus;
    p->mm_part_cap = (int)(((size_t)N + 255) / 256 * M + 8192);
    // the power-of-two tables of the plan's mode (a mixed-radix plan keeps those of a power-of-two dimension for the slab primitives)
    std::vector<float2> t;
    int rc = FDR_OK;
    if (fdr_is_pow2(N)) {
        build_twiddles(N, p->mode, false, t); if ((rc = upload(&p->tw_row_f, t)) != FDR_OK) return rc;
        build_twiddles(N, p->mode, true, t);  if ((rc = upload(&p->tw_row_i, t)) != FDR_OK) return rc;
    }
    if (fdr_is_pow2(M)) {
        build_twiddles(M, p->mode, false, t); if ((rc = upload(&p->tw_col_f, t)) != FDR_OK) return rc;
        build_twiddles(M, p->mode, true, t);  if ((rc = upload(&p->tw_col_i, t)) != FDR_OK) return rc;
    }
    rc = mixed ? layout_mixed(p, t) : layout_radix2(p, t);  // (each sets p->path)
    if (rc != FDR_OK) return rc;
    if ((!p->tables_only && hipMalloc((void**)&p->filt, p->ws_elems * sizeof(float2)) != hipSuccess) || alloc_slot(p, p->slots[0]) != FDR_OK)
        return fail(FDR_ERR_ALLOC, "fdr_plan_create: hipMalloc of the plan workspace failed");
    return FDR_OK;
}

// the Wiener / CLS target of set_psf: gamma finite and >= 0, a plan with workspaces, and gamma > 0 only on a fast-mode plan
// (parity mode exists to be bit-identical to ./serial, which has no CLS)
int filter_check(const fdr_plan* p, const char* fn, float gamma) {
    if (!(gamma >= 0.f) || std::isinf(gamma)) return fail(FDR_ERR_ARG, std::string(fn) + ": gamma must be finite and >= 0");
    const int rc = check_plan(p, fn, NEED_PLAN);
    if (rc != FDR_OK) return rc;
    if (gamma > 0.f && p->mode != FDR_MODE_FAST)
        return fail(FDR_ERR_ARG, std::string(fn) + ": a constrained least-squares filter (gamma > 0) needs a FDR_MODE_FAST plan; "
                                                   "parity mode (and every FDR_FLAG_ANY_SIZE plan) has the Wiener filter only");
    return FDR_OK;
}

int ensure_psf_staging(fdr_plan* p, size_t elems) {
    if (p->psf_cap >= elems) return FDR_OK;
    if (p->psf_dev) { (void)hipFree(p->psf_dev); p->psf_dev = nullptr; p->psf_cap = 0; }
    FDR_HIP(hipMalloc((void**)&p->psf_dev, elems * sizeof(float)));
    p->psf_cap = elems;
    return FDR_OK;
}

// rows x cols floats between host and device: one linear copy when both sides are dense (the 2-D form of a pageable buffer goes
// row by row, several times slower; LAB_NOTES "host-pointer calls")
hipError_t copy_window(float* dst, int dst_stride, const float* src, int src_stride, int rows, int cols, hipMemcpyKind kind) {
    if (dst_stride == cols && src_stride == cols) return hipMemcpy(dst, src, (size_t)rows * cols * sizeof(float), kind);
    return hipMemcpy2D(dst, (size_t)dst_stride * sizeof(float), src, (size_t)src_stride * sizeof(float), (size_t)cols * sizeof(float), rows,
                       kind);
}

}  // namespace

namespace fdr {

int set_psf(fdr_plan* p, const char* fn, const PsfSource& src, bool op, float K, float gamma, hipStream_t s) {
    if (!p || ((src.kind == PSF_DEV || src.kind == PSF_HOST) && !src.ptr)) return null_arg(fn);
    int rc = op ? check_plan(p, fn, NEED_OPERATOR) : filter_check(p, fn, gamma);
    if (rc != FDR_OK) return rc;
    if (src.rows <= 0 || src.cols <= 0 || src.stride < src.cols) return fail(FDR_ERR_ARG, std::string(fn) + ": bad PSF shape");
    if (src.rows > p->M || src.cols > p->N)
        return fail(FDR_ERR_ARG, std::string(fn) + ": PSF larger than the padded image (copyMakeBorder would throw, fft_serial.cpp:168)");
    FDR_HIP(hipSetDevice(p->device));
    const float* d_psf = src.ptr;
    int stride = src.stride;
    if (src.kind != PSF_DEV) {  // into the plan's PSF staging, dense
        rc = ensure_psf_staging(p, (size_t)src.rows * src.cols);
        if (rc != FDR_OK) return rc;
        d_psf = p->psf_dev;
        stride = src.cols;
        if (src.kind == PSF_MOTION) {
            FDR_HIP(launch_psf_motion(src.rows, src.angle_deg, p->psf_dev, s));
        } else if (src.kind == PSF_DISK) {
            FDR_HIP(launch_psf_disk(src.rows, src.angle_deg, p->psf_dev, s));
        } else {
            ScopedPhase ph(p, FDR_PHASE_H2D, nullptr);
            FDR_HIP(hipMemcpy2D(p->psf_dev, (size_t)src.cols * sizeof(float), src.ptr, (size_t)src.stride * sizeof(float),
                                (size_t)src.cols * sizeof(float), src.rows, hipMemcpyHostToDevice));
        }
    }
    rc = op ? set_operator_psf_impl(p, d_psf, src.rows, src.cols, stride, s) : set_psf_dev_impl(p, d_psf, src.rows, src.cols, stride, K, s, gamma);
    if (rc != FDR_OK || src.kind != PSF_HOST) return rc;
    FDR_HIP(hipStreamSynchronize(nullptr));
    resolve_phases(p);
    return FDR_OK;
}

int host_image_call(fdr_plan* p, const char* fn, const float* in, int rows, int cols, int stride, float* out, int out_rows, int out_cols,
                    int out_stride, const std::function<int(const float* d_in, float* d_out)>& run) {
    if (!p->stage_in) {  // two M x N float buffers, made on first use and kept (the per-channel loop of the drivers calls this three
                         // times; the reference's _optimized version hoists its buffers the same way, fft/fft_gpu.cu:304-322)
        const size_t cap = (size_t)p->M * p->N * sizeof(float);
        if (hipMalloc((void**)&p->stage_in, cap) != hipSuccess || hipMalloc((void**)&p->stage_out, cap) != hipSuccess) {
            (void)hipFree(p->stage_in); p->stage_in = nullptr;
            return fail(FDR_ERR_ALLOC, std::string(fn) + ": hipMalloc of the staging buffers failed");
        }
    }
    int rc = FDR_OK;
    hipError_t e;
    {
        ScopedPhase ph(p, FDR_PHASE_H2D, nullptr);
        e = copy_window(p->stage_in, cols, in, stride, rows, cols, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        ScopedPhase ph(p, FDR_PHASE_COMPUTE, nullptr);
        rc = run(p->stage_in, p->stage_out);
    }
    if (e == hipSuccess && rc == FDR_OK && out) {
        ScopedPhase ph(p, FDR_PHASE_D2H, nullptr);
        e = copy_window(out, out_stride, p->stage_out, out_cols, out_rows, out_cols, hipMemcpyDeviceToHost);
    }
    if (e == hipSuccess) resolve_phases(p);
    if (rc != FDR_OK) return rc;
    FDR_HIP(e);
    return FDR_OK;
}

// the dense copy of the host weights for one call (no plane of the workspace is free over the whole iteration)
int stage_crop_weights(const char* fn, const float* weights_host, int rows, int cols, int wstride, DeviceBuffer* d_w) {
    if (!weights_host) return FDR_OK;
    FDR_ALLOC(*d_w, (size_t)rows * cols * sizeof(float), fn);
    FDR_HIP(hipMemcpy2D(d_w->ptr, (size_t)cols * sizeof(float), weights_host, (size_t)wstride * sizeof(float), (size_t)cols * sizeof(float),
                        (size_t)rows, hipMemcpyHostToDevice));
    return FDR_OK;
}

bool tv_batch_begin(const char* fn, const void* p, const void* params, int count, const void* imgs, const void* out, int* rc) {
    if (!p || !params) *rc = null_arg(fn);
    else if (count < 0) *rc = fail(FDR_ERR_ARG, std::string(fn) + ": negative count");
    else if (count == 0) *rc = FDR_OK;
    else if (!imgs || !out) *rc = null_arg(fn);
    else return true;
    return false;
}

// host pointers: every image in (dense), `run` on the dense device batch on the null stream, every output window back; one-shot
// device buffers
int host_batch_call(fdr_plan* p, const char* fn, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride, float* out_host,
                    size_t out_pitch, int out_stride, int out_rows, int out_cols, const HostBatchRun& run) {
    const size_t px = (size_t)rows * cols, opx = (size_t)out_rows * out_cols;
    DeviceBuffer d_in, d_out;
    FDR_ALLOC(d_in, (size_t)count * px * sizeof(float), fn);
    FDR_ALLOC(d_out, (size_t)count * opx * sizeof(float), fn);
    int rc = FDR_OK;
    {
        ScopedPhase phase(p, FDR_PHASE_H2D, nullptr);
        for (int i = 0; i < count; ++i)
            FDR_HIP(hipMemcpy2D(d_in.as<float>() + (size_t)i * px, (size_t)cols * sizeof(float), imgs_host + (size_t)i * img_pitch,
                                (size_t)stride * sizeof(float), (size_t)cols * sizeof(float), (size_t)rows, hipMemcpyHostToDevice));
    }
    {
        ScopedPhase phase(p, FDR_PHASE_COMPUTE, nullptr);
        rc = run(d_in.as<float>(), px, d_out.as<float>(), opx);
    }
    if (rc == FDR_OK) {
        ScopedPhase phase(p, FDR_PHASE_D2H, nullptr);
        for (int i = 0; i < count; ++i)
            FDR_HIP(hipMemcpy2D(out_host + (size_t)i * out_pitch, (size_t)out_stride * sizeof(float), d_out.as<float>() + (size_t)i * opx,
                                (size_t)out_cols * sizeof(float), (size_t)out_cols * sizeof(float), (size_t)out_rows, hipMemcpyDeviceToHost));
    }
    (void)hipStreamSynchronize(nullptr);  // (also on an error: the one-shot buffers are freed on return)
    resolve_phases(p);
    return rc;
}

}  // namespace fdr

extern "C" {

int fdr_version(void) { return FDR_VERSION; }
const char* fdr_last_error(void) { return g_last_error.c_str(); }

int fdr_device_count(int* count) {
    if (!count) return fail(FDR_ERR_ARG, "fdr_device_count: null");
    FDR_HIP(hipGetDeviceCount(count));
    return FDR_OK;
}

int fdr_next_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }  // utils.hpp:27-37
int fdr_is_pow2(int n) { return n > 0 && ((n & (n - 1)) == 0); }           // utils.hpp:50-52

// cv::getOptimalDFTSize as the serial path uses it (fft/fft_serial.cpp:153-154): smallest 2^a 3^b 5^c >= n
int fdr_optimal_dft_size(int n) {
    if (n <= 1) return n < 0 ? -1 : 1;
    for (long long best = -1, p2 = 1; p2 < 2LL * n; p2 *= 2) {
        for (long long p3 = p2; p3 < 2LL * n; p3 *= 3)
            for (long long p5 = p3; p5 < 2LL * n; p5 *= 5)
                if (p5 >= n && (best < 0 || p5 < best)) best = p5;
        if (p2 * 2 >= 2LL * n) return (int)best;
    }
    return -1;
}

int fdr_plan_create(int device, int M, int N, int mode, unsigned flags, fdr_plan** out) {
    if (!out) return fail(FDR_ERR_ARG, "fdr_plan_create: null out");
    *out = nullptr;
    if (M <= 0 || N <= 0) return fail(FDR_ERR_ARG, "fdr_plan_create: non-positive dimension");
    if (mode != FDR_MODE_PARITY && mode != FDR_MODE_FAST) return fail(FDR_ERR_ARG, "fdr_plan_create: unknown mode");
    const bool mixed = mode == FDR_MODE_FAST && (flags & FDR_FLAG_MIXED_RADIX) != 0 && !(fdr_is_pow2(M) && fdr_is_pow2(N));
    if (mixed) {
        if (!is_smooth(M) || !is_smooth(N) || M > kMixMaxLen || N > kMixMaxLen)
            return fail(FDR_ERR_ARG, "fdr_plan_create: FDR_FLAG_MIXED_RADIX takes dimensions 2^a 3^b 5^c up to 8192 "
                                     "(pad each to fdr_optimal_dft_size(n))");
        if ((flags & (FDR_FLAG_TABLES_ONLY | FDR_FLAG_SIMPLE_PATH)) != 0)
            return fail(FDR_ERR_ARG, "fdr_plan_create: FDR_FLAG_MIXED_RADIX does not combine with FDR_FLAG_TABLES_ONLY or FDR_FLAG_SIMPLE_PATH");
    } else if (!fdr_is_pow2(M) || !fdr_is_pow2(N)) {
        if ((flags & FDR_FLAG_ANY_SIZE) == 0)
            return fail(FDR_ERR_NOT_POW2, "fdr_plan_create: M and N must be powers of two (pad first, utils.hpp:40-47) unless FDR_FLAG_ANY_SIZE is set");
        if ((!fdr_is_pow2(M) && M > kMaxNaiveLen) || (!fdr_is_pow2(N) && N > kMaxNaiveLen))
            return fail(FDR_ERR_ARG, "fdr_plan_create: non-power-of-two dimension above 4096 (naive-DFT twiddle table)");
    }
    if (M > (1 << kMaxLongLog) || N > (1 << kMaxLongLog))
        return fail(FDR_ERR_ARG, "fdr_plan_create: dimension above 32768");
    FDR_HIP(hipSetDevice(device));
    // registered behind the first HIP call, i.e. after the HIP runtime's own exit handlers: it runs BEFORE them
    static std::once_flag exit_hook;
    std::call_once(exit_hook, [] { std::atexit([] { g_process_exiting.store(true); }); });
    const auto t0 = std::chrono::steady_clock::now();
    fdr_plan* p = new (std::nothrow) fdr_plan();
    if (!p) return fail(FDR_ERR_ALLOC, "fdr_plan_create: out of host memory");
    const int rc = plan_create_impl(p, device, M, N, mode, flags);
    if (rc != FDR_OK) {
        const std::string msg = g_last_error;  // fdr_plan_destroy does not touch it, but keep the first failure's text
        fdr_plan_destroy(p);
        g_last_error = msg;
        return rc;
    }
    p->phase_ms[FDR_PHASE_ALLOC] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = p;
    return FDR_OK;
}

int fdr_plan_destroy(fdr_plan* p) {
    if (!p) return FDR_OK;
    if (g_process_exiting.load()) {  // static destructors / late atexit handlers: the HIP runtime may be gone; the
        delete p;                    // process's device memory goes with it, only the host side is ours to free
        return FDR_OK;
    }
    (void)hipSetDevice(p->device);
    for (fdr_plan::Slot& w : p->slots) release_slot(w);
    for (int k = 0; k < 3; ++k) {
        (void)hipFree(p->pipe.d_in[k]); (void)hipFree(p->pipe.d_out[k]);
        if (p->pipe.e_in[k]) (void)hipEventDestroy(p->pipe.e_in[k]);
        if (p->pipe.e_cmp[k]) (void)hipEventDestroy(p->pipe.e_cmp[k]);
        if (p->pipe.e_out[k]) (void)hipEventDestroy(p->pipe.e_out[k]);
    }
    if (p->pipe.s_in) (void)hipStreamDestroy(p->pipe.s_in);
    if (p->pipe.s_cmp) (void)hipStreamDestroy(p->pipe.s_cmp);
    if (p->pipe.s_out) (void)hipStreamDestroy(p->pipe.s_out);
    if (p->graph_exec) (void)hipGraphExecDestroy(p->graph_exec);
    if (p->cap_stream) (void)hipStreamDestroy(p->cap_stream);
    if (p->fork) (void)hipEventDestroy(p->fork);
    (void)hipFree(p->tw_row_f); (void)hipFree(p->tw_row_i); (void)hipFree(p->tw_col_f); (void)hipFree(p->tw_col_i);
    if (p->naive_col != p->naive_row) (void)hipFree(p->naive_col);
    if (p->mix_col.tw != p->mix_row.tw) { (void)hipFree(const_cast<float2*>(p->mix_col.tw)); (void)hipFree(const_cast<int4*>(p->mix_col.st)); }
    (void)hipFree(const_cast<float2*>(p->mix_row.tw)); (void)hipFree(const_cast<int4*>(p->mix_row.st));
    (void)hipFree(p->naive_row);
    for (auto& r : p->phase_pending) { p->timer.pool.push_back(r.a); p->timer.pool.push_back(r.b); }
    p->phase_pending.clear();
    p->timer.destroy();
    (void)hipFree(p->filt); (void)hipFree(p->psf_dev); (void)hipFree(p->lap); (void)hipFree(p->op_h);
    (void)hipFree(p->stage_in); (void)hipFree(p->stage_out);
    for (fdr::Workspace* w : p->workspaces()) w->free_with(device_free);
    delete p;
    return FDR_OK;
}

int fdr_plan_dims(const fdr_plan* p, int* M, int* N, int* mode) {
    if (!p) return fail(FDR_ERR_ARG, "fdr_plan_dims: null plan");
    if (M) *M = p->M;
    if (N) *N = p->N;
    if (mode) *mode = p->mode;
    return FDR_OK;
}

int fdr_plan_set_option(fdr_plan* p, int option, long long value) {
    if (!p) return fail(FDR_ERR_ARG, "fdr_plan_set_option: null plan");
    switch (option) {
        case FDR_OPT_BATCH_GRAPH:
            if (value != 0 && value != 1) return fail(FDR_ERR_ARG, "fdr_plan_set_option: FDR_OPT_BATCH_GRAPH takes 0 or 1");
            p->batch_graph = value != 0;
            return FDR_OK;
        case FDR_OPT_CE_CHUNK_MB:
            if (value < 0 || value > (1 << 20)) return fail(FDR_ERR_ARG, "fdr_plan_set_option: FDR_OPT_CE_CHUNK_MB takes 0 .. 1048576");
            p->ce_chunk_bytes = (size_t)value << 20;
            return FDR_OK;
        case FDR_OPT_TWO_SWEEP_NORM:
            if (value != 0 && value != 1) return fail(FDR_ERR_ARG, "fdr_plan_set_option: FDR_OPT_TWO_SWEEP_NORM takes 0 or 1");
            p->two_sweep = value != 0;
            return FDR_OK;
        case FDR_OPT_PAD_MODE:
            // the padding is made by pass A of the fast panel path (fdr_panel_rows.hip); no other path has the smooth form
            if (p->tables_only || !on_panel_path(p))
                return fail(FDR_ERR_ARG, "fdr_plan_set_option: FDR_OPT_PAD_MODE needs a FDR_MODE_FAST plan on the panel path (M, N powers of two, "
                                         "8 .. 8192; not FDR_FLAG_SIMPLE_PATH, FDR_FLAG_ANY_SIZE, FDR_FLAG_MIXED_RADIX sizes or FDR_FLAG_TABLES_ONLY)");
            if (value != FDR_PAD_ZERO && value != FDR_PAD_SMOOTH)
                return fail(FDR_ERR_ARG, "fdr_plan_set_option: FDR_OPT_PAD_MODE takes FDR_PAD_ZERO (0) or FDR_PAD_SMOOTH (1)");
            p->pad_mode = (int)value;
            return FDR_OK;
        default:
            return fail(FDR_ERR_ARG, "fdr_plan_set_option: unknown option");
    }
}

int fdr_plan_set_batching(fdr_plan* p, int nstreams, int group) {
    if (!p) return fail(FDR_ERR_ARG, "fdr_plan_set_batching: null plan");
    if (nstreams < 1 || group < 1 || group > kMaxGroup || nstreams * group > fdr_plan::kMaxSlots)
        return fail(FDR_ERR_ARG, "fdr_plan_set_batching: need 1 <= group <= 8 and nstreams * group <= 16");
    FDR_HIP(hipSetDevice(p->device));
    if (!p->fork) FDR_HIP(hipEventCreateWithFlags(&p->fork, hipEventDisableTiming));
    const int nslots = nstreams * group;
    for (int k = 0; k < nslots; ++k) {
        fdr_plan::Slot& w = p->slots[k];
        if (!w.stream) FDR_HIP(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
        if (!w.done) FDR_HIP(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
        if (k > 0 && !w.mm_part && alloc_slot(p, w) != FDR_OK)
            return fail(FDR_ERR_ALLOC, "fdr_plan_set_batching: hipMalloc of an extra workspace failed");
    }
    p->nslots = nslots; p->nstreams = nstreams; p->group = group;
    return FDR_OK;
}

int fdr_plan_set_concurrency(fdr_plan* p, int nstreams) { return fdr_plan_set_batching(p, nstreams, 1); }

int fdr_plan_phase_times(fdr_plan* p, float ms[FDR_N_PHASES], int reset) {
    if (!p || !ms) return fail(FDR_ERR_ARG, "fdr_plan_phase_times: null argument");
    FDR_HIP(hipSetDevice(p->device));
    resolve_phases(p);
    for (int i = 0; i < FDR_N_PHASES; ++i) ms[i] = (float)p->phase_ms[i];
    if (reset)
        for (int i = 0; i < FDR_N_PHASES; ++i) p->phase_ms[i] = 0.0;
    return FDR_OK;
}

int fdr_plan_profile(fdr_plan* p, int enable) {
    if (!p) return fail(FDR_ERR_ARG, "fdr_plan_profile: null plan");
    FDR_HIP(hipSetDevice(p->device));
    p->timer.reset();
    p->timer.enabled = enable != 0;
    return FDR_OK;
}

int fdr_plan_pass_times(fdr_plan* p, int* n_passes, float* mean_ms, const char** names, int* launches) {
    if (!p || !n_passes) return fail(FDR_ERR_ARG, "fdr_plan_pass_times: null argument");
    FDR_HIP(hipSetDevice(p->device));
    double sum[FDR_MAX_PASSES] = {0};
    int cnt[FDR_MAX_PASSES] = {0};
    for (auto& r : p->timer.recs) {
        FDR_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        FDR_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        sum[r.pass] += ms;
        cnt[r.pass] += 1;
    }
    *n_passes = p->timer.n_names;
    for (int i = 0; i < p->timer.n_names; ++i) {
        if (mean_ms) mean_ms[i] = cnt[i] ? (float)(sum[i] / cnt[i]) : 0.f;
        if (names) names[i] = p->timer.names[i];
        if (launches) launches[i] = cnt[i];
    }
    p->timer.reset();
    return FDR_OK;
}

}  // extern "C"

#ifdef FDR_DIAG  // diagnostic builds only (tools/diag): the addresses of a slot's intermediates
extern "C" int fdr_debug_slot_ptrs(fdr_plan* p, int slot, void** work, void** raw, void** mm_part, size_t* ws_elems) {
    if (!p || slot < 0 || slot >= fdr_plan::kMaxSlots) return FDR_ERR_ARG;
    *work = p->slots[slot].work; *raw = p->slots[slot].raw; *mm_part = p->slots[slot].mm_part; *ws_elems = p->ws_elems;
    return FDR_OK;
}
#endif
