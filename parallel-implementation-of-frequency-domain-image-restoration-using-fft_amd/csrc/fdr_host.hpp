// fdr_host.hpp -- private to the host files of libfdr.so (fdr_api_*.hip): the plan with its one path, the pass and phase
// timers, the error helpers and the helpers that more than one entry point uses (the checks, the PSF path, the argument builders
// of the panel and mixed passes).  The C ABI is include/fdr.h alone: the shared helpers live in namespace fdr, so none of them
// is an fdr_* symbol of the library.
#pragma once
#include "../../include/fdr.h"
#include "fdr_kernels.hpp"
#include "fdr_workspace.hpp"

#include <hip/hip_runtime.h>
#include <array>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#pragma clang diagnostic error "-Wswitch"  // a switch over PlanPath names every path: a new path does not compile until each does

namespace fdr {

// The path of a plan: the passes its Wiener call runs and the layout of its intermediate spectrum and filter ("paths
// of a plan").  Chosen once, by layout_radix2 / layout_mixed (fdr_api_plan.hip).
enum PlanPath {
    PATH_SIMPLE,        // rows, transpose, rows, transpose on a row-major spectrum, in either mode: dimensions below 8 or above 8192,
                        // FDR_FLAG_ANY_SIZE sizes, FDR_FLAG_SIMPLE_PATH; the only path whose slots have `work2`
    PATH_PARITY_PANEL,  // parity mode: passes A B C D E on a PANEL-major full spectrum (N / 4 panels): contiguous column tiles
    PATH_FAST_FULL,     // fast mode: A B' C' E on the panel-major full spectrum (N < 32 or FDR_FLAG_FULL_SPECTRUM)
    PATH_FAST_HALF,     // fast mode: A B' C1 C2 (or C' E) on the non-redundant half of the Hermitian spectrum (N / 8 panels, Nyquist
                        // packed into column 0); the path of the blur operator, Richardson-Lucy, TV and FDR_OPT_PAD_MODE
    PATH_MIXED          // FDR_FLAG_MIXED_RADIX in fast mode with a dimension that is not a power of two: the four passes of
                        // fdr_mixed.hip on a panel-major full spectrum (mix_P columns per panel)
};

extern thread_local std::string g_last_error;  // what fdr_last_error returns
int fail(int code, const std::string& msg);     // g_last_error = msg, returns code
int null_arg(const char* fn);                   // FDR_ERR_ARG, "<fn>: null argument"

#define FDR_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            char buf_[512];                                                                        \
            snprintf(buf_, sizeof buf_, "%s:%d: %s: %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return ::fdr::fail(FDR_ERR_HIP, buf_);                                                 \
        }                                                                                          \
    } while (0)

// Device scratch of a one-shot host-pointer call: hipMalloc in alloc, hipFree when the scope ends, so every return is safe.
struct DeviceBuffer {
    void* ptr = nullptr;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }  // move-only: no copy, no assignment
    ~DeviceBuffer() { if (ptr) (void)hipFree(ptr); }
    hipError_t alloc(size_t bytes) { return ptr ? hipErrorInvalidValue : hipMalloc(&ptr, bytes); }  // once: a second call would leak
    template <class T> T* as() const { return static_cast<T*>(ptr); }
};
// buf.alloc(bytes) or return FDR_ERR_ALLOC, "<fn>: hipMalloc"
#define FDR_ALLOC(buf, bytes, fn)                                                                           \
    do {                                                                                                    \
        if ((buf).alloc(bytes) != hipSuccess) return ::fdr::fail(FDR_ERR_ALLOC, std::string(fn) + ": hipMalloc"); \
    } while (0)

struct PassTimer {
    static constexpr int kMaxRecords = 8192;
    struct Rec { hipEvent_t a, b; int pass; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    bool enabled = false;
    const char* names[FDR_MAX_PASSES] = {nullptr};
    int n_names = 0;

    int pass_id(const char* name) {
        for (int i = 0; i < n_names; ++i)
            if (names[i] == name) return i;
        if (n_names < FDR_MAX_PASSES) { names[n_names] = name; return n_names++; }
        return FDR_MAX_PASSES - 1;
    }
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    void reset() {
        for (auto& r : recs) { pool.push_back(r.a); pool.push_back(r.b); }
        recs.clear();
    }
    void destroy() {
        reset();
        for (auto e : pool) (void)hipEventDestroy(e);
        pool.clear();
    }
};

// ---- the on-demand workspaces of a plan.  fdr_workspace.hpp has the handle, and per block its pointers and its layout; here one
// struct per feature adds the handle of every block the feature owns and what the plan remembers about their contents.  Each is
// made by the feature's first call and kept until fdr_plan_destroy; a block for a group (or for frames) grows on the first use with
// a larger count, `ws.count` = the images (frames) it holds, and nothing it held outlives the call that grew it.
inline void* device_alloc(size_t bytes) {
    void* b = nullptr;
    if (hipMalloc(&b, bytes) == hipSuccess) return b;
    (void)hipGetLastError();  // (the failure is reported as FDR_ERR_ALLOC: no sticky error is left behind)
    return nullptr;
}
inline void device_free(void* b) { (void)hipFree(b); }  // (waits for the device: nothing queued still uses an outgrown block)
// The one routine of every ensure_*: ws for `n` by `layout(carver, n)`, from hipMalloc.  The new block is had before the old one is
// let go: FDR_ERR_ALLOC, "<fn>: hipMalloc of the <noun> failed", leaves the plan and the block it had intact.  *made: a new block.
template <class Layout>
int ensure_workspace(Workspace& ws, const char* fn, const char* noun, int n, Layout&& layout, bool* made = nullptr) {
    const Workspace::Grown g = ws.grow(n, layout, device_alloc, device_free);
    if (made) *made = g == Workspace::MADE;
    if (g == Workspace::NO_MEMORY) return fail(FDR_ERR_ALLOC, std::string(fn) + ": hipMalloc of the " + noun + " failed");
    if (g == Workspace::BAD_LAYOUT) return fail(FDR_ERR_STATE, std::string(fn) + ": the " + noun + " does not meet the alignments of its layout");
    return FDR_OK;
}
// T was built for (mu, rho) and the operator tables of generation `gen` (0 = not built) or, fr_gen != 0, for the frame tables of
// that generation (gen is 0 then, so the operator's calls build theirs again); rhs lives in slot k's `raw`
struct TvWorkspace : TvLayout<float2> { Workspace ws; float mu = 0.f, rho = 0.f; unsigned gen = 0, fr_gen = 0; };
struct TvFreeWorkspace : TvFreeLayout { Workspace ws; };    // beside the TV workspace, which it shares; its table is tv.T with mu = nu
struct TvAutoWorkspace : TvAutoLayout { Workspace ws; };    // beside the workspaces of the free form, which it shares
struct TvFramesWorkspace : TvFramesLayout<float2> { Workspace ws; };  // beside the TV workspace of one image, which it shares
struct RlFreeWorkspace : RlFreeLayout { Workspace ws; };    // (r lives in slot k's `raw`)
struct RlAccelWorkspace : RlAccelLayout { Workspace ws; };
struct RlTvWorkspace : RlTvLayout { Workspace ws; };        // made by the first call with lambda > 0
// n_part: the workgroups of the plan's inverse row grid; trace: the internal trace, 2 doubles per step of trace_ws.count steps (it
// grows only when a call with a rule and without the caller's trace asks for more); planes, free-boundary form with weights only:
// the dense weights W and the dense copy of d that the ratio pass reads beside them
struct RlStopWorkspace : RlStopLayout {
    Workspace ws, trace_ws, planes_ws;
    int n_part = 0;
    double* trace = nullptr;
    float* planes = nullptr;
};
// tables: made or regrown by fdr_set_frame_psfs* alone, for tables_ws.count frames: frame k's H_k / (M N) at tables + 2 k ws_elems,
// its conj(H_k) / (M N) ws_elems behind (layout of `filt`); count = the frames of the last set, gen counts the sets.  Only the
// multi-frame calls read them, nothing else writes them, and they touch neither op_h / op_c, filt nor op_gen.  The block of the
// calls is made for one frame by fdr_blur_frames_f32_dev, which needs acc only.
struct FramesWorkspace : FramesLayout<float2> {
    Workspace ws, tables_ws;
    float2* tables = nullptr;
    int count = 0;
    unsigned gen = 0;
};
// w, made by the first free-boundary blind call: the dense weights W (M x N floats), which the coverage of every new PSF and the PSF
// step's denominator are computed from
struct BlindWorkspace : BlindLayout<float2> { Workspace ws, w_ws; float* w = nullptr; };
struct RegWorkspace : RegLayout { Workspace ws; std::vector<double> cand_host, res_host; };  // host copies of cand and res
// the score table and the per-angle (cos, sin) table grow on demand (their counts: entries); host copies of both
struct MotionWorkspace : MotionLayout<float2> {
    Workspace ws, table_ws, trig_ws;
    float* table = nullptr;
    double* trig = nullptr;
    std::vector<float> table_host;
    std::vector<double> trig_host;
};
struct RegisterWorkspace : RegisterLayout<float2> { Workspace ws; };  // beside the motion workspace
struct DefocusWorkspace : DefocusLayout { Workspace ws; std::vector<double> trig_host; std::vector<float> profile_host; };  // beside the motion workspace

}  // namespace fdr

struct fdr_plan {
    int device = 0, M = 0, N = 0, logM = 0, logN = 0, mode = 0;
    unsigned flags = 0;
    fdr::PlanPath path = fdr::PATH_SIMPLE;
    // facts next to the path: which row kernel PATH_SIMPLE uses (generic, big), and that there is no workspace (tables_only)
    bool generic = false;  // FDR_FLAG_ANY_SIZE with a non-power-of-two dimension: naive DFT along that dimension
    bool big = false;  // a power-of-two dimension above 8192: simple sequence with the long row pass (fdr_simple.hip)
    bool tables_only = false;  // FDR_FLAG_TABLES_ONLY: no workspaces, slab primitives only
    int num_cu = 256;
    float2 *naive_row = nullptr, *naive_col = nullptr;  // n x n tables of the non-power-of-two dimensions (length N / M)
    fdr::MixLen mix_row{}, mix_col{};  // PATH_MIXED: lengths N and M
    int mix_P = 1, mix_logP = 0, mix_B = 1;  // columns per panel, row-pass transforms per workgroup
    size_t pstride = 0;  // panel stride (float2 elements)
    int npanels = 0;  // every path but PATH_SIMPLE: panel-major intermediate spectrum and filter
    float2 *tw_row_f = nullptr, *tw_row_i = nullptr, *tw_col_f = nullptr, *tw_col_i = nullptr;
    float2* filt = nullptr;   // H (parity) or W (fast)
    float* psf_dev = nullptr; // staging for host-pointer / generated PSFs
    float *stage_in = nullptr, *stage_out = nullptr;  // device staging of the host-pointer single-image calls: M x N each, kept between calls
    size_t psf_cap = 0;
    int mm_part_cap = 0;  // elements of a slot's mm_part
    float K = 0.f;
    bool have_psf = false;
    double* lap = nullptr;  // CLS filters (fdr_set_psf_cls*) and the TV solve table: a_u = 4 sin^2(pi u / M), u < M, then b_v = 4 sin^2(pi v / N), v < N
    // blur / Richardson-Lucy operator (fdr_set_operator_psf*): H / (M N) and conj(H) / (M N) in the layout of `filt`, one allocation
    // of 2 ws_elems (op_c = op_h + ws_elems), made by the first fdr_set_operator_psf* call; independent of `filt`
    float2* op_h = nullptr;
    float2* op_c = nullptr;
    bool have_op = false;
    unsigned op_gen = 0;  // counts the fdr_set_operator_psf* calls that rebuilt the tables
    // the on-demand workspaces, one member per feature (the structs above; fdr_workspace.hpp says what each block holds)
    fdr::TvWorkspace tv;              // fdr_tv_deconv_f32*, and x, b, the duals and T of every other TV form
    fdr::TvFreeWorkspace tvfree;      // fdr_tv_deconv_free_f32*
    fdr::TvAutoWorkspace tvauto;      // fdr_tv_deconv_auto_f32*
    fdr::TvFramesWorkspace tvframes;  // fdr_tv_deconv_frames_f32*
    fdr::RlFreeWorkspace rlfree;      // fdr_richardson_lucy_free_f32*
    fdr::RlAccelWorkspace rlaccel;    // fdr_richardson_lucy_accel_f32*, fdr_richardson_lucy_free_accel_f32*
    fdr::RlTvWorkspace rltv;          // fdr_richardson_lucy_tv_f32*
    fdr::RlStopWorkspace rlstop;      // fdr_richardson_lucy_auto_f32*
    fdr::FramesWorkspace frames;      // fdr_set_frame_psfs*, fdr_blur_frames_f32_dev, fdr_richardson_lucy_frames_f32*
    fdr::BlindWorkspace blind;        // fdr_richardson_lucy_blind_f32*
    fdr::RegWorkspace reg;            // fdr_reg_curve_f32*, fdr_choose_reg_f32*
    fdr::MotionWorkspace motion;      // fdr_cepstrum_f32*, fdr_estimate_motion_f32*
    fdr::DefocusWorkspace defocus;    // fdr_estimate_defocus_f32*, fdr_estimate_blur_f32*
    fdr::RegisterWorkspace regist;    // fdr_register_frames_f32*
    // every block of the members above, for fdr_plan_destroy: a block that a feature gains is added here, beside its member
    std::array<fdr::Workspace*, 20> workspaces() {
        return {&tv.ws, &tvfree.ws, &tvauto.ws, &tvframes.ws, &rlfree.ws, &rlaccel.ws, &rltv.ws, &rlstop.ws,
                &rlstop.trace_ws, &rlstop.planes_ws, &frames.ws, &frames.tables_ws, &blind.ws, &blind.w_ws, &reg.ws,
                &motion.ws, &motion.table_ws, &motion.trig_ws, &defocus.ws, &regist.ws};
    }
    // sectioned restoration (fdr_restore_tiled_f32*): the host copy of the last call's weight tables (one entry per picture row, then one
    // per picture column), kept here while the upload may still read it; everything else of such a call lies in the caller's workspace
    std::vector<fdr::TiledCover> tl_tab_host;
    fdr::PassTimer timer;
    // the reference Profiler's buckets (fdr_plan_phase_times): resolved sums + event pairs not read back yet
    struct PhaseRec { hipEvent_t a, b; int phase; };
    double phase_ms[FDR_N_PHASES] = {0, 0, 0, 0, 0, 0};
    std::vector<PhaseRec> phase_pending;
    // The workspaces.  Slot 0 is the one of every single-image call; in batched mode images alternate over `nslots` private
    // workspaces, each on its own internal stream, so the tail of one image's kernels overlaps the head of the next image's
    struct Slot {
        float2* work = nullptr;     // the working spectrum, ws_elems
        float2* work2 = nullptr;    // PATH_SIMPLE: N x M transpose buffer
        float* raw = nullptr;       // M x N real plane before normalisation
        float* mm = nullptr;        // final {min, max}
        float2* mm_part = nullptr;  // per-workgroup partials
        hipStream_t stream = nullptr; hipEvent_t done = nullptr;
    };
    static constexpr int kMaxSlots = 16;
    Slot slots[kMaxSlots];
    int nslots = 1;   // = nstreams * group
    int nstreams = 1;
    int group = 1;    // images per pass-B' launch (panel path)
    hipEvent_t fork = nullptr;
    size_t ws_elems = 0;  // elements of one work / raw buffer
    int pad_mode = FDR_PAD_ZERO;     // FDR_OPT_PAD_MODE: what pass A of the fdr_wiener_* calls puts outside the picture (panel path)
    bool two_sweep = true;           // FDR_OPT_TWO_SWEEP_NORM: passes C1 + C2 instead of C' + E (fast half-spectrum path)
    size_t ce_chunk_bytes = (size_t)160 << 20;  // FDR_OPT_CE_CHUNK_MB: spectrum bytes per C1 + C2 launch pair of a multi-stream batch (0 = whole group)
    // FDR_OPT_BATCH_GRAPH: the launches of one fdr_wiener_batch_f32_dev call (fork, every pass of every group on the
    // internal streams, join) captured once as a hipGraph and replayed while the call's arguments stay the same
    struct GraphKey {
        const float* in; float* out; size_t in_pitch, out_pitch; int count, rows, cols, stride, out_stride, norm_area, nstreams, group;
        bool two_sweep; float K; size_t ce_cache; int pad_mode;
        bool operator==(const GraphKey& o) const {
            return in == o.in && out == o.out && in_pitch == o.in_pitch && out_pitch == o.out_pitch && count == o.count && rows == o.rows &&
                   cols == o.cols && stride == o.stride && out_stride == o.out_stride && norm_area == o.norm_area && nstreams == o.nstreams &&
                   group == o.group && two_sweep == o.two_sweep && K == o.K && ce_cache == o.ce_cache && pad_mode == o.pad_mode;
        }
    };
    // host-pointer batch (fdr_wiener_batch_*_f32): three streams, three images in flight; created on first use and kept --
    // a driver that calls wienerDeblur_RGB_optimized once per picture (3 channels per call) would otherwise pay three
    // hipStreamCreate, six hipMalloc / hipFree and nine event creations per call, most of such a call's time
    // (LAB_NOTES "host-pointer calls")
    struct HostPipe {
        hipStream_t s_in = nullptr, s_cmp = nullptr, s_out = nullptr;
        float* d_in[3] = {nullptr, nullptr, nullptr};
        float* d_out[3] = {nullptr, nullptr, nullptr};
        hipEvent_t e_in[3] = {nullptr, nullptr, nullptr}, e_cmp[3] = {nullptr, nullptr, nullptr}, e_out[3] = {nullptr, nullptr, nullptr};
        size_t cap = 0;  // bytes of each d_in / d_out buffer
        bool ready = false;  // all three streams and nine events exist
    } pipe;
    bool batch_graph = false;
    hipGraphExec_t graph_exec = nullptr;
    GraphKey graph_key{};
    hipStream_t cap_stream = nullptr;
};

namespace fdr {

// on one of the two fast panel paths (passes A, B', C of fdr_panel_rows.hip / fdr_panel_cols.hip)
inline bool on_panel_path(const fdr_plan* p) { return p->path == PATH_FAST_FULL || p->path == PATH_FAST_HALF; }

struct ScopedPass {
    fdr_plan* p; hipStream_t s; PassTimer::Rec rec; bool on;
    ScopedPass(fdr_plan* plan, hipStream_t st, const char* name) : p(plan), s(st), on(false) {
        if (p->timer.enabled && (int)p->timer.recs.size() < PassTimer::kMaxRecords) {
            rec.a = p->timer.get(); rec.b = p->timer.get(); rec.pass = p->timer.pass_id(name);
            on = rec.a && rec.b;
            if (on) (void)hipEventRecord(rec.a, s);
        }
    }
    ~ScopedPass() {
        if (on) { (void)hipEventRecord(rec.b, s); p->timer.recs.push_back(rec); }
    }
};

// folds the pending pairs whose end event has already completed (no waiting) into the sums; keeps the others
void resolve_finished_phases(fdr_plan* p);
// waits for every pending pair and folds it into the sums
void resolve_phases(fdr_plan* p);

// One hipEvent pair on stream s around a phase of the reference's Profiler (fft/fft_gpu.cu:17-57); read back by
// resolve_phases.  Bounded at 1024 unread pairs; from 768 on, pairs that have completed are folded in first (no waiting), so only
// a caller with more than 1024 phases IN FLIGHT at once loses records.
struct ScopedPhase {
    fdr_plan* p; hipStream_t s; fdr_plan::PhaseRec rec; bool on;
    ScopedPhase(fdr_plan* plan, int phase, hipStream_t st) : p(plan), s(st), on(false) {
        if (p->phase_pending.size() >= 768) resolve_finished_phases(p);  // long host batches / many PSF rebuilds: fold what has completed
        if (p->phase_pending.size() < 1024) {
            rec.a = p->timer.get(); rec.b = p->timer.get(); rec.phase = phase;
            on = rec.a && rec.b;
            if (on) (void)hipEventRecord(rec.a, s);
        }
    }
    ~ScopedPhase() {
        if (on) { (void)hipEventRecord(rec.b, s); p->phase_pending.push_back(rec); }
    }
};

// ---- twiddle tables (fdr_api_plan.hip) ----
int ilog2(int n);
void build_twiddles(int n, int mode, bool inverse, std::vector<float2>& out);
void build_naive_table(int n, std::vector<float2>& out);
constexpr int kMaxNaiveLen = 4096;  // 128 MiB of table

// ---- the checks of the entry points (fdr_api_plan.hip): a refusal names the entry point `fn` that was called and comes
// before its first HIP call.  The kind of plan a call needs:
enum PlanNeed {
    NEED_PLAN,          // any plan with workspaces (not FDR_FLAG_TABLES_ONLY)
    NEED_FILTER,        // ... holding a Wiener / CLS filter
    NEED_OPERATOR,      // ... on the path of the blur operator (fast mode, half-spectrum panel path)
    NEED_OPERATOR_PSF,  // ... holding the operator tables as well
    NEED_MOTION         // ... that the motion estimate runs on
};
int check_plan(const fdr_plan* p, const char* fn, PlanNeed need);
// check_plan, then the rows x cols window (row stride `stride`, of the result `out_stride`): at least min x min, within M x N
int check_window(const fdr_plan* p, const char* fn, PlanNeed need, int rows, int cols, int stride, int out_stride, int min = 1);

// ---- the one path of the twelve PSF setters (fdr_api_plan.hip) ----
// A PSF is a device or a host pointer (rows x cols, row stride `stride`) or a generated motion or disk PSF (size in all three;
// angle_deg holds the disk's radius).
enum PsfKind { PSF_DEV, PSF_HOST, PSF_MOTION, PSF_DISK };
struct PsfSource { PsfKind kind; const float* ptr; int rows, cols, stride; double angle_deg; };
// Checked completely, staged unless it is a device pointer, and built into the Wiener / CLS filter (op false; gamma 0 is the
// Wiener filter) or into the blur / RL operator tables (op true).  A host PSF is ready when the call returns (fdr_batch_run relies
// on it); device and generated PSFs stay asynchronous on `s`.
int set_psf(fdr_plan* p, const char* fn, const PsfSource& src, bool op, float K, float gamma, hipStream_t s);
// the builders, on a checked device PSF (fdr_api_wiener.hip, fdr_api_operator.hip)
int set_psf_dev_impl(fdr_plan* p, const float* d_psf, int prows, int pcols, int pstride, float K, hipStream_t s, double gamma);
int set_operator_psf_impl(fdr_plan* p, const float* d_psf, int prows, int pcols, int pstride, hipStream_t s);
// the two launches of the operator setter on any pair of tables (ws_elems each, layout of `filt`): the PSF's row spectra into `h`,
// then H / (M N) in place and conj(H) / (M N) into `c`.  Touches nothing else of the plan.
int build_operator_tables(fdr_plan* p, const float* d_psf, int prows, int pcols, int pstride, float2* h, float2* c, hipStream_t s);

// the Laplacian table of the CLS filters and of the TV solve (fdr_api_wiener.hip): built in double on the host and uploaded on first
// use (synchronous), freed with the plan
int ensure_lap_table(fdr_plan* p);

// ---- byte ranges: the one overlap test of the checks ----
struct ByteRange { uintptr_t lo, hi; };  // [lo, hi)
inline ByteRange byte_range(const void* ptr, size_t bytes) { return {(uintptr_t)ptr, (uintptr_t)ptr + bytes}; }
// `count` windows rows x cols (row stride `stride`) that lie `pitch` elements apart
inline ByteRange window_range(const float* base, int rows, int cols, int stride, int count = 1, size_t pitch = 0) {
    return byte_range(base, ((size_t)(count - 1) * pitch + (size_t)(rows - 1) * stride + cols) * sizeof(float));
}
inline bool ranges_overlap(const ByteRange& a, const ByteRange& b) { return a.lo < b.hi && b.lo < a.hi; }

// ---- the operator passes (fdr_api_operator.hip), shared by the blur, Richardson-Lucy and the TV solve ----
// what ROW_OUT_RL_RATIO_STAT takes beside the datum: the weights (dense, the row stride of the datum; null = 1) and the room for the
// (res, kl) partials, one double2 per workgroup of the pass
struct RlFit { const float* weights; double* part; };
// The passes for a group of n >= 1 images on the slots ws[0 .. n) with per-image pointers (blockIdx.y = image; n = 1 is the
// single-image launch): pass A (the window of xs[k], zero elsewhere -> the half spectrum of slot k) keeps FDR_PAD_ZERO, pass B'
// reads `table` once for the group and is timed as `name`, pass C takes the four kinds ROW_OUT_BLUR, _RL_RATIO, _RL_UPDATE and
// _RL_UPDATE_W (src2: the one wgt plane of the group, or with src2_pitch image k's own plane at src2 + k src2_pitch floats, at most
// an M x N plane apart) and, for one image, _RL_RATIO_STAT with `fit`.  An image comes out with the
// bits it gets alone.
int op_rows_fwd_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float* const* xs, int rows, int cols, int stride, hipStream_t s);
int op_cols_table_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float2* table, const char* name, hipStream_t s);
int op_rows_inv_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, RowOut kind, const char* name, const float* const* srcs, int src_stride,
                  const float* src2, float* const* outs, int out_stride, int rows, int cols, hipStream_t s, const RlFit* fit = nullptr,
                  size_t src2_pitch = 0);
int op_cols_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, bool adjoint, hipStream_t s);  // pass B' on H / (M N), `adjoint`: on conj(H) / (M N)
// the single-image forms: a group of one on slot 0
int op_rows_fwd(fdr_plan* p, const float* x, int rows, int cols, int stride, hipStream_t s);
int op_cols_table(fdr_plan* p, const float2* table, const char* name, hipStream_t s);
int op_rows_inv(fdr_plan* p, RowOut kind, const char* name, const float* src, int src_stride, float* out, int out_stride, int rows, int cols,
                hipStream_t s);
// blur (adjoint != 0: blur^T) of the window rows x cols of d_img; the window out_rows x out_cols of the result into d_out
int blur_window_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride, int out_rows, int out_cols,
                    int adjoint, hipStream_t s);
// (the group form writes the window of the input unless out_rows x out_cols names another)
int blur_window_dev_n(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                      float* const* d_outs, int out_stride, int adjoint, hipStream_t s, int out_rows = 0, int out_cols = 0);
// min-max of the window `fin` (row stride fs) to [0, 1] into d_out, timed as `name`: FDR_NORM_CROPPED over the window, FDR_NORM_PADDED
// counting the zeros outside it too
int normalize_window(fdr_plan* p, const char* fn, const char* name, const float* fin, int fs, int rows, int cols, int norm_area, float* d_out,
                     int out_stride, hipStream_t s);
// images of one launch group: the plan's group on the path of the operator, never more than the batch holds
inline int launch_group(const fdr_plan* p, int count) { return p->group < count ? p->group : count; }
// the launch group that starts at image i0 of a batch of `count` (`pitch` elements apart): its n images on the slots 0 .. n - 1
struct LaunchGroup {
    int n;
    fdr_plan::Slot* ws[kMaxGroup];
    const float* ins[kMaxGroup];
    float* outs[kMaxGroup];
    LaunchGroup(fdr_plan* p, int i0, int count, const float* d_imgs, size_t img_pitch, float* d_out, size_t out_pitch)
        : n(launch_group(p, count) < count - i0 ? launch_group(p, count) : count - i0) {
        for (int k = 0; k < n; ++k) { ws[k] = &p->slots[k]; ins[k] = d_imgs + (size_t)(i0 + k) * img_pitch; outs[k] = d_out + (size_t)(i0 + k) * out_pitch; }
    }
};

// ---- Richardson-Lucy, both forms (fdr_api_rl.hip, fdr_api_rlfree.hip): the checks, the step and the driver of each form, on a
// group of n >= 1 images on the slots ws[0 .. n).  The calls that stop from the data (fdr_api_rlstop.hip), the blind call
// (fdr_api_blind.hip) and the batches (fdr_api_rlbatch.hip) are built from them.
// What a driver runs around and inside a step for the blind call, each with the index of the iteration: after_fwd when pass A of
// the estimate has left its row spectra in slot 0 (which it may read, not write), after_ratio when r lies in the window of the raw
// plane (slot 0's spectrum is free then), after_step when the update is written.  No hook changes an operand of the step's own
// passes: the step keeps its bits.  An empty hook is skipped; hooks take one image per step (FDR_ERR_STATE otherwise).
struct RlHooks { std::function<int(int it)> after_fwd, after_ratio, after_step; };
int rl_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* out, int out_stride,
             int iterations, int norm_area, PlanNeed need = NEED_OPERATOR_PSF);
// what the calls that take both forms' arguments refuse in the plain form: weights, and an output window other than the input's.
// `each_alone`: out_rows and out_cols may be 0 or the input's independently (the auto call); otherwise both 0 or both the input's.
// `window_msg` is the call's own wording of the second refusal.
int plain_form_check(const char* fn, const float* weights, int rows, int cols, int out_rows, int out_cols, bool each_alone, const char* window_msg);
// One iteration of the plain form: c = blur(y), r = d+ / c into the window of slot k's raw plane (row stride cols), out = max(y .
// blur^T(r), 0); outs[k] may be ys[k].  With `fit` (one image) the ratio pass also leaves the fit partials of c: same r, same update.
// With `factor` (row stride ystride; image k's plane at factor + k factor_pitch) the update is the weighted one: out = max(y . factor .
// blur^T(r), 0).
int rl_step(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int stride, const float* const* ys, int ystride,
            float* const* outs, int os, int rows, int cols, hipStream_t s, const RlFit* fit = nullptr, const RlHooks* hooks = nullptr, int it = 0,
            const float* factor = nullptr, size_t factor_pitch = 0);
// the start u = max(d, 0) and the closing normalisation of a plain-form call
int rl_init_estimate(fdr_plan* p, const float* d_img, int rows, int cols, int stride, float* u, int us, hipStream_t s);
int rl_normalize(fdr_plan* p, const char* fn, const float* fin, int fs, int rows, int cols, int norm_area, float* d_out, int out_stride,
                 hipStream_t s);
// the plain form on a checked group: start per image, `iterations` steps, normalisation per image
int rl_group_dev(fdr_plan* p, const char* fn, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                 float* const* d_outs, int out_stride, int iterations, int norm_area, hipStream_t s, const RlHooks* hooks = nullptr);
// the accelerated plain form on a checked group with the acceleration workspace for n images: start per image, the recursion of
// rl_accel_loop around rl_step on the group (the estimate alternates between each image's output window and its workspace plane,
// the last update goes to the slot's raw plane under a normalisation), normalisation per image.  Image k's alphas go to
// d_alphas + k alpha_pitch when d_alphas is not null.
int rl_group_accel_dev(fdr_plan* p, const char* fn, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                       float* const* d_outs, int out_stride, int iterations, int norm_area, float* d_alphas, size_t alpha_pitch, hipStream_t s);
// the free-boundary workspace for `group` images (ensure_workspace)
int ensure_rlfree_workspace(fdr_plan* p, const char* fn, int group = 1);
int rlfree_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
                 const float* out, int out_stride, const fdr_rlfree_params* prm, PlanNeed need = NEED_OPERATOR_PSF);
// host weights (rows x cols) dense into u's plane, where the setup pass leaves W anyway: the d_w of the host forms (synchronous)
int stage_weights(fdr_plan* p, const float* weights_host, int rows, int cols, int wstride);
// One iteration of the free-boundary form on the whole plan: c = window(fullblur(y)), r = datum / c into slot k's raw plane, out =
// max(y wgt fullblur^T(pad(r)), 0).  ys[k] and outs[k] are dense M x N planes and may be the same; datums[k] is dense rows x cols:
// dw, or with `fit` (one image; weights dense too) d, from which the ratio pass forms dw = w d+ itself; wgt is the one plane of the call,
// or with wgt_pitch image k's own plane at wgt + k wgt_pitch (the prior's factor wgt / g_k).
int rlfree_step(fdr_plan* p, fdr_plan::Slot* const* ws, int n, const float* const* ys, float* const* outs, const float* const* datums,
                const float* wgt, int rows, int cols, hipStream_t s, const RlFit* fit = nullptr, const RlHooks* hooks = nullptr, int it = 0,
                size_t wgt_pitch = 0);
// begin, image 0 of a call: the setup (dw into rlfree.dw, W = pad(m) into rlfree.u, copied dense to keep_w when that is not null), the
// coverage alpha = fullblur^T(W) and the start (rlfree.wgt = 1 / alpha, u_0 in rlfree.u); *sums, when not null, is where the device holds
// (sum dw, sum W).  d_w may be rlfree.u itself (stage_weights).
int rlfree_begin(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float sigma, float* keep_w,
                 const double** sums, hipStream_t s);
// finish: the output window of the dense M x N estimate u, cropped or normalised, into d_out
int rlfree_finish(fdr_plan* p, const char* fn, const float* u, float* d_out, int out_stride, const fdr_rlfree_params& prm, hipStream_t s);
// `tv` of rlfree_batch_dev, the TV prior of fdr_api_rltv.hip (launch groups of more than one image, no hooks, not accelerated; needs
// the prior's workspace for the group): image k's estimate lives in rltv.u + k M N, and every step is preceded by one factor launch for
// the group and takes factor_k = wgt / g_k, at rltv.f + k M N, in the place of wgt.  `coupled`: the images are the channels of one
// picture and share the prior's norm.
struct RlTvPrior { float lambda, eps; bool coupled; };
// the free-boundary form on a checked batch of `count` images with its workspace (for launch_group(p, count) images): begin, steps in
// place, finish, in launch groups; one image with its hooks and keep_w is the blind call's.  `accel` (no hooks; needs the acceleration
// workspace for the group as well): the recursion of rl_accel_loop around the step, the estimate alternating between image k's u
// plane and its acceleration plane, image i's alphas to d_alphas + i alpha_pitch when d_alphas is not null.
int rlfree_batch_dev(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride, const float* d_w,
                     int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_rlfree_params& prm, hipStream_t s,
                     const RlHooks* hooks = nullptr, float* keep_w = nullptr, bool accel = false, float* d_alphas = nullptr,
                     size_t alpha_pitch = 0, const RlTvPrior* tv = nullptr);
// ---- the TV prior of Richardson-Lucy (fdr_api_rltv.hip) ----
// the factor launch of a group: the n planes rows x cols (row stride `stride`) at rltv.u + k M N to rltv.f + k M N (same stride), w the group's
int rltv_factor_group(fdr_plan* p, int n, int rows, int cols, int stride, const float* w, const RlTvPrior& tv, hipStream_t s);
// what the multi-frame call (fdr_api_frames.hip) shares with the single one: the prior's workspace (2 group planes; it grows as the
// others do), the refusal of a bad lambda or eps, and the factor launch of one image: u (rows x cols, row stride `stride`) and w to rltv.f
int ensure_rltv_workspace(fdr_plan* p, const char* fn, int group = 1);
int prior_check(const char* fn, float lambda, float eps);
int rltv_factor(fdr_plan* p, const float* u, int rows, int cols, int stride, const float* w, float lambda, float eps, hipStream_t s);
// the checks and the driver of fdr_richardson_lucy_batch_f32* (fdr_api_rlbatch.hip), which the batch with the prior shares
int rl_batch_check(const fdr_plan* p, const char* fn, const float* imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                   const float* weights, int wstride, const float* out, size_t out_pitch, int out_stride, const fdr_rl_batch_params& b,
                   fdr_rlfree_params* free_prm);
int rl_batch_run(fdr_plan* p, const char* fn, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                 const float* d_w, int wstride, float* d_out, size_t out_pitch, int out_stride, const fdr_rl_batch_params& b,
                 const fdr_rlfree_params& free_prm, hipStream_t s, bool accel = false, float* d_alphas = nullptr, size_t alpha_pitch = 0);
// ---- the noise estimate (fdr_api_reg.hip): the Immerkaer sum of a device window through `part` (reg_noise_partials + 1 doubles), read
// back: synchronous; and the refusal of a window it cannot work on
int noise_sigma_dev(const float* d_img, int rows, int cols, int stride, double* part, double* sigma, hipStream_t s);
int noise_window_check(const char* fn, int rows, int cols, int stride);
// ---- accelerated Richardson-Lucy (fdr_api_rlaccel.hip), shared by the plain and the free-boundary form ----
// the workspace of the accelerated calls for `group` images (ensure_workspace)
int ensure_rlaccel_workspace(fdr_plan* p, const char* fn, int group = 1);
// image k of a group: the extrapolated point y, the second plane of its estimate, its direction g
float* rlaccel_y_plane(const fdr_plan* p, int k);
float* rlaccel_u_plane(const fdr_plan* p, int k);
float* rlaccel_g_plane(const fdr_plan* p, int k);
// FDR_ERR_ARG when the n floats at d_alphas overlap the rows x cols window at `w` (row stride ws); a null d_alphas is fine
int check_alphas(const char* fn, const float* d_alphas, int n, const float* w, int ws, int rows, int cols, const char* what);
// run(d_alphas) of a host-pointer call: a one-shot device buffer for the n alphas (null for a null host pointer or n <= 0), read back after it
int with_host_alphas(const char* fn, float* alphas_host, int n, const std::function<int(float* d_alphas)>& run);
// One iteration of either form on a group: image i's u_next = step(y) from ys[i], a rows x cols window with row stride ystride, to
// outs[i] (row stride os), another plane
using RlStep = std::function<int(const float* const* ys, int ystride, float* const* outs, int os)>;
// n accelerated iterations on the rows x cols windows of a group of nimg images (1 .. kMaxGroup; one image launches the single-image
// kernels).  Image i's u_k lives in U[i][(first + k) & 1] (row strides us[], common to the group), u_0 there on entry; the last step
// writes to fin[i] (row stride fs) when fin is not null.  result[i], when result is not null, receives the plane of image i's u_n.
// Image i's alpha_0 .. alpha_(n-1) go to d_alphas + i alpha_pitch when d_alphas is not null.  For n <= 2 this is n steps and nothing
// else.  A group makes the launches of one image: one extrapolation, one direction and one alpha launch per iteration.
int rl_accel_loop(fdr_plan* p, int nimg, int n, int rows, int cols, float* const (*U)[2], const int us[2], int first, float* const* fin, int fs,
                  float* d_alphas, size_t alpha_pitch, hipStream_t s, const RlStep& step, float** result);
// iterations k0 .. k1 - 1 of a run of at most n (what rl_accel_loop is made of): u_k0 lies in U[i][(first + k0) & 1] and the state of
// the earlier iterations (g, alpha) in the workspace; result[i] receives the plane of u_k1 (untouched for k0 = k1)
int rl_accel_steps(fdr_plan* p, int nimg, int k0, int k1, int n, int rows, int cols, float* const (*U)[2], const int us[2], int first,
                   float* const* fin, int fs, float* d_alphas, size_t alpha_pitch, hipStream_t s, const RlStep& step, float** result);
// pairs of one fdr_reg_curve_f32* call (fdr_api_reg.hip): what the candidate and result arrays of the plan hold
constexpr int kRegMaxCurve = 4096;
static_assert(kRegMaxCurve % kRegCandidates == 0, "the last sweep reads kRegCandidates pairs");
// ---- total-variation deconvolution (fdr_api_tv.hip), shared with its batch (fdr_api_tvbatch.hip) ----
// everything a TV call refuses for one image, before any device work
int tv_check(const fdr_plan* p, const char* fn, int rows, int cols, int stride, int out_stride, const fdr_tv_params* prm,
             PlanNeed need = NEED_OPERATOR_PSF);
// the TV workspace for `group` images (ensure_workspace; a new block's T is built again by the next call) and the Laplacian table,
// both synchronous and on first use only
int ensure_tv_workspace(fdr_plan* p, const char* fn, int group = 1);
int tv_prepare(fdr_plan* p, const char* fn, int group = 1);
inline size_t tv_image_stride(const fdr_plan* p) { return (size_t)6 * p->M * p->N; }
// The stages the periodic driver and the free-boundary driver (fdr_api_tvfree.hip) share, on the planes 0 .. n - 1 of the TV
// workspace and the slots ws[0 .. n), each timed under the form's pass names (static strings: PassTimer compares them by pointer).
// table: T for the data weight (mu; nu in the free forms) and rho, unless the plan holds it already.  prior half-step of iteration
// `it`: one spatial launch (the duals alternate with `it`; rhs is slot k's raw plane), then the solve into x as forward rows, table
// columns and inverse rows.  output tail: the rows x cols window of every x cropped and clamped into d_outs, or, with a norm_area,
// normalised per image (clamped into rhs first with nonneg).
struct TvPassNames { const char *table, *spatial, *spatial_joint, *solve, *x, *out, *norm; };
int tv_solve_table(fdr_plan* p, const TvPassNames& names, float weight, float rho, hipStream_t s);
int tv_prior_half_step(fdr_plan* p, const TvPassNames& names, fdr_plan::Slot* const* ws, int n, int it, float weight, float rho, int anisotropic,
                       bool coupled, hipStream_t s);
int tv_output_tail(fdr_plan* p, const char* fn, const TvPassNames& names, fdr_plan::Slot* const* ws, int n, float* const* d_outs, int rows, int cols,
                   int out_stride, int nonneg, int norm_area, hipStream_t s);
// The iteration on a checked group of n >= 1 images on the slots ws[0 .. n) and the planes 0 .. n - 1 of the workspace: b and the
// start per group, per iteration one spatial, one forward-row, one solve-column and one x-row launch for the group, the output (and
// its normalisation, per image) at the end.  `coupled`: the images are the channels of one picture and share the shrinkage
// (isotropic).  Uncoupled, every image gets the bits it gets alone; one image makes the launches of the single-image call.
int tv_group_dev(fdr_plan* p, const char* fn, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                 float* const* d_outs, int out_stride, const fdr_tv_params& prm, bool coupled, hipStream_t s);
// one image on slot 0: the group of one
int tv_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, float* d_out, int out_stride,
                const fdr_tv_params& prm, hipStream_t s);
// ---- free-boundary TV deconvolution (fdr_api_tvfree.hip) ----
// the 2 group planes of the free form (ensure_workspace)
int ensure_tvfree_workspace(fdr_plan* p, const char* fn, int group = 1);
// everything a free-boundary TV call refuses, before any device work; the workspaces of a call (the two planes first, then the
// periodic call's for one image and the Laplacian table)
int tvfree_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
                 const float* out, int out_stride, const fdr_tv_free_params* prm, PlanNeed need = NEED_OPERATOR_PSF);
int tvfree_prepare(fdr_plan* p, const char* fn, int group = 1);
// the pass names of the free-boundary forms (static strings: PassTimer compares them by pointer), for the multi-frame form, which
// runs the same kernels: the shared stages, the start and the two data steps
extern const TvPassNames kTfPasses;
extern const char* const kPassTfInit;
extern const char* const kPassTfData;
extern const char* const kPassTpData;
// The data step of a free-boundary iteration, the one thing its forms differ in.  LEAST_SQUARES (fdr_api_tvfree.hip): the term
// mu / 2 m (s - d)^2 on prm.mu.  AUTO (fdr_api_tvauto.hip, fdr_api_tvfreebatch.hip): the same with every image's weight chosen in
// every iteration (prm.mu is not used) from tau and, for every image of the group, the noise level of its discrepancy ball; the
// device writes image k's trace to trace[k] (3 doubles per iteration; null: none); the partials, mu_k and the last step's sums are
// the plan's.  POISSON (fdr_api_tvpoisson.hip): the term mu m [(s + b) - d+ log(s + b)], b = background, on prm.mu.
struct TvDataStep {
    enum Kind { LEAST_SQUARES, AUTO, POISSON } kind;
    double tau, sigma[kMaxGroup];  // AUTO
    double* trace[kMaxGroup];      // AUTO
    float background;              // POISSON
};
inline TvDataStep tv_data_auto(double tau) { TvDataStep d{}; d.kind = TvDataStep::AUTO; d.tau = tau; return d; }
inline TvDataStep tv_data_poisson(float background) { TvDataStep d{}; d.kind = TvDataStep::POISSON; d.background = background; return d; }
// the workspaces of an auto call for `group` images: the free call's, then the auto block (ensure_tvauto_workspace: it grows as the
// free call's does); the auto call's own arguments (sigma, tau, nu) checked and nu resolved into *fp, the free call's parameters
struct TvAutoArgs {
    fdr_tv_free_params fp;  // the free call's, with nu resolved; mu is a placeholder
    double sigma, tau;
    bool estimate;
};
int tvauto_check(const fdr_plan* p, const char* fn, const float* img, int rows, int cols, int stride, const float* weights, int wstride,
                 const float* out, int out_stride, const fdr_tv_auto_params* prm, const double* d_trace, TvAutoArgs* a);
int ensure_tvauto_workspace(fdr_plan* p, const char* fn, int group = 1);
int tvauto_prepare(fdr_plan* p, const char* fn, int group = 1);
// the noise level of one window as fdr_noise_sigma_f32 estimates it, on the auto block's partials: one launch, one read-back
int tvauto_noise_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, double* sigma, hipStream_t s);
// The iteration on a checked group of n >= 1 images on the slots ws[0 .. n) and the planes 0 .. n - 1 of the workspaces: x, b, the
// duals, q, c / r and rhs (slot k's raw plane) are full M x N planes; every d and the one weights window are read from the caller's
// windows by every data step.  Per iteration one blur, the window launches, one adjoint blur, one spatial launch and the three solve
// passes, each over the n images; then the output (and the per-image normalisation).  `data` selects the data step, each kind
// under its own pass name; every other pass, workspace and table is the same for all.  The AUTO step takes image k's weight from the
// norm and mu launches before it, and the auto block must hold the group.  `coupled`: the images are the channels of one picture and
// share the shrinkage (isotropic only); everything else stays per image.  One image, uncoupled, makes the launches and the bits the
// single-image calls have always made.
int tvfree_group_dev(fdr_plan* p, const char* fn, fdr_plan::Slot* const* ws, int n, const float* const* d_imgs, int rows, int cols, int stride,
                     const float* d_w, int wstride, float* const* d_outs, int out_stride, const fdr_tv_free_params& prm, bool coupled, hipStream_t s,
                     const TvDataStep& data = TvDataStep());
// one image on slot 0: the group of one
int tvfree_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const float* d_w, int wstride, float* d_out,
                    int out_stride, const fdr_tv_free_params& prm, hipStream_t s, const TvDataStep& data = TvDataStep());
// what the crop batches (fdr_api_tvfreebatch.hip, fdr_api_tvpoisson.hip) share beyond the single call's checks on image 0: the
// refusals of a batch (an unknown coupling, the coupled form with anisotropic != 0 or count > group, outputs that overlap any input
// or the weights)
int crop_batch_check(const fdr_plan* p, const char* fn, const float* imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                     const float* weights, int wstride, const float* out, size_t out_pitch, int out_stride, const fdr_tv_free_params& one,
                     int coupling);

// ---- the frame passes of multi-frame Richardson-Lucy (fdr_api_frames.hip), shared with multi-frame TV (fdr_api_tvframes.hip) ----
// frame k's table H_k / (M N), or conj(H_k) / (M N); the span of a window in floats
const float2* frame_table(const fdr_plan* p, int k, bool adjoint);
inline size_t window_span(int rows, int cols, int stride) { return (size_t)(rows - 1) * stride + cols; }
// the frames i0 .. i0 + n - 1 on the slots ws[0 .. n): pass B' of each on its own table; then their spectra into the accumulator `acc`
// (ws_elems, 16-byte aligned; `first`: stored, else added to what it holds); then pass C of the accumulator
int frames_cols(fdr_plan* p, fdr_plan::Slot* const* ws, int n, int i0, bool adjoint, hipStream_t s);
int frames_sum(fdr_plan* p, float2* acc, fdr_plan::Slot* const* ws, int n, bool first, hipStream_t s);
int frames_rows_inv(fdr_plan* p, float2* acc, RowOut kind, const char* name, const float* src, int src_stride, const float* src2, float* out,
                    int out_stride, int rows, int cols, hipStream_t s);
extern const char* const kPassFrBlur;  // pass C with ROW_OUT_BLUR on frames

// ---- the motion-blur estimate (fdr_api_motion.hip), shared with the defocus and the combined estimate (fdr_api_defocus.hip) ----
// the search arguments with their defaults (0 selects one), after the plan and window checks; FDR_ERR_ARG for anything outside
// the documented ranges (`what` names the searched quantity in the message: "length", or "diameter" for the defocus search)
struct MotionArgs { int min_length, max_length, n_angles, n_lengths; double step; };
int motion_args(const fdr_plan* p, const char* fn, int rows, int cols, int stride, int min_length, int max_length, double step, MotionArgs* a,
                const char* what = "length");
// the fixed part of the workspace (first call on the plan)
int ensure_motion_workspace(fdr_plan* p, const char* fn);
// c (scaled by 1 / (M N) already) in the real parts of motion.plane, and sum |x| in motion.part[motion_pad_partials]
int motion_cepstrum_plane(fdr_plan* p, const float* d_img, int rows, int cols, int stride, hipStream_t s);
// the search on the plane, in three steps around the cepstrum: prepare (before it: the table grown to `a`, the trig table uploaded),
// launch (after it: the score gather, the table to d_scores when that is not null and to the host copy, asynchronous on `s`) and,
// once `s` is synchronised and `sum` (sum |x|) read back, the pick from the host copy
int motion_search_prepare(fdr_plan* p, const char* fn, const MotionArgs& a, hipStream_t s);
int motion_search_launch(fdr_plan* p, const MotionArgs& a, float* d_scores, hipStream_t s);
void motion_search_pick(const fdr_plan* p, const MotionArgs& a, double sum, fdr_motion_estimate* est);
// median of v (destroys its order), as numpy.median: the mean of the two middle values for an even count
double median_of(std::vector<double>& v);

// ---- the host-pointer forms of a single-image call and of a TV batch (fdr_api_plan.hip) ----
// The rows x cols image in through the plan's staging, run(d_in, d_out) on the null stream, the out_rows x out_cols result back
// (none when `out` is null), in the phases H2D, COMPUTE and D2H; synchronous.  The caller has checked everything that can be refused.
int host_image_call(fdr_plan* p, const char* fn, const float* in, int rows, int cols, int stride, float* out, int out_rows, int out_cols,
                    int out_stride, const std::function<int(const float* d_in, float* d_out)>& run);
// the dense one-shot device copy of the host weights of a crop call (none for null: d_w stays empty)
int stage_crop_weights(const char* fn, const float* weights_host, int rows, int cols, int wstride, DeviceBuffer* d_w);
// What every TV batch entry refuses first, in this order: a null plan or params, a negative count, then (count == 0 is FDR_OK with
// nothing done) null images or output.  False: the entry returns *rc now; true: there is a batch to check.
bool tv_batch_begin(const char* fn, const void* p, const void* params, int count, const void* imgs, const void* out, int* rc);
// the host-pointer form of a TV batch: every image in (dense, one-shot device buffers), run(d_in, in_pitch, d_out, out_pitch) on the
// null stream, every out_rows x out_cols window back, in the phases H2D, COMPUTE and D2H; synchronous
using HostBatchRun = std::function<int(const float* d_in, size_t in_pitch, float* d_out, size_t out_pitch)>;
int host_batch_call(fdr_plan* p, const char* fn, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride, float* out_host,
                    size_t out_pitch, int out_stride, int out_rows, int out_cols, const HostBatchRun& run);

// ---- the plan's transforms (fdr_api_misc.hip) ----
// unscaled 2-D transform in place on d (M x N), rows then columns as fft/fft_serial.cpp:113-139
int dft2d_dev(fdr_plan* p, float2* d, float2* work2, bool inverse, hipStream_t s);
// what every pass of a path takes from the plan; the caller adds its buffers and windows
MixRowArgs mixed_row_args(const fdr_plan* p);
MixColArgs mixed_col_args(const fdr_plan* p);
RowArgs panel_row_args(const fdr_plan* p);  // M, pstride, half, num_cu (a pass over fewer rows, as the PSF's, overrides M)
ColArgs panel_col_args(const fdr_plan* p);  // N, num_cu, pstride, npanels, packed0

}  // namespace fdr
