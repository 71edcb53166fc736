// fft/fft.hpp -- drop-in counterpart of the reference's fft/fft.hpp for the GPU namespace (reference fft/fft.hpp:31-45)
// and the serial namespace (:9-18).  Same names, same argument meaning, same error behaviour (print
// "Error: file:line, msg" and exit(1), fft/fft_gpu.cu:59-66); everything is a thin call into the C ABI of libfdr.so
// (include/fdr.h).  Link with -lfdr.
//
//   fft_gpu::wienerDeblur_RGB_optimized / _naive   fft/fft_gpu.cu:279-394 / :400-512
//   fft_gpu::fft_radix2_kernel / transform_row_kernel / dft_naive_kernel / my_dft2D / wienerDeblur_myfft
//                                                  declared at fft/fft.hpp:35-44, empty or missing in the reference
//   fft_serial::*                                  fft/fft_serial.cpp:40-261, run on the GPU in the parity mode
// Differences that are deliberate: the PSF spectrum is built once per call, not once per
// channel; wienerDeblur_RGB_* follow the SERIAL DRIVER's semantics by default (normalise over the padded area, then
// crop: serial.cpp:34-39) because ./serial is the parity target -- Options::norm_area = FDR_NORM_CROPPED gives the
// reference GPU order (fft/fft_gpu.cu:367-368,379-381).  Every entry point takes its mode / area / device as an
// argument (Options); the argument-free overloads of the reference's signatures use process-wide defaults.
#pragma once
#include "../utils.hpp"
#include <algorithm>
#include <atomic>
#include <complex>
#include <iostream>
#include <map>
#include <string>
#include <vector>

namespace fft_gpu {

struct Options {
    int mode = FDR_MODE_FAST;         // FDR_MODE_FAST or FDR_MODE_PARITY (bit-identical FFT arithmetic to fft_serial)
    int norm_area = FDR_NORM_PADDED;  // FDR_NORM_PADDED (./serial semantics) or FDR_NORM_CROPPED (reference ./gpu, fft_gpu.cu:379-381)
    int device = 0;
    bool mixed_radix = false;         // FDR_MODE_FAST: 2^a 3^b 5^c plan sizes by mixed-radix FFTs (FDR_FLAG_MIXED_RADIX) in wienerDeblur_myfft
    float cls_gamma = 0.f;            // > 0: constrained least-squares filter W = conj(H) / (|H|^2 + K + gamma L^2) (fdr_set_psf_cls,
                                      // FDR_MODE_FAST only: a parity plan refuses it); 0: the Wiener filter
    int pad_mode = FDR_PAD_ZERO;      // FDR_PAD_SMOOTH: wienerDeblur_RGB_optimized / _naive continue the picture smoothly into the padding
                                      // (FDR_OPT_PAD_MODE, FDR_MODE_FAST only: a parity plan refuses it) on a plan of the next powers of two of
                                      // rows + psf.rows - 1 and cols + psf.cols - 1 -- up to 4x the plan of FDR_PAD_ZERO for a picture whose
                                      // sides are powers of two already
};
// process-wide defaults of the reference-signature overloads (the drivers' --mode / --norm flags); atomics: reading
// them from several threads is safe, and no entry point ever changes them behind the caller's back
inline std::atomic<int>& default_mode() { static std::atomic<int> m{FDR_MODE_FAST}; return m; }
inline std::atomic<int>& default_norm() { static std::atomic<int> n{FDR_NORM_PADDED}; return n; }
inline std::atomic<float>& default_cls_gamma() { static std::atomic<float> g{0.f}; return g; }
inline void set_mode(int mode) { default_mode().store(mode); }
inline void set_norm_area(int area) { default_norm().store(area); }
inline void set_cls_gamma(float gamma) { default_cls_gamma().store(gamma); }
inline std::atomic<int>& default_pad_mode() { static std::atomic<int> m{FDR_PAD_ZERO}; return m; }
inline void set_pad_mode(int pad_mode) { default_pad_mode().store(pad_mode); }
inline Options defaults() {
    Options o;
    o.mode = default_mode().load(); o.norm_area = default_norm().load(); o.cls_gamma = default_cls_gamma().load();
    o.pad_mode = default_pad_mode().load();
    return o;
}

// the plan's filter from a host PSF: Wiener, or CLS when o.cls_gamma != 0
inline void set_psf_opts(fdr_plan* plan, const Mat& psf, float K, const Options& o) {
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    if (o.cls_gamma != 0.f) FDR_CHECK(fdr_set_psf_cls(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols, K, o.cls_gamma));
    else FDR_CHECK(fdr_set_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols, K));
}

// the plan's padding: plans are cached between calls, so a plan that served FDR_PAD_SMOOTH is set back (a plan that has no
// smooth padding refuses the option and pads with zeros anyway)
inline void set_pad_opts(fdr_plan* plan, const Options& o) {
    if (o.pad_mode != FDR_PAD_ZERO) FDR_CHECK(fdr_plan_set_option(plan, FDR_OPT_PAD_MODE, o.pad_mode));
    else (void)fdr_plan_set_option(plan, FDR_OPT_PAD_MODE, FDR_PAD_ZERO);
}
// the plan of the RGB entry points: the next powers of two of the picture's sides, with FDR_PAD_SMOOTH of the sides plus the PSF's reach
inline int pad_plan_rows(int rows, const Mat& psf, const Options& o) { return nextPowerOfTwo(o.pad_mode == FDR_PAD_SMOOTH ? rows + psf.rows - 1 : rows); }
inline int pad_plan_cols(int cols, const Mat& psf, const Options& o) { return nextPowerOfTwo(o.pad_mode == FDR_PAD_SMOOTH ? cols + psf.cols - 1 : cols); }

// The reference's Profiler buckets (fft/fft_gpu.cu:17-57).  alloc / h2d / pre / compute / d2h come from
// fdr_plan_phase_times (hipEvent pairs on the streams the work ran on); post is the host time of wrapping the results.
struct Profiler {
    double t_alloc = 0, t_h2d = 0, t_pre = 0, t_compute = 0, t_d2h = 0, t_post = 0;
    void add(fdr_plan* plan) {
        float ms[FDR_N_PHASES];
        FDR_CHECK(fdr_plan_phase_times(plan, ms, 1));
        t_alloc += ms[FDR_PHASE_ALLOC]; t_h2d += ms[FDR_PHASE_H2D]; t_pre += ms[FDR_PHASE_PRE];
        t_compute += ms[FDR_PHASE_COMPUTE]; t_d2h += ms[FDR_PHASE_D2H]; t_post += ms[FDR_PHASE_POST];
    }
    void print(const std::string& title) const {
        std::cout << "=== " << title << " Profiling (3 Channels) ===" << std::endl;
        std::cout << "[1. Allocation]  Time: " << t_alloc << " ms (plan: twiddles + workspaces)" << std::endl;
        std::cout << "[2. H2D Copy]    Time: " << t_h2d << " ms (Raw Img + PSF)" << std::endl;
        std::cout << "[3. Pre-process] Time: " << t_pre << " ms (Padding + PSF FFT)" << std::endl;
        std::cout << "[4. GPU Compute] Time: " << t_compute << " ms (FFT + Filter + IFFT + Normalize)" << std::endl;
        std::cout << "[5. D2H Copy]    Time: " << t_d2h << " ms (Result Transfer)" << std::endl;
        std::cout << "[6. Post-process]Time: " << t_post << " ms (CPU Copy)" << std::endl;
        std::cout << "--------------------------------------------" << std::endl;
        std::cout << "Total (Sum)      Time: " << (t_alloc + t_h2d + t_pre + t_compute + t_d2h + t_post) << " ms" << std::endl;
        std::cout << "============================================" << std::endl;
    }
};

// Plans kept BETWEEN calls of wienerDeblur_RGB_optimized and of the per-channel operator wienerDeblur_myfft ("Reuse Memory"
// taken one step further than fft/fft_gpu.cu:304-322, which still allocates once per call): a driver that warms up and then
// times the entry point (gpu.cpp:96-105), loops over the channels (serial.cpp:34-39) or calls once per picture of one size
// pays for the twiddle tables, the workspaces and their hipFree once per thread (measured on 782 x 1920: the timed
// _optimized call 17.6 -> 1.1 ms).  wienerDeblur_RGB_naive keeps allocating per channel, as its name says.  Per thread (a plan serves
// one host thread at a time), at most plan_cache_capacity() plans (default 4), least recently used evicted.  The reference
// frees everything per call (fft/fft_gpu.cu:389-393); what this header retains instead is bounded and released:
//   * when the owning thread ends (the cache is a thread_local OBJECT; its destructor destroys every plan -- on the main
//     thread that happens at exit() before any atexit handler, i.e. while the HIP runtime is still up; once the process is
//     past that point fdr_plan_destroy only frees host memory, see fdr.h),
//   * on demand: fft_gpu::release_cached_plans() (this thread's), fft_gpu::set_plan_cache_capacity(n) (0 = keep nothing
//     between calls: the reference's behaviour).
struct PlanCache {
    struct Entry { int device, M, N, mode; unsigned flags; fdr_plan* plan; };
    std::vector<Entry> entries;
    PlanCache() = default;
    PlanCache(const PlanCache&) = delete;
    PlanCache& operator=(const PlanCache&) = delete;
    ~PlanCache() { clear(); }
    void clear() {
        for (Entry& e : entries) fdr_plan_destroy(e.plan);
        entries.clear();
    }
    static std::atomic<int>& capacity() { static std::atomic<int> c{4}; return c; }
    // A plan handed out with capacity 0 is not retained: the caller destroys it (see PlanLease).
    fdr_plan* get(int device, int M, int N, int mode, bool* created, unsigned flags = 0u) {
        for (size_t i = 0; i < entries.size(); ++i)
            if (entries[i].device == device && entries[i].M == M && entries[i].N == N && entries[i].mode == mode && entries[i].flags == flags) {
                const Entry e = entries[i];
                entries.erase(entries.begin() + (long)i);
                entries.push_back(e);  // most recently used last
                *created = false;
                return e.plan;
            }
        const int cap = capacity().load();
        while (!entries.empty() && (int)entries.size() >= (cap > 0 ? cap : 1)) { fdr_plan_destroy(entries.front().plan); entries.erase(entries.begin()); }
        fdr_plan* plan = nullptr;
        FDR_CHECK(fdr_plan_create(device, M, N, mode, flags, &plan));
        entries.push_back(Entry{device, M, N, mode, flags, plan});
        *created = true;
        return plan;
    }
    // end of an entry point: with capacity 0 nothing stays allocated between calls
    void settle() { if (capacity().load() <= 0) clear(); }
};
inline PlanCache& plan_cache() { static thread_local PlanCache c; return c; }
// Destroys the calling thread's cached plans now (device workspaces, filter, staging buffers, streams).
inline void release_cached_plans() { plan_cache().clear(); }
// Plans kept per thread between calls (default 4); 0 = allocate and free inside every call, as fft/fft_gpu.cu:304-322,389-393.
inline void set_plan_cache_capacity(int n) { PlanCache::capacity().store(n < 0 ? 0 : n); if (n <= 0) plan_cache().clear(); }
inline int plan_cache_capacity() { return PlanCache::capacity().load(); }
struct PlanCacheSettle { ~PlanCacheSettle() { plan_cache().settle(); } };

inline Mat run_channel(fdr_plan* plan, const Mat& img, int norm_area) {
    Mat src = img.isContinuous() ? img : img.clone();
    Mat out(img.rows, img.cols, CV_32F);
    FDR_CHECK(fdr_wiener_f32(plan, src.ptr<float>(0), img.rows, img.cols, img.cols, out.ptr<float>(0), img.cols, norm_area));
    return out;
}

// Version A (fft/fft_gpu.cu:279-394): one plan, one PSF spectrum, all channels; replaces every element of `channels`.
inline void wienerDeblur_RGB_optimized(std::vector<Mat>& channels, const Mat& psf, float K, const Options& o) {
    if (channels.empty()) return;
    Profiler p;
    const int imgRows = channels[0].rows, imgCols = channels[0].cols;
    bool created = false;
    PlanCacheSettle settle_;
    fdr_plan* plan = plan_cache().get(o.device, pad_plan_rows(imgRows, psf, o), pad_plan_cols(imgCols, psf, o), o.mode, &created);
    if (!created) { float discard[FDR_N_PHASES]; FDR_CHECK(fdr_plan_phase_times(plan, discard, 1)); }  // this call's phases only ([1. Allocation] = 0: reused)
    set_pad_opts(plan, o);
    set_psf_opts(plan, psf, K, o);
    // all channels through the host batch pipeline: upload, restoration and download of consecutive channels overlap
    // (what the stream + pinned-buffer set-up of fft/fft_gpu.cu:304-350 is after)
    bool same = true;
    for (const Mat& c : channels) same = same && c.rows == imgRows && c.cols == imgCols && c.type() == CV_32F;
    if (same) {
        std::vector<Mat> src, out;
        std::vector<const float*> ins;
        std::vector<float*> outs;
        auto a = high_resolution_clock::now();
        for (const Mat& c : channels) {
            src.push_back(c.isContinuous() ? c : c.clone());
            out.push_back(Mat(imgRows, imgCols, CV_32F));
        }
        p.t_post += getElapsedMs(a, high_resolution_clock::now());
        for (size_t i = 0; i < channels.size(); ++i) { ins.push_back(src[i].ptr<float>(0)); outs.push_back(out[i].ptr<float>(0)); }
        FDR_CHECK(fdr_wiener_batch_ptrs_f32(plan, ins.data(), outs.data(), (int)channels.size(), imgRows, imgCols, imgCols, imgCols, o.norm_area));
        for (size_t i = 0; i < channels.size(); ++i) channels[i] = out[i];
    } else {
        for (size_t i = 0; i < channels.size(); ++i) channels[i] = run_channel(plan, channels[i], o.norm_area);
    }
    p.add(plan);
    p.print("FAST (Reuse Memory)");
}
inline void wienerDeblur_RGB_optimized(std::vector<Mat>& channels, const Mat& psf, float K) {
    wienerDeblur_RGB_optimized(channels, psf, K, defaults());
}

// Version B (fft/fft_gpu.cu:400-512): every channel allocates, builds the PSF spectrum and frees.
inline void wienerDeblur_RGB_naive(std::vector<Mat>& channels, const Mat& psf, float K, const Options& o) {
    Profiler p;
    for (size_t i = 0; i < channels.size(); ++i) {
        fdr_plan* plan = nullptr;
        FDR_CHECK(fdr_plan_create(o.device, pad_plan_rows(channels[i].rows, psf, o), pad_plan_cols(channels[i].cols, psf, o), o.mode, 0, &plan));
        set_pad_opts(plan, o);
        set_psf_opts(plan, psf, K, o);
        channels[i] = run_channel(plan, channels[i], o.norm_area);
        p.add(plan);
        fdr_plan_destroy(plan);
    }
    p.print("SLOW (Naive Allocation)");
}
inline void wienerDeblur_RGB_naive(std::vector<Mat>& channels, const Mat& psf, float K) {
    wienerDeblur_RGB_naive(channels, psf, K, defaults());
}

// The Richardson-Lucy of every channel as ONE batched call (fdr_richardson_lucy_batch_f32, accelerated:
// fdr_richardson_lucy_batch_accel_f32, include/fdr.h): the channels
// of a picture share the PSF (and the weights), so a launch group of channels.size() images (at most 8) runs every pass of the
// iteration once for all of them -- with the bits of the per-channel calls.  False (nothing done) when the channels differ in size
// or type: the caller then loops.
inline bool rl_channels_batched(fdr_plan* plan, std::vector<Mat>& channels, const float* weights, fdr_rl_batch_params prm, bool accelerate = false) {
    const int rows = channels[0].rows, cols = channels[0].cols, count = (int)channels.size();
    for (const Mat& c : channels)
        if (c.rows != rows || c.cols != cols || c.type() != CV_32F) return false;
    const int out_rows = rows, out_cols = cols;
    const size_t px = (size_t)rows * cols;
    std::vector<float> in(px * count), out(px * count);
    for (int i = 0; i < count; ++i)
        for (int r = 0; r < rows; ++r) std::copy(channels[i].ptr<float>(r), channels[i].ptr<float>(r) + cols, in.begin() + i * px + (size_t)r * cols);
    if (prm.free_boundary) { prm.out_rows = out_rows; prm.out_cols = out_cols; }
    FDR_CHECK(fdr_plan_set_batching(plan, 1, std::min(count, 8)));
    if (accelerate)
        FDR_CHECK(fdr_richardson_lucy_batch_accel_f32(plan, in.data(), px, count, rows, cols, cols, weights, cols, out.data(), px, cols, &prm, nullptr, 0));
    else
        FDR_CHECK(fdr_richardson_lucy_batch_f32(plan, in.data(), px, count, rows, cols, cols, weights, cols, out.data(), px, cols, &prm));
    FDR_CHECK(fdr_plan_set_batching(plan, 1, 1));  // the cached plan goes back as it came
    for (int i = 0; i < count; ++i) {
        Mat o(rows, cols, CV_32F);
        std::copy(out.begin() + i * px, out.begin() + (i + 1) * px, o.ptr<float>(0));
        channels[i] = o;
    }
    return true;
}

// Richardson-Lucy deconvolution (fdr_richardson_lucy_f32, include/fdr.h) of every channel, `iterations` steps each, in place: one
// cached FDR_MODE_FAST plan (each dimension padded to the next power of two, at least 8 rows and 32 columns; the padding stays
// zero), the operator PSF set once, each channel normalised by o.norm_area.  o.mode and o.cls_gamma do not apply.  accelerate: the
// iteration with Biggs & Andrews' vector extrapolation (fdr_richardson_lucy_accel_f32).  Either way the channels go through one
// batched call (rl_channels_batched); channels of different sizes or types run one by one.
inline void richardsonLucy_RGB(std::vector<Mat>& channels, const Mat& psf, int iterations, const Options& o, bool accelerate = false) {
    if (channels.empty()) return;
    const int rows = channels[0].rows, cols = channels[0].cols;
    bool created = false;
    PlanCacheSettle settle_;
    fdr_plan* plan = plan_cache().get(o.device, std::max(8, nextPowerOfTwo(rows)), std::max(32, nextPowerOfTwo(cols)), FDR_MODE_FAST, &created);
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    FDR_CHECK(fdr_set_operator_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols));
    if (rl_channels_batched(plan, channels, nullptr, fdr_rl_batch_params{iterations, o.norm_area, 0, 0.f, 0, 0}, accelerate)) return;
    for (Mat& c : channels) {
        Mat src = c.isContinuous() ? c : c.clone();
        Mat out(c.rows, c.cols, CV_32F);
        if (accelerate)
            FDR_CHECK(fdr_richardson_lucy_accel_f32(plan, src.ptr<float>(0), c.rows, c.cols, c.cols, out.ptr<float>(0), c.cols, iterations,
                                                    o.norm_area, nullptr));
        else
            FDR_CHECK(fdr_richardson_lucy_f32(plan, src.ptr<float>(0), c.rows, c.cols, c.cols, out.ptr<float>(0), c.cols, iterations, o.norm_area));
        c = out;
    }
}
inline void richardsonLucy_RGB(std::vector<Mat>& channels, const Mat& psf, int iterations, bool accelerate = false) {
    richardsonLucy_RGB(channels, psf, iterations, defaults(), accelerate);
}
// Free-boundary, weighted Richardson-Lucy (fdr_richardson_lucy_free_f32, include/fdr.h) of every channel, in place, for a picture
// that is a crop of a larger scene: one cached FDR_MODE_FAST plan with room for the PSF's reach beyond the picture (the next powers
// of two of rows + psf.rows - 1 and cols + psf.cols - 1, at least 8 x 32), the operator PSF set once, `weights` (CV_32F, the
// picture's size, in [0, 1]; empty = all ones; 0 = ignore the pixel) shared by the channels, each channel normalised by o.norm_area.
// accelerate as richardsonLucy_RGB (fdr_richardson_lucy_free_accel_f32); one batched call either way, the coverage computed once.
inline void richardsonLucyFree_RGB(std::vector<Mat>& channels, const Mat& psf, int iterations, const Mat& weights, const Options& o,
                                   float sigma = FDR_RL_SIGMA, bool accelerate = false) {
    if (channels.empty()) return;
    const int rows = channels[0].rows, cols = channels[0].cols;
    if (!weights.empty() && (weights.rows != rows || weights.cols != cols || weights.type() != CV_32F)) {
        std::cerr << "richardsonLucyFree_RGB: the weights must be CV_32F and have the picture's size\n";
        exit(1);
    }
    bool created = false;
    PlanCacheSettle settle_;
    fdr_plan* plan = plan_cache().get(o.device, std::max(8, nextPowerOfTwo(rows + psf.rows - 1)), std::max(32, nextPowerOfTwo(cols + psf.cols - 1)),
                                      FDR_MODE_FAST, &created);
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    FDR_CHECK(fdr_set_operator_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols));
    Mat w = weights.empty() || weights.isContinuous() ? weights : weights.clone();
    if (rl_channels_batched(plan, channels, w.empty() ? nullptr : w.ptr<float>(0), fdr_rl_batch_params{iterations, o.norm_area, 1, sigma, rows, cols},
                            accelerate))
        return;
    for (Mat& c : channels) {
        Mat src = c.isContinuous() ? c : c.clone();
        Mat out(c.rows, c.cols, CV_32F);
        const fdr_rlfree_params prm = {iterations, sigma, o.norm_area, c.rows, c.cols};
        if (accelerate)
            FDR_CHECK(fdr_richardson_lucy_free_accel_f32(plan, src.ptr<float>(0), c.rows, c.cols, c.cols, w.empty() ? nullptr : w.ptr<float>(0),
                                                         cols, out.ptr<float>(0), c.cols, &prm, nullptr));
        else
            FDR_CHECK(fdr_richardson_lucy_free_f32(plan, src.ptr<float>(0), c.rows, c.cols, c.cols, w.empty() ? nullptr : w.ptr<float>(0), cols,
                                                   out.ptr<float>(0), c.cols, &prm));
        c = out;
    }
}
inline void richardsonLucyFree_RGB(std::vector<Mat>& channels, const Mat& psf, int iterations, const Mat& weights = Mat(),
                                   bool accelerate = false) {
    richardsonLucyFree_RGB(channels, psf, iterations, weights, defaults(), FDR_RL_SIGMA, accelerate);
}
// The channels of richardsonLucyTV_RGB as ONE batched call (fdr_richardson_lucy_tv_batch_f32, include/fdr.h): a launch group of
// channels.size() images (at most 8) runs the factor launch and every pass of the iteration once for all of them.  False (nothing
// done) when the channels differ in size or type or are more than 8: the caller then loops.
inline bool rltv_channels_batched(fdr_plan* plan, std::vector<Mat>& channels, const float* weights, fdr_rl_tv_batch_params prm) {
    const int rows = channels[0].rows, cols = channels[0].cols, count = (int)channels.size();
    if (count > 8) return false;
    for (const Mat& c : channels)
        if (c.rows != rows || c.cols != cols || c.type() != CV_32F) return false;
    const size_t px = (size_t)rows * cols;
    std::vector<float> in(px * count), out(px * count);
    for (int i = 0; i < count; ++i)
        for (int r = 0; r < rows; ++r) std::copy(channels[i].ptr<float>(r), channels[i].ptr<float>(r) + cols, in.begin() + i * px + (size_t)r * cols);
    prm.out_rows = rows; prm.out_cols = cols;
    FDR_CHECK(fdr_plan_set_batching(plan, 1, count));
    FDR_CHECK(fdr_richardson_lucy_tv_batch_f32(plan, in.data(), px, count, rows, cols, cols, weights, cols, out.data(), px, cols, &prm));
    FDR_CHECK(fdr_plan_set_batching(plan, 1, 1));  // the cached plan goes back as it came
    for (int i = 0; i < count; ++i) {
        Mat o(rows, cols, CV_32F);
        std::copy(out.begin() + i * px, out.begin() + (i + 1) * px, o.ptr<float>(0));
        channels[i] = o;
    }
    return true;
}
// Richardson-Lucy with a total-variation prior (fdr_richardson_lucy_tv_f32, include/fdr.h) of every channel, in place:
// lambda in 0 .. FDR_RLTV_MAX_LAMBDA weighs the prior (0 is the unregularised form), eps (the units of the picture; 0 =
// FDR_RLTV_EPS) smooths |grad u|.  free_boundary: on the plan and with the weights and sigma of richardsonLucyFree_RGB, for a picture
// that is a crop; otherwise on the plan of richardsonLucy_RGB, and `weights` must be empty.  Each channel normalised by o.norm_area.
// The channels go through one batched call (rltv_channels_batched) with the bits of the per-channel calls; channels of different
// sizes or types run one by one.  coupled: the channels share one vectorial TV prior (FDR_TV_COUPLE_CHANNELS: an edge falls in the
// same place in every channel); it needs channels of one size and type, at most 8.
inline void richardsonLucyTV_RGB(std::vector<Mat>& channels, const Mat& psf, int iterations, float lambda, float eps, bool free_boundary,
                                 const Mat& weights, const Options& o, float sigma = FDR_RL_SIGMA, bool coupled = false) {
    if (channels.empty()) return;
    const int rows = channels[0].rows, cols = channels[0].cols;
    if (!weights.empty() && (!free_boundary || weights.rows != rows || weights.cols != cols || weights.type() != CV_32F)) {
        std::cerr << "richardsonLucyTV_RGB: weights belong to the free-boundary form, must be CV_32F and have the picture's size\n";
        exit(1);
    }
    bool created = false;
    PlanCacheSettle settle_;
    const int M = free_boundary ? nextPowerOfTwo(rows + psf.rows - 1) : nextPowerOfTwo(rows);
    const int N = free_boundary ? nextPowerOfTwo(cols + psf.cols - 1) : nextPowerOfTwo(cols);
    fdr_plan* plan = plan_cache().get(o.device, std::max(8, M), std::max(32, N), FDR_MODE_FAST, &created);
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    FDR_CHECK(fdr_set_operator_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols));
    Mat w = weights.empty() || weights.isContinuous() ? weights : weights.clone();
    if (rltv_channels_batched(plan, channels, w.empty() ? nullptr : w.ptr<float>(0),
                              fdr_rl_tv_batch_params{iterations, free_boundary ? 1 : 0, lambda, eps, o.norm_area, sigma, rows, cols,
                                                     coupled ? FDR_TV_COUPLE_CHANNELS : FDR_TV_COUPLE_NONE}))
        return;
    if (coupled) {
        std::cerr << "richardsonLucyTV_RGB: coupled channels must have one size, be CV_32F and be at most 8\n";
        exit(1);
    }
    for (Mat& c : channels) {
        Mat src = c.isContinuous() ? c : c.clone();
        Mat out(c.rows, c.cols, CV_32F);
        const fdr_rl_tv_params prm = {iterations, free_boundary ? 1 : 0, lambda, eps, o.norm_area, sigma, c.rows, c.cols};
        FDR_CHECK(fdr_richardson_lucy_tv_f32(plan, src.ptr<float>(0), c.rows, c.cols, c.cols, w.empty() ? nullptr : w.ptr<float>(0), cols,
                                             out.ptr<float>(0), c.cols, &prm));
        c = out;
    }
}
inline void richardsonLucyTV_RGB(std::vector<Mat>& channels, const Mat& psf, int iterations, float lambda, float eps = 0.f,
                                 bool free_boundary = false, const Mat& weights = Mat(), bool coupled = false) {
    richardsonLucyTV_RGB(channels, psf, iterations, lambda, eps, free_boundary, weights, defaults(), FDR_RL_SIGMA, coupled);
}
// What the two multi-frame drivers below share.  frames[k] holds the channels of exposure k of ONE scene, psfs[k] its PSF (CV_32F;
// top-left in the plan as for richardsonLucyFree_RGB; sums are not normalised: a PSF's sum is its frame's relative exposure, a
// registration shift goes into the PSF).  One cached FDR_MODE_FAST plan with room for the largest PSF's reach, the frame tables set
// ONCE, then restore(plan, in, px, weights or null, out) once per channel -- `in` that channel of all K <= FDR_MAX_FRAMES exposures,
// dense, px floats apart -- on launch groups of K frames; every channel of frames[0] is replaced by the joint estimate.  `weights`
// (CV_32F, the picture's size; empty = all ones) serves every frame.
// register_frames of the two multi-frame drivers: the exposures are NOT registered to each other (hand shake).  Each frame's translation
// against frame 0 is estimated with the PSFs on the mean of its channels (fdr_register_frames_f32, search range max_shift pixels, 0 =
// min(rows, cols) / 4), folded into its PSF (fdr_psf_shift_f32, padded by max_shift + 2) and the frame tables are set from the shifted
// PSFs, laid into plan-sized planes rolled back by the padding so that the estimate stays where frame 0 is.  `shifts`, when not null,
// receives the K estimates.
struct RegisterOptions {
    bool on = false;
    int max_shift = 0;
    std::vector<fdr_frame_shift>* shifts = nullptr;
};
template <class Restore>
inline void frames_each_channel(const char* who, std::vector<std::vector<Mat>>& frames, const std::vector<Mat>& psfs, const Mat& weights,
                                const Options& o, const Restore& restore, const RegisterOptions& reg = RegisterOptions()) {
    const int K = (int)frames.size();
    if (K == 0 || frames[0].empty()) return;
    const int rows = frames[0][0].rows, cols = frames[0][0].cols;
    const size_t nch = frames[0].size();
    bool ok = K <= FDR_MAX_FRAMES && (int)psfs.size() == K && (weights.empty() || (weights.rows == rows && weights.cols == cols && weights.type() == CV_32F));
    int pr = 0, pc = 0;
    for (int k = 0; k < K && ok; ++k) {
        ok = frames[k].size() == nch && psfs[k].type() == CV_32F && psfs[k].rows > 0 && psfs[k].cols > 0;
        for (size_t c = 0; c < nch && ok; ++c) ok = frames[k][c].rows == rows && frames[k][c].cols == cols && frames[k][c].type() == CV_32F;
        if (ok) { pr = std::max(pr, psfs[k].rows); pc = std::max(pc, psfs[k].cols); }
    }
    if (!ok) {
        std::cerr << who << ": 1 .. 8 frames of the same CV_32F channels and size, one CV_32F PSF each, CV_32F weights of the picture's size\n";
        exit(1);
    }
    bool created = false;
    PlanCacheSettle settle_;
    const int pad = reg.on ? (reg.max_shift > 0 ? reg.max_shift : std::min(rows, cols) / 4) + 2 : 0;  // the room of a registration
    const int M = std::max(8, nextPowerOfTwo(rows + pr + 2 * pad - 1)), N = std::max(32, nextPowerOfTwo(cols + pc + 2 * pad - 1));
    fdr_plan* plan = plan_cache().get(o.device, M, N, FDR_MODE_FAST, &created);
    const size_t ppx = (size_t)pr * pc, px = (size_t)rows * cols;
    std::vector<float> tabs(ppx * K, 0.f), in(px * K);  // the PSFs padded with zeros (bottom, right) to one shape: top-left, nothing changes
    for (int k = 0; k < K; ++k)
        for (int r = 0; r < psfs[k].rows; ++r) std::copy(psfs[k].ptr<float>(r), psfs[k].ptr<float>(r) + psfs[k].cols, tabs.begin() + k * ppx + (size_t)r * pc);
    if (reg.on) {
        for (int k = 0; k < K; ++k)  // the mean of the channels, summed in channel order
            for (size_t i = 0; i < px; ++i) {
                float acc = 0.f;
                for (size_t c = 0; c < nch; ++c) acc += frames[k][c].ptr<float>((int)(i / cols))[i % cols];
                in[k * px + i] = acc / (float)nch;
            }
        std::vector<fdr_frame_shift> est(K);
        const fdr_register_params rp = {0, reg.max_shift, reg.max_shift, 0.f, nullptr};
        FDR_CHECK(fdr_register_frames_f32(plan, in.data(), px, K, rows, cols, cols, tabs.data(), ppx, pr, pc, pc, &rp, est.data()));
        if (reg.shifts) *reg.shifts = est;
        const int sr = pr + 2 * pad, sc = pc + 2 * pad;
        std::vector<float> moved((size_t)sr * sc * K), planes((size_t)M * N * K, 0.f);
        const fdr_psf_shift_params sp = {pad, pad, nullptr};
        FDR_CHECK(fdr_psf_shift_f32(o.device, tabs.data(), ppx, K, pr, pc, pc, est.data(), &sp, moved.data(), (size_t)sr * sc, sc));
        for (int k = 0; k < K; ++k)  // top-left in the plan, rolled back by the padding (periodic)
            for (int r = 0; r < sr; ++r)
                for (int c = 0; c < sc; ++c)
                    planes[(size_t)k * M * N + (size_t)((r - pad + M) % M) * N + (c - pad + N) % N] = moved[(size_t)k * sr * sc + (size_t)r * sc + c];
        FDR_CHECK(fdr_set_frame_psfs(plan, planes.data(), (size_t)M * N, K, M, N, N));
    } else {
        FDR_CHECK(fdr_set_frame_psfs(plan, tabs.data(), ppx, K, pr, pc, pc));
    }
    Mat w = weights.empty() || weights.isContinuous() ? weights : weights.clone();
    FDR_CHECK(fdr_plan_set_batching(plan, 1, K));
    for (size_t c = 0; c < nch; ++c) {
        for (int k = 0; k < K; ++k)
            for (int r = 0; r < rows; ++r) std::copy(frames[k][c].ptr<float>(r), frames[k][c].ptr<float>(r) + cols, in.begin() + k * px + (size_t)r * cols);
        Mat out(rows, cols, CV_32F);
        FDR_CHECK(restore(plan, in.data(), px, w.empty() ? nullptr : w.ptr<float>(0), out.ptr<float>(0)));
        frames[0][c] = out;
    }
    FDR_CHECK(fdr_plan_set_batching(plan, 1, 1));  // the cached plan goes back as it came
}
// Multi-frame Richardson-Lucy (fdr_richardson_lucy_frames_f32, include/fdr.h) of the channels of K exposures (frames_each_channel
// above): the joint free-boundary estimate, normalised by o.norm_area; lambda > 0 adds the TV prior of richardsonLucyTV_RGB.
inline void richardsonLucyFrames_RGB(std::vector<std::vector<Mat>>& frames, const std::vector<Mat>& psfs, int iterations, float lambda,
                                     float eps, const Mat& weights, const Options& o, float sigma = FDR_RL_SIGMA,
                                     const RegisterOptions& register_frames = RegisterOptions()) {
    if (frames.empty() || frames[0].empty()) return;
    const int K = (int)frames.size(), rows = frames[0][0].rows, cols = frames[0][0].cols;
    const fdr_rl_frames_params prm = {iterations, sigma, o.norm_area, rows, cols, lambda, eps};
    frames_each_channel("richardsonLucyFrames_RGB", frames, psfs, weights, o, [&](fdr_plan* plan, const float* in, size_t px, const float* w, float* out) {
        return fdr_richardson_lucy_frames_f32(plan, in, px, K, rows, cols, cols, w, 0, cols, out, cols, &prm);
    }, register_frames);
}
inline void richardsonLucyFrames_RGB(std::vector<std::vector<Mat>>& frames, const std::vector<Mat>& psfs, int iterations, float lambda = 0.f,
                                     float eps = 0.f, const Mat& weights = Mat()) {
    richardsonLucyFrames_RGB(frames, psfs, iterations, lambda, eps, weights, defaults());
}
// Multi-frame TV deconvolution (fdr_tv_deconv_frames_f32, include/fdr.h) of the channels of K exposures (frames_each_channel above):
// min mu sum_k Phi_k(blur_k(x)) + TV(x) by `iterations` ADMM steps, Phi_k least squares or, with poisson, the Poisson likelihood
// with the known background; normalised by o.norm_area.
inline void tvDeblurFrames_RGB(std::vector<std::vector<Mat>>& frames, const std::vector<Mat>& psfs, float mu, int iterations, bool poisson,
                               float background, const Mat& weights, const Options& o, float rho = 2.f, float nu = 0.f, bool anisotropic = false,
                               bool nonneg = false, const RegisterOptions& register_frames = RegisterOptions()) {
    if (frames.empty() || frames[0].empty()) return;
    const int K = (int)frames.size(), rows = frames[0][0].rows, cols = frames[0][0].cols;
    const fdr_tv_frames_params prm = {mu, rho, nu, background, poisson ? FDR_TV_FRAMES_POISSON : FDR_TV_FRAMES_LEAST_SQUARES, iterations,
                                      anisotropic ? 1 : 0, nonneg ? 1 : 0, o.norm_area, rows, cols, nullptr};
    frames_each_channel("tvDeblurFrames_RGB", frames, psfs, weights, o, [&](fdr_plan* plan, const float* in, size_t px, const float* w, float* out) {
        return fdr_tv_deconv_frames_f32(plan, in, px, K, rows, cols, cols, w, 0, cols, out, cols, &prm);
    }, register_frames);
}
inline void tvDeblurFrames_RGB(std::vector<std::vector<Mat>>& frames, const std::vector<Mat>& psfs, float mu, int iterations, bool poisson = false,
                               float background = 0.f, const Mat& weights = Mat()) {
    tvDeblurFrames_RGB(frames, psfs, mu, iterations, poisson, background, weights, defaults());
}
// What richardsonLucyBlind_RGB takes beside the picture and the start PSF: the form, the steps the PSF is held for, and the weights and
// coverage threshold of the free form.
struct BlindOptions {
    bool free_boundary = false;
    int psf_hold = 0;
    Mat weights;  // free form: CV_32F, the picture's size; empty = all ones
    float cov_sigma = FDR_RL_SIGMA;
};
// Blind Richardson-Lucy (fdr_richardson_lucy_blind_f32, include/fdr.h) of a picture, in place: the PSF is refined from psf_start
// (usually fdr_psf_gaussian) on the per-pixel mean of the channels with FDR_NORM_NONE, on the plan of richardsonLucy_RGB (free form: of
// richardsonLucyFree_RGB); then each channel goes through the non-blind call of the same form with that PSF -- the plan's operator
// tables are already its -- and the same iteration count, normalised by o.norm_area.  Returns the refined PSF.  It refines a PSF: a
// flat start does not move, zeros of the start stay zeros.
inline Mat richardsonLucyBlind_RGB(std::vector<Mat>& channels, const Mat& psf_start, int iterations, const BlindOptions& b, const Options& o) {
    if (channels.empty()) return Mat();
    const int rows = channels[0].rows, cols = channels[0].cols;
    if (!b.weights.empty() && (!b.free_boundary || b.weights.rows != rows || b.weights.cols != cols || b.weights.type() != CV_32F)) {
        std::cerr << "richardsonLucyBlind_RGB: the weights belong to the free-boundary form, must be CV_32F and have the picture's size\n";
        exit(1);
    }
    bool created = false;
    PlanCacheSettle settle_;
    const int M = b.free_boundary ? nextPowerOfTwo(rows + psf_start.rows - 1) : nextPowerOfTwo(rows);
    const int N = b.free_boundary ? nextPowerOfTwo(cols + psf_start.cols - 1) : nextPowerOfTwo(cols);
    fdr_plan* plan = plan_cache().get(o.device, std::max(8, M), std::max(32, N), FDR_MODE_FAST, &created);
    Mat psf = psf_start.clone();  // continuous; receives p_n
    Mat w = b.weights.empty() || b.weights.isContinuous() ? b.weights : b.weights.clone();
    const float* wp = w.empty() ? nullptr : w.ptr<float>(0);
    Mat mean(rows, cols, CV_32F), out(rows, cols, CV_32F);
    const float inv = (float)channels.size();
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            float sum = channels[0].ptr<float>(r)[c];
            for (size_t k = 1; k < channels.size(); ++k) sum += channels[k].ptr<float>(r)[c];
            mean.ptr<float>(r)[c] = sum / inv;
        }
    const fdr_blind_params bp = {iterations, b.free_boundary ? 1 : 0, b.psf_hold, FDR_NORM_NONE, b.cov_sigma, rows, cols};
    FDR_CHECK(fdr_richardson_lucy_blind_f32(plan, mean.ptr<float>(0), rows, cols, cols, wp, cols, psf.ptr<float>(0), psf.rows, psf.cols, psf.cols,
                                            out.ptr<float>(0), cols, &bp));
    for (Mat& c : channels) {
        Mat src = c.isContinuous() ? c : c.clone();
        Mat res(rows, cols, CV_32F);
        const fdr_rlfree_params prm = {iterations, b.cov_sigma, o.norm_area, rows, cols};
        if (b.free_boundary)
            FDR_CHECK(fdr_richardson_lucy_free_f32(plan, src.ptr<float>(0), rows, cols, cols, wp, cols, res.ptr<float>(0), cols, &prm));
        else
            FDR_CHECK(fdr_richardson_lucy_f32(plan, src.ptr<float>(0), rows, cols, cols, res.ptr<float>(0), cols, iterations, o.norm_area));
        c = res;
    }
    return psf;
}
inline Mat richardsonLucyBlind_RGB(std::vector<Mat>& channels, const Mat& psf_start, int iterations, const BlindOptions& b = BlindOptions()) {
    return richardsonLucyBlind_RGB(channels, psf_start, iterations, b, defaults());
}
// What richardsonLucyAuto_RGB takes beside the picture: the rule (FDR_RL_STOP_*) and its arguments as fdr_rl_auto_params has them
// (sigma 0 = estimated per channel; tau and check_every 0 = 1), the form, and the weights and coverage threshold of the free form.
struct RlAutoOptions {
    float sigma = 0.f, gain = 0.f, tau = 0.f;
    int check_every = 0;
    bool free_boundary = false, accelerate = false;
    Mat weights;
    float cov_sigma = FDR_RL_SIGMA;
};
// Richardson-Lucy that chooses its own iteration count (fdr_richardson_lucy_auto_f32, include/fdr.h) of every channel, in place: at
// most max_iterations steps of the form a.free_boundary / a.accelerate asks for, on the plan and operator PSF of richardsonLucy_RGB
// (free form: of richardsonLucyFree_RGB), stopped per channel by `rule`.  Returns the channels' results (iterations_done, stopped,
// sigma, target, statistic), in order.
inline std::vector<fdr_rl_auto_result> richardsonLucyAuto_RGB(std::vector<Mat>& channels, const Mat& psf, int max_iterations, int rule,
                                                              const RlAutoOptions& a, const Options& o) {
    std::vector<fdr_rl_auto_result> results;
    if (channels.empty()) return results;
    const int rows = channels[0].rows, cols = channels[0].cols;
    if (!a.weights.empty() && (!a.free_boundary || a.weights.rows != rows || a.weights.cols != cols || a.weights.type() != CV_32F)) {
        std::cerr << "richardsonLucyAuto_RGB: the weights belong to the free-boundary form, must be CV_32F and have the picture's size\n";
        exit(1);
    }
    bool created = false;
    PlanCacheSettle settle_;
    const int pr = a.free_boundary ? rows + psf.rows - 1 : rows, pc = a.free_boundary ? cols + psf.cols - 1 : cols;
    fdr_plan* plan = plan_cache().get(o.device, std::max(8, nextPowerOfTwo(pr)), std::max(32, nextPowerOfTwo(pc)), FDR_MODE_FAST, &created);
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    FDR_CHECK(fdr_set_operator_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols));
    Mat w = a.weights.empty() || a.weights.isContinuous() ? a.weights : a.weights.clone();
    for (Mat& c : channels) {
        Mat src = c.isContinuous() ? c : c.clone();
        Mat out(c.rows, c.cols, CV_32F);
        const fdr_rl_auto_params prm = {max_iterations, a.free_boundary ? 1 : 0, a.accelerate ? 1 : 0, rule, a.sigma, a.gain, a.tau, a.check_every,
                                        o.norm_area, a.cov_sigma, c.rows, c.cols};
        fdr_rl_auto_result res = {};
        FDR_CHECK(fdr_richardson_lucy_auto_f32(plan, src.ptr<float>(0), c.rows, c.cols, c.cols, w.empty() ? nullptr : w.ptr<float>(0), cols,
                                               out.ptr<float>(0), c.cols, &prm, &res, nullptr));
        results.push_back(res);
        c = out;
    }
    return results;
}
inline std::vector<fdr_rl_auto_result> richardsonLucyAuto_RGB(std::vector<Mat>& channels, const Mat& psf, int max_iterations, int rule,
                                                              const RlAutoOptions& a = RlAutoOptions()) {
    return richardsonLucyAuto_RGB(channels, psf, max_iterations, rule, a, defaults());
}
// Total-variation deconvolution (fdr_tv_deconv_f32, include/fdr.h) of every channel, in place: the plan and operator PSF of
// richardsonLucy_RGB, `iterations` ADMM steps of mu / 2 ||blur(x) - d||^2 + TV(x) (isotropic) with penalty rho, the output clamped
// at 0 and normalised by o.norm_area.  o.mode and o.cls_gamma do not apply.  The channels go through ONE batched call
// (fdr_tv_deconv_batch_f32) on a launch group of channels.size() images (at most 8), with the bits of the per-channel calls;
// channels of different sizes or types run one by one.  coupled: vectorial TV -- the channels share one shrinkage by their joint
// gradient norm (FDR_TV_COUPLE_CHANNELS; at most 8 channels of one size), so edges fall in the same place in every channel.
inline void tvDeblur_RGB(std::vector<Mat>& channels, const Mat& psf, float mu, int iterations, float rho, const Options& o, bool coupled = false) {
    if (channels.empty()) return;
    const int rows = channels[0].rows, cols = channels[0].cols, count = (int)channels.size();
    bool created = false;
    PlanCacheSettle settle_;
    fdr_plan* plan = plan_cache().get(o.device, std::max(8, nextPowerOfTwo(rows)), std::max(32, nextPowerOfTwo(cols)), FDR_MODE_FAST, &created);
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    FDR_CHECK(fdr_set_operator_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols));
    bool same = true;
    for (const Mat& c : channels) same = same && c.rows == rows && c.cols == cols && c.type() == CV_32F;
    if (same || coupled) {
        if (!same) {
            std::cerr << "tvDeblur_RGB: the coupled form needs CV_32F channels of one size\n";
            exit(1);
        }
        const size_t px = (size_t)rows * cols;
        std::vector<float> in(px * count), out(px * count);
        for (int i = 0; i < count; ++i)
            for (int r = 0; r < rows; ++r) std::copy(channels[i].ptr<float>(r), channels[i].ptr<float>(r) + cols, in.begin() + i * px + (size_t)r * cols);
        const fdr_tv_batch_params bp = {mu, rho, iterations, 0, 1, o.norm_area, coupled ? FDR_TV_COUPLE_CHANNELS : FDR_TV_COUPLE_NONE};
        FDR_CHECK(fdr_plan_set_batching(plan, 1, std::min(count, 8)));
        const int rc = fdr_tv_deconv_batch_f32(plan, in.data(), px, count, rows, cols, cols, out.data(), px, cols, &bp);
        FDR_CHECK(fdr_plan_set_batching(plan, 1, 1));  // the cached plan goes back as it came
        FDR_CHECK(rc);
        for (int i = 0; i < count; ++i) {
            Mat m(rows, cols, CV_32F);
            std::copy(out.begin() + i * px, out.begin() + (i + 1) * px, m.ptr<float>(0));
            channels[i] = m;
        }
        return;
    }
    const fdr_tv_params prm = {mu, rho, iterations, 0, 1, o.norm_area};
    for (Mat& c : channels) {
        Mat src = c.isContinuous() ? c : c.clone();
        Mat out(c.rows, c.cols, CV_32F);
        FDR_CHECK(fdr_tv_deconv_f32(plan, src.ptr<float>(0), c.rows, c.cols, c.cols, out.ptr<float>(0), c.cols, &prm));
        c = out;
    }
}
inline void tvDeblur_RGB(std::vector<Mat>& channels, const Mat& psf, float mu, int iterations = 50, float rho = 2.0f, bool coupled = false) {
    tvDeblur_RGB(channels, psf, mu, iterations, rho, defaults(), coupled);
}
// Free-boundary, weighted total-variation deconvolution (fdr_tv_deconv_free_f32, include/fdr.h) of every channel, in place, for a
// picture that is a crop of a larger scene: the plan, operator PSF and `weights` of richardsonLucyFree_RGB, `iterations` ADMM steps
// (isotropic, penalties rho and nu = rho), the output clamped at 0 and normalised by o.norm_area.  The channels go through ONE
// batched call (fdr_tv_deconv_free_batch_f32) on a launch group of channels.size() images (at most 8), with the bits of the
// per-channel calls; channels of different sizes or types run one by one.  coupled: vectorial TV -- the channels share one
// shrinkage by their joint gradient norm (FDR_TV_COUPLE_CHANNELS; at most 8 channels of one size); the data step stays per channel.
inline void tvDeblurFree_RGB(std::vector<Mat>& channels, const Mat& psf, float mu, int iterations, float rho, const Mat& weights, const Options& o,
                             bool coupled = false) {
    if (channels.empty()) return;
    const int rows = channels[0].rows, cols = channels[0].cols, count = (int)channels.size();
    if (!weights.empty() && (weights.rows != rows || weights.cols != cols || weights.type() != CV_32F)) {
        std::cerr << "tvDeblurFree_RGB: the weights must be CV_32F and have the picture's size\n";
        exit(1);
    }
    bool created = false;
    PlanCacheSettle settle_;
    fdr_plan* plan = plan_cache().get(o.device, std::max(8, nextPowerOfTwo(rows + psf.rows - 1)), std::max(32, nextPowerOfTwo(cols + psf.cols - 1)),
                                      FDR_MODE_FAST, &created);
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    FDR_CHECK(fdr_set_operator_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols));
    Mat w = weights.empty() || weights.isContinuous() ? weights : weights.clone();
    bool same = true;
    for (const Mat& c : channels) same = same && c.rows == rows && c.cols == cols && c.type() == CV_32F;
    if (same || coupled) {
        if (!same) {
            std::cerr << "tvDeblurFree_RGB: the coupled form needs CV_32F channels of one size\n";
            exit(1);
        }
        const size_t px = (size_t)rows * cols;
        std::vector<float> in(px * count), out(px * count);
        for (int i = 0; i < count; ++i)
            for (int r = 0; r < rows; ++r) std::copy(channels[i].ptr<float>(r), channels[i].ptr<float>(r) + cols, in.begin() + i * px + (size_t)r * cols);
        const fdr_tv_free_batch_params bp = {mu, rho, 0.f, iterations, 0, 1, o.norm_area, rows, cols, coupled ? FDR_TV_COUPLE_CHANNELS : FDR_TV_COUPLE_NONE};
        FDR_CHECK(fdr_plan_set_batching(plan, 1, std::min(count, 8)));
        const int rc = fdr_tv_deconv_free_batch_f32(plan, in.data(), px, count, rows, cols, cols, w.empty() ? nullptr : w.ptr<float>(0), cols, out.data(), px,
                                                    cols, &bp);
        FDR_CHECK(fdr_plan_set_batching(plan, 1, 1));  // the cached plan goes back as it came
        FDR_CHECK(rc);
        for (int i = 0; i < count; ++i) {
            Mat m(rows, cols, CV_32F);
            std::copy(out.begin() + i * px, out.begin() + (i + 1) * px, m.ptr<float>(0));
            channels[i] = m;
        }
        return;
    }
    for (Mat& c : channels) {
        Mat src = c.isContinuous() ? c : c.clone();
        Mat out(c.rows, c.cols, CV_32F);
        const fdr_tv_free_params prm = {mu, rho, 0.f, iterations, 0, 1, o.norm_area, c.rows, c.cols};
        FDR_CHECK(fdr_tv_deconv_free_f32(plan, src.ptr<float>(0), c.rows, c.cols, c.cols, w.empty() ? nullptr : w.ptr<float>(0), cols,
                                         out.ptr<float>(0), c.cols, &prm));
        c = out;
    }
}
inline void tvDeblurFree_RGB(std::vector<Mat>& channels, const Mat& psf, float mu, int iterations = 50, float rho = 2.0f, const Mat& weights = Mat(),
                             bool coupled = false) {
    tvDeblurFree_RGB(channels, psf, mu, iterations, rho, weights, defaults(), coupled);
}
// Poisson-likelihood total-variation deconvolution (fdr_tv_deconv_poisson_f32, include/fdr.h) of every channel, in place, for a
// photon-limited picture that is a crop of a larger scene: tvDeblurFree_RGB with the data term mu sum m [(blur(x) + b) - d+ log(blur(x)
// + b)], b = background >= 0 in the units of the channels, mu = photons per unit times the weight wanted on the likelihood.  The
// plan, operator PSF, `weights`, penalties, clamp and normalisation of tvDeblurFree_RGB; the channels go through ONE batched call
// (fdr_tv_deconv_poisson_batch_f32) with the bits of the per-channel calls, channels of different sizes or types one by one.
// coupled: vectorial TV, the data step per channel (at most 8 channels of one size).
inline void tvDeblurPoisson_RGB(std::vector<Mat>& channels, const Mat& psf, float mu, int iterations, float rho, const Mat& weights, float background,
                                const Options& o, bool coupled = false) {
    if (channels.empty()) return;
    const int rows = channels[0].rows, cols = channels[0].cols, count = (int)channels.size();
    if (!weights.empty() && (weights.rows != rows || weights.cols != cols || weights.type() != CV_32F)) {
        std::cerr << "tvDeblurPoisson_RGB: the weights must be CV_32F and have the picture's size\n";
        exit(1);
    }
    bool created = false;
    PlanCacheSettle settle_;
    fdr_plan* plan = plan_cache().get(o.device, std::max(8, nextPowerOfTwo(rows + psf.rows - 1)), std::max(32, nextPowerOfTwo(cols + psf.cols - 1)),
                                      FDR_MODE_FAST, &created);
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    FDR_CHECK(fdr_set_operator_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols));
    Mat w = weights.empty() || weights.isContinuous() ? weights : weights.clone();
    bool same = true;
    for (const Mat& c : channels) same = same && c.rows == rows && c.cols == cols && c.type() == CV_32F;
    if (same || coupled) {
        if (!same) {
            std::cerr << "tvDeblurPoisson_RGB: the coupled form needs CV_32F channels of one size\n";
            exit(1);
        }
        const size_t px = (size_t)rows * cols;
        std::vector<float> in(px * count), out(px * count);
        for (int i = 0; i < count; ++i)
            for (int r = 0; r < rows; ++r) std::copy(channels[i].ptr<float>(r), channels[i].ptr<float>(r) + cols, in.begin() + i * px + (size_t)r * cols);
        const fdr_tv_poisson_batch_params bp = {mu, rho, 0.f, background, iterations, 0, 1, o.norm_area, rows, cols,
                                                coupled ? FDR_TV_COUPLE_CHANNELS : FDR_TV_COUPLE_NONE};
        FDR_CHECK(fdr_plan_set_batching(plan, 1, std::min(count, 8)));
        const int rc = fdr_tv_deconv_poisson_batch_f32(plan, in.data(), px, count, rows, cols, cols, w.empty() ? nullptr : w.ptr<float>(0), cols,
                                                       out.data(), px, cols, &bp);
        FDR_CHECK(fdr_plan_set_batching(plan, 1, 1));  // the cached plan goes back as it came
        FDR_CHECK(rc);
        for (int i = 0; i < count; ++i) {
            Mat m(rows, cols, CV_32F);
            std::copy(out.begin() + i * px, out.begin() + (i + 1) * px, m.ptr<float>(0));
            channels[i] = m;
        }
        return;
    }
    for (Mat& c : channels) {
        Mat src = c.isContinuous() ? c : c.clone();
        Mat out(c.rows, c.cols, CV_32F);
        const fdr_tv_poisson_params prm = {mu, rho, 0.f, background, iterations, 0, 1, o.norm_area, c.rows, c.cols};
        FDR_CHECK(fdr_tv_deconv_poisson_f32(plan, src.ptr<float>(0), c.rows, c.cols, c.cols, w.empty() ? nullptr : w.ptr<float>(0), cols,
                                            out.ptr<float>(0), c.cols, &prm));
        c = out;
    }
}
inline void tvDeblurPoisson_RGB(std::vector<Mat>& channels, const Mat& psf, float mu, int iterations = 50, float rho = 2.0f, const Mat& weights = Mat(),
                                float background = 0.f, bool coupled = false) {
    tvDeblurPoisson_RGB(channels, psf, mu, iterations, rho, weights, background, defaults(), coupled);
}
// Sectioned restoration (fdr_restore_tiled_f32, include/fdr.h) of every channel, in place, for a picture of any size: overlapping
// tiles of `tile` pixels (a picture no larger is one tile), `overlap` of them shared with the neighbour, every tile restored as a
// crop of a larger scene by the free-boundary iteration of `method` with the PSF taken as CENTRED (the result is registered with the
// picture), the tiles blended with a partition of unity.  One tiled call per channel on one tile plan, the smallest of
// fdr_tiled_layout_get.  norm_area: FDR_NORM_NONE or FDR_NORM_CROPPED (there is no padded area).
struct TiledOptions {
    int method = FDR_TILED_RL_FREE;   // FDR_TILED_RL_FREE / FDR_TILED_TV_FREE
    int tile = 1024, overlap = 64;    // both axes
    int iterations = 30;
    float sigma = FDR_RL_SIGMA;       // RL: coverage threshold
    float mu = 200.f, rho = 2.f;      // TV (nu = rho, isotropic, clamped at 0)
    int norm_area = FDR_NORM_NONE;
    int device = 0;
};
inline void restoreTiled_RGB(std::vector<Mat>& channels, const Mat& psf, const TiledOptions& t, const Mat& weights = Mat()) {
    if (channels.empty()) return;
    const int rows = channels[0].rows, cols = channels[0].cols;
    if (!weights.empty() && (weights.rows != rows || weights.cols != cols || weights.type() != CV_32F)) {
        std::cerr << "restoreTiled_RGB: the weights must be CV_32F and have the picture's size\n";
        exit(1);
    }
    for (const Mat& c : channels)
        if (c.rows != rows || c.cols != cols || c.type() != CV_32F) {
            std::cerr << "restoreTiled_RGB: needs CV_32F channels of one size\n";
            exit(1);
        }
    const fdr_tiled_params prm = {t.method, t.tile, t.tile, t.overlap, t.overlap, t.iterations, t.sigma, t.mu, t.rho, 0.f, 0, 1, t.norm_area};
    fdr_tiled_layout lay;
    FDR_CHECK(fdr_tiled_layout_get(rows, cols, psf.rows, psf.cols, &prm, &lay));
    bool created = false;
    PlanCacheSettle settle_;
    fdr_plan* plan = plan_cache().get(t.device, lay.min_M, lay.min_N, FDR_MODE_FAST, &created);
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    Mat w = weights.empty() || weights.isContinuous() ? weights : weights.clone();
    for (Mat& c : channels) {
        Mat src = c.isContinuous() ? c : c.clone();
        Mat out(rows, cols, CV_32F);
        FDR_CHECK(fdr_restore_tiled_f32(plan, src.ptr<float>(0), rows, cols, cols, w.empty() ? nullptr : w.ptr<float>(0), cols, psfc.ptr<float>(0),
                                        (size_t)psf.rows * psf.cols, 1, psf.rows, psf.cols, psf.cols, out.ptr<float>(0), cols, &prm));
        c = out;
    }
}
// Noise-constrained total-variation deconvolution (fdr_tv_deconv_auto_f32, include/fdr.h) of every channel, in place: tvDeblurFree_RGB
// without mu.  The caller states the noise standard deviation sigma of the channels (0: estimated per channel, fdr_noise_sigma_f32)
// and tau (0: 1); every step takes its weight from the discrepancy ball tau sigma^2 sum(weights).  The plan, operator PSF and
// `weights` of tvDeblurFree_RGB, `iterations` ADMM steps (isotropic, penalties rho and nu = FDR_TV_AUTO_NU_RATIO rho), the output
// clamped at 0 and normalised by o.norm_area.  The channels go through ONE batched call (fdr_tv_deconv_auto_batch_f32) on a launch
// group of channels.size() images (at most 8), with the bits of the per-channel calls; channels of different sizes or types run
// one by one.  coupled: vectorial TV -- one shrinkage by the joint gradient norm of the channels (at most 8 of one size), every
// channel with its own ball and its own mu_k.  Returns the channels' results (sigma, target, mu, discrepancy, S), in order.
inline std::vector<fdr_tv_auto_result> tvDeblurAuto_RGB(std::vector<Mat>& channels, const Mat& psf, float sigma, int iterations, float rho, float tau,
                                                        const Mat& weights, const Options& o, bool coupled = false) {
    std::vector<fdr_tv_auto_result> results;
    if (channels.empty()) return results;
    const int rows = channels[0].rows, cols = channels[0].cols, count = (int)channels.size();
    if (!weights.empty() && (weights.rows != rows || weights.cols != cols || weights.type() != CV_32F)) {
        std::cerr << "tvDeblurAuto_RGB: the weights must be CV_32F and have the picture's size\n";
        exit(1);
    }
    bool created = false;
    PlanCacheSettle settle_;
    fdr_plan* plan = plan_cache().get(o.device, std::max(8, nextPowerOfTwo(rows + psf.rows - 1)), std::max(32, nextPowerOfTwo(cols + psf.cols - 1)),
                                      FDR_MODE_FAST, &created);
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    FDR_CHECK(fdr_set_operator_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols));
    Mat w = weights.empty() || weights.isContinuous() ? weights : weights.clone();
    bool same = true;
    for (const Mat& c : channels) same = same && c.rows == rows && c.cols == cols && c.type() == CV_32F;
    if (same || coupled) {
        if (!same) {
            std::cerr << "tvDeblurAuto_RGB: the coupled form needs CV_32F channels of one size\n";
            exit(1);
        }
        const size_t px = (size_t)rows * cols;
        std::vector<float> in(px * count), out(px * count);
        for (int i = 0; i < count; ++i)
            for (int r = 0; r < rows; ++r) std::copy(channels[i].ptr<float>(r), channels[i].ptr<float>(r) + cols, in.begin() + i * px + (size_t)r * cols);
        const fdr_tv_auto_batch_params bp = {sigma, tau, rho, 0.f, iterations, 0, 1, o.norm_area, rows, cols,
                                             coupled ? FDR_TV_COUPLE_CHANNELS : FDR_TV_COUPLE_NONE};
        results.resize(count);
        FDR_CHECK(fdr_plan_set_batching(plan, 1, std::min(count, 8)));
        const int rc = fdr_tv_deconv_auto_batch_f32(plan, in.data(), px, count, rows, cols, cols, w.empty() ? nullptr : w.ptr<float>(0), cols, out.data(), px,
                                                    cols, &bp, nullptr, results.data(), nullptr, 0);
        FDR_CHECK(fdr_plan_set_batching(plan, 1, 1));  // the cached plan goes back as it came
        FDR_CHECK(rc);
        for (int i = 0; i < count; ++i) {
            Mat m(rows, cols, CV_32F);
            std::copy(out.begin() + i * px, out.begin() + (i + 1) * px, m.ptr<float>(0));
            channels[i] = m;
        }
        return results;
    }
    for (Mat& c : channels) {
        Mat src = c.isContinuous() ? c : c.clone();
        Mat out(c.rows, c.cols, CV_32F);
        const fdr_tv_auto_params prm = {sigma, tau, rho, 0.f, iterations, 0, 1, o.norm_area, c.rows, c.cols};
        fdr_tv_auto_result res = {};
        FDR_CHECK(fdr_tv_deconv_auto_f32(plan, src.ptr<float>(0), c.rows, c.cols, c.cols, w.empty() ? nullptr : w.ptr<float>(0), cols,
                                         out.ptr<float>(0), c.cols, &prm, &res, nullptr));
        results.push_back(res);
        c = out;
    }
    return results;
}
inline std::vector<fdr_tv_auto_result> tvDeblurAuto_RGB(std::vector<Mat>& channels, const Mat& psf, float sigma = 0.f, int iterations = 100,
                                                        float rho = 2.0f, float tau = 0.f, const Mat& weights = Mat(), bool coupled = false) {
    return tvDeblurAuto_RGB(channels, psf, sigma, iterations, rho, tau, weights, defaults(), coupled);
}
// The motion blur of a one-channel picture of unknown blur (fdr_estimate_motion_f32, include/fdr.h): length and angle in the
// convention of motionBlurKernel, the table minimum and the confidence (below about 10: no clear blur).  Its own FDR_MODE_FAST plan
// (each dimension padded to fdr_optimal_dft_size, at least 32; FDR_FLAG_MIXED_RADIX), made and freed inside the call.  0 selects an
// argument's default (min_length 3, max_length min(100, min(rows, cols) / 4), angle_step 0.5 deg).
inline fdr_motion_estimate estimateMotionBlur(const Mat& gray, int min_length = 0, int max_length = 0, double angle_step = 0) {
    Mat src = gray.isContinuous() ? gray : gray.clone();
    fdr_plan* plan = nullptr;
    FDR_CHECK(fdr_plan_create(defaults().device, std::max(32, fdr_optimal_dft_size(src.rows)), std::max(32, fdr_optimal_dft_size(src.cols)),
                              FDR_MODE_FAST, FDR_FLAG_MIXED_RADIX, &plan));
    fdr_motion_estimate est{};
    const int rc = fdr_estimate_motion_f32(plan, src.ptr<float>(0), src.rows, src.cols, src.cols, min_length, max_length, angle_step, &est,
                                           nullptr);
    const std::string err = rc == FDR_OK ? std::string() : std::string(fdr_last_error());
    fdr_plan_destroy(plan);
    if (rc != FDR_OK) {
        std::cerr << "Error: " << __FILE__ << ":" << __LINE__ << ", " << err << "\n";
        exit(1);
    }
    return est;
}
// The translation of every picture of a burst against imgs[reference] (fdr_register_frames_f32, include/fdr.h): one-channel CV_32F
// pictures of one size; psfs: one CV_32F PSF per picture, whose phases the estimate undoes, or empty for plain phase correlation
// (right only for frames of one common PSF).  Frame k's result is the shift that belongs in its PSF (fdr_psf_shift_f32).  Plan as
// estimateMotionBlur, made and freed inside the call; max_shift 0 selects min(rows, cols) / 4.
inline std::vector<fdr_frame_shift> registerFrames(const std::vector<Mat>& imgs, const std::vector<Mat>& psfs = std::vector<Mat>(),
                                                   int reference = 0, int max_shift = 0) {
    const int K = (int)imgs.size();
    bool ok = K >= 1 && K <= FDR_MAX_FRAMES && (psfs.empty() || (int)psfs.size() == K);
    int pr = 0, pc = 0;
    for (int k = 0; k < K && ok; ++k) {
        ok = imgs[k].type() == CV_32F && imgs[k].rows == imgs[0].rows && imgs[k].cols == imgs[0].cols;
        if (ok && !psfs.empty()) { ok = psfs[k].type() == CV_32F && psfs[k].rows > 0 && psfs[k].cols > 0; pr = std::max(pr, psfs[k].rows); pc = std::max(pc, psfs[k].cols); }
    }
    if (!ok) {
        std::cerr << "registerFrames: 1 .. 8 CV_32F pictures of one size, and no PSFs or one CV_32F PSF each\n";
        exit(1);
    }
    const int rows = imgs[0].rows, cols = imgs[0].cols;
    const size_t px = (size_t)rows * cols, ppx = (size_t)pr * pc;
    std::vector<float> in(px * K), tabs(ppx * K, 0.f);
    for (int k = 0; k < K; ++k) {
        for (int r = 0; r < rows; ++r) std::copy(imgs[k].ptr<float>(r), imgs[k].ptr<float>(r) + cols, in.begin() + k * px + (size_t)r * cols);
        if (!psfs.empty())
            for (int r = 0; r < psfs[k].rows; ++r) std::copy(psfs[k].ptr<float>(r), psfs[k].ptr<float>(r) + psfs[k].cols, tabs.begin() + k * ppx + (size_t)r * pc);
    }
    fdr_plan* plan = nullptr;
    FDR_CHECK(fdr_plan_create(defaults().device, std::max(32, fdr_optimal_dft_size(std::max(rows, pr))), std::max(32, fdr_optimal_dft_size(std::max(cols, pc))),
                              FDR_MODE_FAST, FDR_FLAG_MIXED_RADIX, &plan));
    std::vector<fdr_frame_shift> est(K);
    const fdr_register_params rp = {reference, max_shift, max_shift, 0.f, nullptr};
    const int rc = fdr_register_frames_f32(plan, in.data(), px, K, rows, cols, cols, psfs.empty() ? nullptr : tabs.data(), ppx, pr, pc, pc, &rp, est.data());
    const std::string err = rc == FDR_OK ? std::string() : std::string(fdr_last_error());
    fdr_plan_destroy(plan);
    if (rc != FDR_OK) {
        std::cerr << "Error: " << __FILE__ << ":" << __LINE__ << ", " << err << "\n";
        exit(1);
    }
    return est;
}
// The defocus blur of a one-channel picture (fdr_estimate_defocus_f32, include/fdr.h): the radius of the uniform disk, which goes
// straight into diskBlurKernel, the ring it was read from and the confidence (below FDR_DEFOCUS_CONF_MIN: no ring).  Plan and
// defaults as estimateMotionBlur.
inline fdr_defocus_estimate estimateDefocusBlur(const Mat& gray, int min_diameter = 0, int max_diameter = 0, double angle_step = 0) {
    Mat src = gray.isContinuous() ? gray : gray.clone();
    fdr_plan* plan = nullptr;
    FDR_CHECK(fdr_plan_create(defaults().device, std::max(32, fdr_optimal_dft_size(src.rows)), std::max(32, fdr_optimal_dft_size(src.cols)),
                              FDR_MODE_FAST, FDR_FLAG_MIXED_RADIX, &plan));
    fdr_defocus_estimate est{};
    const int rc = fdr_estimate_defocus_f32(plan, src.ptr<float>(0), src.rows, src.cols, src.cols, min_diameter, max_diameter, angle_step, &est,
                                            nullptr);
    const std::string err = rc == FDR_OK ? std::string() : std::string(fdr_last_error());
    fdr_plan_destroy(plan);
    if (rc != FDR_OK) {
        std::cerr << "Error: " << __FILE__ << ":" << __LINE__ << ", " << err << "\n";
        exit(1);
    }
    return est;
}
// Both estimates of a one-channel picture from one cepstrum and the kind of blur they point to (fdr_estimate_blur_f32): each
// estimate is what estimateMotionBlur / estimateDefocusBlur return with their defaults, kind one of FDR_BLUR_NONE / _MOTION / _DEFOCUS.
struct BlurEstimate { int kind; fdr_motion_estimate motion; fdr_defocus_estimate defocus; };
inline BlurEstimate estimateBlur(const Mat& gray) {
    Mat src = gray.isContinuous() ? gray : gray.clone();
    fdr_plan* plan = nullptr;
    FDR_CHECK(fdr_plan_create(defaults().device, std::max(32, fdr_optimal_dft_size(src.rows)), std::max(32, fdr_optimal_dft_size(src.cols)),
                              FDR_MODE_FAST, FDR_FLAG_MIXED_RADIX, &plan));
    BlurEstimate b{};
    const int rc = fdr_estimate_blur_f32(plan, src.ptr<float>(0), src.rows, src.cols, src.cols, 0, 0, 0.0, 0, 0, 0.0, &b.motion, &b.defocus, &b.kind);
    const std::string err = rc == FDR_OK ? std::string() : std::string(fdr_last_error());
    fdr_plan_destroy(plan);
    if (rc != FDR_OK) {
        std::cerr << "Error: " << __FILE__ << ":" << __LINE__ << ", " << err << "\n";
        exit(1);
    }
    return b;
}
// K or gamma of the Wiener / CLS filter for one blurred channel and its PSF (fdr_choose_reg_f32, include/fdr.h): by generalised
// cross-validation or the discrepancy principle (method), searching K or gamma (param) with the other weight at `fixed`; sigma 0 =
// estimated from the picture (discrepancy principle only).  Its own FDR_MODE_FAST plan (the one of richardsonLucy_RGB: each dimension
// padded to the next power of two, at least 8 rows and 32 columns), made and freed inside the call.  The value goes into
// set_cls_gamma / the K argument of the Wiener entry points.
inline fdr_reg_choice chooseRegularisation(const Mat& channel, const Mat& psf, int method = FDR_REG_GCV, int param = FDR_REG_PARAM_GAMMA,
                                           float fixed = 0.f, float sigma = 0.f) {
    Mat src = channel.isContinuous() ? channel : channel.clone();
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    fdr_plan* plan = nullptr;
    FDR_CHECK(fdr_plan_create(defaults().device, std::max(8, nextPowerOfTwo(src.rows)), std::max(32, nextPowerOfTwo(src.cols)), FDR_MODE_FAST, 0,
                              &plan));
    fdr_reg_params prm{};
    prm.method = method; prm.param = param; prm.fixed = fixed; prm.sigma = sigma; prm.refine = -1;
    fdr_reg_choice choice{};
    int rc = fdr_set_operator_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols);
    if (rc == FDR_OK) rc = fdr_choose_reg_f32(plan, src.ptr<float>(0), src.rows, src.cols, src.cols, &prm, &choice);
    const std::string err = rc == FDR_OK ? std::string() : std::string(fdr_last_error());
    fdr_plan_destroy(plan);
    if (rc != FDR_OK) {
        std::cerr << "Error: " << __FILE__ << ":" << __LINE__ << ", " << err << "\n";
        exit(1);
    }
    return choice;
}
// Immerkaer's estimate of the noise standard deviation of a one-channel picture, at least 3 x 3 (fdr_noise_sigma_f32)
inline double estimateNoiseSigma(const Mat& gray) {
    Mat src = gray.isContinuous() ? gray : gray.clone();
    double sigma = 0.0;
    FDR_CHECK(fdr_noise_sigma_f32(defaults().device, src.ptr<float>(0), src.rows, src.cols, src.cols, &sigma));
    return sigma;
}
// The operator exactly as fft_serial::wienerDeblur_myfft defines it (fft/fft_serial.cpp:141-261; the fft_gpu
// declaration at fft/fft.hpp:44 has no body in the reference): pad to getOptimalDFTSize (2^a 3^b 5^c, :153-154 -- a
// non-power-of-two dimension is transformed by the naive DFT, :100-101), restore, crop to img's size, normalise over
// the cropped plane (:243-246).  For the pre-padded channels the drivers pass (serial.cpp:36) pad and crop are no-ops.
inline Mat wienerDeblur_myfft(const Mat& img, const Mat& psf, float K, const Options& o) {
    const int M = fdr_optimal_dft_size(img.rows), N = fdr_optimal_dft_size(img.cols);
    unsigned flags = (isPowerOfTwo(M) && isPowerOfTwo(N)) ? 0u : FDR_FLAG_ANY_SIZE;
    if (o.mixed_radix && o.mode == FDR_MODE_FAST) flags |= FDR_FLAG_MIXED_RADIX;
    bool created = false;
    PlanCacheSettle settle_;
    fdr_plan* plan = plan_cache().get(o.device, M, N, o.mode, &created, flags);
    (void)fdr_plan_set_option(plan, FDR_OPT_PAD_MODE, FDR_PAD_ZERO);  // (a cached plan may have served FDR_PAD_SMOOTH; o.pad_mode does not apply here)
    set_psf_opts(plan, psf, K, o);
    return run_channel(plan, img, FDR_NORM_CROPPED);
}
inline Mat wienerDeblur_myfft(const Mat& img, const Mat& psf, float K) { return wienerDeblur_myfft(img, psf, K, defaults()); }

// fft/fft.hpp:35-39: n interleaved complex values by host pointer, unscaled
inline void fft_radix2_kernel(float* data, int n, bool inverse) { FDR_CHECK(fdr_fft1d_c2c(data, n, inverse ? 1 : 0, FDR_MODE_PARITY)); }
inline void dft_naive_kernel(float* data, int n, bool inverse) { FDR_CHECK(fdr_dft_naive_c2c(data, n, inverse ? 1 : 0)); }
inline void transform_row_kernel(float* rowPtr, int N, bool inverse) { FDR_CHECK(fdr_fft1d_c2c(rowPtr, N, inverse ? 1 : 0, FDR_MODE_PARITY)); }

// fft/fft.hpp:40-42: in-place unscaled 2-D transform of a CV_32FC2 Mat (rows, transpose, rows, transpose); any size
// up to 32768 for powers of two (above 8192: 8192-point blocks + radix-2 stages in global memory), non-powers of two up to
// 4096 (naive DFT along that dimension, as fft_serial.cpp:100-101)
inline void my_dft2D(Mat& complexMat, bool inverse) {
    if (complexMat.type() != CV_32FC2) { std::fprintf(stderr, "Error: %s:%d, my_dft2D needs CV_32FC2\n", __FILE__, __LINE__); std::exit(1); }
    const int M = complexMat.rows, N = complexMat.cols;
    Mat c = complexMat.isContinuous() ? complexMat : complexMat.clone();
    fdr_plan* plan = nullptr;
    const unsigned flags = (isPowerOfTwo(M) && isPowerOfTwo(N)) ? 0u : FDR_FLAG_ANY_SIZE;
    FDR_CHECK(fdr_plan_create(0, M, N, FDR_MODE_PARITY, flags, &plan));
    FDR_CHECK(fdr_fft2d_c2c(plan, c.ptr<float>(0), inverse ? 1 : 0));
    fdr_plan_destroy(plan);
    if (c.data != complexMat.data)
        for (int r = 0; r < M; ++r) std::memcpy(complexMat.ptr<float>(r), c.ptr<float>(r), sizeof(float) * 2 * (size_t)N);
}
inline void my_dft2D_forward(Mat& complexMat) { my_dft2D(complexMat, false); }
inline void my_dft2D_inverse(Mat& complexMat) { my_dft2D(complexMat, true); }

}  // namespace fft_gpu

// fft/fft.hpp:9-18 of the reference: the serial back-end's names.  Here they run on the GPU in the PARITY mode, whose
// FFT arithmetic is bit-identical to fft/fft_serial.cpp (per-stage twiddles replayed from its float recurrence, no FMA;
// tests/test_gpu_parity.py holds the proof against the CPU restatement), so a serial.cpp-style caller gets the pixels
// ./serial would give without a CPU path in this library.
namespace fft_serial {

inline void fft_radix2_inplace(std::vector<std::complex<float>>& a, bool inverse) {  // fft/fft_serial.cpp:40-68
    if (a.empty()) return;
    FDR_CHECK(fdr_fft1d_c2c(reinterpret_cast<float*>(a.data()), (int)a.size(), inverse ? 1 : 0, FDR_MODE_PARITY));
}
inline void dft_naive_inplace(std::vector<std::complex<float>>& a, bool inverse) {   // fft/fft_serial.cpp:71-87
    if (a.empty()) return;
    FDR_CHECK(fdr_dft_naive_c2c(reinterpret_cast<float*>(a.data()), (int)a.size(), inverse ? 1 : 0));
}
inline void transform_row_inplace(cv::Vec2f* rowPtr, int N, bool inverse) {          // fft/fft_serial.cpp:90-108
    FDR_CHECK(fdr_fft1d_c2c(reinterpret_cast<float*>(rowPtr), N, inverse ? 1 : 0, FDR_MODE_PARITY));
}
inline void my_dft2D(Mat& complexMat, bool inverse) { fft_gpu::my_dft2D(complexMat, inverse); }  // :113-139 (parity plan)
inline void my_dft2D_forward(Mat& complexMat) { my_dft2D(complexMat, false); }
inline void my_dft2D_inverse(Mat& complexMat) { my_dft2D(complexMat, true); }

// The accumulated phase timers of fft/fft_serial.cpp:13-35: "Serial: ..." names (:158-236), printed once, when the
// call count reaches CHANNELS = 3 (:249-258; never reset afterwards, as in the reference).  The figures are DEVICE
// times (hipEvent pairs): uploads -> "Pre-process" (the padding happens on load inside the first pass); the PSF
// spectrum -> "FFT PSF"; passes A + B (forward rows, forward columns with the Wiener quotient fused into their
// epilogue) -> "FFT Image"; "Wiener Filter" stays 0 because the quotient has no pass of its own here; passes C + D
// (inverse rows, inverse columns + real part + min/max) -> "IFFT"; normalise + crop + download -> "Post-process".
struct PhaseAccum {
    int callCount = 0;
    std::map<std::string, double> accum;
};
inline PhaseAccum& phase_accum() { static PhaseAccum a; return a; }

// fft/fft_serial.cpp:141-261: pads to getOptimalDFTSize, crops to img's size, normalises over the cropped plane
inline Mat wienerDeblur_myfft(const Mat& img, const Mat& psf, float K) {
    PhaseAccum& acc = phase_accum();
    if (acc.callCount == 0) acc.accum.clear();
    acc.callCount++;
    const int M = fdr_optimal_dft_size(img.rows), N = fdr_optimal_dft_size(img.cols);
    const unsigned flags = (isPowerOfTwo(M) && isPowerOfTwo(N)) ? 0u : FDR_FLAG_ANY_SIZE;
    bool created = false;
    fft_gpu::PlanCacheSettle settle_;
    fdr_plan* plan = fft_gpu::plan_cache().get(0, M, N, FDR_MODE_PARITY, &created, flags);  // kept between the channels of a driver's loop
    float ph[FDR_N_PHASES] = {0}, ms[FDR_MAX_PASSES] = {0};
    if (!created) FDR_CHECK(fdr_plan_phase_times(plan, ph, 1));  // this call's phases only
    Mat psfc = psf.isContinuous() ? psf : psf.clone();
    FDR_CHECK(fdr_set_psf(plan, psfc.ptr<float>(0), psf.rows, psf.cols, psf.cols, K));
    FDR_CHECK(fdr_plan_profile(plan, 1));
    Mat out = fft_gpu::run_channel(plan, img, FDR_NORM_CROPPED);
    const char* names[FDR_MAX_PASSES] = {nullptr};
    int n = 0, launches[FDR_MAX_PASSES] = {0};
    FDR_CHECK(fdr_plan_phase_times(plan, ph, 1));
    FDR_CHECK(fdr_plan_pass_times(plan, &n, ms, names, launches));
    FDR_CHECK(fdr_plan_profile(plan, 0));
    double fwd = 0, inv = 0, post = 0;
    for (int i = 0; i < n; ++i) {
        const std::string nm = names[i] ? names[i] : "";
        const double t = (double)ms[i] * launches[i];
        if (nm.rfind("A ", 0) == 0 || nm.rfind("B ", 0) == 0 || nm.rfind("simple", 0) == 0) fwd += t;
        else if (nm.rfind("C ", 0) == 0 || nm.rfind("D ", 0) == 0) inv += t;
        else post += t;  // E normalize + crop
    }
    acc.accum["Serial: Pre-process"] += ph[FDR_PHASE_H2D];
    acc.accum["Serial: FFT Image"] += fwd;
    acc.accum["Serial: FFT PSF"] += ph[FDR_PHASE_PRE];
    acc.accum["Serial: Wiener Filter"] += 0.0;
    acc.accum["Serial: IFFT"] += inv;
    acc.accum["Serial: Post-process"] += post + ph[FDR_PHASE_D2H];
    if (acc.callCount == 3) {
        std::cout << "=== Accumulated Time ===" << std::endl;
        float this_round_total = 0;
        for (auto& p : acc.accum) {
            std::cout << p.first << " total: " << p.second << " ms" << std::endl;
            this_round_total += (float)p.second;
        }
        std::cout << "this round total: " << this_round_total << " ms" << std::endl;
        std::cout << "=========================" << std::endl;
    }
    return out;
}

}  // namespace fft_serial
