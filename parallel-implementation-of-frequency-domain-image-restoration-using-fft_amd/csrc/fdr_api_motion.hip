// fdr_api_motion.hip -- the motion-blur estimate (fdr_motion.hip): window / pad, the plan's complex 2-D transform forward, log |G|,
// the transform inverse, then the score gather (fdr_estimate_motion_f32*) or the real part (fdr_cepstrum_f32*).  The arguments, the
// workspace, the cepstrum and the search are shared with the defocus and the combined estimate (fdr_api_defocus.hip; fdr_host.hpp).
#include "fdr_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace fdr;

namespace {

constexpr int kMotionMinWindow = 16;
constexpr size_t kMotionMaxTable = (size_t)1 << 26;

// the table (device and host) and the trig table for `a`, grown when a larger one is asked for
int ensure_motion_table(fdr_plan* p, const char* fn, const MotionArgs& a) {
    const size_t nt = (size_t)a.n_angles * a.n_lengths;  // (at most kMotionMaxTable: motion_args)
    int rc = ensure_workspace(p->motion.table_ws, fn, "table", (int)nt, [p](auto& c, int n) { layout(c, p->motion.table, (size_t)n, 4); });
    if (rc == FDR_OK)
        rc = ensure_workspace(p->motion.trig_ws, fn, "table", 2 * a.n_angles, [p](auto& c, int n) { layout(c, p->motion.trig, (size_t)n, 8); });
    if (rc == FDR_OK && p->motion.table_host.size() < nt) p->motion.table_host.resize(nt);
    return rc;
}

}  // namespace

namespace fdr {

int motion_args(const fdr_plan* p, const char* fn, int rows, int cols, int stride, int min_length, int max_length, double step, MotionArgs* a,
                const char* what) {
    const std::string f(fn), w(what);
    const int rc = check_window(p, fn, NEED_MOTION, rows, cols, stride, cols, kMotionMinWindow);
    if (rc != FDR_OK) return rc;
    if (min_length < 0 || max_length < 0) return fail(FDR_ERR_ARG, f + ": negative " + w);
    if (!std::isfinite(step) || step < 0.0 || step > 90.0) return fail(FDR_ERR_ARG, std::string(fn) + ": the angle step must be finite and in (0, 90]");
    a->min_length = min_length ? min_length : 3;
    a->max_length = max_length ? max_length : std::min(100, std::min(rows, cols) / 4);
    a->step = step != 0.0 ? step : 0.5;
    if (a->min_length < 2) return fail(FDR_ERR_ARG, f + ": min_" + w + " < 2");
    if (a->min_length > a->max_length) return fail(FDR_ERR_ARG, f + ": min_" + w + " > max_" + w);
    if (a->max_length > std::min(p->M, p->N) / 2 - 2) return fail(FDR_ERR_ARG, f + ": max_" + w + " > min(M, N) / 2 - 2");
    const double na = std::ceil(180.0 / a->step);
    a->n_lengths = a->max_length - a->min_length + 1;
    if (na * a->n_lengths > (double)kMotionMaxTable) return fail(FDR_ERR_ARG, std::string(fn) + ": score table above 2^26 entries");
    a->n_angles = (int)na;
    return FDR_OK;
}

int ensure_motion_workspace(fdr_plan* p, const char* fn) {
    return ensure_workspace(p->motion.ws, fn, "workspace", 1, [p](auto& c, int) {
        layout(c, p->motion, (size_t)p->M, (size_t)p->N, (size_t)motion_pad_partials(p->M, p->N));
    });
}

int motion_cepstrum_plane(fdr_plan* p, const float* d_img, int rows, int cols, int stride, hipStream_t s) {
    ScopedPass t(p, s, "cepstrum");
    FDR_HIP(launch_motion_window(d_img, rows, cols, stride, p->motion.hann, p->motion.plane, p->M, p->N, p->motion.part, s));
    int rc = dft2d_dev(p, p->motion.plane, p->slots[0].work2, false, s);
    if (rc != FDR_OK) return rc;
    FDR_HIP(launch_motion_log(p->motion.plane, p->M, p->N, p->motion.part + motion_pad_partials(p->M, p->N), s));
    return dft2d_dev(p, p->motion.plane, p->slots[0].work2, true, s);
}

double median_of(std::vector<double>& v) {
    const size_t n = v.size(), h = n / 2;
    std::nth_element(v.begin(), v.begin() + h, v.end());
    const double hi = v[h];
    if (n % 2) return hi;
    const double lo = *std::max_element(v.begin(), v.begin() + h);
    return 0.5 * (lo + hi);
}

int motion_search_prepare(fdr_plan* p, const char* fn, const MotionArgs& a, hipStream_t s) {
    const int rc = ensure_motion_table(p, fn, a);
    if (rc != FDR_OK) return rc;
    const double pi = 3.14159265358979323846;
    p->motion.trig_host.resize(2 * (size_t)a.n_angles);
    for (int k = 0; k < a.n_angles; ++k) {
        const double th = (double)k * a.step * (pi / 180.0);
        p->motion.trig_host[k] = std::cos(th);
        p->motion.trig_host[(size_t)a.n_angles + k] = std::sin(th);
    }
    FDR_HIP(hipMemcpyAsync(p->motion.trig, p->motion.trig_host.data(), p->motion.trig_host.size() * sizeof(double), hipMemcpyHostToDevice, s));
    return FDR_OK;
}

int motion_search_launch(fdr_plan* p, const MotionArgs& a, float* d_scores, hipStream_t s) {
    const size_t nt = (size_t)a.n_angles * a.n_lengths;
    ScopedPass t(p, s, "motion score");
    FDR_HIP(launch_motion_score(p->motion.plane, p->M, p->N, p->motion.trig, a.n_angles, a.min_length, a.n_lengths, p->motion.table, s));
    if (d_scores) FDR_HIP(hipMemcpyAsync(d_scores, p->motion.table, nt * sizeof(float), hipMemcpyDeviceToDevice, s));
    FDR_HIP(hipMemcpyAsync(p->motion.table_host.data(), p->motion.table, nt * sizeof(float), hipMemcpyDeviceToHost, s));
    return FDR_OK;
}

void motion_search_pick(const fdr_plan* p, const MotionArgs& a, double sum, fdr_motion_estimate* est) {
    const size_t nt = (size_t)a.n_angles * a.n_lengths;
    *est = fdr_motion_estimate{0, 0.0, 0.f, 0.f, a.n_angles, a.n_lengths};
    if (!(sum > 0.0)) return;  // an all-zero window: the defined zero result (the table is all zeros)
    const float* S = p->motion.table_host.data();
    size_t kmin = 0;
    for (size_t k = 1; k < nt; ++k)
        if (S[k] < S[kmin]) kmin = k;  // strict: exact ties keep the lowest flat index
    std::vector<double> v(S, S + nt);
    const double med = median_of(v);
    for (size_t k = 0; k < nt; ++k) v[k] = std::fabs((double)S[k] - med);
    const double mad = median_of(v);
    const double smin = (double)S[kmin];
    est->length = a.min_length + (int)(kmin % a.n_lengths);
    est->angle_deg = (double)(kmin / a.n_lengths) * a.step;
    est->score = S[kmin];
    est->confidence = mad > 0.0 ? (float)((med - smin) / (1.4826 * mad)) : 0.f;
}

}  // namespace fdr

namespace {

int cepstrum_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, float* d_out, hipStream_t s) {
    int rc = ensure_motion_workspace(p, fn);
    if (rc == FDR_OK) rc = motion_cepstrum_plane(p, d_img, rows, cols, stride, s);
    if (rc != FDR_OK) return rc;
    FDR_HIP(launch_real_part(p->motion.plane, d_out, (size_t)p->M * p->N, s));
    return FDR_OK;
}

// the whole estimate on `s`, synchronous: d_scores (may be null) gets a copy of the table
int estimate_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const MotionArgs& a,
                      fdr_motion_estimate* est, float* d_scores, hipStream_t s) {
    int rc = ensure_motion_workspace(p, fn);
    if (rc == FDR_OK) rc = motion_search_prepare(p, fn, a, s);
    if (rc == FDR_OK) rc = motion_cepstrum_plane(p, d_img, rows, cols, stride, s);
    if (rc == FDR_OK) rc = motion_search_launch(p, a, d_scores, s);
    if (rc != FDR_OK) return rc;
    double sum = 0.0;
    FDR_HIP(hipMemcpyAsync(&sum, p->motion.part + motion_pad_partials(p->M, p->N), sizeof(double), hipMemcpyDeviceToHost, s));
    FDR_HIP(hipStreamSynchronize(s));
    motion_search_pick(p, a, sum, est);
    return FDR_OK;
}

}  // namespace

extern "C" {

int fdr_cepstrum_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, float* d_out, void* stream) {
    const char* fn = "fdr_cepstrum_f32_dev";
    if (!p || !d_img || !d_out) return null_arg(fn);
    const int rc = check_window(p, fn, NEED_MOTION, rows, cols, stride, cols, kMotionMinWindow);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return cepstrum_dev_impl(p, fn, d_img, rows, cols, stride, d_out, (hipStream_t)stream);
}

int fdr_cepstrum_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, float* out_host) {
    const char* fn = "fdr_cepstrum_f32";
    if (!p || !img_host || !out_host) return null_arg(fn);
    const int rc = check_window(p, fn, NEED_MOTION, rows, cols, stride, cols, kMotionMinWindow);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return host_image_call(p, fn, img_host, rows, cols, stride, out_host, p->M, p->N, p->N, [&](const float* d_in, float* d_out) {
        return cepstrum_dev_impl(p, fn, d_in, rows, cols, cols, d_out, nullptr);
    });
}

int fdr_estimate_motion_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, int min_length, int max_length,
                                double angle_step_deg, fdr_motion_estimate* est, float* d_scores, void* stream) {
    const char* fn = "fdr_estimate_motion_f32_dev";
    if (!p || !d_img || !est) return null_arg(fn);
    MotionArgs a{};
    const int rc = motion_args(p, fn, rows, cols, stride, min_length, max_length, angle_step_deg, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return estimate_dev_impl(p, fn, d_img, rows, cols, stride, a, est, d_scores, (hipStream_t)stream);
}

int fdr_estimate_motion_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, int min_length, int max_length,
                            double angle_step_deg, fdr_motion_estimate* est, float* scores_host) {
    const char* fn = "fdr_estimate_motion_f32";
    if (!p || !img_host || !est) return null_arg(fn);
    MotionArgs a{};
    int rc = motion_args(p, fn, rows, cols, stride, min_length, max_length, angle_step_deg, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = host_image_call(p, fn, img_host, rows, cols, stride, nullptr, 0, 0, 0, [&](const float* d_in, float*) {
        return estimate_dev_impl(p, fn, d_in, rows, cols, cols, a, est, nullptr, nullptr);
    });
    if (rc != FDR_OK) return rc;
    if (scores_host) std::memcpy(scores_host, p->motion.table_host.data(), (size_t)a.n_angles * a.n_lengths * sizeof(float));
    return FDR_OK;
}

}  // extern "C"
