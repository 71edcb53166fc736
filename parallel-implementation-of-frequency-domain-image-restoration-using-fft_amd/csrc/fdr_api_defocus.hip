// fdr_api_defocus.hip -- the defocus estimate (fdr_defocus.hip): the disk PSF and its three setters, the angular-median profile of
// the cepstrum and the pick of the ring (fdr_estimate_defocus_f32*), and both searches on one cepstrum (fdr_estimate_blur_f32*).
// The cepstrum, its workspace and the motion search are those of fdr_api_motion.hip.
#include "fdr_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace fdr;

namespace {

constexpr int kDefocusMaxDiameters = 4096;  // max_diameter <= min(M, N) / 2 - 2 <= 4094
constexpr double kDiskMaxRadius = 127.0;    // of the setters: size 2 ceil(radius) + 1 <= 255

int disk_check(const char* fn, int size, double radius, const float* out) {
    if (!out) return null_arg(fn);
    if (size <= 0 || size > kDiskMaxSize) return fail(FDR_ERR_ARG, std::string(fn) + ": size must lie in 1 .. 256");
    const int c = size / 2;
    if (!std::isfinite(radius) || !(radius > 0.0) || radius > std::min(c, size - 1 - c) + 0.5)
        return fail(FDR_ERR_ARG, std::string(fn) + ": radius must be finite and in (0, min(c, size - 1 - c) + 0.5], c = size / 2");
    return FDR_OK;
}

// the disk of size 2 ceil(radius) + 1 as the generated PSF of set_psf
int set_psf_disk(fdr_plan* p, const char* fn, double radius, bool op, float K, float gamma, hipStream_t s) {
    if (!p) return null_arg(fn);
    if (!std::isfinite(radius) || !(radius > 0.0) || radius > kDiskMaxRadius)
        return fail(FDR_ERR_ARG, std::string(fn) + ": radius must be finite and in (0, 127]");
    const int size = 2 * (int)std::ceil(radius) + 1;
    return set_psf(p, fn, {PSF_DISK, nullptr, size, size, size, radius}, op, K, gamma, s);
}

// the motion estimate's arguments and refusals with diameters for lengths, and at most kDefocusMaxAngles angles
int defocus_args(const fdr_plan* p, const char* fn, int rows, int cols, int stride, int min_diameter, int max_diameter, double step, MotionArgs* a) {
    const int rc = motion_args(p, fn, rows, cols, stride, min_diameter, max_diameter, step, a, "diameter");
    if (rc != FDR_OK) return rc;
    if (a->n_angles > kDefocusMaxAngles) return fail(FDR_ERR_ARG, std::string(fn) + ": more than 4096 angles");
    return FDR_OK;
}

int ensure_defocus_workspace(fdr_plan* p, const char* fn) {
    bool made = false;
    const int rc = ensure_workspace(p->defocus.ws, fn, "workspace", 1,
                                    [p](auto& c, int) { layout(c, p->defocus, (size_t)kDefocusMaxAngles, (size_t)kDefocusMaxDiameters); }, &made);
    if (rc != FDR_OK || !made) return rc;
    p->defocus.trig_host.resize(2 * (size_t)kDefocusMaxAngles);
    p->defocus.profile_host.resize(kDefocusMaxDiameters);
    return FDR_OK;
}

// the search in the three steps of the motion search (fdr_host.hpp): before the cepstrum ...
int defocus_search_prepare(fdr_plan* p, const char* fn, const MotionArgs& a, hipStream_t s) {
    const int rc = ensure_defocus_workspace(p, fn);
    if (rc != FDR_OK) return rc;
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < a.n_angles; ++k) {
        const double th = (double)k * a.step * (pi / 180.0);
        p->defocus.trig_host[k] = std::cos(th);
        p->defocus.trig_host[(size_t)a.n_angles + k] = std::sin(th);
    }
    FDR_HIP(hipMemcpyAsync(p->defocus.trig, p->defocus.trig_host.data(), 2 * (size_t)a.n_angles * sizeof(double), hipMemcpyHostToDevice, s));
    return FDR_OK;
}

// ... after it ...
int defocus_search_launch(fdr_plan* p, const MotionArgs& a, float* d_profile, hipStream_t s) {
    const size_t bytes = (size_t)a.n_lengths * sizeof(float);
    ScopedPass t(p, s, "defocus profile");
    FDR_HIP(launch_defocus_profile(p->motion.plane, p->M, p->N, p->defocus.trig, a.n_angles, a.min_length, a.n_lengths, p->defocus.profile, s));
    if (d_profile) FDR_HIP(hipMemcpyAsync(d_profile, p->defocus.profile, bytes, hipMemcpyDeviceToDevice, s));
    FDR_HIP(hipMemcpyAsync(p->defocus.profile_host.data(), p->defocus.profile, bytes, hipMemcpyDeviceToHost, s));
    return FDR_OK;
}

// ... and, once the stream is synchronised, the pick from the host copy of T, in double
void defocus_search_pick(const fdr_plan* p, const MotionArgs& a, double sum, fdr_defocus_estimate* est) {
    *est = fdr_defocus_estimate{0, 0.0, 0.0, 0.f, 0.f, a.n_angles, a.n_lengths};
    if (!(sum > 0.0)) return;  // an all-zero window: the defined zero result (the profile is all zeros)
    const float* T = p->defocus.profile_host.data();
    const int n = a.n_lengths;
    int k = 0;
    for (int i = 1; i < n; ++i)
        if (T[i] < T[k]) k = i;  // strict: exact ties keep the lowest index
    std::vector<double> v(T, T + n);
    const double med = median_of(v);
    for (int i = 0; i < n; ++i) v[i] = std::fabs((double)T[i] - med);
    const double mad = median_of(v);
    double off = 0.0;
    if (k > 0 && k < n - 1) {
        const double tm = T[k - 1], t0 = T[k], tp = T[k + 1];
        const double den = tm - 2.0 * t0 + tp;
        if (den != 0.0) off = std::min(0.5, std::max(-0.5, 0.5 * (tm - tp) / den));
    }
    est->diameter = a.min_length + k;
    est->ring = (double)est->diameter + off;
    est->radius = FDR_DEFOCUS_A * est->ring + FDR_DEFOCUS_B;
    est->score = T[k];
    est->confidence = mad > 0.0 ? (float)((med - (double)T[k]) / (1.4826 * mad)) : 0.f;
}

int read_sum_and_wait(fdr_plan* p, double* sum, hipStream_t s) {
    FDR_HIP(hipMemcpyAsync(sum, p->motion.part + motion_pad_partials(p->M, p->N), sizeof(double), hipMemcpyDeviceToHost, s));
    FDR_HIP(hipStreamSynchronize(s));
    return FDR_OK;
}

// the whole estimate on `s`, synchronous: d_profile (may be null) gets a copy of T
int defocus_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const MotionArgs& a,
                     fdr_defocus_estimate* est, float* d_profile, hipStream_t s) {
    int rc = ensure_motion_workspace(p, fn);
    if (rc == FDR_OK) rc = defocus_search_prepare(p, fn, a, s);
    if (rc == FDR_OK) rc = motion_cepstrum_plane(p, d_img, rows, cols, stride, s);
    if (rc == FDR_OK) rc = defocus_search_launch(p, a, d_profile, s);
    double sum = 0.0;
    if (rc == FDR_OK) rc = read_sum_and_wait(p, &sum, s);
    if (rc != FDR_OK) return rc;
    defocus_search_pick(p, a, sum, est);
    return FDR_OK;
}

// both searches on one cepstrum, synchronous
int blur_dev_impl(fdr_plan* p, const char* fn, const float* d_img, int rows, int cols, int stride, const MotionArgs& am, const MotionArgs& ad,
                  fdr_motion_estimate* motion, fdr_defocus_estimate* defocus, int* kind, hipStream_t s) {
    int rc = ensure_motion_workspace(p, fn);
    if (rc == FDR_OK) rc = motion_search_prepare(p, fn, am, s);
    if (rc == FDR_OK) rc = defocus_search_prepare(p, fn, ad, s);
    if (rc == FDR_OK) rc = motion_cepstrum_plane(p, d_img, rows, cols, stride, s);
    if (rc == FDR_OK) rc = motion_search_launch(p, am, nullptr, s);
    if (rc == FDR_OK) rc = defocus_search_launch(p, ad, nullptr, s);
    double sum = 0.0;
    if (rc == FDR_OK) rc = read_sum_and_wait(p, &sum, s);
    if (rc != FDR_OK) return rc;
    motion_search_pick(p, am, sum, motion);
    defocus_search_pick(p, ad, sum, defocus);
    *kind = fdr_blur_kind(motion->confidence, defocus->confidence);
    return FDR_OK;
}

}  // namespace

extern "C" {

int fdr_psf_disk_dev(int device, int size, double radius, float* d_out, void* stream) {
    const int rc = disk_check("fdr_psf_disk_dev", size, radius, d_out);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(device));
    FDR_HIP(launch_psf_disk(size, radius, d_out, (hipStream_t)stream));
    return FDR_OK;
}

int fdr_psf_disk(int size, double radius, float* out_host) {
    const char* fn = "fdr_psf_disk";
    const int rc = disk_check(fn, size, radius, out_host);
    if (rc != FDR_OK) return rc;
    const size_t bytes = (size_t)size * size * sizeof(float);
    DeviceBuffer d;
    FDR_ALLOC(d, bytes, fn);
    FDR_HIP(launch_psf_disk(size, radius, d.as<float>(), nullptr));
    FDR_HIP(hipMemcpy(out_host, d.ptr, bytes, hipMemcpyDeviceToHost));
    return FDR_OK;
}

int fdr_set_psf_disk(fdr_plan* p, double radius, float K, void* stream) {
    return set_psf_disk(p, "fdr_set_psf_disk", radius, false, K, 0.f, (hipStream_t)stream);
}

int fdr_set_psf_disk_cls(fdr_plan* p, double radius, float K, float gamma, void* stream) {
    return set_psf_disk(p, "fdr_set_psf_disk_cls", radius, false, K, gamma, (hipStream_t)stream);
}

int fdr_set_operator_psf_disk(fdr_plan* p, double radius, void* stream) {
    return set_psf_disk(p, "fdr_set_operator_psf_disk", radius, true, 0.f, 0.f, (hipStream_t)stream);
}

int fdr_blur_kind(double motion_confidence, double defocus_confidence) {
    const double m = motion_confidence / FDR_MOTION_CONF_MIN, f = defocus_confidence / FDR_DEFOCUS_CONF_MIN;
    if (m < 1.0 && f < 1.0) return FDR_BLUR_NONE;
    return m >= f ? FDR_BLUR_MOTION : FDR_BLUR_DEFOCUS;
}

int fdr_estimate_defocus_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, int min_diameter, int max_diameter,
                                 double angle_step_deg, fdr_defocus_estimate* est, float* d_profile, void* stream) {
    const char* fn = "fdr_estimate_defocus_f32_dev";
    if (!p || !d_img || !est) return null_arg(fn);
    MotionArgs a{};
    const int rc = defocus_args(p, fn, rows, cols, stride, min_diameter, max_diameter, angle_step_deg, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return defocus_dev_impl(p, fn, d_img, rows, cols, stride, a, est, d_profile, (hipStream_t)stream);
}

int fdr_estimate_defocus_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, int min_diameter, int max_diameter,
                             double angle_step_deg, fdr_defocus_estimate* est, float* profile_host) {
    const char* fn = "fdr_estimate_defocus_f32";
    if (!p || !img_host || !est) return null_arg(fn);
    MotionArgs a{};
    int rc = defocus_args(p, fn, rows, cols, stride, min_diameter, max_diameter, angle_step_deg, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = host_image_call(p, fn, img_host, rows, cols, stride, nullptr, 0, 0, 0, [&](const float* d_in, float*) {
        return defocus_dev_impl(p, fn, d_in, rows, cols, cols, a, est, nullptr, nullptr);
    });
    if (rc != FDR_OK) return rc;
    if (profile_host) std::memcpy(profile_host, p->defocus.profile_host.data(), (size_t)a.n_lengths * sizeof(float));
    return FDR_OK;
}

int fdr_estimate_blur_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, int min_length, int max_length,
                              double motion_step_deg, int min_diameter, int max_diameter, double defocus_step_deg,
                              fdr_motion_estimate* motion, fdr_defocus_estimate* defocus, int* kind, void* stream) {
    const char* fn = "fdr_estimate_blur_f32_dev";
    if (!p || !d_img || !motion || !defocus || !kind) return null_arg(fn);
    MotionArgs am{}, ad{};
    int rc = motion_args(p, fn, rows, cols, stride, min_length, max_length, motion_step_deg, &am);
    if (rc == FDR_OK) rc = defocus_args(p, fn, rows, cols, stride, min_diameter, max_diameter, defocus_step_deg, &ad);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return blur_dev_impl(p, fn, d_img, rows, cols, stride, am, ad, motion, defocus, kind, (hipStream_t)stream);
}

int fdr_estimate_blur_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, int min_length, int max_length,
                          double motion_step_deg, int min_diameter, int max_diameter, double defocus_step_deg, fdr_motion_estimate* motion,
                          fdr_defocus_estimate* defocus, int* kind) {
    const char* fn = "fdr_estimate_blur_f32";
    if (!p || !img_host || !motion || !defocus || !kind) return null_arg(fn);
    MotionArgs am{}, ad{};
    int rc = motion_args(p, fn, rows, cols, stride, min_length, max_length, motion_step_deg, &am);
    if (rc == FDR_OK) rc = defocus_args(p, fn, rows, cols, stride, min_diameter, max_diameter, defocus_step_deg, &ad);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    return host_image_call(p, fn, img_host, rows, cols, stride, nullptr, 0, 0, 0, [&](const float* d_in, float*) {
        return blur_dev_impl(p, fn, d_in, rows, cols, cols, am, ad, motion, defocus, kind, nullptr);
    });
}

}  // extern "C"
