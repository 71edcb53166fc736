// fdr_api_register.hip -- registering the frames of a burst (fdr_register.hip): per frame the pair window pass, the plan's complex
// 2-D transform of the picture pair and of the PSF pair, the cross-power pass, the normalising sweep, the transform inverse and the
// peak pass (fdr_register_frames_f32*); and the bilinear shift of the PSFs by such results (fdr_psf_shift_f32*).  The picture plane
// and the Hann tables are the motion block's (fdr_api_motion.hip); the PSF pair plane, the partials and the results have a block
// of their own.
#include "fdr_host.hpp"

#include <cmath>
#include <cstddef>

using namespace fdr;

static_assert(sizeof(fdr_frame_shift) == 24 && offsetof(fdr_frame_shift, dx) == 8 && offsetof(fdr_frame_shift, peak) == 16 &&
                  offsetof(fdr_frame_shift, confidence) == 20,
              "fdr_register.hip writes and reads a result as two doubles and two floats");

namespace {

constexpr int kRegisterMinWindow = 16;
// the pass names (static strings: PassTimer compares them by pointer)
const char* const kPassRgWindow = "register window";
const char* const kPassRgFft = "register transforms";
const char* const kPassRgCross = "register cross-power";
const char* const kPassRgPeak = "register peak";
constexpr int kShiftMaxPad = 8192;

struct RegisterArgs {
    const float* imgs; size_t img_pitch; int count, rows, cols, stride;
    const float* psfs; size_t psf_pitch; int prows, pcols, pstride;
};
// the parameters with their defaults resolved
struct RegisterRange { int reference, range_rows, range_cols; float eps_rel; };

// everything a registration call refuses, before any device work (`shifts`: where the results go)
int register_check(const fdr_plan* p, const char* fn, const RegisterArgs& a, const fdr_register_params* prm, const void* shifts, bool dev,
                   RegisterRange* r) {
    if (!p || !a.imgs || !prm || !shifts) return null_arg(fn);
    const std::string f(fn);
    const int rc = check_window(p, fn, NEED_MOTION, a.rows, a.cols, a.stride, a.cols, kRegisterMinWindow);
    if (rc != FDR_OK) return rc;
    if (a.count < 1 || a.count > FDR_MAX_FRAMES) return fail(FDR_ERR_ARG, f + ": count must be 1 .. FDR_MAX_FRAMES");
    if (a.count > 1 && a.img_pitch < window_span(a.rows, a.cols, a.stride)) return fail(FDR_ERR_ARG, f + ": img_pitch is below the span of one frame");
    if (prm->reference < 0 || prm->reference >= a.count) return fail(FDR_ERR_ARG, f + ": reference must be 0 .. count - 1");
    if (prm->max_shift_rows < 0 || prm->max_shift_cols < 0) return fail(FDR_ERR_ARG, f + ": negative max_shift");
    const int dflt = (a.rows < a.cols ? a.rows : a.cols) / 4;
    r->reference = prm->reference;
    r->range_rows = prm->max_shift_rows ? prm->max_shift_rows : dflt;
    r->range_cols = prm->max_shift_cols ? prm->max_shift_cols : dflt;
    if (r->range_rows < 1 || 2 * r->range_rows >= p->M) return fail(FDR_ERR_ARG, f + ": max_shift_rows must be 1 .. (M - 1) / 2");
    if (r->range_cols < 1 || 2 * r->range_cols >= p->N) return fail(FDR_ERR_ARG, f + ": max_shift_cols must be 1 .. (N - 1) / 2");
    if (!std::isfinite(prm->eps_rel) || prm->eps_rel < 0.f) return fail(FDR_ERR_ARG, f + ": eps_rel must be finite and >= 0");
    r->eps_rel = prm->eps_rel != 0.f ? prm->eps_rel : FDR_REGISTER_EPS_REL;
    if (a.psfs) {
        if (a.prows < 1 || a.pcols < 1 || a.prows > p->M || a.pcols > p->N || a.pstride < a.pcols)
            return fail(FDR_ERR_ARG, f + ": the PSFs must be at least 1 x 1, fit the plan and have pstride >= pcols");
        if (a.count > 1 && a.psf_pitch < window_span(a.prows, a.pcols, a.pstride)) return fail(FDR_ERR_ARG, f + ": psf_pitch is below the span of one PSF");
    }
    if (dev && reinterpret_cast<uintptr_t>(shifts) % 8 != 0) return fail(FDR_ERR_ARG, f + ": d_shifts must be 8-byte aligned");
    return FDR_OK;
}

int ensure_register_workspace(fdr_plan* p, const char* fn) {
    const int rc = ensure_motion_workspace(p, fn);
    if (rc != FDR_OK) return rc;
    return ensure_workspace(p->regist.ws, fn, "registration workspace", 1, [p](auto& c, int) {
        layout(c, p->regist, (size_t)p->M, (size_t)p->N, (size_t)register_cross_partials(p->M, p->N), (size_t)register_peak_partials(p->M, p->N),
               (size_t)FDR_MAX_FRAMES);
    });
}

// the whole estimate on `s`, asynchronous: frame k's result to d_shifts[k], its correlation plane to d_corr + k M N (d_corr may be null)
int register_dev_impl(fdr_plan* p, const RegisterArgs& a, const RegisterRange& r, fdr_frame_shift* d_shifts, float* d_corr, hipStream_t s) {
    const int M = p->M, N = p->N;
    const size_t P = (size_t)M * N;
    float2* plane = p->motion.plane;
    double* sum = p->regist.part + register_cross_partials(M, N);
    const float* ref = a.imgs + (size_t)r.reference * a.img_pitch;
    {
        ScopedPass t(p, s, kPassRgWindow);
        FDR_HIP(launch_motion_hann(p->motion.hann, a.rows, a.cols, s));
    }
    for (int k = 0; k < a.count; ++k) {
        if (k == r.reference) {
            FDR_HIP(launch_register_reference(d_shifts + k, s));
            if (d_corr) FDR_HIP(hipMemsetAsync(d_corr + (size_t)k * P, 0, P * sizeof(float), s));
            continue;
        }
        {
            ScopedPass t(p, s, kPassRgWindow);
            FDR_HIP(launch_register_pair(ref, a.imgs + (size_t)k * a.img_pitch, a.rows, a.cols, a.stride, p->motion.hann, plane, M, N,
                                         p->regist.peak, sum + 1, s));  // (the peak partials are free until the peak pass)
            if (a.psfs)
                FDR_HIP(launch_register_pair(a.psfs + (size_t)r.reference * a.psf_pitch, a.psfs + (size_t)k * a.psf_pitch, a.prows, a.pcols,
                                             a.pstride, nullptr, p->regist.psf, M, N, nullptr, nullptr, s));
        }
        int rc;
        {
            ScopedPass t(p, s, kPassRgFft);
            rc = dft2d_dev(p, plane, p->slots[0].work2, false, s);
            if (rc == FDR_OK && a.psfs) rc = dft2d_dev(p, p->regist.psf, p->slots[0].work2, false, s);
        }
        if (rc != FDR_OK) return rc;
        {
            ScopedPass t(p, s, kPassRgCross);
            FDR_HIP(launch_register_cross(plane, a.psfs ? p->regist.psf : nullptr, M, N, p->regist.part, s));
            FDR_HIP(launch_register_normalize(plane, M, N, sum, r.eps_rel, s));
        }
        {
            ScopedPass t(p, s, kPassRgFft);
            rc = dft2d_dev(p, plane, p->slots[0].work2, true, s);
        }
        if (rc != FDR_OK) return rc;
        {
            ScopedPass t(p, s, kPassRgPeak);
            FDR_HIP(launch_register_peak(plane, M, N, r.range_rows, r.range_cols, sum, p->regist.peak, d_shifts + k, s));
        }
        if (d_corr) FDR_HIP(launch_real_part(plane, d_corr + (size_t)k * P, P, s));
    }
    return FDR_OK;
}

struct ShiftArgs {
    const float* psfs; size_t psf_pitch; int count, prows, pcols, pstride;
    const fdr_frame_shift* shifts; float* out; size_t out_pitch; int out_stride;
};

int shift_check(const char* fn, const ShiftArgs& a, const fdr_psf_shift_params* prm, bool dev) {
    if (!a.psfs || !a.shifts || !prm || !a.out) return null_arg(fn);
    const std::string f(fn);
    if (a.count < 1 || a.count > FDR_MAX_FRAMES) return fail(FDR_ERR_ARG, f + ": count must be 1 .. FDR_MAX_FRAMES");
    if (a.prows < 1 || a.pcols < 1 || a.prows > 8192 || a.pcols > 8192 || a.pstride < a.pcols)
        return fail(FDR_ERR_ARG, f + ": the PSFs must be 1 .. 8192 per side and have pstride >= pcols");
    if (prm->pad_rows < 1 || prm->pad_cols < 1 || prm->pad_rows > kShiftMaxPad || prm->pad_cols > kShiftMaxPad)
        return fail(FDR_ERR_ARG, f + ": pad_rows and pad_cols must be 1 .. 8192");
    const int orows = a.prows + 2 * prm->pad_rows, ocols = a.pcols + 2 * prm->pad_cols;
    if (a.out_stride < ocols) return fail(FDR_ERR_ARG, f + ": out_stride is below pcols + 2 pad_cols");
    if (a.count > 1 && a.psf_pitch < window_span(a.prows, a.pcols, a.pstride)) return fail(FDR_ERR_ARG, f + ": psf_pitch is below the span of one PSF");
    if (a.count > 1 && a.out_pitch < window_span(orows, ocols, a.out_stride)) return fail(FDR_ERR_ARG, f + ": out_pitch is below the span of one output PSF");
    if (dev && reinterpret_cast<uintptr_t>(a.shifts) % 8 != 0) return fail(FDR_ERR_ARG, f + ": d_shifts must be 8-byte aligned");
    const ByteRange out = window_range(a.out, orows, ocols, a.out_stride, a.count, a.out_pitch);
    if (ranges_overlap(out, window_range(a.psfs, a.prows, a.pcols, a.pstride, a.count, a.psf_pitch)) ||
        ranges_overlap(out, byte_range(a.shifts, (size_t)a.count * sizeof(fdr_frame_shift))))
        return fail(FDR_ERR_ARG, f + ": the output overlaps the PSFs or the shifts");
    return FDR_OK;
}

}  // namespace

extern "C" {

int fdr_register_frames_f32_dev(fdr_plan* p, const float* d_imgs, size_t img_pitch, int count, int rows, int cols, int stride,
                                const float* d_psfs, size_t psf_pitch, int prows, int pcols, int pstride, const fdr_register_params* params,
                                fdr_frame_shift* d_shifts, float* d_corr) {
    const char* fn = "fdr_register_frames_f32_dev";
    const RegisterArgs a{d_imgs, img_pitch, count, rows, cols, stride, d_psfs, psf_pitch, prows, pcols, pstride};
    RegisterRange r{};
    int rc = register_check(p, fn, a, params, d_shifts, true, &r);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = ensure_register_workspace(p, fn);
    if (rc != FDR_OK) return rc;
    return register_dev_impl(p, a, r, d_shifts, d_corr, (hipStream_t)params->stream);
}

// host pointers: every frame and PSF in (dense, one-shot device buffers), the estimate on the null stream into the block's results,
// those back; synchronous
int fdr_register_frames_f32(fdr_plan* p, const float* imgs_host, size_t img_pitch, int count, int rows, int cols, int stride,
                            const float* psfs_host, size_t psf_pitch, int prows, int pcols, int pstride, const fdr_register_params* params,
                            fdr_frame_shift* shifts_host) {
    const char* fn = "fdr_register_frames_f32";
    const RegisterArgs h{imgs_host, img_pitch, count, rows, cols, stride, psfs_host, psf_pitch, prows, pcols, pstride};
    RegisterRange r{};
    int rc = register_check(p, fn, h, params, shifts_host, false, &r);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = ensure_register_workspace(p, fn);
    if (rc != FDR_OK) return rc;
    const size_t in_px = (size_t)rows * cols, psf_px = psfs_host ? (size_t)prows * pcols : 0;
    DeviceBuffer d_in, d_psf;
    FDR_ALLOC(d_in, (size_t)count * in_px * sizeof(float), fn);
    if (psfs_host) FDR_ALLOC(d_psf, (size_t)count * psf_px * sizeof(float), fn);
    {
        ScopedPhase phase(p, FDR_PHASE_H2D, nullptr);
        for (int k = 0; k < count; ++k) {
            FDR_HIP(hipMemcpy2D(d_in.as<float>() + (size_t)k * in_px, (size_t)cols * sizeof(float), imgs_host + (size_t)k * img_pitch,
                                (size_t)stride * sizeof(float), (size_t)cols * sizeof(float), (size_t)rows, hipMemcpyHostToDevice));
            if (psfs_host)
                FDR_HIP(hipMemcpy2D(d_psf.as<float>() + (size_t)k * psf_px, (size_t)pcols * sizeof(float), psfs_host + (size_t)k * psf_pitch,
                                    (size_t)pstride * sizeof(float), (size_t)pcols * sizeof(float), (size_t)prows, hipMemcpyHostToDevice));
        }
    }
    fdr_frame_shift* d_shifts = reinterpret_cast<fdr_frame_shift*>(p->regist.result);
    {
        ScopedPhase phase(p, FDR_PHASE_COMPUTE, nullptr);
        const RegisterArgs a{d_in.as<float>(), in_px, count, rows, cols, cols, d_psf.as<float>(), psf_px, prows, pcols, pcols};
        rc = register_dev_impl(p, a, r, d_shifts, nullptr, nullptr);
    }
    if (rc == FDR_OK) {
        ScopedPhase phase(p, FDR_PHASE_D2H, nullptr);
        FDR_HIP(hipMemcpy(shifts_host, d_shifts, (size_t)count * sizeof(fdr_frame_shift), hipMemcpyDeviceToHost));
    }
    (void)hipStreamSynchronize(nullptr);  // (also on an error: the one-shot buffers are freed on return)
    resolve_phases(p);
    return rc;
}

int fdr_psf_shift_f32_dev(int device, const float* d_psfs, size_t psf_pitch, int count, int prows, int pcols, int pstride,
                          const fdr_frame_shift* d_shifts, const fdr_psf_shift_params* params, float* d_out, size_t out_pitch, int out_stride) {
    const char* fn = "fdr_psf_shift_f32_dev";
    const ShiftArgs a{d_psfs, psf_pitch, count, prows, pcols, pstride, d_shifts, d_out, out_pitch, out_stride};
    const int rc = shift_check(fn, a, params, true);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(device));
    FDR_HIP(launch_psf_shift(d_psfs, psf_pitch, count, prows, pcols, pstride, d_shifts, params->pad_rows, params->pad_cols, d_out, out_pitch,
                             out_stride, (hipStream_t)params->stream));
    return FDR_OK;
}

int fdr_psf_shift_f32(int device, const float* psfs_host, size_t psf_pitch, int count, int prows, int pcols, int pstride,
                      const fdr_frame_shift* shifts_host, const fdr_psf_shift_params* params, float* out_host, size_t out_pitch, int out_stride) {
    const char* fn = "fdr_psf_shift_f32";
    const ShiftArgs h{psfs_host, psf_pitch, count, prows, pcols, pstride, shifts_host, out_host, out_pitch, out_stride};
    const int rc = shift_check(fn, h, params, false);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(device));
    const int orows = prows + 2 * params->pad_rows, ocols = pcols + 2 * params->pad_cols;
    const size_t psf_px = (size_t)prows * pcols, out_px = (size_t)orows * ocols;
    DeviceBuffer d_psf, d_sh, d_out;
    FDR_ALLOC(d_psf, (size_t)count * psf_px * sizeof(float), fn);
    FDR_ALLOC(d_sh, (size_t)count * sizeof(fdr_frame_shift), fn);
    FDR_ALLOC(d_out, (size_t)count * out_px * sizeof(float), fn);
    for (int k = 0; k < count; ++k)
        FDR_HIP(hipMemcpy2D(d_psf.as<float>() + (size_t)k * psf_px, (size_t)pcols * sizeof(float), psfs_host + (size_t)k * psf_pitch,
                            (size_t)pstride * sizeof(float), (size_t)pcols * sizeof(float), (size_t)prows, hipMemcpyHostToDevice));
    FDR_HIP(hipMemcpy(d_sh.ptr, shifts_host, (size_t)count * sizeof(fdr_frame_shift), hipMemcpyHostToDevice));
    FDR_HIP(launch_psf_shift(d_psf.as<float>(), psf_px, count, prows, pcols, pcols, d_sh.ptr, params->pad_rows, params->pad_cols,
                             d_out.as<float>(), out_px, ocols, nullptr));
    for (int k = 0; k < count; ++k)
        FDR_HIP(hipMemcpy2D(out_host + (size_t)k * out_pitch, (size_t)out_stride * sizeof(float), d_out.as<float>() + (size_t)k * out_px,
                            (size_t)ocols * sizeof(float), (size_t)ocols * sizeof(float), (size_t)orows, hipMemcpyDeviceToHost));
    return FDR_OK;
}

}  // extern "C"
