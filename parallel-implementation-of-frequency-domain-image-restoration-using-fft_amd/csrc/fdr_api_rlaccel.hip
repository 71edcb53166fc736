// fdr_api_rlaccel.hip -- what the two accelerated Richardson-Lucy forms share (kernels in fdr_rlaccel.hip): the workspace (for one
// image or a launch group), the check and the host staging of the alphas and the recursion around a step, on 1 to 8 images.  The
// entry points live beside their plain counterparts (fdr_api_rl.hip, fdr_api_rlfree.hip, the batch in fdr_api_rlbatch.hip), whose
// checks and step they use.
#include "fdr_host.hpp"

using namespace fdr;

static_assert(FDR_RL_ACCEL_MAX < 1.f && FDR_RL_ACCEL_MAX == 1.f - 1.f / 1024.f, "FDR_RL_ACCEL_MAX is 1 - 2^-10");

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassRaDirection = "RLA direction + alpha";
const char* const kPassRaExtrapolate = "RLA extrapolate";

}  // namespace

namespace fdr {

// for one image this is the block the single-image calls have always had
int ensure_rlaccel_workspace(fdr_plan* p, const char* fn, int group) {
    return ensure_workspace(p->rlaccel.ws, fn, "acceleration workspace", group, [p](auto& c, int g) {
        layout(c, p->rlaccel, (size_t)p->M * p->N, 2 * (size_t)rlaccel_partials(p->M, p->N), kMaxGroup, g);
    });
}

float* rlaccel_y_plane(const fdr_plan* p, int k) { return k == 0 ? p->rlaccel.y : p->rlaccel.more + (size_t)(3 * (k - 1)) * p->M * p->N; }
float* rlaccel_u_plane(const fdr_plan* p, int k) { return k == 0 ? p->rlaccel.u : p->rlaccel.more + (size_t)(3 * (k - 1) + 1) * p->M * p->N; }
float* rlaccel_g_plane(const fdr_plan* p, int k) { return k == 0 ? p->rlaccel.g : p->rlaccel.more + (size_t)(3 * (k - 1) + 2) * p->M * p->N; }

int check_alphas(const char* fn, const float* d_alphas, int n, const float* w, int ws, int rows, int cols, const char* what) {
    if (!d_alphas || n <= 0) return FDR_OK;
    if (ranges_overlap(byte_range(d_alphas, (size_t)n * sizeof(float)), window_range(w, rows, cols, ws)))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the alphas overlap the " + what);
    return FDR_OK;
}

int with_host_alphas(const char* fn, float* alphas_host, int n, const std::function<int(float* d_alphas)>& run) {
    DeviceBuffer d;
    const size_t bytes = alphas_host && n > 0 ? (size_t)n * sizeof(float) : 0;
    if (bytes) FDR_ALLOC(d, bytes, fn);
    const int rc = run(d.as<float>());
    if (rc == FDR_OK && bytes) FDR_HIP(hipMemcpy(alphas_host, d.ptr, bytes, hipMemcpyDeviceToHost));
    return rc;
}

// y and g are dense (row stride cols) in the workspace.  The direction of iteration k yields alpha_(k+1); it runs while a later
// iteration still extrapolates, so never for n <= 2 and never after the last step.
int rl_accel_loop(fdr_plan* p, int nimg, int n, int rows, int cols, float* const (*U)[2], const int us[2], int first, float* const* fin, int fs,
                  float* d_alphas, size_t alpha_pitch, hipStream_t s, const RlStep& step, float** result) {
    for (int i = 0; i < nimg && d_alphas && n > 0; ++i)  // alpha_0 = alpha_1 = 0
        FDR_HIP(hipMemsetAsync(d_alphas + (size_t)i * alpha_pitch, 0, (size_t)(n < 2 ? n : 2) * sizeof(float), s));
    for (int i = 0; i < nimg && result; ++i) result[i] = U[i][first & 1];
    return rl_accel_steps(p, nimg, 0, n, n, rows, cols, U, us, first, fin, fs, d_alphas, alpha_pitch, s, step, result);
}

int rl_accel_steps(fdr_plan* p, int nimg, int k0, int k1, int n, int rows, int cols, float* const (*U)[2], const int us[2], int first,
                   float* const* fin, int fs, float* d_alphas, size_t alpha_pitch, hipStream_t s, const RlStep& step, float** result) {
    if (nimg < 1 || nimg > kMaxGroup || nimg > p->rlaccel.ws.count) return fail(FDR_ERR_STATE, "rl_accel_steps: the acceleration workspace does not hold the group");
    float *Y[kMaxGroup], *G[kMaxGroup], *out[kMaxGroup];
    const float *y[kMaxGroup], *cur[kMaxGroup], *prev[kMaxGroup];
    for (int i = 0; i < nimg; ++i) { Y[i] = rlaccel_y_plane(p, i); G[i] = rlaccel_g_plane(p, i); }
    const int n_part = rlaccel_partials(rows, cols);
    for (int k = k0; k < k1; ++k) {
        const int ic = (first + k) & 1, ip = ic ^ 1;
        const bool last = k == n - 1;
        for (int i = 0; i < nimg; ++i) { cur[i] = U[i][ic]; prev[i] = U[i][ip]; y[i] = cur[i]; }
        int ys = us[ic];
        if (k >= 2) {  // u_(k-1) lies in U[i][ip]: read here, then overwritten by the step
            ScopedPass t(p, s, kPassRaExtrapolate);
            FDR_HIP(launch_rlaccel_extrapolate_n(nimg, cur, us[ic], prev, us[ip], p->rlaccel.alpha, Y, cols, rows, cols, s));
            for (int i = 0; i < nimg; ++i) y[i] = Y[i];
            ys = cols;
        }
        for (int i = 0; i < nimg; ++i) out[i] = last && fin ? fin[i] : U[i][ip];
        const int os = last && fin ? fs : us[ip];
        const int rc = step(y, ys, out, os);
        if (rc != FDR_OK) return rc;
        for (int i = 0; i < nimg && result; ++i) result[i] = out[i];
        if (last || n <= 2) continue;
        ScopedPass t(p, s, kPassRaDirection);
        FDR_HIP(launch_rlaccel_direction_n(nimg, out, os, y, ys, G, cols, rows, cols, k >= 1 ? p->rlaccel.part : nullptr, s));
        if (k >= 1)
            FDR_HIP(launch_rlaccel_alpha_n(nimg, p->rlaccel.part, n_part, FDR_RL_ACCEL_MAX, p->rlaccel.alpha, d_alphas ? d_alphas + k + 1 : nullptr, alpha_pitch, s));
    }
    return FDR_OK;
}

}  // namespace fdr
