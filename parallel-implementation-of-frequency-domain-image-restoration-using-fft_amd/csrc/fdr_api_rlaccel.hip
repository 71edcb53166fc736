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

// Per image of the group three M x N float planes, 2 rlaccel_partials(M, N) doubles and one alpha.  Layout: the three planes of
// image 0, the partials of the group, its alphas (8 bytes for one image, which keeps the size a multiple of 8; 4 kMaxGroup otherwise,
// which keeps the planes that follow on 16 bytes), the three planes of the images 1 .. group - 1.  For one image this is the block the
// single-image calls have always had.  The new block is had before the old one is let go (nothing it holds outlives a call).
int ensure_rlaccel_workspace(fdr_plan* p, const char* fn, int group) {
    if (p->ra_block && p->ra_group >= group) return FDR_OK;
    const size_t P = (size_t)p->M * p->N;
    const size_t n_part = 2 * (size_t)rlaccel_partials(p->M, p->N);
    const size_t alpha_bytes = group == 1 ? 8 : sizeof(float) * kMaxGroup;
    char* blk = nullptr;
    if (hipMalloc((void**)&blk, (size_t)group * (3 * P * sizeof(float) + n_part * sizeof(double)) + alpha_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FDR_ERR_ALLOC, std::string(fn) + ": hipMalloc of the acceleration workspace failed");
    }
    if (p->ra_block) (void)hipFree(p->ra_block);  // (waits for the device: nothing queued still uses it)
    float* planes = reinterpret_cast<float*>(blk);
    p->ra_block = blk;
    p->ra_group = group;
    p->ra_y = planes;
    p->ra_u = planes + P;
    p->ra_g = planes + 2 * P;
    p->ra_part = reinterpret_cast<double*>(planes + 3 * P);  // 12 P bytes in: a multiple of 16 (P >= 256)
    p->ra_alpha = reinterpret_cast<float*>(p->ra_part + (size_t)group * n_part);
    p->ra_more = reinterpret_cast<float*>(reinterpret_cast<char*>(p->ra_alpha) + alpha_bytes);
    return FDR_OK;
}

float* rlaccel_y_plane(const fdr_plan* p, int k) { return k == 0 ? p->ra_y : p->ra_more + (size_t)(3 * (k - 1)) * p->M * p->N; }
float* rlaccel_u_plane(const fdr_plan* p, int k) { return k == 0 ? p->ra_u : p->ra_more + (size_t)(3 * (k - 1) + 1) * p->M * p->N; }
float* rlaccel_g_plane(const fdr_plan* p, int k) { return k == 0 ? p->ra_g : p->ra_more + (size_t)(3 * (k - 1) + 2) * p->M * p->N; }

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
    if (nimg < 1 || nimg > kMaxGroup || nimg > p->ra_group) return fail(FDR_ERR_STATE, "rl_accel_steps: the acceleration workspace does not hold the group");
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
            FDR_HIP(launch_rlaccel_extrapolate_n(nimg, cur, us[ic], prev, us[ip], p->ra_alpha, Y, cols, rows, cols, s));
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
        FDR_HIP(launch_rlaccel_direction_n(nimg, out, os, y, ys, G, cols, rows, cols, k >= 1 ? p->ra_part : nullptr, s));
        if (k >= 1)
            FDR_HIP(launch_rlaccel_alpha_n(nimg, p->ra_part, n_part, FDR_RL_ACCEL_MAX, p->ra_alpha, d_alphas ? d_alphas + k + 1 : nullptr, alpha_pitch, s));
    }
    return FDR_OK;
}

}  // namespace fdr
