// fdr_api_rlaccel.hip -- what the two accelerated Richardson-Lucy forms share (kernels in fdr_rlaccel.hip): the workspace, the
// check and the host staging of the alphas and the recursion around a step.  The entry points live beside their plain counterparts
// (fdr_api_rl.hip, fdr_api_rlfree.hip), whose checks and step they use.
#include "fdr_host.hpp"

using namespace fdr;

static_assert(FDR_RL_ACCEL_MAX < 1.f && FDR_RL_ACCEL_MAX == 1.f - 1.f / 1024.f, "FDR_RL_ACCEL_MAX is 1 - 2^-10");

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassRaDirection = "RLA direction + alpha";
const char* const kPassRaExtrapolate = "RLA extrapolate";

}  // namespace

namespace fdr {

// three M x N float planes, 2 rlaccel_partials(M, N) doubles, alpha (8 bytes keep the size a multiple of 8)
int ensure_rlaccel_workspace(fdr_plan* p, const char* fn) {
    if (p->ra_block) return FDR_OK;
    const size_t P = (size_t)p->M * p->N;
    const size_t n_part = 2 * (size_t)rlaccel_partials(p->M, p->N);
    char* blk = nullptr;
    if (hipMalloc((void**)&blk, 3 * P * sizeof(float) + n_part * sizeof(double) + 8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FDR_ERR_ALLOC, std::string(fn) + ": hipMalloc of the acceleration workspace failed");
    }
    float* planes = reinterpret_cast<float*>(blk);
    p->ra_block = blk;
    p->ra_y = planes;
    p->ra_u = planes + P;
    p->ra_g = planes + 2 * P;
    p->ra_part = reinterpret_cast<double*>(planes + 3 * P);  // 12 P bytes in: a multiple of 8 (P >= 256)
    p->ra_alpha = reinterpret_cast<float*>(p->ra_part + n_part);
    return FDR_OK;
}

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
int rl_accel_loop(fdr_plan* p, int n, int rows, int cols, float* const U[2], const int us[2], int first, float* fin, int fs, float* d_alphas,
                  hipStream_t s, const RlStep& step, float** result) {
    if (d_alphas && n > 0) FDR_HIP(hipMemsetAsync(d_alphas, 0, (size_t)(n < 2 ? n : 2) * sizeof(float), s));  // alpha_0 = alpha_1 = 0
    if (result) *result = U[first & 1];
    return rl_accel_steps(p, 0, n, n, rows, cols, U, us, first, fin, fs, d_alphas, s, step, result);
}

int rl_accel_steps(fdr_plan* p, int k0, int k1, int n, int rows, int cols, float* const U[2], const int us[2], int first, float* fin, int fs,
                   float* d_alphas, hipStream_t s, const RlStep& step, float** result) {
    float *Y = p->ra_y, *G = p->ra_g;
    const int n_part = rlaccel_partials(rows, cols);
    for (int k = k0; k < k1; ++k) {
        const int ic = (first + k) & 1, ip = ic ^ 1;
        const bool last = k == n - 1;
        const float* y = U[ic];
        int ys = us[ic];
        if (k >= 2) {  // u_(k-1) lies in U[ip]: read here, then overwritten by the step
            ScopedPass t(p, s, kPassRaExtrapolate);
            FDR_HIP(launch_rlaccel_extrapolate(U[ic], us[ic], U[ip], us[ip], p->ra_alpha, Y, cols, rows, cols, s));
            y = Y;
            ys = cols;
        }
        float* out = last && fin ? fin : U[ip];
        const int os = last && fin ? fs : us[ip];
        const int rc = step(y, ys, out, os);
        if (rc != FDR_OK) return rc;
        if (result) *result = out;
        if (last || n <= 2) continue;
        ScopedPass t(p, s, kPassRaDirection);
        FDR_HIP(launch_rlaccel_direction(out, os, y, ys, G, cols, rows, cols, k >= 1 ? p->ra_part : nullptr, s));
        if (k >= 1)
            FDR_HIP(launch_rlaccel_alpha(p->ra_part, n_part, FDR_RL_ACCEL_MAX, p->ra_alpha, d_alphas ? d_alphas + k + 1 : nullptr, s));
    }
    return FDR_OK;
}

}  // namespace fdr
