// fdr_api_reg.hip -- choosing the regularisation weight from the picture (kernels in fdr_reg.hip): the noise estimate
// (fdr_noise_sigma_f32*), the residual / trace curve (fdr_reg_curve_f32*) and the search by the discrepancy principle or by
// generalised cross-validation (fdr_choose_reg_f32*).  The picture's spectrum comes from pass A of fdr_api_operator.hip, unchanged;
// the power pass and the sweeps read the operator tables and write the workspace of this file alone.
#include "fdr_host.hpp"

#include <cmath>
#include <limits>

using namespace fdr;

namespace {

// names are static strings compared by pointer in PassTimer::pass_id
const char* const kPassRegNoise = "R noise: sum |d * n|";
const char* const kPassRegPower = "R cols: FFT -> |G|^2/MN";
const char* const kPassRegSweep = "R sweep: rho, trace";

constexpr int kRegMinNoise = 3;  // the mask needs one interior pixel

// the first call of a plan: the power plane, the partials, the candidate and result arrays in one allocation
int ensure_reg_workspace(fdr_plan* p, const char* fn) {
    bool made = false;
    const int rc = ensure_workspace(p->reg.ws, fn, "workspace", 1, [p](auto& c, int) {
        layout(c, p->reg, p->ws_elems, (size_t)reg_curve_partials(p->M, p->npanels) * 2 * kRegCandidates, (size_t)kRegMaxPartials + 1, (size_t)kRegMaxCurve);
    }, &made);
    if (rc != FDR_OK || !made) return rc;
    try {
        p->reg.cand_host.assign((size_t)kRegMaxCurve * 2, 0.0);
        p->reg.res_host.assign((size_t)kRegMaxCurve * 2, 0.0);
    } catch (const std::bad_alloc&) {
        p->reg.ws.free_with(device_free);
        return fail(FDR_ERR_ALLOC, std::string(fn) + ": out of host memory");
    }
    return FDR_OK;
}

// workspace and Laplacian table (both synchronous, first call only)
int reg_prepare(fdr_plan* p, const char* fn) {
    int rc = ensure_reg_workspace(p, fn);
    if (rc == FDR_OK) rc = ensure_lap_table(p);
    return rc;
}

}  // namespace

namespace fdr {

double sigma_of_sum(double S, int rows, int cols) {
    const double pi = 3.14159265358979323846;
    return std::sqrt(pi / 2.0) * S / (6.0 * (double)(rows - 2) * (double)(cols - 2));
}

// the Immerkaer sum of a device window through `part` (reg_noise_partials + 1 doubles), read back: synchronous
int noise_sigma_dev(const float* d_img, int rows, int cols, int stride, double* part, double* sigma, hipStream_t s) {
    FDR_HIP(launch_reg_noise(d_img, rows, cols, stride, part, s));
    double S = 0.0;
    FDR_HIP(hipMemcpyAsync(&S, part + reg_noise_partials(rows, cols), sizeof(double), hipMemcpyDeviceToHost, s));
    FDR_HIP(hipStreamSynchronize(s));
    *sigma = sigma_of_sum(S, rows, cols);
    return FDR_OK;
}

int noise_window_check(const char* fn, int rows, int cols, int stride) {
    if (rows < kRegMinNoise || cols < kRegMinNoise || stride < cols)
        return fail(FDR_ERR_ARG, std::string(fn) + ": the noise estimate needs a window of at least 3 x 3 and stride >= cols");
    return FDR_OK;
}

}  // namespace fdr

namespace {

// pass A and the power pass: P of the window into reg.power
int reg_power_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, hipStream_t s) {
    const int rc = op_rows_fwd(p, d_img, rows, cols, stride, s);
    if (rc != FDR_OK) return rc;
    ScopedPass t(p, s, kPassRegPower);
    ColArgs ca = panel_col_args(p);
    ca.data = p->slots[0].work;
    ca.nvalid = (rows + 3) & ~3;  // <= M (M is a multiple of 8 on this path): the rows below are zero and not read
    FDR_HIP(launch_cols_panel_power(p->logM, ca, p->reg.power, p->reg.power + p->ws_elems, p->tw_col_f, s));
    return FDR_OK;
}

// rho and trace of the n pairs in reg.cand_host into reg.res_host (pairs (rho, trace)); synchronous.  The pairs up to the next
// multiple of kRegCandidates are zero: the last sweep evaluates and drops them.
int reg_eval(fdr_plan* p, int n, hipStream_t s) {
    const int padded = (n + kRegCandidates - 1) / kRegCandidates * kRegCandidates;
    for (int k = 2 * n; k < 2 * padded; ++k) p->reg.cand_host[k] = 0.0;
    FDR_HIP(hipMemcpyAsync(p->reg.cand, p->reg.cand_host.data(), (size_t)padded * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    for (int at = 0; at < n; at += kRegCandidates) {
        ScopedPass t(p, s, kPassRegSweep);
        const int nc = n - at < kRegCandidates ? n - at : kRegCandidates;
        FDR_HIP(launch_reg_curve(p->op_h, p->reg.power, p->reg.power + p->ws_elems, p->lap, p->reg.cand + 2 * at, nc, p->M, p->N, p->pstride,
                                 p->npanels, p->reg.part, p->reg.res + 2 * at, s));
    }
    FDR_HIP(hipMemcpyAsync(p->reg.res_host.data(), p->reg.res, (size_t)n * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    FDR_HIP(hipStreamSynchronize(s));
    return FDR_OK;
}

bool weight_ok(double v) { return std::isfinite(v) && v >= 0.0; }

int curve_check(const fdr_plan* p, const char* fn, int rows, int cols, int stride, const double* K, const double* gamma, int n) {
    const int rc = check_window(p, fn, NEED_OPERATOR_PSF, rows, cols, stride, cols);
    if (rc != FDR_OK) return rc;
    if (n < 1 || n > kRegMaxCurve) return fail(FDR_ERR_ARG, std::string(fn) + ": n must be in 1 .. 4096");
    for (int i = 0; i < n; ++i)
        if (!weight_ok(K[i]) || !weight_ok(gamma[i])) return fail(FDR_ERR_ARG, std::string(fn) + ": K and gamma must be finite and >= 0");
    return FDR_OK;
}

int curve_dev_impl(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const double* K, const double* gamma, int n,
                   double* residual, double* trace, hipStream_t s) {
    int rc = reg_power_dev(p, d_img, rows, cols, stride, s);
    if (rc != FDR_OK) return rc;
    for (int i = 0; i < n; ++i) { p->reg.cand_host[2 * i] = K[i]; p->reg.cand_host[2 * i + 1] = gamma[i]; }
    rc = reg_eval(p, n, s);
    if (rc != FDR_OK) return rc;
    for (int i = 0; i < n; ++i) { residual[i] = p->reg.res_host[2 * i]; trace[i] = p->reg.res_host[2 * i + 1]; }
    return FDR_OK;
}

// the search arguments with their defaults, after the plan and window checks
struct RegArgs { int method, param, n, refine; double fixed, sigma, tau, lo, hi; bool estimate; };
int reg_args(const fdr_plan* p, const char* fn, int rows, int cols, int stride, const fdr_reg_params* prm, RegArgs* a) {
    const int rc = check_window(p, fn, NEED_OPERATOR_PSF, rows, cols, stride, cols);
    if (rc != FDR_OK) return rc;
    if (prm->method != FDR_REG_DISCREPANCY && prm->method != FDR_REG_GCV) return fail(FDR_ERR_ARG, std::string(fn) + ": unknown method");
    if (prm->param != FDR_REG_PARAM_K && prm->param != FDR_REG_PARAM_GAMMA) return fail(FDR_ERR_ARG, std::string(fn) + ": unknown param");
    if (!weight_ok(prm->fixed)) return fail(FDR_ERR_ARG, std::string(fn) + ": the fixed weight must be finite and >= 0");
    if (!weight_ok(prm->sigma) || !weight_ok(prm->tau)) return fail(FDR_ERR_ARG, std::string(fn) + ": sigma and tau must be finite and >= 0");
    a->method = prm->method; a->param = prm->param;
    a->fixed = prm->fixed; a->sigma = prm->sigma; a->tau = prm->tau != 0.f ? (double)prm->tau : 1.0;
    a->lo = prm->lo; a->hi = prm->hi;
    if (prm->lo == 0.0 && prm->hi == 0.0) { a->lo = 1e-8; a->hi = 1e2; }
    if (!std::isfinite(a->lo) || !std::isfinite(a->hi) || !(a->lo > 0.0) || !(a->lo < a->hi))
        return fail(FDR_ERR_ARG, std::string(fn) + ": the range needs 0 < lo < hi, both finite");
    a->n = prm->n_grid ? prm->n_grid : 32;
    if (a->n < 4 || a->n > 64) return fail(FDR_ERR_ARG, std::string(fn) + ": n_grid must be in 4 .. 64");
    a->refine = prm->refine == -1 ? 2 : prm->refine;
    if (a->refine < 0 || a->refine > 8) return fail(FDR_ERR_ARG, std::string(fn) + ": refine must be in 0 .. 8");
    a->estimate = a->method == FDR_REG_DISCREPANCY && a->sigma == 0.0;
    if (a->estimate) return noise_window_check(fn, rows, cols, stride);
    return FDR_OK;
}

// v[i] = a (b / a)^(i / (n - 1)); the ends are a and b themselves
void log_grid(double a, double b, int n, std::vector<double>& v) {
    v.resize(n);
    for (int i = 1; i < n - 1; ++i) v[i] = a * std::pow(b / a, (double)i / (double)(n - 1));
    v[0] = a; v[n - 1] = b;
}

double gcv_of(double rho, double trace, double mn) { return trace > 0.0 ? mn * rho / (trace * trace) : std::numeric_limits<double>::infinity(); }

// the whole search on `s`, synchronous
int choose_dev_impl(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const RegArgs& a, fdr_reg_choice* out, hipStream_t s) {
    const double mn = (double)p->M * (double)p->N;
    double sigma = a.sigma;
    int rc = FDR_OK;
    if (a.estimate) {
        ScopedPass t(p, s, kPassRegNoise);
        rc = noise_sigma_dev(d_img, rows, cols, stride, p->reg.noise, &sigma, s);
        if (rc != FDR_OK) return rc;
    }
    rc = reg_power_dev(p, d_img, rows, cols, stride, s);
    if (rc != FDR_OK) return rc;
    const int n = a.n;
    std::vector<double> v;
    int evaluations = 0;
    auto sweep = [&](double lo, double hi) {
        log_grid(lo, hi, n, v);
        for (int i = 0; i < n; ++i) {
            p->reg.cand_host[2 * i] = a.param == FDR_REG_PARAM_K ? v[i] : a.fixed;
            p->reg.cand_host[2 * i + 1] = a.param == FDR_REG_PARAM_K ? a.fixed : v[i];
        }
        evaluations += n;
        return reg_eval(p, n, s);
    };
    const double* res = p->reg.res_host.data();  // (rho, trace) of candidate i at 2 i
    auto finish = [&](double value, int nearest, int flags) {
        const double rho = res[2 * nearest], tr = res[2 * nearest + 1];
        *out = fdr_reg_choice{value, sigma, rho, tr, gcv_of(rho, tr, mn), flags, evaluations};
        return FDR_OK;
    };
    rc = sweep(a.lo, a.hi);
    if (rc != FDR_OK) return rc;
    if (a.method == FDR_REG_DISCREPANCY) {
        const double T = a.tau * (double)rows * (double)cols * sigma * sigma;
        if (!(res[2 * (n - 1)] > 0.0)) return finish(a.hi, n - 1, FDR_REG_AT_HIGH);  // an all-zero window
        if (res[0] >= T) return finish(a.lo, 0, FDR_REG_AT_LOW);
        if (res[2 * (n - 1)] < T) return finish(a.hi, n - 1, FDR_REG_AT_HIGH);
        int i = 1;
        for (int round = 0;; ++round) {
            i = 1;
            while (i < n - 1 && res[2 * i] < T) ++i;  // the first candidate at or above the target; the ends bracket it
            if (round == a.refine) break;
            rc = sweep(v[i - 1], v[i]);
            if (rc != FDR_OK) return rc;
        }
        const double va = v[i - 1], vb = v[i], ra = res[2 * (i - 1)], rb = res[2 * i];
        double value = vb;
        const double dr = ra > 0.0 ? std::log(rb) - std::log(ra) : 0.0;
        if (dr > 0.0) {  // (a bracket refined down to neighbouring doubles has dr = 0: its upper end)
            const double la = std::log(va), lb = std::log(vb);
            double f = (std::log(T) - std::log(ra)) / dr;
            f = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
            value = std::exp(la + f * (lb - la));
            value = value < va ? va : (value > vb ? vb : value);
        }
        const bool low = std::log(value) - std::log(va) <= std::log(vb) - std::log(value);
        return finish(value, low ? i - 1 : i, 0);
    }
    int i = 0;
    for (int round = 0;; ++round) {
        i = 0;
        for (int k = 1; k < n; ++k)
            if (gcv_of(res[2 * k], res[2 * k + 1], mn) < gcv_of(res[2 * i], res[2 * i + 1], mn)) i = k;  // strict: the lowest index on ties
        if (round == a.refine) break;
        const double lo = v[i > 0 ? i - 1 : 0], hi = v[i < n - 1 ? i + 1 : n - 1];
        rc = sweep(lo, hi);
        if (rc != FDR_OK) return rc;
    }
    const double value = v[i];
    return finish(value, i, value == a.lo ? FDR_REG_AT_LOW : (value == a.hi ? FDR_REG_AT_HIGH : 0));
}

}  // namespace

extern "C" {

int fdr_noise_sigma_f32_dev(int device, const float* d_img, int rows, int cols, int stride, double* sigma, void* stream) {
    const char* fn = "fdr_noise_sigma_f32_dev";
    if (!d_img || !sigma) return null_arg(fn);
    const int rc = noise_window_check(fn, rows, cols, stride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(device));
    DeviceBuffer part;
    FDR_ALLOC(part, ((size_t)reg_noise_partials(rows, cols) + 1) * sizeof(double), fn);
    return noise_sigma_dev(d_img, rows, cols, stride, part.as<double>(), sigma, (hipStream_t)stream);
}

int fdr_noise_sigma_f32(int device, const float* img_host, int rows, int cols, int stride, double* sigma) {
    const char* fn = "fdr_noise_sigma_f32";
    if (!img_host || !sigma) return null_arg(fn);
    const int rc = noise_window_check(fn, rows, cols, stride);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(device));
    DeviceBuffer img, part;
    FDR_ALLOC(img, (size_t)rows * cols * sizeof(float), fn);
    FDR_ALLOC(part, ((size_t)reg_noise_partials(rows, cols) + 1) * sizeof(double), fn);
    FDR_HIP(hipMemcpy2D(img.ptr, (size_t)cols * sizeof(float), img_host, (size_t)stride * sizeof(float), (size_t)cols * sizeof(float), rows,
                        hipMemcpyHostToDevice));
    return noise_sigma_dev(img.as<float>(), rows, cols, cols, part.as<double>(), sigma, nullptr);
}

int fdr_reg_curve_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const double* K, const double* gamma, int n,
                          double* residual, double* trace, void* stream) {
    const char* fn = "fdr_reg_curve_f32_dev";
    if (!p || !d_img || !K || !gamma || !residual || !trace) return null_arg(fn);
    int rc = curve_check(p, fn, rows, cols, stride, K, gamma, n);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = reg_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    ScopedPhase ph(p, FDR_PHASE_COMPUTE, (hipStream_t)stream);
    return curve_dev_impl(p, d_img, rows, cols, stride, K, gamma, n, residual, trace, (hipStream_t)stream);
}

int fdr_reg_curve_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const double* K, const double* gamma, int n,
                      double* residual, double* trace) {
    const char* fn = "fdr_reg_curve_f32";
    if (!p || !img_host || !K || !gamma || !residual || !trace) return null_arg(fn);
    int rc = curve_check(p, fn, rows, cols, stride, K, gamma, n);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = reg_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    return host_image_call(p, fn, img_host, rows, cols, stride, nullptr, 0, 0, 0, [&](const float* d_in, float*) {
        return curve_dev_impl(p, d_in, rows, cols, cols, K, gamma, n, residual, trace, nullptr);
    });
}

int fdr_choose_reg_f32_dev(fdr_plan* p, const float* d_img, int rows, int cols, int stride, const fdr_reg_params* params,
                           fdr_reg_choice* choice, void* stream) {
    const char* fn = "fdr_choose_reg_f32_dev";
    if (!p || !d_img || !params || !choice) return null_arg(fn);
    RegArgs a{};
    int rc = reg_args(p, fn, rows, cols, stride, params, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = reg_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    ScopedPhase ph(p, FDR_PHASE_COMPUTE, (hipStream_t)stream);
    return choose_dev_impl(p, d_img, rows, cols, stride, a, choice, (hipStream_t)stream);
}

int fdr_choose_reg_f32(fdr_plan* p, const float* img_host, int rows, int cols, int stride, const fdr_reg_params* params,
                       fdr_reg_choice* choice) {
    const char* fn = "fdr_choose_reg_f32";
    if (!p || !img_host || !params || !choice) return null_arg(fn);
    RegArgs a{};
    int rc = reg_args(p, fn, rows, cols, stride, params, &a);
    if (rc != FDR_OK) return rc;
    FDR_HIP(hipSetDevice(p->device));
    rc = reg_prepare(p, fn);
    if (rc != FDR_OK) return rc;
    return host_image_call(p, fn, img_host, rows, cols, stride, nullptr, 0, 0, 0, [&](const float* d_in, float*) {
        return choose_dev_impl(p, d_in, rows, cols, cols, a, choice, nullptr);
    });
}

}  // extern "C"
