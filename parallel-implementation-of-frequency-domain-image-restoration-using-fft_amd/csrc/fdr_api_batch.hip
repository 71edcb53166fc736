// fdr_api_batch.hip -- fdr_batch_run, the multi-GPU batched mode for C / C++ callers: one host thread, one plan, one PSF
// spectrum per device entry; the workers and their start gate, and the RCCL broadcast of a shared filter.
#include "fdr_host.hpp"

#include <dlfcn.h>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>

using namespace fdr;

namespace {

struct BatchWorker {
    int index = 0, device = 0, first = 0, count = 0;
    int status = FDR_OK;
    std::string error;
    double elapsed_ms = 0.0, checksum = 0.0;
    std::chrono::steady_clock::time_point t_end;
};

// `prepared`: a plan that already holds its filter (fdr_batch_desc::bcast_filter: created and filled by the calling thread,
// which has synchronised the device); the worker owns it from here on.  nullptr: the worker builds plan and filter itself.
// Start line of fdr_batch_run's workers: set-up (plan, PSF spectrum, synthesis, warm-up) differs from device to device, so
// every worker waits here until all of them are ready and the timed regions start together; `wall_ms` then spans the work
// itself, not the set-up skew.  A worker that fails before the line still arrives (without waiting), so nobody waits for it.
struct StartGate {
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0, total = 0;
    explicit StartGate(int n) : total(n) {}
    void arrive(bool wait) {
        std::unique_lock<std::mutex> lk(m);
        if (++arrived >= total) { cv.notify_all(); return; }
        if (wait) cv.wait(lk, [&] { return arrived >= total; });
    }
};

int batch_worker_run(const fdr_batch_desc* d, BatchWorker* w, std::chrono::steady_clock::time_point* t_start_out, fdr_plan* prepared, StartGate* gate) {
    fdr_plan* plan = prepared;
    bool at_gate = false;
    auto start_line = [&] { at_gate = true; gate->arrive(true); };
    float *d_in = nullptr, *d_out = nullptr;
    double* d_part = nullptr;
    hipStream_t stream = nullptr;
    int rc = FDR_OK;
    auto body = [&]() -> int {
        if (w->count == 0) return FDR_OK;
        int r = FDR_OK;
        if (!plan) {
            r = fdr_plan_create(w->device, d->M, d->N, d->mode, d->flags, &plan);
            if (r != FDR_OK) return r;
        }
        // the worker's stream exists BEFORE the PSF spectrum is queued, and the generated PSF is prepared ON it: the batches
        // below run on this (non-blocking) stream and its forks, which never synchronise with the null stream by themselves
        // (fdr_set_psf with a host PSF synchronises before it returns)
        FDR_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (!prepared) {
            if (d->psf_host) r = fdr_set_psf(plan, d->psf_host, d->psf_rows, d->psf_cols, d->psf_stride, d->K);
            else r = fdr_set_psf_motion(plan, d->psf_size, d->psf_angle_deg, d->K, stream);
        }
        if (r != FDR_OK) return r;
        if (d->imgs_host) {  // host images: the pipelined host batch over this worker's shard
            FDR_HIP(hipStreamSynchronize(stream));  // (the PSF spectrum is part of the set-up)
            start_line();
            const auto t0 = std::chrono::steady_clock::now();
            *t_start_out = t0;
            r = fdr_wiener_batch_ptrs_f32(plan, d->imgs_host + w->first, d->outs_host + w->first, w->count, d->rows, d->cols, d->stride,
                                          d->out_stride, d->norm_area);
            w->t_end = std::chrono::steady_clock::now();
            w->elapsed_ms = std::chrono::duration<double, std::milli>(w->t_end - t0).count();
            if (r != FDR_OK) return r;
            double acc = 0.0;
            for (int i = 0; i < w->count; ++i)
                for (int y = 0; y < d->rows; ++y) {
                    const float* row = d->outs_host[w->first + i] + (size_t)y * d->out_stride;
                    for (int x = 0; x < d->cols; ++x) acc += (double)row[x];
                }
            w->checksum = acc;
            return FDR_OK;
        }
        // synthetic, device resident
        // defaults as bench.py's: 2 streams; 8 images per launch up to 1024^2, 4 up to 4096^2, larger 2
        const size_t px = (size_t)d->M * (size_t)d->N;
        const int ns = d->nstreams > 0 ? d->nstreams : (d->mode == FDR_MODE_FAST ? 2 : 3);
        const int gr = d->group > 0 ? d->group : (px <= (size_t)1024 * 1024 ? 8 : (px <= (size_t)4096 * 4096 ? 4 : 2));
        r = fdr_plan_set_batching(plan, ns, d->mode == FDR_MODE_FAST ? gr : 1);
        if (r != FDR_OK) return r;
        const size_t P = (size_t)d->rows * d->cols, total = P * (size_t)w->count;
        FDR_HIP(hipMalloc((void**)&d_in, total * sizeof(float)));
        FDR_HIP(hipMalloc((void**)&d_out, total * sizeof(float)));
        FDR_HIP(hipMalloc((void**)&d_part, kChecksumParts * sizeof(double)));
        FDR_HIP(launch_synth(d->synth_seed, (uint64_t)w->first * P, total, d_in, stream));
        for (int k = 0; k < d->warmup && r == FDR_OK; ++k)
            r = fdr_wiener_batch_f32_dev(plan, d_in, P, w->count, d->rows, d->cols, d->cols, d_out, P, d->cols, d->norm_area, stream);
        FDR_HIP(hipStreamSynchronize(stream));
        if (r != FDR_OK) return r;
        start_line();
        const auto t0 = std::chrono::steady_clock::now();
        *t_start_out = t0;
        for (int k = 0; k < d->steps && r == FDR_OK; ++k)
            r = fdr_wiener_batch_f32_dev(plan, d_in, P, w->count, d->rows, d->cols, d->cols, d_out, P, d->cols, d->norm_area, stream);
        FDR_HIP(hipStreamSynchronize(stream));
        w->t_end = std::chrono::steady_clock::now();
        w->elapsed_ms = std::chrono::duration<double, std::milli>(w->t_end - t0).count();
        if (r != FDR_OK) return r;
        FDR_HIP(launch_checksum(d_out, total, d_part, stream));
        std::vector<double> part(kChecksumParts);
        FDR_HIP(hipMemcpyAsync(part.data(), d_part, kChecksumParts * sizeof(double), hipMemcpyDeviceToHost, stream));
        FDR_HIP(hipStreamSynchronize(stream));
        double acc = 0.0;
        for (double v : part) acc += v;
        w->checksum = acc;
        return FDR_OK;
    };
    if (hipSetDevice(w->device) != hipSuccess) rc = fail(FDR_ERR_HIP, "fdr_batch_run: hipSetDevice failed");
    else rc = body();
    if (!at_gate) gate->arrive(false);  // no images, or failed during set-up: count as arrived, do not hold the others up
    if (rc != FDR_OK) w->error = g_last_error;  // thread-local: hand it to the calling thread
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_part);
    if (stream) (void)hipStreamDestroy(stream);
    fdr_plan_destroy(plan);
    w->status = rc;
    return rc;
}

// RCCL, resolved at run time (no link-time dependency: a process that never broadcasts a filter never loads it, and inside
// a PyTorch process the copy of the library that torch has already mapped is the one that answers)
struct Rccl {
    typedef void* comm_t;
    int (*CommInitAll)(comm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(comm_t) = nullptr;
    int (*GroupStart)(void) = nullptr;
    int (*GroupEnd)(void) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, comm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
    Rccl() {
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) != nullptr) break;
        if (!h) return;
        *(void**)&CommInitAll = dlsym(h, "ncclCommInitAll");
        *(void**)&CommDestroy = dlsym(h, "ncclCommDestroy");
        *(void**)&GroupStart = dlsym(h, "ncclGroupStart");
        *(void**)&GroupEnd = dlsym(h, "ncclGroupEnd");
        *(void**)&Broadcast = dlsym(h, "ncclBroadcast");
        *(void**)&GetErrorString = dlsym(h, "ncclGetErrorString");
        ok = CommInitAll && CommDestroy && GroupStart && GroupEnd && Broadcast;
    }
};

// fdr_batch_desc::bcast_filter: plans[0] holds the filter; every other plan gets its bytes.  Distinct devices: ONE
// ncclBroadcast over a communicator of all of them (RCCL over xGMI: the MPI_Bcast of fft/fft_mpi.cpp:334-378); an ordinal
// that repeats (two workers on one device -- RCCL refuses that) or a missing RCCL: device-to-device / peer copies.
// Returns the path taken (FDR_FILTER_*) or a negative status.
int distribute_filter(const std::vector<fdr_plan*>& plans, float K, bool force_rccl) {
    const int G = (int)plans.size();
    const size_t bytes = plans[0]->ws_elems * sizeof(float2);
    bool distinct = true;
    for (int a = 0; a < G; ++a)
        for (int b = a + 1; b < G; ++b) distinct = distinct && plans[a]->device != plans[b]->device;
    int path = FDR_FILTER_PEER_COPY;
    static Rccl rccl;  // (thread-safe initialisation; loaded on first use)
    if (distinct && (G > 1 || force_rccl) && rccl.ok) {
        std::vector<int> devs(G);
        for (int g = 0; g < G; ++g) devs[g] = plans[g]->device;
        std::vector<Rccl::comm_t> comms(G, nullptr);
        int nr = rccl.CommInitAll(comms.data(), G, devs.data());
        if (nr == 0) {
            nr = rccl.GroupStart();
            for (int g = 0; g < G && nr == 0; ++g) {
                if (hipSetDevice(devs[g]) != hipSuccess) { nr = -1; break; }
                nr = rccl.Broadcast(plans[g]->filt, plans[g]->filt, bytes, 0 /* ncclChar */, 0, comms[g], nullptr);
            }
            const int ne = rccl.GroupEnd();
            if (nr == 0) nr = ne;
            for (int g = 0; g < G; ++g)
                if (hipSetDevice(devs[g]) == hipSuccess && hipDeviceSynchronize() != hipSuccess && nr == 0) nr = -1;
            for (int g = 0; g < G; ++g)
                if (comms[g]) (void)rccl.CommDestroy(comms[g]);
        }
        if (nr == 0) path = FDR_FILTER_RCCL_BROADCAST;
        else  // the G > 1 RCCL path has not met multi-GPU hardware yet: an error there must not cost the batch
            std::fprintf(stderr, "fdr_batch_run: RCCL broadcast of the filter failed (%s); falling back to peer copies\n",
                         rccl.GetErrorString && nr > 0 ? rccl.GetErrorString(nr) : "error");
    }
    if (path != FDR_FILTER_RCCL_BROADCAST) {
        for (int g = 1; g < G; ++g) {
            FDR_HIP(hipSetDevice(plans[g]->device));
            if (plans[g]->device == plans[0]->device) FDR_HIP(hipMemcpy(plans[g]->filt, plans[0]->filt, bytes, hipMemcpyDeviceToDevice));
            else FDR_HIP(hipMemcpyPeer(plans[g]->filt, plans[g]->device, plans[0]->filt, plans[0]->device, bytes));
        }
    }
    for (int g = 1; g < G; ++g) { plans[g]->K = K; plans[g]->have_psf = true; }
    return path;
}

}  // namespace

extern "C" int fdr_batch_run(const fdr_batch_desc* d, fdr_batch_stats* st) {
    if (!d) return fail(FDR_ERR_ARG, "fdr_batch_run: null descriptor");
    if (d->n_devices < 1 || d->n_devices > FDR_BATCH_MAX_DEVICES || !d->devices)
        return fail(FDR_ERR_ARG, "fdr_batch_run: need 1..16 device entries");
    if (d->count < 0 || d->rows <= 0 || d->cols <= 0 || d->rows > d->M || d->cols > d->N)
        return fail(FDR_ERR_ARG, "fdr_batch_run: bad batch shape");
    if (d->imgs_host && (!d->outs_host || d->stride < d->cols || d->out_stride < d->cols))
        return fail(FDR_ERR_ARG, "fdr_batch_run: host images need outs_host and strides >= cols");
    if (!d->imgs_host && d->steps < 1) return fail(FDR_ERR_ARG, "fdr_batch_run: synthetic run needs steps >= 1");
    if (!d->psf_host && d->psf_size <= 0) return fail(FDR_ERR_ARG, "fdr_batch_run: no PSF given");
    int ndev = 0;
    FDR_HIP(hipGetDeviceCount(&ndev));
    for (int g = 0; g < d->n_devices; ++g)
        if (d->devices[g] < 0 || d->devices[g] >= ndev) return fail(FDR_ERR_ARG, "fdr_batch_run: device ordinal out of range");
    const int G = d->n_devices;
    std::vector<BatchWorker> ws((size_t)G);
    std::vector<std::chrono::steady_clock::time_point> starts((size_t)G);
    // fft/fft_mpi.cpp:89-100 applied to images: floor(count / G) each, the first count % G workers one more
    for (int g = 0, first = 0; g < G; ++g) {
        ws[g].index = g; ws[g].device = d->devices[g];
        ws[g].count = d->count / G + (g < d->count % G ? 1 : 0);
        ws[g].first = first;
        first += ws[g].count;
    }
    // bcast_filter: worker 0's filter for everyone -- plans created and the filter distributed here, before the workers start
    std::vector<fdr_plan*> prepared((size_t)G, nullptr);
    int filter_path = FDR_FILTER_LOCAL;
    if (d->bcast_filter && (G > 1 || d->bcast_filter == 2) && d->count >= G) {  // (every worker has at least one image, so every plan is used)
        int prc = FDR_OK;
        for (int g = 0; g < G && prc == FDR_OK; ++g) prc = fdr_plan_create(ws[g].device, d->M, d->N, d->mode, d->flags, &prepared[g]);
        if (prc == FDR_OK) {
            if (d->psf_host) prc = fdr_set_psf(prepared[0], d->psf_host, d->psf_rows, d->psf_cols, d->psf_stride, d->K);
            else prc = fdr_set_psf_motion(prepared[0], d->psf_size, d->psf_angle_deg, d->K, nullptr);
        }
        if (prc == FDR_OK && (hipSetDevice(prepared[0]->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
            prc = fail(FDR_ERR_HIP, "fdr_batch_run: preparing the filter on worker 0's device failed");
        if (prc == FDR_OK) { filter_path = distribute_filter(prepared, d->K, d->bcast_filter == 2); if (filter_path < 0) prc = filter_path; }
        if (prc != FDR_OK) {
            const std::string msg0 = g_last_error;
            for (auto* pl : prepared) fdr_plan_destroy(pl);
            return fail(prc, "fdr_batch_run: " + msg0);
        }
    }
    const auto t_launch = std::chrono::steady_clock::now();
    for (int g = 0; g < G; ++g) { starts[g] = t_launch; ws[g].t_end = t_launch; }
    std::vector<std::thread> threads;
    StartGate gate(G);
    for (int g = 1; g < G; ++g) threads.emplace_back(batch_worker_run, d, &ws[g], &starts[g], prepared[g], &gate);
    batch_worker_run(d, &ws[0], &starts[0], prepared[0], &gate);  // worker 0 on the calling thread
    for (auto& t : threads) t.join();
    int rc = FDR_OK;
    std::string msg;
    auto t_first = starts[0], t_last = ws[0].t_end;
    bool any = false;
    long long done = 0;
    for (int g = 0; g < G; ++g) {
        if (ws[g].status != FDR_OK && rc == FDR_OK) { rc = ws[g].status; msg = "worker " + std::to_string(g) + " (device " + std::to_string(ws[g].device) + "): " + ws[g].error; }
        if (ws[g].count > 0 && ws[g].status == FDR_OK) {
            if (!any || starts[g] < t_first) t_first = starts[g];
            if (!any || ws[g].t_end > t_last) t_last = ws[g].t_end;
            any = true;
            done += (long long)ws[g].count * (d->imgs_host ? 1 : d->steps);
        }
    }
    if (st) {
        memset(st, 0, sizeof *st);
        st->n_devices = G;
        for (int g = 0; g < G; ++g) {
            st->first[g] = ws[g].first; st->images[g] = ws[g].count; st->elapsed_ms[g] = ws[g].elapsed_ms;
            st->checksum[g] = ws[g].checksum; st->status[g] = ws[g].status;
        }
        st->wall_ms = any ? std::chrono::duration<double, std::milli>(t_last - t_first).count() : 0.0;
        st->images_done = done;
        st->mpixels_per_s = st->wall_ms > 0.0 ? (double)done * d->rows * d->cols / 1e6 / (st->wall_ms * 1e-3) : 0.0;
        st->filter_path = filter_path;
    }
    if (rc != FDR_OK) return fail(rc, "fdr_batch_run: " + msg);
    return FDR_OK;
}
