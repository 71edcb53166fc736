// fdr_panel_cols.hip -- the column kernels of the fast panel path (layout: fdr_panel.hpp): the PSF column pass (COL_FWD_FILTER)
// and pass B' (COL_FUSED: column FFTs . W . column IFFTs, in place) as the persistent, the 16-value and the split kernel.
#include "fdr_panel.hpp"

namespace fdr {

// forward column FFT of every panel, in place, for the fast path's PSF preparation: only the first
// `nvalid` rows of a panel hold data -- the row pass before it transformed just the row groups the PSF reaches, everything
// below is taken as zero without being read -- and the spectrum leaves as W = conj(H) / (|H|^2 + K) directly; the packed
// DC / Nyquist column (column 0 of panel 0, half spectrum) leaves as its filter slots (packed_column_filter_slot).
// Against the separate row pass over all M rows + column pass + make_filter pass this drops 20 of 24 bytes per pixel.
template <int LOGM>
__global__ __launch_bounds__(PanelGeom<LOGM>::THREADS, PanelGeom<LOGM>::WAVES_PER_SIMD) void fft_cols_panel_fwd_filter_kernel(
    float2* __restrict__ data, const float2* __restrict__ tw_fwd, const size_t pstride, const int npanels, const int nvalid, const float K,
    const int packed0) {
    using St = Steps<LOGM>;
    using Geo = PanelGeom<LOGM>;
    constexpr int G = Geo::G, T = St::T;
    using Core = FftCore<LOGM, 4, 2, PolicyFast>;
    __shared__ float2 lds[G * 2 * St::BUF];
    const int g = threadIdx.x >> St::LOGT, tid = threadIdx.x & (T - 1);
    const int p = blockIdx.x * G + g;
    const bool active = p < npanels;
    float2* pbase = data + (size_t)(active ? p : 0) * pstride;
    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);
    float2 v[4][8];
    FDR_PANEL_LOAD_VALID(Core, pbase, tid, nvalid, v)
    Core::template run<0, false>(v, lds + g * 2 * St::BUF, tw_fwd, bases, tid);
    const bool raw0 = packed0 && p == 0;  // uniform per thread group
    if (packed0 && blockIdx.x == 0) {     // uniform per workgroup: the packed column's slots need C[k] and C[M - k]
        float2* buf = lds + g * 2 * St::BUF;
        __syncthreads();  // the transform's last exchange has been read by every wave
        FDR_JITTER(4021);
        if (raw0) {
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) buf[Core::out_index(tid, u, q)] = v[0][u * Core::RHOL + q];
        }
        __syncthreads();
        FDR_JITTER(4022);
        if (raw0) {
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) {
                    const int s = u * Core::RHOL + q, k = Core::out_index(tid, u, q);
                    v[0][s] = packed_column_filter_slot(v[0][s], buf[(St::L - k) & (St::L - 1)], k, St::L, K);
                }
        }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if (!raw0) v[0][s] = wiener_filter_fast(v[0][s], K);
        v[1][s] = wiener_filter_fast(v[1][s], K);
        v[2][s] = wiener_filter_fast(v[2][s], K);
        v[3][s] = wiener_filter_fast(v[3][s], K);
    }
    if (active) panel_store_out<Core>(pbase, tid, v);
}

// One panel of pass B' on register set `cur` (spectrum, first-step order) with the filter in `flt`
// (last-step order): forward, multiply, then -- `flt` now free -- queue the NEXT panel's spectrum
// into it, inverse, store, and queue the next panel's filter into `cur`.
// Packed column (half-spectrum mode, column 0 of panel 0): the column carries c[m] = X[m,0] + i X[m,N/2] with both
// parts real, so its transform is C = F0 + i FN with F0, FN Hermitian.  Separate them with the mirrored value
// C[M-k] (one LDS round trip), filter each with its own W, and re-pack Z0 + i ZN; the inverse transform then
// returns the two filtered real columns in the real and imaginary parts.  The filter slot of this column holds
//   S[k] = W0[k] (0 < k < M/2),  S[k] = WN[M-k] (M/2 < k < M),  S[0] = (W0[0], WN[0]),  S[M/2] = (W0[M/2], WN[M/2])
// (W0 = W[.,0], WN = W[.,N/2]; both Hermitian, their values at 0 and M/2 real), built by the PSF column pass (packed_column_filter_slot).
template <int LOGM, class Core, int SEQ>
__device__ __forceinline__ void packed_column_filter(float2 (&cur)[4][8], const float2 (&flt)[4][8], float2* grp_lds, int tid,
                                                     bool apply) {
    using St = Steps<LOGM>;
    constexpr int M = St::L;
    float2* bufc = grp_lds + (SEQ & 1) * St::BUF;
    float2* bufs = grp_lds + ((SEQ + 1) & 1) * St::BUF;
    __syncthreads();  // the other buffer was read by the last exchange of the forward transform
    FDR_JITTER(4001);
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) {
            const int k = Core::out_index(tid, u, q);
            bufc[k] = cur[0][u * Core::RHOL + q];
            bufs[k] = flt[0][u * Core::RHOL + q];
        }
    __syncthreads();
    FDR_JITTER(4002);
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) {
            const int s = u * Core::RHOL + q;
            const int k = Core::out_index(tid, u, q);
            const int km = (M - k) & (M - 1);
            const float2 c = cur[0][s], cm = bufc[km], sl = flt[0][s], sm = bufs[km];
            const float2 f0 = make_float2(0.5f * (c.x + cm.x), 0.5f * (c.y - cm.y));
            const float2 fn = make_float2(0.5f * (c.y + cm.y), 0.5f * (cm.x - c.x));
            float2 w0, wn;
            if (k == 0 || k == M / 2) { w0 = make_float2(sl.x, 0.f); wn = make_float2(sl.y, 0.f); }
            else if (k < M / 2) { w0 = sl; wn = sm; }
            else { w0 = make_float2(sm.x, -sm.y); wn = make_float2(sl.x, -sl.y); }
            const float2 z0 = cmul_fma(f0, w0), zn = cmul_fma(fn, wn);
            // thread groups of this workgroup that hold other panels only came along for the barriers
            cur[0][s] = apply ? make_float2(z0.x - zn.y, z0.y + zn.x) : cmul_fma(c, sl);
        }
    __syncthreads();  // both buffers were just read: the next exchange may overwrite either
}

// Tile addressing of the persistent kernel: a wave-uniform tile base (SGPRs) plus ONE 32-bit per-lane element offset
// `loff` = (thread group's panel inside the tile) * pstride + tid * 4, so every load / store is
// `global_* v, v_off, s[base:base+1]` and no 64-bit per-lane address lives in VGPRs.  `scale` (0 or 1, uniform)
// collapses a prefetch onto the first 32 bytes of `ubase` when there is no next tile: the loads stay UNCONDITIONAL
// -- a conditional prefetch makes PHIs of (loaded, old) values whose copies hipcc places right behind the loads,
// i.e. it waits for the prefetch before the transform it was meant to hide behind (seen in the ISA as
// `vmcnt(11) .. vmcnt(1)` directly after the 16 loads).
// Pins a wave-uniform GLOBAL address in an SGPR pair.  Without it hipcc re-associates (uniform base + constant) +
// lane offset into (base + lane offset) + constant: one 64-bit VGPR address per load, kept alive for the stores of the
// same tile -- 30+ registers that end up spilled in the 128-data-register kernels.  The pointer keeps its address
// space through the asm (a generic pointer would turn every access into a flat_load).
typedef float nfloat4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) char gchar;
typedef __attribute__((address_space(1))) nfloat4 g_nfloat4;
__device__ __forceinline__ gchar* uniform_gptr(const void* p) {
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return (gchar*)(((unsigned long long)hi << 32) | lo);
}
// 32 bytes at (uniform base) + (32-bit lane byte offset): global_load_dwordx4 v, v_off, s[base:base+1] {offset:16}.
// (HIP's float4, field by field: with native vector types the two halves reach the register arrays as <2 x float>
// stores, which SROA does not promote -- the arrays then live in scratch memory.)
#define FDR_GLOAD32(ub, lane_bytes, a, b, c, d)                                                       \
    do {                                                                                              \
        const float4* p_ = reinterpret_cast<const float4*>((const char*)(ub) + (lane_bytes));         \
        const float4 x0_ = p_[0], x1_ = p_[1];                                                        \
        a = make_float2(x0_.x, x0_.y); b = make_float2(x0_.z, x0_.w);                                 \
        c = make_float2(x1_.x, x1_.y); d = make_float2(x1_.z, x1_.w);                                 \
    } while (0)
__device__ __forceinline__ void gstore32(gchar* ub, unsigned lane_bytes, float2 a, float2 b, float2 c, float2 d) {
    float4* p = reinterpret_cast<float4*>((char*)ub + lane_bytes);
    p[0] = make_float4(a.x, a.y, b.x, b.y);
    p[1] = make_float4(c.x, c.y, d.x, d.y);
}

template <class Core, bool OUT_ORDER>
__device__ __forceinline__ void tile_load(const float2* __restrict__ ubase, unsigned loff, unsigned scale, float2 (&d)[4][Core::V]) {
    constexpr int NU = OUT_ORDER ? Core::NUL : Core::NU0, RHO = OUT_ORDER ? Core::RHOL : Core::RHO0;
    constexpr int LOGQ = OUT_ORDER ? Core::LOGOUT : Core::LOGR0;
    // byte offsets in 32 bits: (uniform 64-bit base) + zext(32-bit lane offset) is the form hipcc turns into
    // `global_load_dwordx4 v, v_off, s[base:base+1]`, i.e. ONE address VGPR for the whole tile
    const unsigned lo = loff * scale * 8u;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int q = 0; q < RHO; ++q) {
            const int s = u * RHO + q;
            const unsigned uoff = (unsigned)(((q << LOGQ) + u * Core::T) * 4) * scale;  // uniform, elements
#ifdef FDR_DEBUG_SKIP_MEM  // timing-only builds: pass B' without its HBM traffic
            (void)ubase; (void)uoff;
            d[0][s] = d[1][s] = d[2][s] = d[3][s] = make_float2(__uint_as_float(lo), 1.0f);
#else
            const gchar* ub = uniform_gptr(ubase + uoff);
            FDR_GLOAD32(ub, lo, d[0][s], d[1][s], d[2][s], d[3][s]);
            // keep the two 16-byte halves of a row together in the instruction stream: left alone the scheduler issues the
            // 16 first halves of a tile, then the 16 second halves, and with every wave of an XCD doing the same (8 MB of
            // lines requested before the first second half) part of the lines has left the 4 MiB L2 again by then
            // (LAB_NOTES "pass B' tile loads")
            asm volatile("" ::: "memory");
#endif
        }
}
template <class Core>
__device__ __forceinline__ void tile_store(float2* __restrict__ ubase, unsigned loff, const float2 (&d)[4][Core::V]) {
    const unsigned lo = loff * 8u;
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) {
            const int s = u * Core::RHOL + q;
            const unsigned uoff = (unsigned)(((q << Core::LOGOUT) + u * Core::T) * 4);
#ifdef FDR_DEBUG_SKIP_MEM
            if (d[0][s].x != 1.2345e-30f) continue;
#endif
            gstore32(uniform_gptr(ubase + uoff), lo, d[0][s], d[1][s], d[2][s], d[3][s]);
        }
}

// Reads every register of a prefetched set through an empty asm, so the compiler places the wait for those loads HERE
// and treats them as landed afterwards.  Used right before the tile's stores are issued: vmcnt counts loads and
// stores in issue order, so a wait for the spectrum prefetch placed after the stores (where the values are first
// used) would also wait for the stores to drain, time that the next forward transform should hide.
__device__ __forceinline__ void landed(const float2 (&d)[4][8]) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int s = 0; s < 8; s += 4)
            asm volatile("" ::"v"(d[b][s].x), "v"(d[b][s].y), "v"(d[b][s + 1].x), "v"(d[b][s + 1].y), "v"(d[b][s + 2].x),
                         "v"(d[b][s + 2].y), "v"(d[b][s + 3].x), "v"(d[b][s + 3].y));
}

struct PanelTile {
    float2* data;        // uniform: image base + first panel of the tile
    const float2* filt;  // uniform: filter, same panel
    unsigned loff;       // per lane: (group's panel in the tile) * pstride + tid * 4   [float2 elements]
    int tl;              // tile index inside its image
    bool ok;             // this thread group's panel exists (else it reads the tile's first panel and stores nothing)
};

template <int LOGM, class Core>
__device__ __forceinline__ void panel_tile(float2 (&cur)[4][8], float2 (&flt)[4][8], const PanelTile& c, const PanelTile& n,
                                           unsigned nscale, float2* grp_lds, const typename Core::Bases& bases,
                                           const float2* __restrict__ tw_fwd, int tid, bool packed_tile, bool packed_group) {
    Core::template run<0, false>(cur, grp_lds, tw_fwd, bases, tid);
    // column 0 of panel 0 in half-spectrum mode: uniform branch per workgroup (barriers inside); thread groups of
    // the same workgroup that hold other panels go through the same barriers and keep the plain product
    if (packed_tile) {
        packed_column_filter<LOGM, Core, Core::SLOTS>(cur, flt, grp_lds, tid, packed_group);
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) cur[0][s] = cmul_fma(cur[0][s], flt[0][s]);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        cur[1][s] = cmul_fma(cur[1][s], flt[1][s]);
        cur[2][s] = cmul_fma(cur[2][s], flt[2][s]);
        cur[3][s] = cmul_fma(cur[3][s], flt[3][s]);
    }
    tile_load<Core, false>(n.data, n.loff, nscale, flt);  // next spectrum streams in behind the inverse transform
    constexpr int SEQ1 = Core::SLOTS;
    Core::permute_out_to_in(cur);  // (a renaming of registers when the first and the last radix differ)
    Core::template run<SEQ1, true>(cur, grp_lds, tw_fwd, bases, tid);
    landed(flt);
    if (c.ok) tile_store<Core>(c.data, c.loff, cur);
    tile_load<Core, true>(n.filt, n.loff, nscale, cur);   // next filter streams in behind the next forward transform
}

// The tile sequence of one launch runs over the panels of up to 4 images (PanelBatch): global tile
// t = image * ntiles + tile.  With several images per launch the un-overlapped prologue (first spectrum) and
// epilogue (last inverse + store) of the persistent workgroups amortise over more tiles, and small images fill the chip.
template <int LOGM>
__global__ __launch_bounds__(PanelGeom<LOGM>::THREADS, PanelGeom<LOGM>::PIPE_WAVES_PER_SIMD) void fft_cols_panel_fused_kernel(
    const PanelBatch pb, const float2* __restrict__ filt, const float2* __restrict__ tw_fwd, const unsigned pstride,
    const int npanels, const int ntiles, const int packed0) {
    using St = Steps<LOGM>;
    using Geo = PanelGeom<LOGM>;
    constexpr int G = Geo::G, T = St::T;
    using Core = FftCore<LOGM, 4, 2, PolicyFast>;
    __shared__ float2 lds[G * 2 * St::BUF];
    // one thread group per workgroup (M >= 4096): everything about a tile except tid is wave-uniform
    const int g = G == 1 ? 0 : (int)(threadIdx.x >> St::LOGT);
    const int tid = threadIdx.x & (T - 1);
    float2* grp_lds = lds + g * 2 * St::BUF;
    const int total = ntiles * pb.nimg;
    int t = blockIdx.x;
    if (t >= total) return;  // uniform over the workgroup

    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);

    // (image, tile) advance by scalar add / subtract: an integer division per tile would run on the VALU and drag
    // every tile address into VGPRs
    auto tile_of = [&](int img, int tl) {
        PanelTile r;
        r.tl = tl;
        r.ok = tl * G + g < npanels;
        r.loff = (r.ok ? (unsigned)g : 0u) * pstride + (unsigned)tid * 4u;
        const size_t tbase = (size_t)(tl * G) * pstride;
        r.data = pick_image(pb.data, img) + tbase;
        r.filt = filt + tbase;
        return r;
    };
    int img = 0, tl = t;
    while (tl >= ntiles) { tl -= ntiles; ++img; }
    auto advance = [&](int& im, int& tt) {
        tt += (int)gridDim.x;
        while (tt >= ntiles) { tt -= ntiles; ++im; }
    };

    float2 P[4][8], Q[4][8];
    PanelTile c = tile_of(img, tl);
    tile_load<Core, false>(c.data, c.loff, 1u, P);
    tile_load<Core, true>(c.filt, c.loff, 1u, Q);
    while (true) {
        int tn = t + gridDim.x;
        bool more = tn < total;
        int nimg = img, ntl = tl;
        if (more) advance(nimg, ntl);
        PanelTile n = tile_of(nimg, ntl);
        if (!more) n.data = const_cast<float2*>(n.filt);  // dummy prefetch source: read-only memory
        panel_tile<LOGM, Core>(P, Q, c, n, more ? 1u : 0u, grp_lds, bases, tw_fwd, tid, packed0 && c.tl == 0, g == 0);
        if (!more) break;
        t = tn; c = n; img = nimg; tl = ntl;
        tn = t + gridDim.x;
        more = tn < total;
        if (more) advance(nimg, ntl);
        n = tile_of(nimg, ntl);
        if (!more) n.data = const_cast<float2*>(n.filt);
        panel_tile<LOGM, Core>(Q, P, c, n, more ? 1u : 0u, grp_lds, bases, tw_fwd, tid, packed0 && c.tl == 0, g == 0);
        if (!more) break;
        t = tn; c = n; img = nimg; tl = ntl;
    }
}

// ---------------------------------------------------------------------------------------------
// Pass B' with 16 values per thread (radix-16 steps): a 4096-point column takes 256 threads, so a 4-column tile is
// ONE 256-thread workgroup holding 128 data registers per lane, and two such workgroups share a CU (2 x 74 KB of LDS,
// 256 VGPRs each): the hardware overlaps one tile's loads / stores with the other tile's transforms, which the
// single persistent workgroup of the radix-8 kernel has to arrange by hand (and only half manages: DESIGN.md 5).
// 8192-point columns: 512 threads, one workgroup per CU, no spills (the radix-8 kernel needs 1024 threads at 128
// VGPRs there).  One tile per workgroup; the tile sequence runs over the images of the launch.
// ---------------------------------------------------------------------------------------------
// Phase stamps of pass B' (timing-only debug builds, -DFDR_DEBUG_STAMPS; read back by tools/microbench/passbench): the
// shader-clock counter of wave 0 of every workgroup at start / tile landed / forward transform done / filter applied /
// inverse transform done / stores issued / stores retired.  The waits the "landed" and "retired" stamps need are part of
// such a build only.
#ifdef FDR_DEBUG_STAMPS
// (the record itself -- fdr_dbg_stamps, 32 entries per workgroup -- lives in fdr_fft_core.hpp: the core stamps its steps too)
#define FDR_STAMP(i) do { if (threadIdx.x == 0) fdr_dbg_stamps[((blockIdx.x + gridDim.x * blockIdx.y) & 8191) * 32 + (i)] = __builtin_readcyclecounter(); } while (0)
#define FDR_STAMP_WAIT_VM() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
// every value of the tile is final here and nothing that uses it starts earlier: makes the stamp a real phase boundary
// (VALU work and the waits in front of it would otherwise drift across the stamp's store)
#define FDR_STAMP_PIN(v) do { _Pragma("unroll") for (int b_ = 0; b_ < 4; ++b_) _Pragma("unroll") for (int s_ = 0; s_ < 16; ++s_) asm volatile("" : "+v"(v[b_][s_].x), "+v"(v[b_][s_].y)); } while (0)
extern "C" int fdr_debug_read_stamps(unsigned long long* out, size_t count) {
    if (count > 8192 * 32) count = 8192 * 32;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(fdr_dbg_stamps), count * sizeof(unsigned long long));
}
#else
#define FDR_STAMP(i) ((void)0)
#define FDR_STAMP_WAIT_VM() ((void)0)
#define FDR_STAMP_PIN(v) ((void)0)
#endif

template <int LOGM>
struct Panel16Geom {
    static constexpr int T = Steps<LOGM, 4>::T;
    // one panel per workgroup at every size: with short columns (64 or 128 threads per transform) grouping several
    // panels into a 256-thread workgroup is slower and leaves CUs idle (LAB_NOTES "pass B' tile shape")
    static constexpr int G = 1;
    static constexpr int THREADS = T * G;
};

template <int LOGM>
__global__ __launch_bounds__(Panel16Geom<LOGM>::THREADS, 2) void fft_cols_panel_fused16_kernel(
    const PanelBatch pb, const float2* __restrict__ filt, const float2* __restrict__ tw_fwd, const unsigned pstride,
    const int npanels, const int ntiles, const int packed0, const int img_shift) {
    using St = Steps<LOGM, 4>;
    constexpr int G = Panel16Geom<LOGM>::G, T = St::T, M = St::L, V = 16;
    using Core = FftCore<LOGM, 4, 2, PolicyFast, 4, (St::lr(0) == 1 && T >= 64)>;  // 8192 points: wave-local first exchange
    __shared__ float2 lds[G * 2 * St::BUF];
    const int g = G == 1 ? 0 : (int)(threadIdx.x >> St::LOGT);
    const int tid = Core::thread_index(threadIdx.x & (T - 1));
    float2* grp_lds = lds + g * 2 * St::BUF;
    // Two mappings of workgroups to (tile, image), both free of integer divisions (which would run on the VALU and drag
    // every tile address into VGPRs).  img_shift < 0: grid (ntiles, images).  Otherwise (2, 4 or 8 images, tiles a multiple
    // of 8): a flat grid in which the workgroups that share a tile -- and so its slice of the filter W -- are neighbours
    // on the SAME XCD (workgroup b lands on XCD b % 8), so W crosses the fabric once per tile, not once per image.
    int img, tl;
    if (img_shift < 0) { img = blockIdx.y; tl = blockIdx.x; }
    else {
        const int b = blockIdx.x, j = b >> 3;
        img = j & ((1 << img_shift) - 1);
        tl = ((j >> img_shift) << 3) | (b & 7);
    }
    const bool active = tl * G + g < npanels;
    const size_t tbase = (size_t)(tl * G) * pstride;
    float2* __restrict__ data = pick_image(pb.data, img) + tbase;
    const float2* __restrict__ tfilt = filt + tbase;
    const unsigned loff = (active ? (unsigned)g : 0u) * pstride + (unsigned)tid * 4u;

    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);
    // 8192 points: the tile fills 128 of the 256 registers a lane has and the filter phase needs the rest, so the hoisted
    // twiddle bases (one float2 per radix-16 step) do not survive it in registers -- left to hipcc they are spilled in the
    // forward transform and reloaded from scratch in the inverse.  They are parked in the 12 KB of LDS the exchange buffers
    // leave instead and picked up again for the inverse: an LDS read where a scratch load was.
    constexpr bool kParkBases = LOGM == 13;
    __shared__ float2 parked[kParkBases ? (St::S - 1) * T : 1];
    if constexpr (kParkBases) {
#pragma unroll
        for (int j = 1; j < St::S; ++j) parked[(j - 1) * T + tid] = bases.b[j][0];  // (the logical index: one slot per thread)
    }

    // (Schedules of this kernel that were built and measured slower are listed in LAB_NOTES "pass B' schedules".)
    float2 v[4][V];
    FDR_STAMP(0);
    tile_load<Core, false>(data, loff, 1u, v);
    FDR_STAMP_WAIT_VM();
    FDR_STAMP_PIN(v);
    FDR_STAMP(1);
    Core::template run<0, false>(v, grp_lds, tw_fwd, bases, tid);
    FDR_STAMP_PIN(v);
    FDR_STAMP(2);

    const bool packed_tile = packed0 && tl == 0;  // uniform per workgroup
    constexpr int SEQ = Core::SLOTS;
    if (packed_tile) {  // column 0 of panel 0 (packed DC + i Nyquist) finished on its own; see the lean kernel
        float2* bufc = grp_lds + (SEQ & 1) * St::BUF;
        float2* bufs = grp_lds + ((SEQ + 1) & 1) * St::BUF;
        __syncthreads();
        FDR_JITTER(4011);
        // (once per image, on one workgroup: kept cheap in REGISTERS, not in time -- the filter values go to LDS two at
        // a time behind compiler barriers and every slot is finished before the next one starts, so this path adds
        // nothing to the pressure of the common one)
#pragma unroll
        for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHOL; ++q) bufc[Core::out_index(tid, u, q)] = v[0][u * Core::RHOL + q];
#pragma unroll
        for (int s = 0; s < V; s += 2) {
            const int k0 = Core::out_index(tid, s / Core::RHOL, s % Core::RHOL), k1 = Core::out_index(tid, (s + 1) / Core::RHOL, (s + 1) % Core::RHOL);
            const float2 f0 = tfilt[loff - (unsigned)tid * 4u + (unsigned)k0 * 4u], f1 = tfilt[loff - (unsigned)tid * 4u + (unsigned)k1 * 4u];
            bufs[k0] = f0; bufs[k1] = f1;
            asm volatile("" ::: "memory");
        }
        __syncthreads();
        FDR_JITTER(4012);
        if (g == 0) {
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) {
                    const int s = u * Core::RHOL + q;
                    const int k = Core::out_index(tid, u, q);
                    const int km = (M - k) & (M - 1);
                    const float2 c = v[0][s], cm = bufc[km], sm = bufs[km], sl_s = bufs[k];
                    const float2 f0 = make_float2(0.5f * (c.x + cm.x), 0.5f * (c.y - cm.y));
                    const float2 fn = make_float2(0.5f * (c.y + cm.y), 0.5f * (cm.x - c.x));
                    float2 a0, an;
                    if (k == 0 || k == M / 2) { a0 = make_float2(sl_s.x, 0.f); an = make_float2(sl_s.y, 0.f); }
                    else if (k < M / 2) { a0 = sl_s; an = sm; }
                    else { a0 = make_float2(sm.x, -sm.y); an = make_float2(sl_s.x, -sl_s.y); }
                    const float2 z0 = cmul_fma(f0, a0), zn = cmul_fma(fn, an);
                    v[0][s] = make_float2(z0.x - zn.y, z0.y + zn.x);
                    asm volatile("" ::: "memory");
                }
        }
        __syncthreads();  // both buffers were read above
    }
    {
        const bool col0_done = packed_tile && g == 0;
        // W in pieces of PC slots, the next piece requested before the current one is used; the compiler barriers keep
        // hipcc from hoisting all the loads to the top, in front of the forward transform, where they spill
        // (LAB_NOTES "pass B' filter pieces")
        constexpr int PC = 4;  // slots per piece: 8 VGPRs per slot, two pieces in flight
        auto wload = [&](int h, float2 (&w)[PC][4]) {
#pragma unroll
            for (int i = 0; i < PC; ++i) {
                const int s = PC * h + i, u = s / Core::RHOL, q = s % Core::RHOL;
                const unsigned uoff = (unsigned)(((q << Core::LOGOUT) + u * Core::T) * 4);
#ifdef FDR_DEBUG_SKIP_W  // timing-only builds: pass B' without its filter traffic
                (void)uoff;
                w[i][0] = w[i][1] = w[i][2] = w[i][3] = make_float2(1.0f, __uint_as_float(loff) * 0.f);
#else
                const gchar* ub = uniform_gptr(tfilt + uoff);
                FDR_GLOAD32(ub, loff * 8u, w[i][0], w[i][1], w[i][2], w[i][3]);
#endif
            }
        };
        auto wmul = [&](int h, const float2 (&w)[PC][4]) {
#pragma unroll
            for (int i = 0; i < PC; ++i) {
                const int s = PC * h + i;
                v[0][s] = cmul_fma(v[0][s], col0_done ? make_float2(1.f, 0.f) : w[i][0]);
                v[1][s] = cmul_fma(v[1][s], w[i][1]);
                v[2][s] = cmul_fma(v[2][s], w[i][2]);
                v[3][s] = cmul_fma(v[3][s], w[i][3]);
            }
        };
        float2 wa[PC][4], wb[PC][4];
        wload(0, wa);
#pragma unroll
        for (int h = 0; h < V / PC; h += 2) {
            asm volatile("" ::: "memory");
            wload(h + 1, wb);
            wmul(h, wa);
            asm volatile("" ::: "memory");
            if (h + 2 < V / PC) wload(h + 2, wa);
            wmul(h + 1, wb);
        }
    }
    FDR_STAMP_PIN(v);
    FDR_STAMP(3);
    {
        // opaque copy of the thread index: the inverse transform's LDS addresses equal the forward transform's, and as
        // common subexpressions they would stay alive across the filter phase, where register pressure peaks
        int ti = tid;
        asm volatile("" : "+v"(ti));
        Core::permute_out_to_in(v);  // (a renaming of registers when the first and the last radix differ)
        if constexpr (kParkBases) {
            typename Core::Bases inv_bases;
#pragma unroll
            for (int j = 1; j < St::S; ++j) inv_bases.b[j][0] = parked[(j - 1) * T + ti];
            Core::template run<SEQ, true>(v, grp_lds, tw_fwd, inv_bases, ti);
        } else {
            Core::template run<SEQ, true>(v, grp_lds, tw_fwd, bases, ti);
        }
    }
    FDR_STAMP_PIN(v);
    FDR_STAMP(4);
    if (active) tile_store<Core>(data, loff, v);
    FDR_STAMP(5);
    FDR_STAMP_WAIT_VM();
    FDR_STAMP(6);
}

// ---------------------------------------------------------------------------------------------
// Pass B' for ONE small image (the single-image call of BASELINE config 2: M <= 2048).  The tile kernels above give a
// 4-column tile to one thread group (64 threads at 1024 points): with a single image in flight that is 128 one-wave
// workgroups, each running eight 1024-point transforms back to back on one SIMD -- a long chain of dependent VALU and
// memory latency on a chip that is nearly idle (LAB_NOTES "single small image").
// Here the four columns of a panel go to four thread groups of one workgroup (B = 1 transform per group, same FftCore
// step plan and policy as the tile kernel of that length, so the bits are the same), the filter is requested together with
// the spectrum (16 or 8 values per lane leave the registers for it), and nothing is staged.  The thread groups are
// INTERLEAVED over the lanes -- column = lane & 3, logical thread = lane >> 2 -- so that for every (u, q) slot the 64 lanes
// of a wave touch 16 rows x 4 columns = 512 contiguous bytes: dense 8-byte-per-lane accesses (with column = lane / T each
// wave read 8 of every 32 bytes, which held the 2048-row case at the tile kernel's time).  The groups' exchange buffers are
// 16 dwords apart modulo the 64 banks, so the four 8-lane runs of a half wave fall on disjoint banks in the contiguous
// phases of an exchange.
// ---------------------------------------------------------------------------------------------
template <int LOGM>
struct PanelSplitGeom {
    static constexpr int LOGV = LOGM >= 10 ? 4 : 3;  // as the tile kernels: radix-16 steps from 1024 points on, radix-8 below
    using St = Steps<LOGM, LOGV>;
    static constexpr int T = St::T;
    static constexpr int THREADS = 4 * T;
};

template <int LOGM, int NBUF = 2>
__global__ __launch_bounds__(PanelSplitGeom<LOGM>::THREADS) void fft_cols_panel_split_kernel(
    const PanelBatch pb, const float2* __restrict__ filt, const float2* __restrict__ tw_fwd, const unsigned pstride, const int packed0,
    const int img_shift) {
    using Geo = PanelSplitGeom<LOGM>;
    using St = typename Geo::St;
    constexpr int M = St::L, V = St::V;
    using Core = FftCore<LOGM, 1, NBUF, PolicyFast, Geo::LOGV, false>;
    constexpr int GRP = NBUF * St::BUF + ((24 - (NBUF * St::BUF) % 32) & 31);  // float2 elements per group, = 24 (mod 32): 48 dwords (mod 64)
    static_assert(GRP % 32 == 24, "group stride");
    __shared__ float2 lds[4 * GRP];
    const int c = (int)(threadIdx.x & 3);   // column of the panel
    const int tid = (int)(threadIdx.x >> 2);  // logical thread of that column's transform
    float2* grp_lds = lds + c * GRP;
    int img = 0, tl = (int)blockIdx.x;
    if (img_shift >= 0) {  // flat grid: the workgroups that share a tile (and its slice of W) are neighbours on one XCD
        const int b = (int)blockIdx.x, jj = b >> 3;
        img = jj & ((1 << img_shift) - 1);
        tl = ((jj >> img_shift) << 3) | (b & 7);
    } else {
        img = (int)blockIdx.y;
    }
    // element (m, c) of the panel lies at panel[4 m + c]: a wave-uniform base per (u, q) slot (SGPRs) plus ONE 32-bit lane
    // offset for every access of the kernel -- no 64-bit per-lane address lives in VGPRs (see uniform_gptr)
    float2* __restrict__ panel = pick_image(pb.data, img) + (size_t)tl * pstride;
    const float2* __restrict__ wpanel = filt + (size_t)tl * pstride;
    const float2* __restrict__ wcol = wpanel + c;
    const unsigned lane_off = (unsigned)threadIdx.x * 8u;  // (4 tid + c) float2 elements

    typename Core::Bases bases;
    Core::init_bases(bases, tw_fwd, tid);

    float2 v[1][V], w[V];
#pragma unroll
    for (int u = 0; u < Core::NU0; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHO0; ++q) {
            const gchar* ub = uniform_gptr(panel + (unsigned)(((q << Core::LOGR0) + u * Core::T) * 4));
            v[0][u * Core::RHO0 + q] = *reinterpret_cast<const float2*>((const char*)ub + lane_off);
        }
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) {
            const gchar* ub = uniform_gptr(wpanel + (unsigned)(((q << Core::LOGOUT) + u * Core::T) * 4));
            w[u * Core::RHOL + q] = *reinterpret_cast<const float2*>((const char*)ub + lane_off);
        }

    Core::template run<0, false>(v, grp_lds, tw_fwd, bases, tid);

    constexpr int SEQ = Core::SLOTS;
    const bool packed_tile = packed0 && tl == 0;  // uniform per workgroup
    if (packed_tile) {  // column 0 of panel 0 carries DC + i Nyquist (see packed_column_filter): finished by its own thread group
        // (two buffers: the buffer of slot SEQ is free -- its last readers passed the barrier of the exchange after it;
        //  one buffer: it was read by the last exchange, hence the barrier)
        float2* bufc = grp_lds + (SEQ % NBUF) * St::BUF;
        if constexpr (NBUF == 1) __syncthreads();
        FDR_JITTER(4031);
        if (c == 0) {
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) bufc[Core::out_index(tid, u, q)] = v[0][u * Core::RHOL + q];
        }
        __syncthreads();
        FDR_JITTER(4032);
        if (c == 0) {
#pragma unroll
            for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
                for (int q = 0; q < Core::RHOL; ++q) {
                    const int s = u * Core::RHOL + q;
                    const int k = Core::out_index(tid, u, q);
                    const int km = (M - k) & (M - 1);
                    const float2 cc = v[0][s], cm = bufc[km], sl = w[s], sm = wcol[(size_t)km * 4];
                    const float2 f0 = make_float2(0.5f * (cc.x + cm.x), 0.5f * (cc.y - cm.y));
                    const float2 fn = make_float2(0.5f * (cc.y + cm.y), 0.5f * (cm.x - cc.x));
                    float2 a0, an;
                    if (k == 0 || k == M / 2) { a0 = make_float2(sl.x, 0.f); an = make_float2(sl.y, 0.f); }
                    else if (k < M / 2) { a0 = sl; an = sm; }
                    else { a0 = make_float2(sm.x, -sm.y); an = make_float2(sl.x, -sl.y); }
                    const float2 z0 = cmul_fma(f0, a0), zn = cmul_fma(fn, an);
                    v[0][s] = make_float2(z0.x - zn.y, z0.y + zn.x);
                    w[s] = make_float2(1.f, 0.f);
                }
        }
        __syncthreads();  // bufc was read: the inverse transform's first exchange writes it
    }
#pragma unroll
    for (int s = 0; s < V; ++s) v[0][s] = cmul_fma(v[0][s], w[s]);

    Core::permute_out_to_in(v);
    Core::template run<SEQ, true>(v, grp_lds, tw_fwd, bases, tid);

    {
        unsigned lo = (unsigned)threadIdx.x * 8u;  // opaque copy: recomputed here instead of living across both transforms
        asm volatile("" : "+v"(lo));
#pragma unroll
        for (int u = 0; u < Core::NUL; ++u)
#pragma unroll
            for (int q = 0; q < Core::RHOL; ++q) {
                gchar* ub = uniform_gptr(panel + (unsigned)(((q << Core::LOGOUT) + u * Core::T) * 4));
                *reinterpret_cast<float2*>((char*)ub + lo) = v[0][u * Core::RHOL + q];
            }
    }
}

template <int LOGM>
static hipError_t launch_cols_panel_t(ColKind kind, const ColArgs& a, const float2* tw, hipStream_t s) {
    using Geo = PanelGeom<LOGM>;
    const size_t ps = a.pstride;
    const int npanels = a.npanels > 0 ? a.npanels : a.N / 4;  // half spectrum: N/8
    const int ntiles = (npanels + Geo::G - 1) / Geo::G;
    if (kind == COL_FWD_FILTER) {
        hipLaunchKernelGGL((fft_cols_panel_fwd_filter_kernel<LOGM>), dim3(ntiles), dim3(Geo::THREADS), 0, s, a.data, tw, ps, npanels, a.nvalid, a.K,
                           a.packed0);
    } else if (kind == COL_FUSED) {
        PanelBatch pb = a.batch;
        if (pb.nimg <= 0) { pb.nimg = 1; pb.data[0] = a.data; }
        for (int k = pb.nimg; k < kMaxGroup; ++k) pb.data[k] = pb.data[0];
        if constexpr (LOGM >= 8 && LOGM <= 11) {
            if (pb.nimg == 1) {  // a single small image: latency, not bandwidth (see fft_cols_panel_split_kernel)
                hipLaunchKernelGGL((fft_cols_panel_split_kernel<LOGM, 2>), dim3(npanels), dim3(PanelSplitGeom<LOGM>::THREADS), 0, s, pb, a.filt, tw,
                                   (unsigned)ps, a.packed0, -1);
                return hipGetLastError();
            }
        }
        if constexpr (LOGM >= 10) {  // 16 values per thread: one workgroup per tile, grid (tiles, images)
            using G16 = Panel16Geom<LOGM>;
            const int nt16 = (npanels + G16::G - 1) / G16::G;
            const int ishift = (nt16 % 8 == 0) ? (pb.nimg == 2 ? 1 : pb.nimg == 4 ? 2 : pb.nimg == 8 ? 3 : -1) : -1;
            const dim3 grid16 = ishift < 0 ? dim3(nt16, pb.nimg) : dim3(nt16 * pb.nimg);
            hipLaunchKernelGGL((fft_cols_panel_fused16_kernel<LOGM>), grid16, dim3(G16::THREADS), 0, s, pb, a.filt, tw,
                               (unsigned)ps, npanels, nt16, a.packed0, ishift);
        } else {                     // short columns: persistent radix-8 kernel, register double-buffered
            const int total = ntiles * pb.nimg;
            int grid = (a.num_cu > 0 ? a.num_cu : 256) * Geo::PIPE_WG_PER_CU;
            if (grid > total) grid = total;
            hipLaunchKernelGGL((fft_cols_panel_fused_kernel<LOGM>), dim3(grid), dim3(Geo::THREADS), 0, s, pb, a.filt, tw, (unsigned)ps,
                               npanels, ntiles, a.packed0);
        }
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_cols_panel(int logm, ColKind kind, const ColArgs& a, const float2* tw_fwd, hipStream_t s) {
    FDR_DISPATCH_LOG(logm, launch_cols_panel_t<LG>(kind, a, tw_fwd, s));
    return hipErrorInvalidValue;
}

}  // namespace fdr
