// fdr_workspace.hpp -- the on-demand device blocks of a plan: the handle that owns one (Workspace), the carver that lays one out,
// and per block its pointers and its layout, written ONCE as an ordered list of "n elements of T, aligned to a bytes".  The same
// list is run twice, on a carver without a block to measure it and on one with the block to place the pointers, so size and carving
// cannot disagree.  Host arithmetic only -- no HIP type, no HIP call, the complex element is a template parameter, the allocator a
// pair of arguments -- so that tools/cli/workspace_check.cpp can print every layout and drive the failure branch without a device
// (tests/test_workspace_host.py).  fdr_host.hpp gives the layouts their float2, their plan and hipMalloc / hipFree.
#pragma once

#include <cstddef>
#include <cstdint>

namespace fdr {

// One pass over a layout.  Without a block (base null) it only measures; with one it places every member at base + its offset.
// Both check that every member starts on the alignment its description states (offsets when measuring: a block from hipMalloc
// starts on 256 bytes, and no description asks for more).  A carver that prints (the check tool's) has the same three members.
struct Carver {
    char* base = nullptr;
    size_t at = 0;        // bytes so far: the size of the block when the list ends
    bool aligned = true;  // every member so far met its stated alignment
    template <class T> void put(const char* /*name*/, T*& member, size_t n, size_t align) {
        aligned = aligned && (reinterpret_cast<uintptr_t>(base) + at) % align == 0;
        if (base) member = reinterpret_cast<T*>(base + at);
        at += n * sizeof(T);
    }
    // members that only accessors reach (the planes of the images k > 0 of a group): room, no pointer
    template <class T> void room(const char* name, size_t n, size_t align) { T* unused = nullptr; put(name, unused, n, align); }
    void pad(size_t align) { at = (at + align - 1) / align * align; }  // the next member starts on a multiple of `align`
};

// The owning handle of one device block: what it was made for (`count`: the images of a group, the frames, the entries of a
// table; 1 for a block of fixed size) and its size.  It does NOT free in a destructor: on the process-exit path fdr_plan_destroy
// deletes the plan without touching the HIP runtime, which may be gone; releasing is the explicit call of the normal path.
struct Workspace {
    enum Grown { KEPT, MADE, NO_MEMORY, BAD_LAYOUT };
    void* block = nullptr;
    size_t bytes = 0;
    int count = 0;
    // The block for `n`: nothing when it holds n already; else `layout(carver, n)` measured, the new block from `alloc(bytes)` (null:
    // NO_MEMORY, and block, count and every pointer are what they were), then the old block to `release` and the members placed.
    template <class Layout, class Alloc, class Release>
    Grown grow(int n, Layout&& layout, Alloc&& alloc, Release&& release) {
        if (block && count >= n) return KEPT;
        Carver measure;
        layout(measure, n);
        if (!measure.aligned) return BAD_LAYOUT;
        void* fresh = alloc(measure.at);
        if (!fresh) return NO_MEMORY;
        if (block) release(block);
        Carver place{static_cast<char*>(fresh)};
        layout(place, n);
        block = fresh; bytes = measure.at; count = n;
        return place.at == measure.at && place.aligned ? MADE : BAD_LAYOUT;
    }
    template <class Release> void free_with(Release&& release) {
        if (block) release(block);
        block = nullptr; bytes = 0; count = 0;
    }
};

// ---- the layouts.  P = M N (one real plane), ws_elems = the complex elements of one spectrum in the layout of the filter, Cx = the
// complex element (float2); every partial count is the caller's (the kernels' own functions give them).  Float planes state 16
// bytes where a launch picks its vector width from the address (P >= 256 on the operator path, so 4 P is a multiple of 16).

// Total-variation deconvolution: the solve table T (rounded up to 256 bytes), then six planes per image of the group -- x, b and
// the two pairs of duals w[pair][0 = wx, 1 = wy] of image 0, then those of image 1, .. (image k's lie 6 k P floats behind image 0's)
template <class Cx> struct TvLayout {
    Cx* T = nullptr;
    float *x = nullptr, *b = nullptr, *w[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
};
template <class C, class Cx> void layout(C& c, TvLayout<Cx>& m, size_t P, size_t ws_elems, int group) {
    c.put("T", m.T, ws_elems, 256);
    c.pad(256);
    c.put("x", m.x, P, 256);
    c.put("b", m.b, P, 16);
    c.put("w00", m.w[0][0], P, 16); c.put("w01", m.w[0][1], P, 16);
    c.put("w10", m.w[1][0], P, 16); c.put("w11", m.w[1][1], P, 16);
    c.template room<float>("rest", 6 * (size_t)(group - 1) * P, 16);
}

// Free-boundary TV: the group's planes q first (image k's at q + k P, so that one memset clears a group's), then its planes c / r
struct TvFreeLayout { float *q = nullptr, *c = nullptr; };
template <class C> void layout(C& c, TvFreeLayout& m, size_t P, int group) {
    c.put("q", m.q, (size_t)group * P, 16);
    c.put("c", m.c, (size_t)group * P, 16);
}

// Noise-constrained TV: per image 3 n_part double partials (image k's at part + k 3 n of the window) and its four sums (stat + 4 k),
// the n_noise doubles of the one noise estimate, then every image's mu_k
struct TvAutoLayout { double *part = nullptr, *stat = nullptr, *noise = nullptr; float* mu = nullptr; };
template <class C> void layout(C& c, TvAutoLayout& m, size_t n_part, size_t n_noise, int group) {
    c.put("part", m.part, (size_t)group * 3 * n_part, 8);
    c.put("stat", m.stat, 4 * (size_t)group, 8);
    c.put("noise", m.noise, n_noise, 8);
    c.put("mu", m.mu, (size_t)group, 4);
}

// Multi-frame TV: the accumulator spectrum (rounded up to 256 bytes; the sum kernel reads it in 16-byte requests), the frames'
// planes q together (frame k's at q + k P), then their planes c / r
template <class Cx> struct TvFramesLayout { Cx* acc = nullptr; float *q = nullptr, *c = nullptr; };
template <class C, class Cx> void layout(C& c, TvFramesLayout<Cx>& m, size_t P, size_t ws_elems, int frames) {
    c.put("acc", m.acc, ws_elems, 256);
    c.pad(256);
    c.put("q", m.q, (size_t)frames * P, 256);
    c.put("c", m.c, (size_t)frames * P, 16);
}

// Free-boundary Richardson-Lucy: u_0, the one wgt, dw_0, then u_k, dw_k for k = 1 .. group - 1 (rlfree_u_plane, rlfree_dw_plane), then
// per image one set of part_set double partials (2 rlfree_partials(M, N) + 2)
struct RlFreeLayout { float *u = nullptr, *wgt = nullptr, *dw = nullptr; double* part = nullptr; };
template <class C> void layout(C& c, RlFreeLayout& m, size_t P, size_t part_set, int group) {
    c.put("u", m.u, P, 16);
    c.put("wgt", m.wgt, P, 16);
    c.put("dw", m.dw, P, 16);
    c.template room<float>("rest", 2 * (size_t)(group - 1) * P, 16);
    c.put("part", m.part, (size_t)group * part_set, 8);
}

// Accelerated Richardson-Lucy: the planes y, u, g of image 0, the group's partials (n_part doubles per image, an even count), its
// alphas -- 8 bytes for one image, which keeps the size a multiple of 8; max_group floats otherwise, which keeps the planes that
// follow on 16 bytes -- then y, u, g of the images 1 .. group - 1 at `more` (empty, and on 8 bytes only, for one image)
struct RlAccelLayout { float *y = nullptr, *u = nullptr, *g = nullptr, *alpha = nullptr, *more = nullptr; double* part = nullptr; };
template <class C> void layout(C& c, RlAccelLayout& m, size_t P, size_t n_part, int max_group, int group) {
    c.put("y", m.y, P, 16);
    c.put("u", m.u, P, 16);
    c.put("g", m.g, P, 16);
    c.put("part", m.part, (size_t)group * n_part, 16);
    c.put("alpha", m.alpha, group == 1 ? 2 : (size_t)max_group, 8);
    c.put("more", m.more, 3 * (size_t)(group - 1) * P, group == 1 ? 8 : 16);
}

// The TV prior of Richardson-Lucy: the group's factor planes first (image k's at f + k P), then its estimates (u + k P)
struct RlTvLayout { float *f = nullptr, *u = nullptr; };
template <class C> void layout(C& c, RlTvLayout& m, size_t P, int group) {
    c.put("f", m.f, (size_t)group * P, 16);
    c.put("u", m.u, (size_t)group * P, 16);
}

// Stopping Richardson-Lucy from the data: the (res, kl) partials of the ratio pass (one pair of doubles per workgroup), then the
// n_noise doubles of the noise estimate
struct RlStopLayout { double *part = nullptr, *noise = nullptr; };
template <class C> void layout(C& c, RlStopLayout& m, size_t n_part, size_t n_noise) {
    c.put("part", m.part, 2 * n_part, 8);
    c.put("noise", m.noise, n_noise, 8);
}

// Multi-frame Richardson-Lucy: the accumulator spectrum (first: 16-byte requests of the sum kernel), u, wgt, the frames' planes dw
// (frame k's at dw + k P), per frame one set of part_set double partials, then the folded pair of sums
template <class Cx> struct FramesLayout {
    Cx* acc = nullptr;
    float *u = nullptr, *wgt = nullptr, *dw = nullptr;
    double *part = nullptr, *sums = nullptr;
};
template <class C, class Cx> void layout(C& c, FramesLayout<Cx>& m, size_t P, size_t ws_elems, size_t part_set, int frames) {
    c.put("acc", m.acc, ws_elems, 16);
    c.put("u", m.u, P, 8);
    c.put("wgt", m.wgt, P, 8);
    c.put("dw", m.dw, (size_t)frames * P, 8);
    c.put("part", m.part, (size_t)frames * part_set, 8);
    c.put("sums", m.sums, 2, 8);
}

// Blind Richardson-Lucy: the table conj(U) / (M N), four PSF planes of max_psf floats (p_k, num, den, the host form's staging),
// the status word
template <class Cx> struct BlindLayout {
    Cx* table = nullptr;
    float *p = nullptr, *num = nullptr, *den = nullptr, *stage = nullptr;
    int* status = nullptr;
};
template <class C, class Cx> void layout(C& c, BlindLayout<Cx>& m, size_t ws_elems, size_t max_psf) {
    c.put("table", m.table, ws_elems, 8);
    c.put("p", m.p, max_psf, 4);
    c.put("num", m.num, max_psf, 4);
    c.put("den", m.den, max_psf, 4);
    c.put("stage", m.stage, max_psf, 4);
    c.put("status", m.status, 1, 4);
}

// Choosing the regularisation weight: the power plane (one float per bin and the two extras of the packed column), the partials of
// the sweep, those of the noise sum, the candidate and the result pairs -- each rounded up to 256 bytes
struct RegLayout { float* power = nullptr; double *part = nullptr, *noise = nullptr, *cand = nullptr, *res = nullptr; };
template <class C> void layout(C& c, RegLayout& m, size_t ws_elems, size_t n_part, size_t n_noise, size_t max_curve) {
    c.put("power", m.power, ws_elems + 2, 256); c.pad(256);
    c.put("part", m.part, n_part, 256); c.pad(256);
    c.put("noise", m.noise, n_noise, 256); c.pad(256);
    c.put("cand", m.cand, 2 * max_curve, 256); c.pad(256);
    c.put("res", m.res, 2 * max_curve, 256); c.pad(256);
}

// The motion-blur estimate: the complex plane (any M x N), the pad partials and their sum, the Hann tables of M + N floats
template <class Cx> struct MotionLayout { Cx* plane = nullptr; double* part = nullptr; float* hann = nullptr; };
template <class C, class Cx> void layout(C& c, MotionLayout<Cx>& m, size_t M, size_t N, size_t n_part) {
    c.put("plane", m.plane, M * N, 8);
    c.put("part", m.part, n_part + 1, 8);
    c.put("hann", m.hann, M + N, 4);
}

// Registering the frames of a burst (beside the motion block, whose plane and Hann tables it uses): the plane of the PSF pair (any
// M x N), the cross-power partials, their sum and the zero-frame gate, four doubles per workgroup of the peak pass, then the results of max_frames frames
// (24 bytes each: two doubles and two floats, held as three doubles)
template <class Cx> struct RegisterLayout { Cx* psf = nullptr; double *part = nullptr, *peak = nullptr, *result = nullptr; };
template <class C, class Cx> void layout(C& c, RegisterLayout<Cx>& m, size_t M, size_t N, size_t n_cross, size_t n_peak, size_t max_frames) {
    c.put("psf", m.psf, M * N, 8);
    c.put("part", m.part, n_cross + 2, 8);
    c.put("peak", m.peak, 4 * n_peak, 8);
    c.put("result", m.result, 3 * max_frames, 8);
}

// The defocus estimate: the trig table (cos, then sin, of max_angles angles), then the profile of max_diameters floats
struct DefocusLayout { double* trig = nullptr; float* profile = nullptr; };
template <class C> void layout(C& c, DefocusLayout& m, size_t max_angles, size_t max_diameters) {
    c.put("trig", m.trig, 2 * max_angles, 8);
    c.put("profile", m.profile, max_diameters, 4);
}

// The buffers that grow on demand by themselves (the frame tables, the score and trig tables of the motion search, the internal
// trace and the weight planes of the stopping call, the blind call's weights): one member of n elements
template <class C, class T> void layout(C& c, T*& array, size_t n, size_t align) { c.put("array", array, n, align); }

}  // namespace fdr
