// fdr_panel.hpp -- what the units of the fast-mode passes on a PANEL-MAJOR intermediate spectrum share (device side):
// fdr_panel_rows.hip (pass A; passes C' / C1 / C2 and the operator kinds), fdr_panel_cols.hip (pass B' and the Wiener PSF column
// pass), and the PSF column passes of fdr_cls.hip and fdr_rl.hip.
//
// Why: a column pass that keeps 4 adjacent columns of a row-major M x N array touches 32 of the
// 128 bytes of every line; four workgroups share each line, and with >= 128 KB of lines in flight
// per CU the sharing cannot be served from the 4 MiB XCD L2, and each line moves about four times
// (LAB_NOTES "panel layout").  The fix is a layout in which every pass moves whole lines:
//
//     panel_index(m, n) = (n >> 2) * PS + m * 4 + (n & 3)     (M rows, N columns, float2 elements)
//
// i.e. panels of 4 columns, each panel a contiguous M x 4 array; the panel stride PS = 4 M + 16 is
// deliberately not a power of two, so the 128-byte lines a row workgroup scatters over all panels
// do not all fall on the same memory channel.  A column tile (4 columns, all
// rows) is then ONE contiguous 32*M-byte chunk, and a row workgroup that owns 4 consecutive rows
// writes / reads complete 128-byte lines (4 rows x 4 columns) in every panel.
//
//   pass A  : 4 real rows  (zero-padded on load) -> row FFTs -> panel layout
//   pass B' : one panel: column FFTs . W . column IFFTs, in place, persistent + register
//             double-buffered (next panel's spectrum / filter stream in behind the butterflies)
//   pass C' : 4 rows gathered from the panels -> row IFFTs -> real plane + min/max partial
// The layout is private to a plan (never visible through the C ABI); W is stored the same way.
#pragma once
#include "fdr_fft_core.hpp"
#include "fdr_kernels.hpp"

namespace fdr {

// ---------------------------------------------------------------------------------------------
// columns of one panel (contiguous M x 4 chunk)
// ---------------------------------------------------------------------------------------------
template <int LOGM>
struct PanelGeom {
    static constexpr int T = Steps<LOGM>::T;
    static constexpr int G = T >= 512 ? 1 : (T >= 256 ? 2 : 4);  // panels per workgroup
    static constexpr int THREADS = T * G;
    // persistent pipelined kernel: two register sets, one workgroup per CU for 512 threads
    static constexpr int PIPE_WAVES_PER_SIMD = THREADS >= 1024 ? 4 : (THREADS >= 512 ? 2 : 1);
    static constexpr int PIPE_WG_PER_CU = THREADS >= 512 ? 1 : 512 / THREADS;
    static constexpr int WAVES_PER_SIMD = THREADS >= 512 ? 4 : 1;
};

// First-step operands of a panel's four column transforms (row m of the panel at m * 4); rows >= nvalid are taken as zero without
// being read.  A macro, not a function: as a __forceinline__ function the same loop reaches the optimiser in another order and 18 of
// the 22 Wiener and operator PSF column kernels come out with other registers and schedules (tools/kernel_diff.py).
#define FDR_PANEL_LOAD_VALID(Core, pbase, tid, nvalid, v)                                                   \
    _Pragma("unroll") for (int u = 0; u < Core::NU0; ++u)                                                   \
        _Pragma("unroll") for (int q = 0; q < Core::RHO0; ++q) {                                            \
            const int s = u * Core::RHO0 + q;                                                               \
            const int m = Core::in_index(tid, u, q);                                                        \
            if (m < nvalid) load4(pbase + (size_t)m * 4, v[0][s], v[1][s], v[2][s], v[3][s]);               \
            else v[0][s] = v[1][s] = v[2][s] = v[3][s] = make_float2(0.f, 0.f);                             \
        }

// element offsets inside a panel: row m -> m*4 ; the uniform part (q) stays in SGPRs
template <class Core>
__device__ __forceinline__ void panel_store_out(float2* __restrict__ pbase, int tid, const float2 (&d)[4][8]) {
#pragma unroll
    for (int u = 0; u < Core::NUL; ++u) {
        const unsigned toff = (unsigned)(tid + u * Core::T) * 4u;
#pragma unroll
        for (int q = 0; q < Core::RHOL; ++q) {
            const int s = u * Core::RHOL + q;
            store4(pbase + ((size_t)(q << Core::LOGOUT) * 4) + toff, d[0][s], d[1][s], d[2][s], d[3][s]);
        }
    }
}

}  // namespace fdr
