// fdr_mixed_plan.hpp -- what a FDR_FLAG_MIXED_RADIX plan decides on the host: which lengths it takes, the Stockham stage list and
// the two-level twiddle table of a length, the threads per transform, and the panel width P / row transforms per workgroup B of an
// M x N plan.  Host arithmetic only -- no HIP type, no HIP call -- so that tools/cli/mixed_plan_check.cpp can check every
// length and every layout without a device (tests/test_mixed_plan_host.py).  fdr_api_plan.hip uploads what this builds;
// fdr_mixed.hip (mx_stage) reads it.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

namespace fdr {

constexpr int kMixMaxElems = 16;              // values one thread holds per stage: threads per transform nt >= L / 16
constexpr size_t kMixMaxLds = 144 * 1024;     // dynamic LDS of one workgroup (the rest: twiddles, reduction)
constexpr int kMixMaxLen = 8192;
constexpr int kMixTwLo = 64;                  // twiddle table = lo[64] then hi[ceil(L / 64)]: w^m = lo[m % 64] hi[m / 64]
constexpr size_t kMixLdsTarget = 78 * 1024;   // two workgroups per CU (with the static twiddle / reduction arrays)

struct MixTwiddle { float x, y; };            // one table entry, the layout of a float2
struct MixStage { int radix, ns, magic, twstep; };  // one Stockham stage, the layout of the int4 the kernels read (x, y, z, w)

inline bool is_smooth(int n) {  // 2^a 3^b 5^c
    if (n <= 0) return false;
    for (int f : {2, 3, 5})
        while (n % f == 0) n /= f;
    return n == 1;
}

// Stockham schedule of a length 2^a 3^b 5^c (radix 4 first, then 2, 3, 5) and the twiddle table exp(-2 pi i m / L) in two
// levels (w^m = lo[m mod 64] hi[m / 64], each entry evaluated in double and rounded once); per stage {radix, ns, ceil(2^32 / ns) (0 for ns = 1), L / (ns radix)}
inline void build_mixed_tables(int L, std::vector<MixTwiddle>& tw, std::vector<MixStage>& st) {
    const double PI = 3.1415926535897932384626433832795;
    const int nhi = (L + kMixTwLo - 1) / kMixTwLo;
    tw.resize((size_t)(kMixTwLo + nhi));
    for (int i = 0; i < kMixTwLo + nhi; ++i) {  // two levels (LDS-sized): lo[i] = w^i, hi[i] = w^(64 i)
        const double m = i < kMixTwLo ? (double)i : (double)kMixTwLo * (i - kMixTwLo);
        const double a = -2.0 * PI * m / (double)L;
        tw[i] = MixTwiddle{(float)std::cos(a), (float)std::sin(a)};
    }
    std::vector<int> radix;
    int r = L;
    while (r % 4 == 0) { radix.push_back(4); r /= 4; }
    while (r % 2 == 0) { radix.push_back(2); r /= 2; }
    while (r % 3 == 0) { radix.push_back(3); r /= 3; }
    while (r % 5 == 0) { radix.push_back(5); r /= 5; }
    st.clear();
    int ns = 1;
    for (int R : radix) {
        const unsigned magic = ns == 1 ? 0u : (unsigned)((0x100000000ull + (unsigned long long)ns - 1) / (unsigned long long)ns);
        st.push_back(MixStage{R, ns, (int)magic, L / (ns * R)});
        ns *= R;
    }
}

// threads per transform of length L: a multiple of 64 with L <= kMixMaxElems * nt
inline int mixed_threads(int L) {
    int nt = (L + kMixMaxElems - 1) / kMixMaxElems;
    nt = (nt + 63) / 64 * 64;
    return nt < 64 ? 64 : nt;
}

// panel width P = 1 << logP (divides N, a panel of M rows within kMixLdsTarget, P column transforms within 1024 threads) and
// row-pass transforms per workgroup B (1 .. 16) of an M x N plan
struct MixLayout { int logP, B; };
inline MixLayout mixed_layout(int M, int N) {
    MixLayout l{0, 1};
    for (int lp = 2; lp > 0; --lp) {
        const int P = 1 << lp;
        if (N % P == 0 && ((size_t)M * P * sizeof(MixTwiddle) <= kMixLdsTarget) && mixed_threads(M) * P <= 1024) { l.logP = lp; break; }
    }
    while (l.B < 16 && mixed_threads(N) * l.B * 2 <= 1024 && (size_t)N * l.B * 2 * sizeof(MixTwiddle) <= kMixLdsTarget) l.B *= 2;
    return l;
}

}  // namespace fdr
