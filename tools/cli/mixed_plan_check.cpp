// mixed_plan_check -- the host side of FDR_FLAG_MIXED_RADIX plans (csrc/fdr_mixed_plan.hpp) checked without a device.
//
//   mixed_plan_check                      every length 2^a 3^b 5^c <= 8192 and every mixed (M, N) pair; exit 1 on any violation
//   mixed_plan_check --dump [MxN ...]     plain text: every length's stages and twiddle table, then the layout of the pairs
//
// Per length L (what mx_stage of csrc/fdr_mixed.hip relies on):
//   - the radices are 2, 3, 4 or 5 and multiply to L; each stage's ns is the product of the earlier radices and its twiddle
//     step is L / (ns R);
//   - q = umulhi(j, magic) equals j / ns for every butterfly j < L / R (magic = 0 only where ns = 1);
//   - every twiddle index m = r k step (r < R, k < ns) is < L, so lo[m % 64] and hi[m / 64] are inside the table of
//     64 + ceil(L / 64) entries, which fits the kernels' LDS array of 64 + 8192 / 64;
//   - nt is a multiple of 64, at most 1024, and nt * ceil(kMixMaxElems / R) >= L / R for every stage (each thread keeps at most
//     that many butterflies in registers).
// Per pair (both 2^a 3^b 5^c <= 8192, not both powers of two): P divides N, the threads of the row launch (B nt(N)) and of
// the column launch (P nt(M)) are <= 1024, and the dynamic LDS of both (B N and P M complex values) is <= kMixMaxLds.
//
// The dump (read by tests/test_mixed_plan_host.py and tests/_mixed_model.py):
//   length L nt NT stages S hi H
//   stage R NS MAGIC STEP          (S lines)
//   lo I X Y                       (64 lines, %.9g: exact for a float)
//   hi I X Y                       (H lines)
//   layout M N logP B ntM ntN      (one per pair asked for)
#include "../../parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd/csrc/fdr_mixed_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace fdr;

namespace {

int g_bad = 0;

void bad(const char* fmt, int a, int b = 0, int c = 0, int d = 0) {
    if (++g_bad <= 40) {
        std::fprintf(stderr, "mixed_plan_check: ");
        std::fprintf(stderr, fmt, a, b, c, d);
        std::fprintf(stderr, "\n");
    }
}

bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

std::vector<int> smooth_lengths() {
    std::vector<int> v;
    for (int n = 1; n <= kMixMaxLen; ++n)
        if (is_smooth(n)) v.push_back(n);
    return v;
}

void check_length(int L) {
    std::vector<MixTwiddle> tw;
    std::vector<MixStage> st;
    build_mixed_tables(L, tw, st);
    const int nt = mixed_threads(L);
    const int nhi = (L + kMixTwLo - 1) / kMixTwLo;
    if ((int)tw.size() != kMixTwLo + nhi || (int)tw.size() > kMixTwLo + kMixMaxLen / kMixTwLo) bad("L=%d: twiddle table of %d entries", L, (int)tw.size());
    if (nt % 64 != 0 || nt < 64 || nt > 1024) bad("L=%d: nt=%d is not a multiple of 64 in 64 .. 1024", L, nt);
    long long prod = 1;
    int ns = 1;
    for (size_t i = 0; i < st.size(); ++i) {
        const MixStage& s = st[i];
        const int R = s.radix;
        if (R < 2 || R > 5) { bad("L=%d stage %d: radix %d", L, (int)i, R); return; }
        prod *= R;
        if (s.ns != ns) bad("L=%d stage %d: ns=%d, the earlier radices multiply to %d", L, (int)i, s.ns, ns);
        if (L % (ns * R) != 0 || s.twstep != L / (ns * R)) bad("L=%d stage %d: twiddle step %d", L, (int)i, s.twstep);
        const unsigned magic = (unsigned)s.magic;
        if ((magic == 0) != (ns == 1)) bad("L=%d stage %d: magic=%d with ns=%d", L, (int)i, s.magic, ns);
        const int nb = L / R;
        for (int j = 0; j < nb && magic != 0; ++j) {
            const int q = (int)(((unsigned long long)(unsigned)j * magic) >> 32);
            if (q != j / ns) { bad("L=%d stage %d: umulhi(%d, magic) = %d", L, (int)i, j, q); break; }
        }
        for (int r = 1; r < R; ++r)
            for (int k = 0; k < ns; ++k) {
                const long long m = (long long)r * k * s.twstep;
                if (m >= L || (m >> 6) >= nhi) { bad("L=%d stage %d: twiddle index %d out of the table (r=%d)", L, (int)i, (int)m, r); r = R; break; }
            }
        const int nit = (kMixMaxElems + R - 1) / R;
        if ((long long)nt * nit < nb) bad("L=%d stage %d: %d butterflies for %d threads", L, (int)i, nb, nt);
        ns *= R;
    }
    if (prod != L) bad("L=%d: the radices multiply to %d", L, (int)prod);
    // the table's own values: |w| = 1 to float rounding, lo[0] = hi[0] = 1
    if (tw[0].x != 1.f || tw[0].y != 0.f || tw[kMixTwLo].x != 1.f || tw[kMixTwLo].y != 0.f) bad("L=%d: w^0 is not 1", L);
    for (size_t i = 0; i < tw.size(); ++i) {
        const double n2 = (double)tw[i].x * tw[i].x + (double)tw[i].y * tw[i].y;
        if (!(std::fabs(n2 - 1.0) < 4e-7)) { bad("L=%d: |tw[%d]| is not 1", L, (int)i); break; }
    }
}

void check_pair(int M, int N) {
    const MixLayout l = mixed_layout(M, N);
    const int P = 1 << l.logP;
    if (l.logP < 0 || l.logP > 2 || N % P != 0) bad("%d x %d: logP=%d does not divide N", M, N, l.logP);
    if (l.B < 1 || l.B > 16 || !is_pow2(l.B)) bad("%d x %d: B=%d", M, N, l.B);
    if (l.B * mixed_threads(N) > 1024) bad("%d x %d: row launch of %d threads", M, N, l.B * mixed_threads(N));
    if (P * mixed_threads(M) > 1024) bad("%d x %d: column launch of %d threads", M, N, P * mixed_threads(M));
    if ((size_t)l.B * N * sizeof(MixTwiddle) > kMixMaxLds) bad("%d x %d: row launch LDS with B=%d", M, N, l.B);
    if ((size_t)P * M * sizeof(MixTwiddle) > kMixMaxLds) bad("%d x %d: column launch LDS with P=%d", M, N, P);
}

void dump_length(int L) {
    std::vector<MixTwiddle> tw;
    std::vector<MixStage> st;
    build_mixed_tables(L, tw, st);
    const int nhi = (int)tw.size() - kMixTwLo;
    std::printf("length %d nt %d stages %d hi %d\n", L, mixed_threads(L), (int)st.size(), nhi);
    for (const MixStage& s : st) std::printf("stage %d %d %u %d\n", s.radix, s.ns, (unsigned)s.magic, s.twstep);
    for (int i = 0; i < kMixTwLo; ++i) std::printf("lo %d %.9g %.9g\n", i, tw[i].x, tw[i].y);
    for (int i = 0; i < nhi; ++i) std::printf("hi %d %.9g %.9g\n", i, tw[kMixTwLo + i].x, tw[kMixTwLo + i].y);
}

}  // namespace

int main(int argc, char** argv) {
    const std::vector<int> S = smooth_lengths();
    if (argc >= 2 && std::strcmp(argv[1], "--dump") == 0) {
        std::printf("constants maxelems %d maxlds %d maxlen %d twlo %d ldstarget %d\n", kMixMaxElems, (int)kMixMaxLds, kMixMaxLen, kMixTwLo,
                    (int)kMixLdsTarget);
        for (int L : S) dump_length(L);
        for (int i = 2; i < argc; ++i) {
            int M = 0, N = 0;
            if (std::sscanf(argv[i], "%dx%d", &M, &N) != 2 || !is_smooth(M) || !is_smooth(N) || M > kMixMaxLen || N > kMixMaxLen ||
                (is_pow2(M) && is_pow2(N))) {
                std::fprintf(stderr, "mixed_plan_check: '%s' is not a mixed-radix plan size MxN\n", argv[i]);
                return 2;
            }
            const MixLayout l = mixed_layout(M, N);
            std::printf("layout %d %d %d %d %d %d\n", M, N, l.logP, l.B, mixed_threads(M), mixed_threads(N));
        }
        return 0;
    }
    if (argc != 1) {
        std::fprintf(stderr, "usage: mixed_plan_check [--dump [MxN ...]]\n");
        return 2;
    }
    for (int L : S) check_length(L);
    size_t pairs = 0;
    bool seen[3][17] = {};
    for (int M : S)
        for (int N : S) {
            if (is_pow2(M) && is_pow2(N)) continue;
            check_pair(M, N);
            const MixLayout l = mixed_layout(M, N);
            if (l.logP >= 0 && l.logP <= 2 && l.B >= 1 && l.B <= 16) seen[l.logP][l.B] = true;
            ++pairs;
        }
    int layouts = 0;
    for (auto& row : seen)
        for (bool b : row) layouts += b;
    if (g_bad) {
        std::fprintf(stderr, "mixed_plan_check: %d violation(s)\n", g_bad);
        return 1;
    }
    std::printf("mixed plan ok: %d lengths, %zu pairs, %d (logP, B) layouts\n", (int)S.size(), pairs, layouts);
    return 0;
}
