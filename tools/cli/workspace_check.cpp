// workspace_check -- the layouts of a plan's on-demand device blocks and the handle that grows them (csrc/fdr_workspace.hpp),
// checked without a device.  Built with -fsanitize=address,undefined (Makefile); read by tests/test_workspace_host.py.
//
//   workspace_check CASE ...     CASE = key=value,key=value,...: the plain numbers the layouts take --
//        M N ws (ws_elems) group frames  ta (tvauto_max_partials) rf (2 rlfree_partials + 2) ra (2 rlaccel_partials) rs (the row grid's
//        workgroups) rg (the doubles of the curve partials) mo (motion_pad_partials) noise (kRegMaxPartials + 1) maxgroup psf (kBlindMaxPsf)
//        curve (kRegMaxCurve) angles diameters (the defocus limits) trace table trig (entries of the buffers that grow alone)
//
//   workspace_check register:CASE ...   the block of the frame registration alone, from its own numbers: M N rc (register_cross_partials)
//        rp (register_peak_partials) frames (FDR_MAX_FRAMES)
//
// First the handle's failure branch on a host allocator that fails on request (exit 1 unless: a failed grow leaves block, count,
// size and pointers as they were and frees nothing; a satisfied count allocates nothing; a grow has the new block before it lets the
// old one go; free_with leaves an empty handle).  Then per case and workspace, each grown through Workspace::grow on the host
// allocator and then walked by a printing carver over the very block, which checks every placed pointer against its own offset:
//   case CASE
//   workspace NAME bytes TOTAL count COUNT
//   member NAME offset OFFSET bytes BYTES align ALIGN      (in layout order)
#include "../../parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd/csrc/fdr_workspace.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

using namespace fdr;

namespace {

struct Complex { float x, y; };  // the layout of a float2

int g_bad = 0;
void expect(bool ok, const char* what) {
    if (!ok) { ++g_bad; std::fprintf(stderr, "workspace_check: %s\n", what); }
}

// the host stand-in for hipMalloc / hipFree: 256-byte aligned blocks, a failure on request, a log of what was called
struct HostAllocator {
    bool fail_next = false;
    std::string log;  // 'a' per block handed out, 'f' per block freed, 'x' per refused request
    void* alloc(size_t bytes) {
        if (fail_next) { fail_next = false; log += 'x'; return nullptr; }
        log += 'a';
        return std::aligned_alloc(256, (bytes + 255) / 256 * 256);
    }
    void release(void* b) { log += 'f'; std::free(b); }
};

// the printing carver: the members of fdr::Carver, on a placed block
struct Printer {
    char* base;
    size_t at = 0;
    bool aligned = true;
    template <class T> void put(const char* name, T*& member, size_t n, size_t align) {
        expect(reinterpret_cast<char*>(member) == base + at, "a placed pointer is not at its offset");
        line(name, n * sizeof(T), align);
    }
    template <class T> void room(const char* name, size_t n, size_t align) { line(name, n * sizeof(T), align); }
    void pad(size_t align) { at = (at + align - 1) / align * align; }
    void line(const char* name, size_t bytes, size_t align) {
        aligned = aligned && at % align == 0;
        std::printf("member %s offset %zu bytes %zu align %zu\n", name, at, bytes, align);
        at += bytes;
    }
};

template <class Layout>
void show(const char* name, int count, Layout&& layout) {
    HostAllocator host;
    Workspace ws;
    const auto alloc = [&](size_t b) { return host.alloc(b); };
    const auto release = [&](void* b) { host.release(b); };
    expect(ws.grow(count, layout, alloc, release) == Workspace::MADE, "grow did not make the block");
    std::printf("workspace %s bytes %zu count %d\n", name, ws.bytes, ws.count);
    Printer pr{static_cast<char*>(ws.block)};
    layout(pr, count);
    expect(pr.at == ws.bytes && pr.aligned, "the printed layout does not end at the measured size, or misses an alignment");
    ws.free_with(release);
    expect(host.log == "af", "one block made, one block freed");
}

void check_handle() {
    HostAllocator host;
    const auto alloc = [&](size_t b) { return host.alloc(b); };
    const auto release = [&](void* b) { host.release(b); };
    Workspace ws;
    RlAccelLayout m;
    const auto lay = [&](auto& c, int g) { layout(c, m, 256, 2, 8, g); };
    expect(ws.grow(2, lay, alloc, release) == Workspace::MADE && host.log == "a" && ws.count == 2 && m.y == ws.block, "first grow");
    const Workspace was = ws;
    const RlAccelLayout had = m;
    const auto same = [&] {
        return ws.block == was.block && ws.bytes == was.bytes && ws.count == was.count && m.y == had.y && m.u == had.u && m.g == had.g &&
               m.part == had.part && m.alpha == had.alpha && m.more == had.more;
    };
    expect(ws.grow(2, lay, alloc, release) == Workspace::KEPT && ws.grow(1, lay, alloc, release) == Workspace::KEPT && host.log == "a" && same(),
           "a satisfied count allocates nothing and changes nothing");
    host.fail_next = true;
    expect(ws.grow(3, lay, alloc, release) == Workspace::NO_MEMORY && host.log == "ax" && same(), "a failed grow leaves the handle and the pointers as they were");
    m.y[0] = 1.f; m.more[3 * 256 - 1] = 2.f; m.alpha[7] = 3.f;  // (the old block is still the handle's: the sanitizer would tell)
    expect(ws.grow(3, lay, alloc, release) == Workspace::MADE && host.log == "axaf" && ws.count == 3 && !same(), "a grow has the new block before it frees the old one");
    Carver measure;
    lay(measure, 3);
    expect(ws.bytes == measure.at && m.more + 6 * 256 == static_cast<float*>(ws.block) + ws.bytes / sizeof(float), "the placed block ends at the measured size");
    const auto crooked = [&](auto& c, int) { float* f = nullptr; double* d = nullptr; c.put("f", f, 1, 4); c.put("d", d, 1, 8); };
    Workspace none;
    expect(none.grow(1, crooked, alloc, release) == Workspace::BAD_LAYOUT && host.log == "axaf" && !none.block, "a member off its stated alignment is refused before any block is made");
    ws.free_with(release);
    expect(host.log == "axaff" && !ws.block && ws.bytes == 0 && ws.count == 0, "free_with leaves an empty handle");
    ws.free_with(release);
    expect(host.log == "axaff", "an empty handle frees nothing");
}

}  // namespace

int main(int argc, char** argv) {
    check_handle();
    for (int i = 1; i < argc; ++i) {
        std::map<std::string, size_t> v;
        const std::string whole = argv[i];
        const bool regist = whole.rfind("register:", 0) == 0;
        const std::string arg = regist ? whole.substr(9) : whole;
        for (size_t a = 0; a < arg.size();) {
            const size_t e = arg.find('=', a), b = arg.find(',', a) == std::string::npos ? arg.size() : arg.find(',', a);
            if (e == std::string::npos || e > b) { std::fprintf(stderr, "workspace_check: bad case %s\n", argv[i]); return 2; }
            v[arg.substr(a, e - a)] = std::strtoull(arg.c_str() + e + 1, nullptr, 10);
            a = b + 1;
        }
        if (regist) {
            if (v.size() != 5) { std::fprintf(stderr, "workspace_check: case %s does not give the 5 numbers\n", argv[i]); return 2; }
            std::printf("case %s\n", argv[i]);
            RegisterLayout<Complex> rg;
            show("register", 1, [&](auto& c, int) { layout(c, rg, v["M"], v["N"], v["rc"], v["rp"], v["frames"]); });
            continue;
        }
        if (v.size() != 20) { std::fprintf(stderr, "workspace_check: case %s does not give the 20 numbers\n", argv[i]); return 2; }
        const size_t M = v["M"], N = v["N"], P = M * N, ws = v["ws"], noise = v["noise"];
        const int group = (int)v["group"], frames = (int)v["frames"];
        std::printf("case %s\n", argv[i]);
        TvLayout<Complex> tv;
        show("tv", group, [&](auto& c, int g) { layout(c, tv, P, ws, g); });
        TvFreeLayout tvfree;
        show("tvfree", group, [&](auto& c, int g) { layout(c, tvfree, P, g); });
        TvAutoLayout tvauto;
        show("tvauto", group, [&](auto& c, int g) { layout(c, tvauto, v["ta"], noise, g); });
        TvFramesLayout<Complex> tvframes;
        show("tvframes", frames, [&](auto& c, int n) { layout(c, tvframes, P, ws, n); });
        RlFreeLayout rlfree;
        show("rlfree", group, [&](auto& c, int g) { layout(c, rlfree, P, v["rf"], g); });
        RlAccelLayout rlaccel;
        show("rlaccel", group, [&](auto& c, int g) { layout(c, rlaccel, P, v["ra"], (int)v["maxgroup"], g); });
        RlTvLayout rltv;
        show("rltv", group, [&](auto& c, int g) { layout(c, rltv, P, g); });
        RlStopLayout rlstop;
        show("rlstop", 1, [&](auto& c, int) { layout(c, rlstop, v["rs"], noise); });
        FramesLayout<Complex> fr;
        show("frames", frames, [&](auto& c, int n) { layout(c, fr, P, ws, v["rf"], n); });
        BlindLayout<Complex> blind;
        show("blind", 1, [&](auto& c, int) { layout(c, blind, ws, v["psf"]); });
        RegLayout reg;
        show("reg", 1, [&](auto& c, int) { layout(c, reg, ws, v["rg"], noise, v["curve"]); });
        MotionLayout<Complex> motion;
        show("motion", 1, [&](auto& c, int) { layout(c, motion, M, N, v["mo"]); });
        DefocusLayout defocus;
        show("defocus", 1, [&](auto& c, int) { layout(c, defocus, v["angles"], v["diameters"]); });
        // the buffers that grow alone, as their ensure_* calls lay them out
        Complex* tables = nullptr;
        show("frames.tables", frames, [&](auto& c, int n) { layout(c, tables, 2 * (size_t)n * ws, 16); });
        double* trace = nullptr;
        show("rlstop.trace", (int)v["trace"], [&](auto& c, int n) { layout(c, trace, 2 * (size_t)n, 8); });
        float* planes = nullptr;
        show("rlstop.planes", 1, [&](auto& c, int) { layout(c, planes, 2 * P, 16); });
        float* w = nullptr;
        show("blind.w", 1, [&](auto& c, int) { layout(c, w, P, 16); });
        float* table = nullptr;
        show("motion.table", (int)v["table"], [&](auto& c, int n) { layout(c, table, (size_t)n, 4); });
        double* trig = nullptr;
        show("motion.trig", (int)v["trig"], [&](auto& c, int n) { layout(c, trig, (size_t)n, 8); });
    }
    if (g_bad) return 1;
    std::printf("workspace check ok: %d cases\n", argc - 1);
    return 0;
}
