"""The layouts of a plan's on-demand device blocks (csrc/fdr_workspace.hpp), checked without a GPU: tools/cli/workspace_check (the
header behind its own main, under the address and undefined-behaviour sanitizers) first drives the failure branch of the handle on
a host allocator, then grows every workspace for the cases below and prints each total and each member's offset, size and stated
alignment.  Every number is compared here with the arithmetic the hand-written ensure_* functions had before there was a shared
layout, written out again in `expected` from those functions and from the size formulas of include/fdr.h -- not taken from the
header.  The checks are pinned by faults injected into a copy of the parsed dump."""
import copy
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the library's limits (csrc/fdr_kernels.hpp, fdr_api_reg.hip, fdr_api_defocus.hip, fdr_api_rlstop.hip)
MAX_GROUP, NOISE, MAX_PSF, MAX_CURVE, CANDIDATES, MAX_ANGLES, MAX_DIAMETERS, TRACE_STEPS = 8, 1024 + 1, 65536, 4096, 16, 4096, 4096, 1024

# 16 x 16: the smallest P, where "a multiple of 16 because P >= 256" is tightest; the long and the tall plan; 1024^2; a non-square one
SHAPES = [(16, 16), (16, 2048), (2048, 16), (1024, 1024), (256, 512)]
COUNTS = [(1, 1), (2, 2), (3, 8), (8, 2)]  # (images of a group, frames): groups 1, 2, 3, 8 and frames 1, 2, 8


def ceil_div(a, b):
    return -(-a // b)


def numbers(M, N, group, frames):
    """the plain numbers a half-spectrum plan hands to the layouts: ws_elems with its panel padding (N / 8 panels of 4 M + 16) and
    the partial counts of the kernels' own functions"""
    npanels = N // 8
    return dict(M=M, N=N, ws=npanels * (4 * M + 16), group=group, frames=frames,
                ta=ceil_div(N, 1024) * ceil_div(M, 4),                          # tvauto_max_partials
                rf=2 * M * ceil_div(N, 1024) + 2,                               # 2 rlfree_partials + 2
                ra=2 * ceil_div(M, 8) * ceil_div(N, 1024),                      # 2 rlaccel_partials
                rs=M // 4,                                                      # workgroups of the inverse row grid, at most
                rg=min(ceil_div(npanels * M, 256), 1024) * 2 * CANDIDATES,      # reg_curve_partials * 2 kRegCandidates
                mo=M * ceil_div(N, 1024),                                       # motion_pad_partials
                noise=NOISE, maxgroup=MAX_GROUP, psf=MAX_PSF, curve=MAX_CURVE, angles=MAX_ANGLES, diameters=MAX_DIAMETERS,
                trace=max(TRACE_STEPS, 300 * frames), table=360 * (7 + group), trig=2 * 360)


def up(b):
    return (b + 255) & ~255


def expected(v):
    """{workspace: (total bytes, [(member, offset, bytes)])} as the ensure_* functions carved them by hand"""
    P, ws, g, K, F, D = v["M"] * v["N"], v["ws"], v["group"], v["frames"], 4, 8
    out = {}

    def seq(name, members, total):
        out[name] = (total, members)

    t = up(ws * 8)  # ensure_tv_workspace: t_bytes, then group * 6 planes
    seq("tv", [("T", 0, ws * 8)] + [(n, t + i * P * F, P * F) for i, n in enumerate(("x", "b", "w00", "w01", "w10", "w11"))] +
        [("rest", t + 6 * P * F, (g - 1) * 6 * P * F)], t + g * 6 * P * F)
    seq("tvfree", [("q", 0, g * P * F), ("c", g * P * F, g * P * F)], g * 2 * P * F)
    n_part = g * 3 * v["ta"]
    doubles = n_part + 4 * g + v["noise"]
    seq("tvauto", [("part", 0, n_part * D), ("stat", n_part * D, 4 * g * D), ("noise", (n_part + 4 * g) * D, v["noise"] * D),
                   ("mu", doubles * D, g * F)], doubles * D + g * F)
    seq("tvframes", [("acc", 0, ws * 8), ("q", t, K * P * F), ("c", t + K * P * F, K * P * F)], t + 2 * K * P * F)
    planes = 1 + 2 * g
    seq("rlfree", [("u", 0, P * F), ("wgt", P * F, P * F), ("dw", 2 * P * F, P * F), ("rest", 3 * P * F, 2 * (g - 1) * P * F),
                   ("part", planes * P * F, g * v["rf"] * D)], planes * P * F + g * v["rf"] * D)
    alpha_bytes = 8 if g == 1 else F * MAX_GROUP
    a0 = 3 * P * F + g * v["ra"] * D
    seq("rlaccel", [("y", 0, P * F), ("u", P * F, P * F), ("g", 2 * P * F, P * F), ("part", 3 * P * F, g * v["ra"] * D), ("alpha", a0, alpha_bytes),
                    ("more", a0 + alpha_bytes, 3 * (g - 1) * P * F)], g * (3 * P * F + v["ra"] * D) + alpha_bytes)
    seq("rltv", [("f", 0, g * P * F), ("u", g * P * F, g * P * F)], 2 * g * P * F)
    seq("rlstop", [("part", 0, v["rs"] * 2 * D), ("noise", v["rs"] * 2 * D, v["noise"] * D)], (v["rs"] * 2 + v["noise"]) * D)
    fr = [("acc", 0, ws * 8), ("u", ws * 8, P * F), ("wgt", ws * 8 + P * F, P * F), ("dw", ws * 8 + 2 * P * F, K * P * F)]
    fp = ws * 8 + (2 + K) * P * F
    seq("frames", fr + [("part", fp, K * v["rf"] * D), ("sums", fp + K * v["rf"] * D, 2 * D)], fp + (K * v["rf"] + 2) * D)
    table, psf = ws * 8, v["psf"] * F
    seq("blind", [("table", 0, table)] + [(n, table + i * psf, psf) for i, n in enumerate(("p", "num", "den", "stage"))] +
        [("status", table + 4 * psf, 4)], table + 4 * psf + 4)
    power, part, noise, pairs = up((ws + 2) * F), up(v["rg"] * D), up(v["noise"] * D), up(v["curve"] * 2 * D)
    seq("reg", [("power", 0, (ws + 2) * F), ("part", power, v["rg"] * D), ("noise", power + part, v["noise"] * D),
                ("cand", power + part + noise, v["curve"] * 2 * D), ("res", power + part + noise + pairs, v["curve"] * 2 * D)],
        power + part + noise + 2 * pairs)
    plane, mpart, hann = P * 8, (v["mo"] + 1) * D, (v["M"] + v["N"]) * F
    seq("motion", [("plane", 0, plane), ("part", plane, mpart), ("hann", plane + mpart, hann)], plane + mpart + hann)
    seq("defocus", [("trig", 0, 2 * v["angles"] * D), ("profile", 2 * v["angles"] * D, v["diameters"] * F)], 2 * v["angles"] * D + v["diameters"] * F)
    for name, nbytes in (("frames.tables", 2 * K * ws * 8), ("rlstop.trace", v["trace"] * 2 * D), ("rlstop.planes", 2 * P * F), ("blind.w", P * F),
                         ("motion.table", v["table"] * F), ("motion.trig", v["trig"] * D)):
        seq(name, [("array", 0, nbytes)], nbytes)
    return out


def single_image_totals(v):
    """the block the single-image calls have always had, from the sentences of include/fdr.h (M, N and the documented counts alone)"""
    M, N, MN = v["M"], v["N"], v["M"] * v["N"]
    filter_bytes = v["ws"] * 8  # fdr_plan_filter_bytes
    return {
        "tv": up(filter_bytes) + 24 * MN,                                      # the table and six M x N float planes
        "tvfree": 8 * MN,                                                      # two M x N planes
        "rlfree": 12 * MN + 8 * (2 * M * ceil_div(N, 1024) + 2),               # 12 M N bytes and the partials of the two sums
        "rlaccel": 12 * MN + 16 * ceil_div(M, 8) * ceil_div(N, 1024) + 8,      # 12 M N + 16 ceil(M / 8) ceil(N / 1024) + 8 bytes
        "rltv": 8 * MN,                                                        # 8 M N bytes
        "rlstop": 16 * v["rs"] + 8 * NOISE,                                    # 16 bytes per workgroup of the inverse row pass, the noise partials
    }


# the alignments the kernels and the hand-written comments relied on: the planes a launch picks its vector width from and the
# accumulators of the sum kernel on 16 bytes, doubles on 8, the 256-byte sections of the TV, multi-frame TV and regularisation blocks
NEEDS = {("tv", "x"): 256, ("tvframes", "acc"): 16, ("tvframes", "q"): 256, ("frames", "acc"): 16, ("frames.tables", "array"): 16,
         ("rlaccel", "part"): 16, ("rlfree", "part"): 8, ("frames", "part"): 8, ("reg", "part"): 256, ("reg", "noise"): 256,
         ("reg", "cand"): 256, ("reg", "res"): 256}
for _ws, _names in (("tv", ("b", "w00", "w01", "w10", "w11", "rest")), ("tvfree", "qc"), ("rlfree", ("u", "wgt", "dw", "rest")), ("rlaccel", "yug"),
                    ("rltv", "fu"), ("tvframes", "c"), ("rlstop.planes", ("array",)), ("blind.w", ("array",))):
    for _n in _names:
        NEEDS[(_ws, _n)] = 16


def exe():
    d = os.path.join(ROOT, "tools", "cli")
    subprocess.check_call(["make", "-C", d, "-s", "workspace_check"])
    return os.path.join(d, "workspace_check")


def parse(text):
    """{case: {workspace: {"total", "count", "members": [(name, offset, bytes, align)]}}}"""
    cases, cur, ws = {}, None, None
    for line in text.splitlines():
        f = line.split()
        if f[:3] == ["workspace", "check", "ok:"]:
            continue
        if f[0] == "case":
            cur = cases.setdefault(f[1], {})
        elif f[0] == "workspace":
            ws = cur[f[1]] = {"total": int(f[3]), "count": int(f[5]), "members": []}
        elif f[0] == "member":
            ws["members"].append((f[1], int(f[3]), int(f[5]), int(f[7])))
        else:
            raise AssertionError(line)
    return cases


def case_key(v):
    return ",".join("%s=%d" % kv for kv in v.items())


@pytest.fixture(scope="module")
def dump():
    cases = [numbers(M, N, g, K) for M, N in SHAPES for g, K in COUNTS]
    r = subprocess.run([exe()] + [case_key(v) for v in cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "workspace check ok: %d cases" % len(cases) in r.stdout, (r.returncode, r.stdout[-800:], r.stderr[-2000:])
    parsed = parse(r.stdout)
    assert len(parsed) == len(cases)
    return [(v, parsed[case_key(v)]) for v in cases]


def violations(v, got):
    """what is wrong with one case of the dump: a list of messages (empty: sound, and byte for byte the hand-carved blocks)"""
    bad, want = [], expected(v)
    if sorted(got) != sorted(want):
        return ["workspaces %s" % sorted(set(got) ^ set(want))]
    for name, (total, members) in want.items():
        w, at = got[name], 0
        for m, off, nbytes, align in w["members"]:
            if off < at:
                bad.append("%s.%s: starts at %d, inside the member before it (ends at %d)" % (name, m, off, at))
            if off % align or align & (align - 1):
                bad.append("%s.%s: offset %d misses its stated alignment %d" % (name, m, off, align))
            if off % NEEDS.get((name, m), 1) or align < NEEDS.get((name, m), 1) and nbytes:
                bad.append("%s.%s: offset %d, stated alignment %d, needs %d" % (name, m, off, align, NEEDS[(name, m)]))
            at = off + nbytes
        pad = 256 if name in ("reg",) else 1
        if -(-at // pad) * pad != w["total"]:
            bad.append("%s: the last member ends at %d, the block at %d" % (name, at, w["total"]))
        if w["total"] != total:
            bad.append("%s: %d bytes, were %d" % (name, w["total"], total))
        if [m[:3] for m in w["members"]] != members:
            diff = [(a, b) for a, b in zip([m[:3] for m in w["members"]], members) if a != b]
            bad.append("%s: members differ, first %s" % (name, diff[:1] or "in number"))
    return bad


def test_every_layout_is_the_hand_carved_one(dump):
    assert len(dump) == len(SHAPES) * len(COUNTS)
    bad = ["%dx%d g=%d K=%d: %s" % (v["M"], v["N"], v["group"], v["frames"], m) for v, got in dump for m in violations(v, got)]
    assert not bad, "\n".join(bad[:40])


def test_one_image_is_the_block_the_single_calls_had(dump):
    seen = 0
    for v, got in dump:
        if v["group"] != 1:
            continue
        seen += 1
        for name, total in single_image_totals(v).items():
            assert got[name]["total"] == total and got[name]["count"] == 1, (v["M"], v["N"], name, got[name]["total"], total)
        # no room for further images, and image 0's members where a group's are
        assert [m for m in got["tv"]["members"] if m[0] == "rest"][0][2] == 0 and got["rlaccel"]["members"][-1][2] == 0
        grown = [g for w, g in dump if (w["M"], w["N"], w["group"]) == (v["M"], v["N"], 8)][0]
        for name in ("tv", "rlfree", "rlaccel"):
            first = [m[:3] for m in got[name]["members"] if m[0] not in ("rest", "more", "part", "alpha")]
            assert first == [m[:3] for m in grown[name]["members"]][:len(first)], name
    assert seen == len(SHAPES)


def test_injected_faults_are_reported(dump):
    for v, got in (dump[0], dump[14]):
        assert not violations(v, got)
        for name in ("tv", "rlaccel", "frames", "reg"):
            f = copy.deepcopy(got)
            m = f[name]["members"][2]
            f[name]["members"][2] = (m[0], m[1] + 4, m[2], m[3])
            assert violations(v, f), (name, "offset off by 4")
            f = copy.deepcopy(got)
            a, b = f[name]["members"][1], f[name]["members"][2]
            f[name]["members"][1], f[name]["members"][2] = (b[0], a[1], b[2], b[3]), (a[0], a[1] + b[2], a[2], a[3])
            assert violations(v, f), (name, "members 1 and 2 swapped")
            f = copy.deepcopy(got)
            f[name]["total"] -= 8
            assert violations(v, f), (name, "total short by 8")
