#!/usr/bin/env python3
"""Are the gfx950 kernels of the working tree the ones a git revision had?

usage: tools/kernel_diff.py <git-rev> [--rename REGEX TEMPLATE]... [--jobs N] [--keep DIR] [EXTRA flags, e.g. -DFDR_DEBUG_JITTER]

Exports csrc/ (with the Makefile and include/) of <git-rev> into a temporary directory, compiles every kernel unit (a csrc/*.hip
file with a __global__ in it) of that tree and of the working tree to device assembly with the flags of the package Makefile
(HIPFLAGS, EXTRA = the extra flags), cuts the text into kernels and compares, kernel by kernel, the instruction stream and the
.amdhsa_* descriptor lines (registers, LDS, scratch, occupancy hints).  Comments, .LBB<n>_ label numbers and the kernel's own
symbol (also inside the names of its LDS arrays) are normalised away, so a kernel may move to another file or another place in
its file.  Kernels are matched by demangled name; which file a kernel lives in does not matter.

Prints the counts `identical / different / only-old / only-new`, names the offenders, and exits non-zero unless every old
kernel has exactly one identical counterpart and nothing is new.  For a kernel that differs, the first differing line is shown;
--keep DIR leaves both trees' assembly in DIR (asm_old/, asm_new/) for a closer look.  Needs hipcc, make, git and c++filt; never a GPU.

--rename REGEX TEMPLATE rewrites the OLD demangled names before matching (re.sub; afterwards `{a+b}` with integer a, b is
replaced by the sum), for changes that respell a kernel's name and nothing else.  The worked example: the inverse row
kernels were templated on `int OUT` 0..6 and are now templated on the RowOut enumerator itself (1..7), so

    tools/kernel_diff.py HEAD~1 --rename '(fft_rows4_inv_\\w+_kernel<.*), (\\d)>' '\\1, (fdr::RowOut){\\2+1}>'

matches old `fdr::fft_rows4_inv_packed_kernel<12, true, 2>` with new `fdr::fft_rows4_inv_packed_kernel<12, true, (fdr::RowOut)3>`.
"""
import argparse, concurrent.futures, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "parallel-implementation-of-frequency-domain-image-restoration-using-fft_amd"


def hipcc_and_flags(pkg_dir, extra):
    """HIPCC and HIPFLAGS as the Makefile of that tree expands them."""
    rule = "kernel-diff-print: ; @echo $(HIPCC) ; echo $(HIPFLAGS)"
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", pkg_dir, "--eval", rule, "kernel-diff-print", "EXTRA=" + " ".join(extra)],
                         check=True, capture_output=True, text=True).stdout.splitlines()
    return out[0].strip(), out[1].split()


def kernel_units(pkg_dir):
    d = os.path.join(pkg_dir, "csrc")
    return sorted(n for n in os.listdir(d) if n.endswith(".hip") and "__global__" in open(os.path.join(d, n)).read())


def compile_unit(hipcc, flags, pkg_dir, unit, out_dir):
    out = os.path.join(out_dir, unit[:-4] + ".s")
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(pkg_dir, "csrc", unit), "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("%s: compile failed\n%s" % (os.path.join(pkg_dir, "csrc", unit), r.stderr[-4000:]))
    return unit, open(out).read()


def kernels_of(asm):
    """{symbol: normalised text} of one unit's assembly: the body label .. .Lfunc_end, then the .amdhsa_ lines of its descriptor."""
    found = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.S | re.M):
        sym, desc = m.group(1), m.group(2)
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), asm, re.S | re.M)
        if body is None:
            sys.exit("no body found for kernel " + sym)
        lines = []
        for line in (body.group(1) + desc).splitlines():
            line = line.split(";", 1)[0].strip()  # comments: register statistics, `; %bb.0:`, encodings
            if not line:
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            line = re.sub(r"\.L(tmp|func_begin|func_end)\d+", r".L\1", line)
            lines.append(line.replace(sym[2:], "@K"))  # the kernel's own symbol, and `_ZZ<kernel>E3lds` of its LDS arrays
        found[sym] = "\n".join(lines)
    return found


def collect(pkg_dir, extra, jobs, tmp, tag):
    hipcc, flags = hipcc_and_flags(pkg_dir, extra)
    out_dir = os.path.join(tmp, "asm_" + tag)
    os.makedirs(out_dir)
    units = kernel_units(pkg_dir)
    kernels = {}  # symbol -> (unit, text)
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
        for unit, asm in pool.map(lambda u: compile_unit(hipcc, flags, pkg_dir, u, out_dir), units):
            for sym, text in kernels_of(asm).items():
                kernels[sym] = (unit, text)
    syms = sorted(kernels)
    names = subprocess.run(["c++filt"], input="\n".join(syms) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    by_name = {}
    for sym, name in zip(syms, names):
        depth, i = 0, len(name)  # template-id only: cut the parameter list (the last top-level parenthesis) and the return type
        while i > 0:
            i -= 1
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                break
        name = re.sub(r"^void ", "", name[:i] if i > 0 else name)
        by_name.setdefault(name, []).append(kernels[sym])
    return by_name, len(units)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], usage=__doc__.split("\n\n")[1][len("usage: "):])
    ap.add_argument("rev")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "TEMPLATE"))
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--keep", metavar="DIR")
    args, extra = ap.parse_known_args()
    jobs = max(1, min(16, args.jobs))

    def renamed(name):
        for rx, tmpl in args.rename:
            name = re.sub(rx, tmpl, name)
        return re.sub(r"\{(-?\d+)\+(-?\d+)\}", lambda m: str(int(m.group(1)) + int(m.group(2))), name)

    with tempfile.TemporaryDirectory(prefix="kernel_diff_") as tmp:
        if args.keep:
            tmp = os.path.abspath(args.keep)
            os.makedirs(tmp)  # (a fresh directory: nothing of an earlier run is mixed in)
        old_root = os.path.join(tmp, "old")
        os.makedirs(old_root)
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.rev, PKG + "/csrc", PKG + "/Makefile", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old_root], input=tar, check=True)
        old, n_old = collect(os.path.join(old_root, PKG), extra, jobs, tmp, "old")
        new, n_new = collect(os.path.join(ROOT, PKG), extra, jobs, tmp, "new")

    identical, different, only_old = [], [], []
    used = set()
    for name, olds in sorted(old.items()):
        target = renamed(name)
        news = new.get(target, [])
        if len(olds) != 1 or len(news) != 1:
            (only_old if not news else different).append("%s [%d old, %d new of that name]" % (name, len(olds), len(news)))
        elif olds[0][1] == news[0][1]:
            identical.append(name)
        else:
            a, b = olds[0][1].splitlines(), news[0][1].splitlines()
            k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            different.append("%s (%s -> %s), %d / %d lines, line %d: `%s` / `%s`" % (name, olds[0][0], news[0][0], len(a), len(b), k + 1,
                                                                                    " ".join(a[k:k + 1]), " ".join(b[k:k + 1])))
        used.add(target)
    only_new = ["%s (%s)" % (n, new[n][0][0]) for n in sorted(new) if n not in used]

    for title, items in (("different", different), ("only-old", only_old), ("only-new", only_new)):
        for it in items:
            print("%s: %s" % (title, it))
    print("kernel_diff %s%s: %d old units, %d new units: %d identical / %d different / %d only-old / %d only-new"
          % (args.rev, " " + " ".join(extra) if extra else "", n_old, n_new, len(identical), len(different), len(only_old), len(only_new)))
    return 0 if not (different or only_old or only_new) else 1


if __name__ == "__main__":
    sys.exit(main())
