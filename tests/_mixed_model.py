"""float64 numpy model of the optimal-size operator (fft_serial::wienerDeblur_myfft padded to M x N): the yardstick of the
mixed-radix fast path at sizes where the naive-DFT oracle is too slow.  Pinned against oracle.wiener in
test_mixed_radix_host.py before it judges the GPU.

Below it, what the sweep of every mixed-radix length shares between test_mixed_plan_host.py and test_mixed_lengths_gpu.py:
the plan list and its layouts (read from tools/cli/mixed_plan_check, not restated), the per-line error metric, and the
float64 replay of a dumped stage list."""
import numpy as np


def wiener_raw(img, psf, K, M, N):
    """The raw M x N plane before normalisation: pad image and PSF top-left to M x N, W = conj(H) / (|H|^2 + K), real part
    of the inverse transform (taken as the inverse of the Hermitian half spectrum)."""
    img = np.asarray(img, dtype=np.float64)
    psf = np.asarray(psf, dtype=np.float64)
    f = np.zeros((M, N))
    f[:img.shape[0], :img.shape[1]] = img
    h = np.zeros((M, N))
    h[:psf.shape[0], :psf.shape[1]] = psf
    G = np.fft.rfft2(f)
    H = np.fft.rfft2(h)
    W = np.conj(H) / (np.abs(H) ** 2 + K)
    return np.fft.irfft2(G * W, s=(M, N))


def wiener_model(img, psf, K, M, N, norm_cropped=True):
    """wiener_raw, crop, min-max normalise over the cropped rows x cols (norm_cropped) or over the padded M x N area."""
    rows, cols = np.shape(img)
    raw = wiener_raw(img, psf, K, M, N)
    area = raw[:rows, :cols] if norm_cropped else raw
    lo, hi = area.min(), area.max()
    out = raw[:rows, :cols]
    return (out - lo) / (hi - lo) if hi > lo else np.zeros_like(out)


def smooth(n):
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


def optimal_size(n):
    m = max(n, 1)
    while not smooth(m):
        m += 1
    return m


# ---- the sweep of every mixed-radix length and layout (test_mixed_lengths_gpu.py, pinned in test_mixed_plan_host.py) ------
# Thresholds of the complex-to-complex sweep against numpy's complex128 transform: LINE_TOL bounds the relative L2 error of
# every single row and column of the result, PEAK_TOL the largest |got - want| over the plane divided by rms(want).  See the
# docstring of test_mixed_lengths_gpu.py for the measured maxima they come from (at most 4x, and never above the 1e-5 of the
# whole-plane check they sharpen).
LINE_TOL = 2.5e-6
PEAK_TOL = 3.5e-6
MAX_LEN = 8192
ROW_PARTNER = 45               # plans (45, L): odd M, so the last real pair is half empty and M is no multiple of 2 B
COL_PARTNERS = (12, 6, 15)     # plans (L, n): P = 4, 2 and 1 where the plan's limits allow
ROLES = (("row", ROW_PARTNER),) + tuple(("col", n) for n in COL_PARTNERS)
NBANDS = 6
# windows and stale spectra: every B (N <= 624: 16, <= 1248: 8, <= 2496: 4, <= 4992: 2, above: 1) and every P, chosen both by
# N (odd: 1, 2 mod 4: 2) and by M (above 2496: 2, above 4992: 1)
WINDOW_PLANS = [(45, 300), (50, 750), (45, 1875), (50, 3000), (45, 6250), (50, 5625), (2700, 1200), (2700, 300), (5000, 300)]
# the CLS filter's column index n0 + c: logP 0, 1, 2 by N with M odd and even, logP 1 and 0 by M
CLS_PLANS = [(45, 75), (50, 75), (45, 750), (50, 750), (45, 300), (50, 300), (2700, 60), (5000, 60)]


def smooth_lengths():
    """the 167 lengths 2^a 3^b 5^c in 1 .. 8192"""
    return [n for n in range(1, MAX_LEN + 1) if smooth(n)]


def bands():
    """smooth_lengths() cut into NBANDS runs of about the same total length (so of about the same work)"""
    S = smooth_lengths()
    total, out, acc = float(sum(S)), [[] for _ in range(NBANDS)], 0
    for L in S:
        out[min(int(acc * NBANDS / total), NBANDS - 1)].append(L)
        acc += L
    return out


def sweep_plans():
    """(role, partner, L, M, N) of all 4 x 167 plans: L as the row length of (45, L), as the column length of (L, 12 / 6 / 15)"""
    return [(role, n, L) + ((n, L) if role == "row" else (L, n)) for role, n in ROLES for L in smooth_lengths()]


def plan_check_exe():
    """tools/cli/mixed_plan_check, built as test_host.py builds cv_shim_test"""
    import os
    import subprocess
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "cli")
    subprocess.check_call(["make", "-C", d, "-s", "mixed_plan_check"])
    return os.path.join(d, "mixed_plan_check")


_dumps = {}


def plan_dump(pairs=()):
    """(lengths, layouts) from `mixed_plan_check --dump MxN ...`: lengths[L] = {"nt", "stages": [(R, ns, magic, step)], "lo",
    "hi": complex128 arrays holding the float32 table entries}, layouts[(M, N)] = (logP, B, nt(M), nt(N))"""
    import subprocess
    pairs = tuple(pairs)
    if pairs not in _dumps:
        out = subprocess.run([plan_check_exe(), "--dump"] + ["%dx%d" % p for p in pairs], capture_output=True, text=True, check=True).stdout
        _dumps[pairs] = parse_dump(out)
    return _dumps[pairs]


def parse_dump(text):
    lengths, layouts, cur = {}, {}, None
    for line in text.splitlines():
        f = line.split()
        if f[0] == "length":
            cur = {"L": int(f[1]), "nt": int(f[3]), "nst": int(f[5]), "nhi": int(f[7]), "stages": [], "lo": [], "hi": []}
            lengths[cur["L"]] = cur
        elif f[0] == "stage":
            cur["stages"].append(tuple(int(v) for v in f[1:5]))
        elif f[0] in ("lo", "hi"):
            assert int(f[1]) == len(cur[f[0]])
            cur[f[0]].append(complex(float(f[2]), float(f[3])))
        elif f[0] == "layout":
            layouts[(int(f[1]), int(f[2]))] = tuple(int(v) for v in f[3:7])
        else:
            assert f[0] == "constants", line
    for e in lengths.values():
        e["lo"] = np.array(e["lo"], dtype=np.complex128)
        e["hi"] = np.array(e["hi"], dtype=np.complex128)
    return lengths, layouts


def sweep_cases():
    """sweep_plans() with the layout mixed_plan_check gives each plan, less the plans whose (L, role, logP, B) another plan
    has already: dicts role, partner, L, M, N, logP, B"""
    plans = sweep_plans()
    _, layouts = plan_dump(tuple(sorted({(M, N) for _, _, _, M, N in plans})))
    seen, out = set(), []
    for role, n, L, M, N in plans:
        logP, B = layouts[(M, N)][:2]
        if (L, role, logP, B) not in seen:
            seen.add((L, role, logP, B))
            out.append({"role": role, "partner": n, "L": L, "M": M, "N": N, "logP": logP, "B": B})
    return out


def line_errors(got, want):
    """(line, peak, where) of a complex plane against its complex128 reference: `line` is the largest relative L2 error of
    any one row or column, ||got - want|| / ||want|| over that line alone, `where` names it; `peak` is the largest
    |got - want| of the plane over rms(want).  NaN or inf in `got` gives NaN (which fails `<=`)."""
    d = np.abs(np.asarray(got, dtype=np.complex128) - np.asarray(want, dtype=np.complex128)) ** 2
    w = np.abs(np.asarray(want, dtype=np.complex128)) ** 2
    if not np.all(np.isfinite(d)):
        return float("nan"), float("nan"), "not finite"
    with np.errstate(divide="ignore", invalid="ignore"):
        rows = np.sqrt(d.sum(axis=1) / w.sum(axis=1))
        cols = np.sqrt(d.sum(axis=0) / w.sum(axis=0))
        peak = float(np.sqrt(d.max() / w.mean()))
    r, c = int(np.argmax(rows)), int(np.argmax(cols))
    if not (np.all(np.isfinite(rows)) and np.all(np.isfinite(cols))):
        return float("nan"), peak, "a line of the reference is zero"
    return (float(rows[r]), peak, "row %d" % r) if rows[r] >= cols[c] else (float(cols[c]), peak, "column %d" % c)


def stage_model(entry, x):
    """The forward transform of x (length L) computed from one dumped length exactly as mx_stage of csrc/fdr_mixed.hip does it,
    in complex128: per stage, butterfly j < L / R gathers s[j + r L / R], q = umulhi(j, magic) (j where magic = 0),
    k = j - q ns, multiplies input r by lo[m % 64] hi[m / 64] with m = r k step, applies the R-point DFT and scatters to
    s[q ns R + k + r ns].  An index outside s or the tables raises IndexError (numpy checks every one; negative ones are
    turned away here)."""
    L = entry["L"]
    s = np.array(x, dtype=np.complex128)
    assert s.shape == (L,)
    lo, hi = entry["lo"], entry["hi"]
    for R, ns, magic, step in entry["stages"]:
        nb = L // R
        j = np.arange(nb, dtype=np.int64)
        q = (j * magic) >> 32 if magic else j
        k = j - q * ns
        v = [s[j + r * nb] for r in range(R)]
        for r in range(1, R):
            m = r * k * step
            if m.size and (m.min() < 0 or (m >> 6).max() >= len(hi)):
                raise IndexError("twiddle index out of the table")
            v[r] = v[r] * (lo[m & 63] * hi[m >> 6])
        F = np.exp(-2j * np.pi * np.outer(np.arange(R), np.arange(R)) / R)
        out = F @ np.stack(v)
        base = q * ns * R + k
        if base.size and base.min() < 0:
            raise IndexError("scatter index below the buffer")
        nxt = np.full(L, np.nan, dtype=np.complex128)  # an element no butterfly writes stays NaN
        for r in range(R):
            nxt[base + r * ns] = out[r]
        s = nxt
    return s
