"""CPU pins of the models that judge the kernels around the transforms in test_aux_kernels_gpu.py: the colour epilogue
(_color_model.py), the affine warp and the motion PSF (_warp_model.py), the synthetic generator, the Wiener quotient of the slab
mode and the one-process restatement of the distributed transpose (all three defined here).  Every model is pinned against an
independent statement of the same operation, and every fault variant must be caught, before a model judges the device.  No GPU needed.
Cases print an `AUX` line with their measured values (pytest -s)."""
import numpy as np
import pytest

import _color_model as cm
import _warp_model as wm


# ---- colour epilogue ------------------------------------------------------------------------------------------------------------
def _color_cases():
    return [(name, shape) for name in cm.INPUTS for shape in cm.SHAPES + (cm.LARGE_SHAPES if name in cm.LARGE_INPUTS else ())]


def test_color_delta_is_the_measured_gap():
    """DELTA = FACTOR x the largest |v32 - v64| over every input and shape; the float32 variant passes the rule everywhere"""
    worst = {}
    for name, shape in _color_cases():
        orig, rest = cm.color_input(name, *shape)
        v32, v64 = cm.epilogue(orig, rest, np.float32), cm.epilogue(orig, rest, np.float64)
        assert v64.shape == shape + (3,) and v64.dtype == np.float64 and np.all(np.isfinite(v64))
        worst[name] = max(worst.get(name, 0.0), float(np.abs(v32 - v64).max()))
        bad, far = cm.rule(cm.quantize(v32), v64)
        assert bad == 0, "%s %s: the float32 variant breaks the rule at %d values, worst |got - v64| = %.6f" % (name, shape, bad, far)
    gap = max(worst.values())
    print("AUX colour: largest |v32 - v64| %.3g (recorded %.3g), DELTA = %d x recorded = %.4g; per input: %s"
          % (gap, cm.MEASURED_GAP, cm.FACTOR, cm.DELTA, ", ".join("%s %.2g" % kv for kv in worst.items())))
    # the recorded value stays the measured one: a quarter above it at most (numpy's float32 pow and cbrt may differ by an ulp from
    # one build to the next) and no more than twice it
    assert gap <= 1.25 * cm.MEASURED_GAP, "the gap of the float32 variant, %.3g, is above the recorded %.3g" % (gap, cm.MEASURED_GAP)
    assert gap >= 0.5 * cm.MEASURED_GAP, "the recorded gap %.3g is more than twice the measured %.3g" % (cm.MEASURED_GAP, gap)
    assert cm.DELTA == cm.FACTOR * cm.MEASURED_GAP and cm.DELTA <= cm.DELTA_MAX


def test_color_inputs_reach_their_branches():
    """what each input is for, on the float64 variant's intermediate facts that the output shows"""
    o, r = cm.color_input("rest_zero", 97, 203)
    assert np.all(cm.epilogue(o, r, np.float64) == 0) and np.all(cm.epilogue(o, r, np.float32) == 0)
    o, r = cm.color_input("gain_gt1", 97, 203)
    moved = cm.quantize(cm.epilogue(o, r, np.float32, fault="no_l_clamp")) != cm.quantize(cm.epilogue(o, r, np.float32))
    print("AUX colour: without the L clamp %.1f %% of the gain_gt1 values move" % (100.0 * moved.mean()))
    assert moved.mean() > 0.1
    o, r = cm.color_input("out_of_range", 97, 203)
    assert o.min() < -0.4 and o.max() > 1.4
    v = cm.epilogue(o, r, np.float64)
    assert v.min() >= 0 and v.max() <= 255.0 + 1e-9
    o, r = cm.color_input("dark", 97, 203)
    assert max(o.max(), r.max()) < 0.06
    o, r = cm.color_input("binary", 97, 203)
    assert set(np.unique(o)) == {0.0, 1.0} and set(np.unique(r)) == {0.0, 1.0}
    o, r = cm.color_input("grey_ramp", 97, 203)
    assert np.array_equal(o[0], o[1]) and np.array_equal(o[0], o[2]) and o.min() == 0 and o.max() == 1


# the input (at 97 x 203) on which each fault must break the rule
COLOR_FAULT_INPUT = {"y_green": "uniform", "xn": "uniform", "matrix_entry": "uniform", "finv_threshold": "grey_ramp",
                     "no_l_clamp": "gain_gt1", "ab_swapped": "uniform", "br_swapped": "uniform", "truncate": "uniform"}


@pytest.mark.parametrize("fault", list(COLOR_FAULT_INPUT))
def test_color_rule_catches_fault(fault):
    caught = []
    for name in cm.INPUTS:
        orig, rest = cm.color_input(name, 97, 203)
        v64 = cm.epilogue(orig, rest, np.float64)
        if fault == "truncate":
            got = cm.quantize(cm.epilogue(orig, rest, np.float32), truncate=True)
        else:
            got = cm.quantize(cm.epilogue(orig, rest, np.float32, fault=fault))
        bad, far = cm.rule(got, v64)
        if bad:
            caught.append("%s (%d values, worst %.4f)" % (name, bad, far))
        if name == COLOR_FAULT_INPUT[fault]:
            assert bad > 0, "fault %s passes the rule on %s: worst |got - v64| = %.6f <= 0.5 + %.4g" % (fault, name, far, cm.DELTA)
    print("AUX colour fault %s: caught on %s" % (fault, "; ".join(caught)))


def test_old_color_rule_lets_the_constant_faults_through():
    """the rule of test_white_balance_epilogue_on_device (off by at most 1, fewer than 2 % off) on the same kind of input"""
    orig, rest = cm.color_input("uniform", 97, 203)
    want = cm.quantize(cm.epilogue(orig, rest, np.float64)).astype(np.int16)
    for fault in ("y_green", "xn", "matrix_entry", "finv_threshold"):
        d = np.abs(cm.quantize(cm.epilogue(orig, rest, np.float32, fault=fault)).astype(np.int16) - want)
        print("AUX colour: fault %s under the old rule: %.3f %% of the values differ, by %d at most" % (fault, 100.0 * np.count_nonzero(d) / d.size, d.max()))
        assert d.max() <= 1 and np.count_nonzero(d) < 0.02 * d.size


# ---- affine warp and motion PSF -------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _psf_grid_mismatches(oracle, fault=None):
    return ["%d/%g" % (size, angle) for size in wm.PSF_SIZES for angle in wm.PSF_ANGLES
            if not np.array_equal(_bits(wm.psf_model(size, angle, fault)), _bits(oracle.motion_blur_kernel(size, angle)))]


def warp_picture():
    return np.random.default_rng(5).random(wm.SRC_SHAPE, dtype=np.float32)


def _exact_gaps(fault=None):
    src = warp_picture()
    return {k: float(np.abs(wm.warp_model(src, M, wm.DSIZE, fault) - wm.bilinear_exact(src, M, wm.DSIZE)).max()) for k, M in wm.MATRICES.items()}


def test_warp_model_equals_the_oracle_psf(oracle):
    bad = _psf_grid_mismatches(oracle)
    print("AUX warp: %d of %d (size, angle) pairs differ from oracle.motion_blur_kernel" % (len(bad), len(wm.PSF_SIZES) * len(wm.PSF_ANGLES)))
    assert bad == [], "psf_model differs from the oracle at %s" % ", ".join(bad)


def test_warp_model_against_exact_bilinear():
    gaps = _exact_gaps()
    print("AUX warp: gap to the exact float64 bilinear: %s (bound %.4f)" % (", ".join("%s %.4f" % kv for kv in gaps.items()), wm.EXACT_GAP))
    for k, g in gaps.items():
        assert g < wm.EXACT_GAP, "%s: the model is %.4f from the exact bilinear" % (k, g)
    src = warp_picture()
    for k, M in wm.MATRICES.items():  # no empty cases: hundreds of destination pixels lie inside the source (the shrunk picture is 21 x 22)
        assert np.count_nonzero(wm.warp_model(src, M, wm.DSIZE)) > 400, k


@pytest.mark.parametrize("fault", wm.FAULTS)
def test_warp_pins_catch_fault(oracle, fault):
    bad = _psf_grid_mismatches(oracle, fault)
    gaps = _exact_gaps(fault)
    over = [k for k, g in gaps.items() if not g < wm.EXACT_GAP]
    print("AUX warp fault %s: %d PSF pairs differ from the oracle; gaps %s; above the bound: %s"
          % (fault, len(bad), ", ".join("%s %.4f" % kv for kv in gaps.items()), over or "none"))
    assert bad, "fault %s equals the oracle on the whole PSF grid" % fault
    if fault in ("w1_w2_swapped", "not_inverted"):  # wrong by whole pixels: the exact interpolation sees them too
        assert len(over) == len(gaps)


def test_warp_model_edges():
    src = warp_picture()
    out = wm.warp_model(src, [[1, 0, -40000], [0, 1, 0]], wm.DSIZE)          # every source x saturates to 32767
    assert np.all(_bits(out) == 0)
    out = wm.warp_model(src, [[1, 2, 0], [2, 4, 0]], wm.DSIZE)               # D = 0: the map is all zero
    assert np.all(_bits(out) == _bits(src[0, 0]))
    assert np.array_equal(_bits(wm.warp_model(src, [[1, 0, 0], [0, 1, 0]], (53, 37))), _bits(src))
    half = wm.warp_model(src, [[1, 0, 0.5], [0, 1, 0]], (53, 37))            # dst(x) = (src(x - 1) + src(x)) / 2
    assert np.array_equal(half[:, 1:], np.float32(0.5) * src[:, :-1] + np.float32(0.5) * src[:, 1:])
    with pytest.raises(AssertionError):
        wm.warp_model(src, [[1, 0, -3e6], [0, 1, 0]], wm.DSIZE)              # 3e6 x 1024 leaves int32


# ---- synthetic generator --------------------------------------------------------------------------------------------------------
MASK64 = (1 << 64) - 1


def synth_model(seed, first_index, count):
    """top 24 bits of splitmix64(seed + first_index + i) / 2^24, i = 0 .. count-1, in numpy uint64 (sums and products wrap)"""
    x = np.arange(count, dtype=np.uint64) + np.uint64((seed + first_index) & MASK64)
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


SYNTH_CASES = [(0x5EED0003, first, count) for first in (0, 2 ** 32 - 3, 2 ** 40) for count in (1, 255, 256, 257, 4096 * 256 + 4097)]
SYNTH_CASES += [(2 ** 64 - 5, first, 257) for first in (0, 2 ** 32 - 3, 2 ** 40)]  # seed + first + i wraps past 2^64


@pytest.mark.parametrize("seed,first,count", SYNTH_CASES)
def test_synth_model_equals_oracle(oracle, seed, first, count):
    got = synth_model(seed, first, count)
    assert got.dtype == np.float32 and got.shape == (count,)
    assert np.array_equal(_bits(got), _bits(oracle.synth_image(seed, first, count)))
    assert got.min() >= 0 and got.max() < 1
    if seed == 2 ** 64 - 5 and first == 0:  # the wrap itself: value i = 5 is the generator's value at index 0 of seed 0
        assert np.array_equal(got[5:], synth_model(0, 0, count - 5))


def test_synth_model_known_value():
    """splitmix64's first output from state 0 is 0xE220A8397B1DCDAF (the published test vector)"""
    assert synth_model(0, 0, 1)[0] == np.float32(0xE220A8 / 16777216.0)


# ---- Wiener quotient of the slab mode -------------------------------------------------------------------------------------------
def quotient_model(G, H, K, fault=None):
    """the parity branch of wiener_pointwise_kernel in float32, operation by operation (every product, sum, square root and division
    rounded on its own); G, H complex64, K float.  fault "no_sqrt": mag2 = hr2 + hi2 without the square root and the square."""
    G, H = np.asarray(G, dtype=np.complex64), np.asarray(H, dtype=np.complex64)
    gx, gy, hx, hy = G.real, G.imag, H.real, H.imag
    K = np.float32(K)
    hr2, hi2 = hx * hx, hy * hy
    if fault == "no_sqrt":
        mag2 = hr2 + hi2
    else:
        mag = np.sqrt(hr2 + hi2)
        mag2 = mag * mag
    denom = mag2 + K
    chi = -hy
    p0, p1, p2, p3 = gx * hx, gy * chi, gx * chi, gy * hx
    nr, ni = p0 - p1, p2 + p3
    assert nr.dtype == np.float32 and denom.dtype == np.float32
    zero = np.float32(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.stack([np.where(denom != 0, nr / denom, zero), np.where(denom != 0, ni / denom, zero)], axis=-1)
    return np.ascontiguousarray(out).view(np.complex64).reshape(G.shape)


QUOTIENT_INPUTS = ("random", "h_zero_k_zero", "h_zero_k_pos", "h_small_k_zero", "k_0.01")
QUOTIENT_COUNTS = (1, 255, 256, 257, 1000)


def quotient_input(name, count):
    """(G, H, K): complex64 arrays whose components have magnitudes in [0.01, 2) (H: about 1e-3 for h_small), random signs: every
    product in the kernel is normal or exactly zero"""
    rng = np.random.default_rng([QUOTIENT_INPUTS.index(name), count])

    def field(lo, hi):
        v = rng.uniform(lo, hi, (count, 2)) * rng.choice([-1.0, 1.0], (count, 2))
        return np.ascontiguousarray(v.astype(np.float32)).view(np.complex64).reshape(count)

    G = field(0.01, 2.0)
    if name == "random":
        return G, field(0.01, 2.0), 0.0
    if name == "h_zero_k_zero":
        return G, np.zeros(count, dtype=np.complex64), 0.0
    if name == "h_zero_k_pos":
        return G, np.zeros(count, dtype=np.complex64), 0.01
    if name == "h_small_k_zero":
        return G, field(0.5e-3, 1.5e-3), 0.0
    if name == "k_0.01":
        return G, field(0.01, 2.0), 0.01
    raise ValueError(name)


@pytest.mark.parametrize("name", QUOTIENT_INPUTS)
def test_quotient_model_against_complex128(name):
    G, H, K = quotient_input(name, 1000)
    got = quotient_model(G, H, K)
    assert got.dtype == np.complex64
    if name.startswith("h_zero"):
        assert np.all(got == 0)  # K = 0: the kernel's own rule for a zero denominator; K > 0: 0 / K
        return
    G2, H2 = G.astype(np.complex128), H.astype(np.complex128)
    ref = G2 * np.conj(H2) / (np.abs(H2) ** 2 + float(np.float32(K)))
    err = float(np.max(np.abs(got - ref) / np.abs(ref)))
    print("AUX quotient %s: largest relative distance from complex128 %.3g (bound 1e-6)" % (name, err))
    assert err <= 1e-6
    faulty = quotient_model(G, H, K, fault="no_sqrt")
    differ = np.count_nonzero(faulty.view(np.uint32) != got.view(np.uint32))
    print("AUX quotient %s: without sqrt and square %d of %d floats differ" % (name, differ, 2 * G.size))
    assert differ > 0


def test_quotient_inputs_keep_products_normal():
    tiny = np.finfo(np.float32).tiny
    for name in QUOTIENT_INPUTS:
        G, H, K = quotient_input(name, 1000)
        g, h = np.abs(G.view(np.float32)).astype(np.float64), np.abs(H.view(np.float32)).astype(np.float64)
        for p in (h * h, g.min() * h, g.max() * h):
            assert np.all((p == 0) | (p >= tiny))
        assert np.all(np.isfinite(quotient_model(G, H, K).view(np.float32)))


# ---- slab pack and the distributed transpose, restated in numpy -----------------------------------------------------------------
def distribution(total, parts):
    """calculate_distribution of the package (batch.py), restated so that this file needs no built library"""
    counts = [total // parts + (1 if g < total % parts else 0) for g in range(parts)]
    return counts, [sum(counts[:g]) for g in range(parts)]


def pack_reference(src, counts):
    """src [rows, ld, ...]: the column blocks of `counts` columns one after the other, each row-major"""
    displs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(int)
    return np.concatenate([src[:, d:d + c].reshape(-1) for d, c in zip(displs, counts)])


DIST_CASES = [(64, 32, 16), (37, 53, 5), (4, 100, 7), (300, 7, 16)]  # R, C, world


def distributed_transpose(X, world, pack, transpose):
    """The scheme of slab.SlabTransposer in one process: X [R, C, ...] split into row slabs by calculate_distribution; every rank's slab
    packed by pack(slab, counts) -> flat; the all-to-all in numpy with SlabTransposer's send_counts / recv_counts; every rank's received
    R x lc block transposed by transpose(block [R, lc, ...]) -> [lc, R, ...].  Ranks without rows skip the pack, ranks without columns
    the transpose, as slab.py does.  Returns the gathered C x R array."""
    R, C = X.shape[:2]
    e = int(np.prod(X.shape[2:], dtype=int))
    rcnt, rdis = distribution(R, world)
    ccnt, cdis = distribution(C, world)
    packed = []
    for g in range(world):
        slab = X[rdis[g]:rdis[g] + rcnt[g]]
        packed.append(pack(slab, ccnt).reshape(-1) if rcnt[g] > 0 else np.zeros(0, dtype=X.dtype))
        assert packed[g].size == rcnt[g] * C * e
    out = []
    for d in range(world):
        lc = ccnt[d]
        blocks = []
        for g in range(world):
            send_counts = [rcnt[g] * c * e for c in ccnt]
            off = sum(send_counts[:d])
            blocks.append(packed[g][off:off + send_counts[d]])
        recv = np.concatenate(blocks)
        assert [b.size for b in blocks] == [r * lc * e for r in rcnt]  # recv_counts of rank d
        if lc > 0:
            out.append(transpose(recv.reshape((R, lc) + X.shape[2:])))
    return np.concatenate(out, axis=0)


def random_bits(shape, seed):
    """random 32-bit patterns (NaN payloads, -0, infinities and denormals among them) with some planted on purpose"""
    a = np.random.default_rng(seed).integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = a.reshape(-1)
    special = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0x7F800001, 0xFFFFFFFF, 0x00000001], dtype=np.uint32)
    n = min(flat.size, special.size)
    flat[:n] = special[:n]
    return a


@pytest.mark.parametrize("R,C,world", DIST_CASES)
@pytest.mark.parametrize("elem", [1, 2], ids=["real", "complex"])
def test_distributed_transpose_scheme_in_numpy(R, C, world, elem):
    X = random_bits((R, C) + ((2,) if elem == 2 else ()), R * 1000 + C)
    got = distributed_transpose(X, world, pack_reference, lambda b: np.swapaxes(b, 0, 1))
    assert np.array_equal(got, np.swapaxes(X, 0, 1))
    rcnt, ccnt = distribution(R, world)[0], distribution(C, world)[0]
    print("AUX slab: R=%d C=%d world=%d: %d ranks without rows, %d without columns" % (R, C, world, rcnt.count(0), ccnt.count(0)))


def test_distribution_equals_the_package(fdr):
    from importlib import import_module
    batch = import_module(fdr.__name__ + ".batch")
    for total, parts in [(300, 7), (5, 16), (64, 16), (37, 5), (4, 7), (7, 16), (100, 7)]:
        assert tuple(map(list, batch.calculate_distribution(total, parts))) == tuple(map(list, distribution(total, parts)))
