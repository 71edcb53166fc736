"""The pass sequence of every path of a plan, one image and batches: which named passes a Wiener call launches and how often.

bench.py's roofline and tools/summarize_profiles.py look passes up by these names, so the names and the launch counts of each
path are pinned here, next to the bits of a batch (== the image-by-image results) and the rule that a refused call launches nothing.
Each case makes its own plan: a plan remembers at most MAX_PASSES names.

The PSF is 5 x 5, cut to the plan where the plan is smaller (the 4 x 4 one): a PSF larger than the plan is refused.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = "A rows: pad+FFT (real->complex)"
B = "B cols: FFT+Wiener"
C = "C rows: IFFT (complex)"
D = "D cols: IFFT+real+minmax"
E = "E normalize+crop"
B_FUSED = "B' cols: FFT*W*IFFT"
C_REAL = "C' rows: IFFT+real+minmax"
C1 = "C1 rows: IFFT+minmax"
C2 = "C2 rows: IFFT+normalize+crop"
SIMPLE = "simple path (reference-shaped)"
MIXED = ("A mixed rows: pad+FFT (real pairs)", "B mixed cols: FFT*W*IFFT", "C mixed rows: IFFT+real+minmax", "E mixed normalize+crop")

PARITY_PANEL = (A, B, C, D, E)
SIMPLE_PATH = (SIMPLE, E)
TWO_SWEEP = (A, B_FUSED, C1, C2)
ONE_SWEEP = (A, B_FUSED, C_REAL, E)

K = 0.01

# (id, M, N, mode, flags, OPT_TWO_SWEEP_NORM or None, expected names)
SINGLE = [
    ("parity-8x8", 8, 8, "MODE_PARITY", (), None, PARITY_PANEL),
    ("parity-4x4-simple", 4, 4, "MODE_PARITY", (), None, SIMPLE_PATH),
    ("parity-8x8-simple-flag", 8, 8, "MODE_PARITY", ("FLAG_SIMPLE_PATH",), None, SIMPLE_PATH),
    ("fast-8x8-simple-flag", 8, 8, "MODE_FAST", ("FLAG_SIMPLE_PATH",), None, SIMPLE_PATH),
    ("fast-8x32", 8, 32, "MODE_FAST", (), None, TWO_SWEEP),
    ("fast-8x32-one-sweep", 8, 32, "MODE_FAST", (), 0, ONE_SWEEP),
    ("fast-8x32-full", 8, 32, "MODE_FAST", ("FLAG_FULL_SPECTRUM",), None, ONE_SWEEP),
    ("fast-8x32-full-opt1", 8, 32, "MODE_FAST", ("FLAG_FULL_SPECTRUM",), 1, ONE_SWEEP),
    ("fast-8x32-full-opt0", 8, 32, "MODE_FAST", ("FLAG_FULL_SPECTRUM",), 0, ONE_SWEEP),
    ("fast-8x16", 8, 16, "MODE_FAST", (), None, ONE_SWEEP),
    ("fast-8x16-opt1", 8, 16, "MODE_FAST", (), 1, ONE_SWEEP),
    ("fast-8x16-opt0", 8, 16, "MODE_FAST", (), 0, ONE_SWEEP),
    ("fast-8x256-split", 8, 256, "MODE_FAST", (), None, TWO_SWEEP),
    ("fast-12x20-mixed", 12, 20, "MODE_FAST", ("FLAG_MIXED_RADIX",), None, MIXED),
]

# (id, M, N, mode, flags, OPT_TWO_SWEEP_NORM or None, kind, single-image names); kind says how a group of g images is launched:
# "grouped" every pass once for the group, "cols" pass B' once for the group and the row passes per image, "each" image by image
BATCH = [
    ("fast-8x32", 8, 32, "MODE_FAST", (), None, "grouped", TWO_SWEEP),
    ("fast-8x32-one-sweep", 8, 32, "MODE_FAST", (), 0, "grouped", ONE_SWEEP),
    ("fast-8x256", 8, 256, "MODE_FAST", (), None, "grouped", TWO_SWEEP),
    ("fast-8x256-one-sweep", 8, 256, "MODE_FAST", (), 0, "grouped", ONE_SWEEP),
    ("fast-8x32-full", 8, 32, "MODE_FAST", ("FLAG_FULL_SPECTRUM",), None, "cols", ONE_SWEEP),
    ("parity-8x8", 8, 8, "MODE_PARITY", (), None, "each", PARITY_PANEL),
    ("parity-4x4-simple", 4, 4, "MODE_PARITY", (), None, "each", SIMPLE_PATH),
    ("parity-8x8-simple-flag", 8, 8, "MODE_PARITY", ("FLAG_SIMPLE_PATH",), None, "each", SIMPLE_PATH),
    ("fast-8x8-simple-flag", 8, 8, "MODE_FAST", ("FLAG_SIMPLE_PATH",), None, "each", SIMPLE_PATH),
    ("fast-12x20-mixed", 12, 20, "MODE_FAST", ("FLAG_MIXED_RADIX",), None, "each", MIXED),
]


def _flags(fdr, names):
    f = 0
    for n in names:
        f |= getattr(fdr, n)
    return f


def _window(M, N):
    """An image window inside the plan with odd sizes where the plan leaves room."""
    return (M - 1 if M > 4 else M), (N - 3 if N > 4 else N)


def _inputs(M, N, count, seed):
    rng = np.random.default_rng(seed)
    rows, cols = _window(M, N)
    imgs = rng.random((count, rows, cols), dtype=np.float32)
    psf = rng.random((min(5, M), min(5, N)), dtype=np.float32)
    return imgs, (psf / psf.sum()).astype(np.float32)


def _plan(fdr, M, N, mode, flags, two_sweep, psf):
    p = fdr.Plan(M, N, getattr(fdr, mode), flags=_flags(fdr, flags))
    if two_sweep is not None:
        p.set_option(fdr.OPT_TWO_SWEEP_NORM, two_sweep)
    if psf is not None:
        p.set_psf(psf, K)
    return p


def _launches(p):
    """{pass name: launches} of what ran since profiling was switched on (names of earlier calls stay listed with 0)."""
    return {name: n for name, _ms, n in p.pass_times() if n > 0}


@pytest.mark.parametrize("case", SINGLE, ids=[c[0] for c in SINGLE])
def test_single_image_pass_sequence(fdr, case):
    _id, M, N, mode, flags, two_sweep, names = case
    imgs, psf = _inputs(M, N, 1, 11)
    with _plan(fdr, M, N, mode, flags, two_sweep, psf) as p:
        p.profile(True)
        out = p.wiener(imgs[0])
        got = _launches(p)
    print(_id, got)
    assert got == {n: 1 for n in names}
    assert np.isfinite(out).all()


@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("case", BATCH, ids=[c[0] for c in BATCH])
def test_batch_pass_sequence_and_bits(fdr, case, g):
    import torch
    _id, M, N, mode, flags, two_sweep, kind, names = case
    count = g + 1
    imgs, psf = _inputs(M, N, count, 23)
    rows, cols = imgs.shape[1:]
    d_in = torch.from_numpy(imgs).cuda()
    d_out = torch.zeros_like(d_in)
    s = torch.cuda.current_stream().cuda_stream
    with _plan(fdr, M, N, mode, flags, two_sweep, psf) as p:
        p.set_batching(1, g)
        p.profile(True)
        p.wiener_batch_dev(d_in.data_ptr(), rows * cols, count, rows, cols, cols, d_out.data_ptr(), rows * cols, cols, stream=s)
        torch.cuda.synchronize()
        got = _launches(p)
        p.profile(False)
        one = np.stack([p.wiener(imgs[i]) for i in range(count)])
    print(_id, g, got)
    suffix = " [%d images]" % g
    if kind == "grouped":  # one group of g, then the last image alone
        want = {n + suffix: 1 for n in names}
        want.update({n: 1 for n in names})
    elif kind == "cols":
        want = {n: count for n in names if n != B_FUSED}
        want.update({B_FUSED + suffix: 1, B_FUSED: 1})
    else:
        want = {n: count for n in names}
    assert got == want
    assert np.count_nonzero(~(d_out.cpu().numpy() == one)) == 0, "batch differs from image by image"


def test_refused_calls_launch_nothing(fdr):
    imgs, psf = _inputs(8, 32, 1, 37)
    with _plan(fdr, 8, 32, "MODE_FAST", (), None, None) as p:  # no PSF set
        p.profile(True)
        with pytest.raises(fdr.FdrError, match="no PSF set on this plan"):
            p.wiener(imgs[0])
        assert sum(n for _name, _ms, n in p.pass_times()) == 0
    with _plan(fdr, 8, 32, "MODE_FAST", (), None, psf) as p:  # a window larger than the plan
        p.profile(True)
        with pytest.raises(fdr.FdrError, match="the image window must be at least 1 x 1, fit the plan"):
            p.wiener(np.zeros((9, 32), np.float32))
        with pytest.raises(fdr.FdrError, match="the image window must be at least 1 x 1, fit the plan"):
            p.wiener(np.zeros((8, 33), np.float32))
        assert sum(n for _name, _ms, n in p.pass_times()) == 0
    pad_text = ("fdr_plan_set_option: FDR_OPT_PAD_MODE needs a FDR_MODE_FAST plan on the panel path (M, N powers of two, "
                "8 .. 8192; not FDR_FLAG_SIMPLE_PATH, FDR_FLAG_ANY_SIZE, FDR_FLAG_MIXED_RADIX sizes or FDR_FLAG_TABLES_ONLY)")
    for M, N, mode, flags in ((8, 8, "MODE_PARITY", ()), (8, 32, "MODE_FAST", ("FLAG_SIMPLE_PATH",)), (12, 20, "MODE_FAST", ("FLAG_MIXED_RADIX",))):
        with _plan(fdr, M, N, mode, flags, None, None) as p:  # FDR_OPT_PAD_MODE on a plan that is not on a panel path
            p.profile(True)
            with pytest.raises(fdr.FdrError) as e:
                p.set_option(fdr.OPT_PAD_MODE, fdr.PAD_SMOOTH)
            assert str(e.value).endswith(": " + pad_text)
            assert sum(n for _name, _ms, n in p.pass_times()) == 0
