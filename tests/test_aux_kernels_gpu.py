"""The kernels around the transforms, each against its model at the shapes where it can go wrong:

  colour epilogue   lab_mean_kernel, lab_apply_kernel (fdr_white_balance_u8_dev / fdr_white_balance_u8) against the float64 variant
                    of _color_model.epilogue under |got - v64| <= 0.5 + DELTA, on eight inputs and up to six shapes, strided planes,
                    a side stream, sentinels in every padding byte
  affine warp       warp_affine_kernel (fdr.warpAffine, fdr_warp_affine_f32) bit-equal to _warp_model.warp_model
  motion PSF        psf_motion_kernel (fdr.motionBlurKernel, fdr_psf_motion_dev) bit-equal to the oracle on 11 sizes x 11 angles
  generator         synth_kernel bit-equal to the splitmix64 model at the block edges, on a second loop trip, at wrapping sums
  slab primitives   slab_pack_kernel, transpose_any_kernel, pad_real_to_complex_kernel, real_part_kernel on random 32-bit patterns
                    compared as integers; the distributed transpose of slab.SlabTransposer in one process at up to 16 ranks; the
                    parity branch of wiener_pointwise_kernel bit-equal to its float32 restatement

The models are pinned on the CPU in test_aux_kernels_host.py.  Every case prints an `AUX` line with its worst value (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest

import _color_model as cm
import _warp_model as wm
from test_aux_kernels_host import (DIST_CASES, QUOTIENT_COUNTS, QUOTIENT_INPUTS, SYNTH_CASES, distributed_transpose, distribution,
                                   pack_reference, quotient_input, quotient_model, random_bits, synth_model, warp_picture)

pytestmark = pytest.mark.gpu

SENT8 = 0xA5
SENT32 = 0x5A5A5A5A


def _p(t):
    return ctypes.c_void_p(int(t.data_ptr()))


def _np(a):
    return ctypes.c_void_p(a.ctypes.data)


def _current_stream():
    import torch
    return ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))


def _err(fdr):
    return fdr.lib.fdr_last_error().decode()


def _to_dev(a):
    """a numpy array of 32-bit words (any 4-byte dtype) -> int32 device tensor of the same shape"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _sentinels(*shape):
    import torch
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda")


def _words(t):
    """device tensor -> uint32 numpy array"""
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- colour epilogue ------------------------------------------------------------------------------------------------------------
COLOR_CASES = [(name, shape) for name in cm.INPUTS for shape in cm.SHAPES + (cm.LARGE_SHAPES if name in cm.LARGE_INPUTS else ())]


@functools.lru_cache(maxsize=None)
def _color_case(name, shape):
    orig, rest = cm.color_input(name, *shape)
    v64 = cm.epilogue(orig, rest, np.float64)
    for a in (orig, rest, v64):
        a.setflags(write=False)
    return orig, rest, v64


@functools.lru_cache(maxsize=None)
def _side_stream():
    import torch
    return torch.cuda.Stream()


def _padded_planes(orig, rest, stride):
    """the six planes, each an array of its own with `stride` floats per row and NaN in the padding (a kernel that read it would show)"""
    rows, cols = orig.shape[1:]
    planes = []
    for p in list(orig) + list(rest):
        h = np.full((rows, stride), np.nan, dtype=np.float32)
        h[:, :cols] = p
        planes.append(h)
    return planes


def _split_out(flat, rows, cols, out_stride, what):
    """the rows x cols x 3 picture in a buffer of rows x out_stride bytes + a tail, whose padding and tail must still hold SENT8"""
    body = flat[:rows * out_stride].reshape(rows, out_stride)
    assert np.all(body[:, 3 * cols:] == SENT8), "%s: padding bytes of the output rows were written" % what
    assert np.all(flat[rows * out_stride:] == SENT8), "%s: bytes behind the output were written" % what
    return body[:, :3 * cols].reshape(rows, cols, 3).copy()


def white_balance_dev(fdr, orig, rest, what, pad=(5, 7)):
    """fdr_white_balance_u8_dev on six separate torch planes with stride = cols + 5, out_stride = 3 cols + 7, on a side stream"""
    import torch
    rows, cols = orig.shape[1:]
    stride, out_stride = cols + pad[0], 3 * cols + pad[1]
    planes = [torch.from_numpy(h).cuda() for h in _padded_planes(orig, rest, stride)]
    out = torch.full((rows * out_stride + 64,), SENT8, dtype=torch.uint8, device="cuda")
    po = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in planes[:3]])
    pr = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in planes[3:]])
    torch.cuda.synchronize()
    s = _side_stream()
    fdr._check(fdr.lib.fdr_white_balance_u8_dev(0, po, pr, rows, cols, stride, _p(out), out_stride, ctypes.c_void_p(int(s.cuda_stream))))
    s.synchronize()
    return _split_out(out.cpu().numpy(), rows, cols, out_stride, what)


def white_balance_host(fdr, orig, rest, what, pad=(5, 7)):
    """fdr_white_balance_u8 on strided numpy planes"""
    rows, cols = orig.shape[1:]
    stride, out_stride = cols + pad[0], 3 * cols + pad[1]
    planes = _padded_planes(orig, rest, stride)
    out = np.full(rows * out_stride + 64, SENT8, dtype=np.uint8)
    po = (ctypes.c_void_p * 3)(*[h.ctypes.data for h in planes[:3]])
    pr = (ctypes.c_void_p * 3)(*[h.ctypes.data for h in planes[3:]])
    fdr._check(fdr.lib.fdr_white_balance_u8(0, po, pr, rows, cols, stride, _np(out), out_stride))
    return _split_out(out, rows, cols, out_stride, what)


@pytest.mark.parametrize("name,shape", COLOR_CASES, ids=["%s-%dx%d" % (n, s[0], s[1]) for n, s in COLOR_CASES])
def test_color_epilogue_against_float64_model(fdr, name, shape):
    orig, rest, v64 = _color_case(name, shape)
    what = "colour %s %dx%d" % ((name,) + shape)
    got = white_balance_dev(fdr, orig, rest, what)
    bad, far = cm.rule(got, v64)
    off = int(np.count_nonzero(got != cm.quantize(v64)))
    print("AUX %s: worst |got - v64| %.6f (bound 0.5 + %.4g), %d of %d values differ from rint(v64), %d break the rule" % (what, far, cm.DELTA, off, got.size, bad))
    if bad:
        d = np.abs(got.astype(np.float64) - v64)
        y, x, c = np.unravel_index(int(np.argmax(d)), d.shape)
        pytest.fail("%s: %d values break |got - v64| <= 0.5 + %.4g; worst %.6f at (%d, %d) channel %d: got %d, v64 %.6f, restored BGR %s"
                    % (what, bad, cm.DELTA, far, y, x, c, got[y, x, c], v64[y, x, c], rest[:, y, x]))
    if name == "rest_zero":
        assert not got.any()


@pytest.mark.parametrize("name,shape", [("uniform", (97, 203)), ("gain_gt1", (520, 517))], ids=["uniform-97x203", "gain_gt1-520x517"])
def test_color_entries_agree_and_repeat(fdr, name, shape):
    """both entries, strided and contiguous, give the same bytes, twice"""
    orig, rest, _ = _color_case(name, shape)
    what = "colour %s %dx%d" % ((name,) + shape)
    first = white_balance_dev(fdr, orig, rest, what)
    assert np.array_equal(white_balance_dev(fdr, orig, rest, what), first), "%s: a second run gives other bytes" % what
    assert np.array_equal(white_balance_host(fdr, orig, rest, what), first), "%s: the host entry on strided views gives other bytes" % what
    assert np.array_equal(white_balance_host(fdr, orig, rest, what, pad=(0, 0)), first), "%s: the contiguous host call gives other bytes" % what
    assert np.array_equal(fdr.applyWhiteBalance_u8(list(orig), list(rest)), first)
    print("AUX %s: device entry twice, host entry strided and contiguous: identical bytes" % what)


def test_color_refusals_leave_the_entries_working(fdr):
    import torch
    orig, rest, v64 = _color_case("uniform", (3, 5))
    rows, cols = 3, 5
    L = fdr.lib
    d = [torch.from_numpy(np.array(p)).cuda() for p in list(orig) + list(rest)]
    d_out = torch.full((rows * cols * 3 + 16,), SENT8, dtype=torch.uint8, device="cuda")
    arr = lambda ptrs: (ctypes.c_void_p * 3)(*ptrs)
    po, pr = arr([t.data_ptr() for t in d[:3]]), arr([t.data_ptr() for t in d[3:]])
    holed = arr([d[0].data_ptr(), None, d[2].data_ptr()])
    st = _current_stream()
    for args, msg in [((holed, pr, rows, cols, cols, _p(d_out), 3 * cols), "null plane"), ((po, holed, rows, cols, cols, _p(d_out), 3 * cols), "null plane"),
                      ((None, pr, rows, cols, cols, _p(d_out), 3 * cols), "null argument"), ((po, pr, rows, cols, cols, None, 3 * cols), "null argument"),
                      ((po, pr, rows, cols, cols - 1, _p(d_out), 3 * cols), "bad shape"), ((po, pr, rows, cols, cols, _p(d_out), 3 * cols - 1), "bad shape"),
                      ((po, pr, 0, cols, cols, _p(d_out), 3 * cols), "bad shape"), ((po, pr, rows, 0, cols, _p(d_out), 3 * cols), "bad shape")]:
        assert L.fdr_white_balance_u8_dev(0, *args, st) == -1 and _err(fdr) == "fdr_white_balance_u8_dev: " + msg, (msg, _err(fdr))
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy() == SENT8), "a refused call wrote to the output"
    h = [np.array(p) for p in list(orig) + list(rest)]
    h_out = np.full(rows * cols * 3 + 16, SENT8, dtype=np.uint8)
    ho, hr = arr([a.ctypes.data for a in h[:3]]), arr([a.ctypes.data for a in h[3:]])
    hholed = arr([h[0].ctypes.data, h[1].ctypes.data, None])
    for args, msg in [((hholed, hr, rows, cols, cols, _np(h_out), 3 * cols), "null plane"), ((ho, hholed, rows, cols, cols, _np(h_out), 3 * cols), "null plane"),
                      ((ho, hr, rows, cols, cols - 1, _np(h_out), 3 * cols), "bad shape"), ((ho, hr, rows, cols, cols, _np(h_out), 3 * cols - 1), "bad shape"),
                      ((ho, hr, 0, cols, cols, _np(h_out), 3 * cols), "bad shape")]:
        assert L.fdr_white_balance_u8(0, *args) == -1 and _err(fdr) == "fdr_white_balance_u8: " + msg, (msg, _err(fdr))
    assert np.all(h_out == SENT8)
    for got in (white_balance_dev(fdr, orig, rest, "after the refusals"), white_balance_host(fdr, orig, rest, "after the refusals")):
        assert cm.rule(got, v64)[0] == 0


# ---- affine warp ----------------------------------------------------------------------------------------------------------------
def _small(rows, cols, seed):
    return np.random.default_rng(seed).random((rows, cols), dtype=np.float32)


# name: (source shape or None for the 37 x 53 picture, forward matrix, dsize = (width, height))
WARP_CASES = {k: (None, M, wm.DSIZE) for k, M in wm.MATRICES.items()}
WARP_CASES.update({
    "shift_minus_40000": (None, [[1, 0, -40000], [0, 1, 0]], wm.DSIZE),     # every source x saturates to 32767: all zero
    "singular": (None, [[1, 2, 0], [2, 4, 0]], wm.DSIZE),                   # D = 0: every pixel is src[0, 0]
    "half_pixel": (None, [[1, 0, 0.5], [0, 1, 0.5]], (53, 37)),
    "larger_destination": (None, wm.MATRICES["shear"], (120, 90)),
    "smaller_destination": (None, wm.MATRICES["shear"], (20, 11)),
    "source_1x1": ((1, 1), [[1, 0, 1.25], [0, 1, 0.75]], (4, 3)),
    "destination_1xn": (None, wm.MATRICES["rot17_scale1.3"], (47, 1)),
    "destination_nx1": (None, wm.MATRICES["rot17_scale1.3"], (1, 61)),
    # 1 100 000 > 4096 x 256 destination pixels: the source scaled by 14, turned by 30 degrees, its centre moved to the destination's
    "second_loop_trip": ((64, 64), wm.rotation_matrix((32, 32), 30.0, 14.0) + np.array([[0, 0, 468.0], [0, 0, 518.0]]), (1000, 1100)),
})


def _warp_source(shape):
    return warp_picture() if shape is None else _small(shape[0], shape[1], 77)


def _assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, what
    differ = int(np.count_nonzero(_bits(got) != _bits(want)))
    print("AUX %s: %d of %d values differ in their bits" % (what, differ, want.size))
    if differ:
        i = np.unravel_index(int(np.argmax(_bits(got) != _bits(want))), want.shape)
        pytest.fail("%s: %d of %d values differ; first at %s: got %r, want %r" % (what, differ, want.size, i, got[i], want[i]))


@pytest.mark.parametrize("case", list(WARP_CASES))
def test_warp_affine_equals_model(fdr, case):
    shape, M, dsize = WARP_CASES[case]
    src = _warp_source(shape)
    want = wm.warp_model(src, M, dsize)
    _assert_bits(fdr.warpAffine(src, M, dsize), want, "warp %s" % case)
    if case == "shift_minus_40000":
        assert not _bits(want).any()
    elif case == "singular":
        assert np.all(_bits(want) == _bits(src[0, 0]))
    else:
        assert np.count_nonzero(want) > 0
    if case == "second_loop_trip":
        assert np.count_nonzero(want.reshape(-1)[4096 * 256:]) > 10000  # the second trip's pixels are no empty ones


@pytest.mark.parametrize("case", ["rot17_scale1.3", "shear"])
def test_warp_affine_strided(fdr, case):
    """fdr_warp_affine_f32 with sstride = scols + 3 (NaN in the padding) and dstride = dcols + 5 (sentinels, which must survive)"""
    src = warp_picture()
    M = wm.MATRICES[case]
    srows, scols = src.shape
    dcols, drows = wm.DSIZE
    s = np.full((srows, scols + 3), np.nan, dtype=np.float32)
    s[:, :scols] = src
    d = np.full(drows * (dcols + 5) + 16, SENT32, dtype=np.uint32).view(np.float32)
    m = (ctypes.c_double * 6)(*np.asarray(M, dtype=np.float64).reshape(6))
    fdr._check(fdr.lib.fdr_warp_affine_f32(_np(s), srows, scols, scols + 3, m, _np(d), drows, dcols, dcols + 5))
    body = d[:drows * (dcols + 5)].reshape(drows, dcols + 5)
    assert np.all(_bits(body[:, dcols:]) == SENT32) and np.all(_bits(d[drows * (dcols + 5):]) == SENT32), "the destination's padding was written"
    _assert_bits(np.ascontiguousarray(body[:, :dcols]), wm.warp_model(src, M, wm.DSIZE), "warp %s strided" % case)


def test_warp_affine_refusals(fdr):
    L = fdr.lib
    src = warp_picture()
    dst = np.full((47, 61), -1.0, dtype=np.float32)
    m = (ctypes.c_double * 6)(1, 0, 0, 0, 1, 0)
    ok = (_np(src), 37, 53, 53, m, _np(dst), 47, 61, 61)

    def refused(msg, **kw):
        names = ("src", "srows", "scols", "sstride", "M", "dst", "drows", "dcols", "dstride")
        args = [kw.get(n, v) for n, v in zip(names, ok)]
        assert L.fdr_warp_affine_f32(*args) == -1 and _err(fdr) == "fdr_warp_affine_f32: " + msg, (kw, _err(fdr))

    for kw in ({"src": None}, {"dst": None}, {"M": None}, {"srows": 0}, {"scols": 0, "sstride": 0}, {"drows": 0}, {"dcols": 0, "dstride": 0},
               {"sstride": 52}, {"dstride": 60}):
        refused("bad argument", **kw)
    for kw in ({"srows": 32768}, {"scols": 32768, "sstride": 32768}, {"drows": 32768}, {"dcols": 32768, "dstride": 32768}):
        refused("image dimension above 32767 (cv::warpAffine's short coordinates)", **kw)
    assert np.all(dst == -1.0)
    fdr._check(L.fdr_warp_affine_f32(*ok))
    assert np.array_equal(_bits(dst), _bits(wm.warp_model(src, [[1, 0, 0], [0, 1, 0]], (61, 47))))


# ---- motion PSF -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", wm.PSF_SIZES)
def test_psf_motion_equals_oracle(fdr, oracle, size):
    """both entries at every angle; 513 x 513 is more than 1024 x 256 values: the loop's second trip"""
    import torch
    d = torch.empty(size * size + 1, dtype=torch.float32, device="cuda")
    worst = 0
    for angle in wm.PSF_ANGLES:
        want = oracle.motion_blur_kernel(size, angle)
        host = fdr.motionBlurKernel(size, angle)
        d.fill_(-7.0)
        fdr._check(fdr.lib.fdr_psf_motion_dev(0, size, float(angle), _p(d), _current_stream()))
        torch.cuda.synchronize()
        dev = d.cpu().numpy()
        assert dev[-1] == -7.0, "PSF %d/%g: the value behind the end was written" % (size, angle)
        for what, got in (("fdr_psf_motion", host), ("fdr_psf_motion_dev", dev[:-1].reshape(size, size))):
            differ = int(np.count_nonzero(_bits(got) != _bits(want)))
            worst = max(worst, differ)
            assert differ == 0, "%s %d/%g: %d of %d values differ from the oracle" % (what, size, angle, differ, want.size)
    print("AUX PSF size %d: %d angles, both entries, at most %d values differ from the oracle" % (size, len(wm.PSF_ANGLES), worst))


# ---- synthetic generator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,first,count", SYNTH_CASES)
def test_synth_equals_model(fdr, seed, first, count):
    import torch
    d = torch.full((count + 1,), -7.0, dtype=torch.float32, device="cuda")
    fdr.synth_image_dev(d.data_ptr(), count, seed, first_index=first)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert got[-1] == -7.0, "the value behind the end was written"
    want = synth_model(seed, first, count)
    differ = int(np.count_nonzero(_bits(got[:-1]) != _bits(want)))
    print("AUX synth seed %#x first %d count %d: %d values differ, range [%.3g, %.8f]" % (seed, first, count, differ, got[:-1].min(), got[:-1].max()))
    assert differ == 0, "%d of %d values differ from the splitmix64 model" % (differ, count)
    assert got[:-1].min() >= 0 and got[:-1].max() < 1


def test_synth_empty_and_null(fdr):
    L = fdr.lib
    assert L.fdr_synth_image_dev(0, 1, 2, 0, None, None) == 0
    assert L.fdr_synth_image_dev(0, 1, 2, 1, None, None) == -1 and _err(fdr) == "fdr_synth_image_dev: null output"


# ---- slab primitives: pure data movement ----------------------------------------------------------------------------------------
PACK_COUNTS = [[ld] for ld in (1, 255, 256, 257, 300)] + [[0, 5, 0, 0, 7, 0], [1] * 16, [0] * 15 + [9], [9] + [0] * 15,
                                                          distribution(300, 7)[0], distribution(5, 16)[0]]


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


def pack_dev(fdr, src, counts):
    """src uint32 [rows, ld] or [rows, ld, 2] -> the packed words, flat, with the sentinel row behind them checked"""
    rows, ld = src.shape[:2]
    es = 4 * (src.size // (rows * ld))
    d_src = _to_dev(src)
    d_dst = _sentinels(src.size + ld * es // 4)
    fdr._check(fdr.lib.fdr_slab_pack_dev(_p(d_src), rows, ld, len(counts), _ints(counts), es, _p(d_dst), _current_stream()))
    got = _words(d_dst)
    assert np.all(got[src.size:] == SENT32), "pack wrote behind its destination"
    return got[:src.size]


def transpose_dev(fdr, src):
    """src uint32 [rows, cols] or [rows, cols, 2] -> [cols, rows(, 2)], the sentinel row behind it checked"""
    rows, cols = src.shape[:2]
    es = 4 * (src.size // (rows * cols))
    d_src = _to_dev(src)
    d_dst = _sentinels(src.size + rows * es // 4)
    fdr._check(fdr.lib.fdr_slab_transpose_dev(_p(d_src), _p(d_dst), rows, cols, es, _current_stream()))
    got = _words(d_dst)
    assert np.all(got[src.size:] == SENT32), "transpose wrote behind its destination"
    return got[:src.size].reshape((cols, rows) + src.shape[2:])


@pytest.mark.parametrize("counts", PACK_COUNTS, ids=["-".join(map(str, c)) for c in PACK_COUNTS])
def test_slab_pack(fdr, counts):
    ld = sum(counts)
    worst = 0
    for es in (4, 8):
        for rows in (1, 3, 33):
            src = random_bits((rows, ld) + ((2,) if es == 8 else ()), 100 * rows + es)
            differ = int(np.count_nonzero(pack_dev(fdr, src, counts) != pack_reference(src, counts)))
            worst = max(worst, differ)
            assert differ == 0, "pack counts %s rows %d element size %d: %d of %d words differ" % (counts, rows, es, differ, src.size)
    print("AUX pack counts %s: rows 1, 3, 33 and element sizes 4, 8: at most %d words differ" % (counts, worst))


def test_slab_pack_empty_and_refusals(fdr):
    L = fdr.lib
    src = _to_dev(random_bits((3, 12), 1))
    dst = _sentinels(3 * 12)
    st = _current_stream()
    assert L.fdr_slab_pack_dev(_p(src), 0, 12, 2, _ints([5, 7]), 4, _p(dst), st) == 0
    msg = "fdr_slab_pack_dev: 1..16 parts with non-negative counts that sum to ld, element size 4 or 8"
    for parts, counts, es in [(0, [12], 4), (17, [1] * 12 + [0] * 5, 4), (2, [-1, 13], 4), (2, [5, 6], 4), (2, [5, 8], 4), (2, [5, 7], 2)]:
        assert L.fdr_slab_pack_dev(_p(src), 3, 12, parts, _ints(counts), es, _p(dst), st) == -1 and _err(fdr) == msg, (parts, counts, es, _err(fdr))
    for args in [(None, 3, 12, 2, _ints([5, 7]), 4, _p(dst)), (_p(src), 3, 12, 2, _ints([5, 7]), 4, None), (_p(src), 3, 12, 2, None, 4, _p(dst)),
                 (_p(src), -1, 12, 2, _ints([5, 7]), 4, _p(dst)), (_p(src), 3, 0, 1, _ints([0]), 4, _p(dst))]:
        assert L.fdr_slab_pack_dev(*args, st) == -1 and _err(fdr) == "fdr_slab_pack_dev: bad argument"
    assert np.all(_words(dst) == SENT32), "an empty or refused pack wrote to its destination"
    assert L.fdr_slab_pack_dev(_p(src), 3, 12, 2, _ints([5, 7]), 4, _p(dst), st) == 0
    assert np.array_equal(_words(dst), pack_reference(_words(src), [5, 7]))


TRANSPOSE_SHAPES = [(1, 1), (1, 100), (100, 1), (31, 33), (32, 32), (33, 65), (257, 3), (1000, 37)]


@pytest.mark.parametrize("shape", TRANSPOSE_SHAPES, ids=["%dx%d" % s for s in TRANSPOSE_SHAPES])
@pytest.mark.parametrize("es", [4, 8])
def test_slab_transpose(fdr, es, shape):
    src = random_bits(shape + ((2,) if es == 8 else ()), shape[0] * 7 + es)
    got = transpose_dev(fdr, src)
    differ = int(np.count_nonzero(got != np.swapaxes(src, 0, 1)))
    print("AUX transpose %dx%d element size %d: %d of %d words differ" % (shape + (es, differ, src.size)))
    assert differ == 0


def test_slab_transpose_empty_and_refusals(fdr):
    L = fdr.lib
    src = _to_dev(random_bits((4, 6), 2))
    dst = _sentinels(24)
    st = _current_stream()
    assert L.fdr_slab_transpose_dev(_p(src), _p(dst), 0, 6, 4, st) == 0
    assert L.fdr_slab_transpose_dev(_p(src), _p(dst), 4, 0, 8, st) == 0
    assert L.fdr_slab_transpose_dev(_p(src), _p(src), 4, 6, 4, st) == -1 and _err(fdr) == "fdr_slab_transpose_dev: bad argument"
    assert L.fdr_slab_transpose_dev(_p(src), _p(dst), 4, 6, 2, st) == -1 and _err(fdr) == "fdr_slab_transpose_dev: element size 4 or 8"
    assert L.fdr_slab_transpose_dev(None, _p(dst), 4, 6, 4, st) == -1 and L.fdr_slab_transpose_dev(_p(src), None, 4, 6, 4, st) == -1
    assert L.fdr_slab_transpose_dev(_p(src), _p(dst), -1, 6, 4, st) == -1
    assert np.all(_words(dst) == SENT32), "an empty or refused transpose wrote to its destination"
    assert L.fdr_slab_transpose_dev(_p(src), _p(dst), 4, 6, 4, st) == 0
    assert np.array_equal(_words(dst).reshape(6, 4), _words(src).T)


@pytest.mark.parametrize("R,C,world", DIST_CASES)
@pytest.mark.parametrize("elem", [1, 2], ids=["real", "complex"])
def test_distributed_transpose_in_one_process(fdr, R, C, world, elem):
    """SlabTransposer's scheme with the device's pack and transpose and the all-to-all in numpy: 16 ranks and empty ranks"""
    X = random_bits((R, C) + ((2,) if elem == 2 else ()), R * 1000 + C)
    got = distributed_transpose(X, world, lambda slab, counts: pack_dev(fdr, slab, counts), lambda block: transpose_dev(fdr, block))
    differ = int(np.count_nonzero(got != np.swapaxes(X, 0, 1)))
    print("AUX distributed transpose R=%d C=%d world=%d %s: %d of %d words differ" % (R, C, world, "complex" if elem == 2 else "real", differ, X.size))
    assert got.shape == (C, R) + X.shape[2:] and differ == 0


PAD_CASES = [(5, 100, 3, 37, 41), (4, 64, 4, 64, 64), (7, 1, 2, 1, 1), (6, 65, 0, 0, 0)]  # rows, N, valid_rows, valid_cols, stride


@pytest.mark.parametrize("rows,N,vr,vc,stride", PAD_CASES)
def test_slab_pad(fdr, rows, N, vr, vc, stride):
    src = random_bits((max(vr, 1), max(stride, 1)), rows * 10 + N)
    d_src = _to_dev(src) if vr and vc else None
    d_dst = _sentinels(rows + 1, N, 2)
    fdr._check(fdr.lib.fdr_slab_pad_dev(_p(d_src) if d_src is not None else None, vr, vc, stride, _p(d_dst), rows, N, _current_stream()))
    got = _words(d_dst)
    assert np.all(got[rows] == SENT32), "pad wrote behind its destination"
    want = np.zeros((rows, N, 2), dtype=np.uint32)  # +0.0 in every imaginary part and in the padding
    want[:vr, :vc, 0] = src[:vr, :vc]
    differ = int(np.count_nonzero(got[:rows] != want))
    print("AUX pad rows %d N %d valid %dx%d stride %d: %d of %d words differ" % (rows, N, vr, vc, stride, differ, want.size))
    assert differ == 0


def test_slab_pad_refusals(fdr):
    L = fdr.lib
    src = _to_dev(random_bits((3, 41), 3))
    dst = _sentinels(5, 100, 2)
    st = _current_stream()
    for args in [(_p(src), 6, 37, 41, _p(dst), 5, 100), (_p(src), 3, 101, 101, _p(dst), 5, 100), (None, 3, 37, 41, _p(dst), 5, 100),
                 (_p(src), 3, 37, 36, _p(dst), 5, 100), (_p(src), 3, 37, 41, None, 5, 100), (_p(src), 3, 37, 41, _p(dst), 5, 0)]:
        assert L.fdr_slab_pad_dev(*args, st) == -1 and _err(fdr) == "fdr_slab_pad_dev: bad argument", args
    assert L.fdr_slab_pad_dev(_p(src), 0, 0, 41, _p(dst), 0, 100, st) == 0  # no rows: nothing to do
    assert np.all(_words(dst) == SENT32)
    assert L.fdr_slab_pad_dev(_p(src), 3, 37, 41, _p(dst), 5, 100, st) == 0
    assert np.array_equal(_words(dst)[:3, :37, 0], _words(src)[:, :37])


@pytest.mark.parametrize("count", [1, 257, 1000])
def test_slab_real_part(fdr, count):
    src = random_bits((count, 2), count)
    d_dst = _sentinels(count + 1)
    fdr._check(fdr.lib.fdr_slab_real_dev(_p(_to_dev(src)), _p(d_dst), count, _current_stream()))
    got = _words(d_dst)
    differ = int(np.count_nonzero(got[:count] != src[:, 0]))
    print("AUX real part count %d: %d words differ" % (count, differ))
    assert differ == 0 and got[count] == SENT32


# ---- slab primitives: the Wiener quotient ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QUOTIENT_INPUTS)
def test_slab_quotient_equals_restatement(fdr, name):
    worst = 0
    with fdr.Plan(8, 8, fdr.MODE_PARITY, flags=fdr.FLAG_TABLES_ONLY) as p:
        for count in QUOTIENT_COUNTS:
            G, H, K = quotient_input(name, count)
            want = quotient_model(G, H, K).view(np.uint32)
            d_g = _to_dev(np.concatenate([G.view(np.uint32), np.full(2, SENT32, dtype=np.uint32)]))
            d_h = _to_dev(H.view(np.uint32))
            fdr._check(fdr.lib.fdr_slab_wiener_dev(p._h, _p(d_g), _p(d_h), count, K, _current_stream()))
            got = _words(d_g)
            assert np.all(got[2 * count:] == SENT32), "the quotient wrote behind its %d values" % count
            differ = int(np.count_nonzero(got[:2 * count] != want))
            worst = max(worst, differ)
            if differ:
                i = int(np.argmax(got[:2 * count] != want)) // 2
                pytest.fail("quotient %s count %d: %d of %d floats differ; first at %d: G %r H %r K %g: got %r, want %r"
                            % (name, count, differ, 2 * count, i, G[i], H[i], K, got[:2 * count].view(np.complex64)[i], want.view(np.complex64)[i]))
            if name == "h_zero_k_zero":
                assert not got[:2 * count].any()  # exactly +0
        d_g = _sentinels(2)
        assert fdr.lib.fdr_slab_wiener_dev(p._h, _p(d_g), _p(d_g), 0, 0.01, _current_stream()) == 0
        assert np.all(_words(d_g) == SENT32)
    print("AUX quotient %s: counts %s: at most %d floats differ from the float32 restatement" % (name, QUOTIENT_COUNTS, worst))
