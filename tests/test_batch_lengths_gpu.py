"""Batched Wiener launches on the MI355X at every column and row length, group size, grid mapping and loop depth, with loose
pitches and strides, with passes C1 + C2 in chunks, and replayed as a graph.

A group of 2 .. 8 images runs other kernels than one image does (tests/_batch_model.py names them), and the persistent kernels loop
only where a launch holds more tiles than the chip has workgroups.  Every case here: images from batch_images (a range and extreme
positions of their own), motion PSF 15 / 30 cut to the plan, K = 0.01, NORM_CROPPED and NORM_PADDED.  Every image of a batch must
equal, bit for bit, the same image restored alone by wiener_dev on the same plan, and lie within _spectral.SPATIAL_TOL of the
float64 model; NaN and inf fail; the sentinel that fills the output buffer must survive in the stride padding, the pitch gap and the
slack in front of and behind the images.  Each case prints a `BATCH` line with its largest max-abs against the model (pytest -s).
The shapes are the smallest that reach the code, not the workload's own; test_batch_host.py proves the coverage of the lists and that
this judge flags the fault models of the batched operator."""
import numpy as np
import pytest

import _batch_model as bm
from _batch_model import (AREA_NAME, AREAS, CHUNK_CASES, CHUNK_DEFAULT_MB, CHUNK_GROUPINGS, COLUMN_PLANS, COUNT, FLAG_FULL_SPECTRUM, GROUPINGS, K32,
                          ONE_SWEEP_M, PITCH_CASES, PITCH_COUNT, PITCH_GROUPINGS, ROW_PLANS, SENTINEL, TILE_CASES, TILE_SECOND)
from _spectral import SPATIAL_TOL

pytestmark = pytest.mark.gpu


class _Batch:
    """images, references and device buffers of one (plan shape, window, layout), shared by the calls of a case"""

    def __init__(self, oracle, M, N, rows, cols, count, loose=False):
        import torch
        self.M, self.N = M, N
        self.psf = bm.fit_psf(oracle.motion_blur_kernel(15, 30.0), M, N)
        self.lay = (bm.loose_layout if loose else bm.tight_layout)(rows, cols, count)
        self.imgs = bm.batch_images(M, N, rows, cols, count, 1000 * bm.log2(M) + bm.log2(N))
        self.refs = bm.references(self.imgs, self.psf, K32, M, N)
        self.d_in = torch.from_numpy(bm.pack_inputs(self.imgs, self.lay)).cuda()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.bad, self.worst, self.calls = [], 0.0, 0

    def sub(self, count):
        return self.lay._replace(count=count)

    def fresh(self, count):
        import torch
        return torch.full((bm.out_size(self.sub(count)),), SENTINEL, dtype=torch.float32, device="cuda")

    def alone(self, p, area):
        """every image by wiener_dev on its own, read from and stored to the places it has in the batch: ([count, rows, cols], their
        max-abs against the model)"""
        import torch
        lay = self.lay
        d_one = self.fresh(lay.count)
        for i in range(lay.count):
            p.wiener_dev(self.d_in.data_ptr() + 4 * i * lay.img_pitch, lay.rows, lay.cols, lay.stride, d_one.data_ptr() + 4 * bm.out_base(lay, i),
                         lay.out_stride, area, stream=self.stream)
        torch.cuda.synchronize()
        one = d_one.cpu().numpy()
        if not bm.outside_untouched(one, lay):
            self.bad.append("%dx%d %s: wiener_dev wrote outside its window" % (self.M, self.N, AREA_NAME[area]))
        ones = bm.unpack(one, lay)
        return ones, bm.model_errors(ones, self.refs[area])

    def batch(self, p, what, area, ones, count=None, d_out=None):
        """one wiener_batch_dev of the first `count` images into a sentinel-filled buffer, judged; returns the flat output"""
        import torch
        lay = self.sub(self.lay.count if count is None else count)
        if d_out is None:
            d_out = self.fresh(lay.count)
        else:
            d_out.fill_(SENTINEL)
        p.wiener_batch_dev(self.d_in.data_ptr(), lay.img_pitch, lay.count, lay.rows, lay.cols, lay.stride, d_out.data_ptr() + 4 * lay.lead, lay.out_pitch,
                           lay.out_stride, area, stream=self.stream)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        v = bm.judge("%dx%d window %dx%d %s %s" % (self.M, self.N, lay.rows, lay.cols, AREA_NAME[area], what), out, lay, ones[0][:lay.count],
                     self.refs[area][:lay.count], ones_err=ones[1][:lay.count])
        self.bad += v.bad
        self.worst = max(self.worst, v.worst) if v.worst == v.worst and self.worst == self.worst else float("nan")
        self.calls += 1
        return out

    def finish(self, lst, what):
        bm.log(lst, "%dx%d window %dx%d %s" % (self.M, self.N, self.lay.rows, self.lay.cols, what), self.worst, SPATIAL_TOL, self.calls)
        assert not self.bad, "%d failures, the first:\n%s" % (len(self.bad), "\n".join(self.bad[:12]))


def _plan(fdr, b, flags=0, two_sweep=None):
    p = fdr.Plan(b.M, b.N, fdr.MODE_FAST, flags=flags)
    p.set_psf(b.psf, K32)
    if two_sweep is not None:
        p.set_option(fdr.OPT_TWO_SWEEP_NORM, two_sweep)
    return p


def _groupings(fdr, b, lst, what, groupings, flags=0, two_sweep=None):
    with _plan(fdr, b, flags, two_sweep) as p:
        for area in AREAS:
            ones = b.alone(p, area)
            for ns, group in groupings:
                p.set_batching(ns, group)
                b.batch(p, "batching %dx%d" % (ns, group), area, ones)
    b.finish(lst, what)


def _sweeps(M):
    return (None, 0) if M in ONE_SWEEP_M else (None,)


# ---- 1. column lengths --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", COLUMN_PLANS, ids=["%dx%d" % s for s in COLUMN_PLANS])
def test_groups_at_every_column_length(fdr, oracle, M, N):
    """M = 2^3 .. 2^13: the persistent radix-8 kernel with an image dimension (a group of 256- or 512-row images reaches it, one image
    does not), fused16 at LOGM 10 .. 13 on the flat grid (N = 64, 2 / 4 / 8 images) and on the (tiles, images) grid; launches of 2, 3,
    4, 5 and 8 images with tails of 1, 2 and 3, one stream and two."""
    rows, cols = bm.short_window(M, N)
    for two_sweep in _sweeps(M):
        b = _Batch(oracle, M, N, rows, cols, COUNT)
        _groupings(fdr, b, "columns", "one-sweep" if two_sweep == 0 else "two-sweep", GROUPINGS, two_sweep=two_sweep)


# ---- 2. row lengths -----------------------------------------------------------------------------------------------------------
ROW_CASES = [(M, N, full) for M, N in ROW_PLANS for full in (True, False)]


@pytest.mark.parametrize("M,N,full", ROW_CASES, ids=["%dx%d-%s" % (M, N, "full" if f else "short") for M, N, f in ROW_CASES])
def test_groups_at_every_row_length(fdr, oracle, M, N, full):
    """N = 2^5 .. 2^13: the packed row kernels with blockIdx.y = image (one image of 256 .. 2048 columns takes the split kernels), the
    persistent forward kernel at 8192 points over groups * images, its interior (full window) and edge variants."""
    rows, cols = (M, N) if full else bm.short_window(M, N)
    _groupings(fdr, _Batch(oracle, M, N, rows, cols, COUNT), "rows", "full window" if full else "short window", GROUPINGS)


# ---- 3. tile loops ------------------------------------------------------------------------------------------------------------
TILE_PARAMS = [c + (full,) for c in TILE_CASES for full in (True, False)]


def _tile_id(c):
    return "%dx%d%s-group%d-%s" % (c[0], c[1], "-fullspec" if c[2] else "", c[3], "full" if c[6] else "short")


def _assert_loop_reached(M, N, flags, group, want):
    """from this device's CU count: the launch must hold more tiles than workgroups, as deep as the case says"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    got = bm.tiles_per_workgroup(M, N, group, bool(flags & FLAG_FULL_SPECTRUM), cus)
    assert got == want, "%d CUs: %dx%d in groups of %d gives %s tiles per workgroup, the case is built for %s" % (cus, M, N, group, got, want)


@pytest.mark.parametrize("case", TILE_PARAMS, ids=[_tile_id(c) for c in TILE_PARAMS])
def test_persistent_tile_loop(fdr, oracle, case):
    """More tiles than workgroups: the ping-pong between the two register sets of pass B', the prefetch of the next image's tile over an
    image boundary, the dummy prefetch of the last tile, the odd and the even exit (3 and 2 tiles per workgroup in one launch of 5
    images).  The 256- and 512-row cases put 2 and 4 (2 and 3) row groups per workgroup through the persistent forward row kernel too."""
    M, N, flags, group, count, want, full = case
    _assert_loop_reached(M, N, flags, group, want)
    rows, cols = (M, N) if full else bm.short_window(M, N)
    ns2, group2, count2 = TILE_SECOND
    b = _Batch(oracle, M, N, rows, cols, max(count, count2))
    with _plan(fdr, b, flags) as p:
        for area in AREAS:
            ones = b.alone(p, area)
            p.set_batching(1, group)
            b.batch(p, "batching 1x%d, %d images" % (group, count), area, ones, count)
            p.set_batching(ns2, group2)
            b.batch(p, "batching %dx%d, %d images" % (ns2, group2, count2), area, ones, count2)
    b.finish("tiles", "%s groups of %d, %s tiles per workgroup" % ("full spectrum" if flags else "half spectrum", group, want))


# ---- 4. pitch and stride ------------------------------------------------------------------------------------------------------
def _pitch_id(c):
    return "%dx%d%s%s" % (c[0], c[1], "-fullspec" if c[4] else "", "-one-sweep" if c[5] == 0 else "")


@pytest.mark.parametrize("case", PITCH_CASES, ids=[_pitch_id(c) for c in PITCH_CASES])
def test_loose_pitch_and_stride(fdr, oracle, case):
    """stride = cols + 7, out_stride = cols + 13, img_pitch = rows * stride + 5, out_pitch = rows * out_stride + 3: per-image base
    pointers and row strides as separate inputs of every batched kernel; the input's gaps hold 1e6."""
    M, N, rows, cols, flags, two_sweep = case
    b = _Batch(oracle, M, N, rows, cols, PITCH_COUNT, loose=True)
    _groupings(fdr, b, "pitch", _pitch_id(case), PITCH_GROUPINGS, flags, two_sweep)


# ---- 5. chunks of passes C1 + C2 ----------------------------------------------------------------------------------------------
def _chunk_id(c):
    return "%dx%d-%dMiB" % c[:3]


def _chunk_run(fdr, oracle, case, graph):
    M, N, mb, want = case
    rows, cols = bm.short_window(M, N)
    b = _Batch(oracle, M, N, rows, cols, COUNT)
    with _plan(fdr, b) as p:
        spec = p.filter_bytes()
        assert spec == bm.spectrum_bytes(M, N)
        if graph:
            p.set_option(fdr.OPT_BATCH_GRAPH, 1)
        for area in AREAS:
            ones = b.alone(p, area)
            for ns, group in CHUNK_GROUPINGS:
                chunk = bm.ce_chunk(spec, mb, group, ns)
                if want is None:
                    assert chunk == group and spec > mb << 20  # one image alone is above the limit: no split
                else:
                    assert chunk == want and 1 <= chunk < group
                p.set_batching(ns, group)
                outs = []
                for value in (mb, 0, CHUNK_DEFAULT_MB):  # in chunks, whole groups, back to the default
                    p.set_option(fdr.OPT_CE_CHUNK_MB, value)
                    d_out = b.fresh(COUNT)
                    for rep in range(3 if graph else 1):  # (graph: capture, then two replays)
                        outs.append(b.batch(p, "batching %dx%d chunk option %d MiB%s" % (ns, group, value, ", replay %d" % rep if graph else ""), area, ones,
                                            d_out=d_out))
                for o in outs[1:]:
                    assert np.array_equal(o, outs[0]), "%dx%d batching %dx%d: FDR_OPT_CE_CHUNK_MB changes the result" % (M, N, ns, group)
    b.finish("chunks", "FDR_OPT_CE_CHUNK_MB %d: %s images per chunk%s" % (mb, want if want else "all", ", graph" if graph else ""))


@pytest.mark.parametrize("case", CHUNK_CASES, ids=[_chunk_id(c) for c in CHUNK_CASES])
def test_inverse_row_chunks_keep_the_bits(fdr, oracle, case):
    """FDR_OPT_CE_CHUNK_MB on two streams: passes C1 + C2 of a group of 4 or 8 in chunks of 1 and of 2 images (computed from
    Plan.filter_bytes() as batch_enqueue does), against the same batch with the option at 0, image by image, and back at the default."""
    _chunk_run(fdr, oracle, case, False)


# ---- 6. graph replay ----------------------------------------------------------------------------------------------------------
def test_graph_replay_of_a_tile_loop(fdr, oracle):
    M, N, flags, group, count, want = TILE_CASES[2]  # 256 x 8192 in groups of 8
    _assert_loop_reached(M, N, flags, group, want)
    rows, cols = bm.short_window(M, N)
    b = _Batch(oracle, M, N, rows, cols, count)
    with _plan(fdr, b, flags) as p, _plan(fdr, b, flags) as q:
        p.set_option(fdr.OPT_BATCH_GRAPH, 1)
        p.set_batching(1, group)
        q.set_batching(1, group)
        for area in AREAS:
            ones = b.alone(q, area)
            plain = b.batch(q, "plain launches", area, ones)
            d_out = b.fresh(count)
            for rep in range(3):
                assert np.array_equal(b.batch(p, "graph, replay %d" % rep, area, ones, d_out=d_out), plain)
    b.finish("graph", "tile loop, groups of %d" % group)


def test_graph_replay_with_loose_pitch_and_stride(fdr, oracle):
    M, N, rows, cols, flags, two_sweep = PITCH_CASES[0]  # 256 x 512, window 201 x 375
    b = _Batch(oracle, M, N, rows, cols, PITCH_COUNT, loose=True)
    with _plan(fdr, b, flags, two_sweep) as p, _plan(fdr, b, flags, two_sweep) as q:
        p.set_option(fdr.OPT_BATCH_GRAPH, 1)
        for area in AREAS:
            ones = b.alone(q, area)
            for ns, group in PITCH_GROUPINGS:
                p.set_batching(ns, group)
                q.set_batching(ns, group)
                plain = b.batch(q, "batching %dx%d plain launches" % (ns, group), area, ones)
                d_out = b.fresh(PITCH_COUNT)
                for rep in range(3):
                    assert np.array_equal(b.batch(p, "batching %dx%d graph, replay %d" % (ns, group, rep), area, ones, d_out=d_out), plain)
    b.finish("graph", "loose pitch and stride")


def test_graph_replay_of_inverse_row_chunks(fdr, oracle):
    _chunk_run(fdr, oracle, CHUNK_CASES[0], True)
