"""CPU pins of tests/_batch_model.py: the launch geometry it restates, the coverage of the case lists that
test_batch_lengths_gpu.py runs, and the proof that its judge, on its inputs, flags every fault model of the float64 batched
operator -- and that the tightly packed, one-tile-per-workgroup batches of the older tests cannot see three of them.  No GPU."""
import numpy as np
import pytest

import _batch_model as bm
from _batch_model import (AREAS, CHUNK_CASES, CHUNK_GROUPINGS, COLUMN_PLANS, COUNT, FAULTS, FLAG_FULL_SPECTRUM, GROUPINGS, K32, NORM_CROPPED,
                          NORM_PADDED, PITCH_CASES, PITCH_COUNT, PITCH_GROUPINGS, ROW_PLANS, SENTINEL, TILE_CASES, TILE_SECOND)
from _mixed_model import wiener_model
from _spectral import SPATIAL_TOL


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def test_panel_geometry_and_persistent_grids():
    # Steps<LOGM>::T = M / 8; G = 4 up to T = 128; THREADS = T G; workgroups per CU = 512 / THREADS, at least 1
    assert [bm.panel_geom(1 << l) for l in (3, 7, 8, 9)] == [(1, 4, 4, 128), (16, 4, 64, 8), (32, 4, 128, 4), (64, 4, 256, 2)]
    assert bm.panel_geom(2048)[:3] == (256, 2, 512) and bm.panel_geom(4096) == (512, 1, 512, 1)
    # the grids named in the issue: 2048, 1024 and 512 workgroups on 256 CUs, capped by the tile count
    assert bm.persistent_grid(128, 8192, 8, full=True) == 2048
    assert bm.persistent_grid(256, 8192, 8) == 1024
    assert bm.persistent_grid(512, 8192, 8) == 512
    assert bm.persistent_grid(512, 8192, 1) == 256  # one image: N / 32 tiles, one each
    assert bm.npanels(64, False) == 8 and bm.npanels(64, True) == 16 and bm.npanels(16, False) == 4  # (N < 32: full spectrum)
    assert bm.cols_tiles(512, 8192) == 256 and bm.cols_tiles(128, 8192, True) == 512 and bm.cols_tiles(1024, 64) == 8 and bm.cols_tiles(8, 32) == 1


def test_which_kernel_a_group_runs():
    for M in (8, 16, 32, 64, 128):
        assert {bm.cols_kernel(M, n) for n in range(1, 9)} == {"radix8-persistent"}
    for M in (256, 512):
        assert bm.cols_kernel(M, 1) == "split" and {bm.cols_kernel(M, n) for n in range(2, 9)} == {"radix8-persistent"}
    for M in (1024, 2048):
        assert bm.cols_kernel(M, 1) == "split"
    for M in (1024, 2048, 4096, 8192):
        assert [bm.cols_kernel(M, n, 64) for n in range(2, 9)] == ["fused16-flat", "fused16-2d", "fused16-flat", "fused16-2d", "fused16-2d",
                                                                    "fused16-2d", "fused16-flat"]
        assert {bm.cols_kernel(M, n, 32) for n in range(2, 9)} == {"fused16-2d"}  # 4 tiles
    assert bm.cols_kernel(4096, 1) == "fused16-2d" and bm.cols_kernel(8192, 1, 32) == "fused16-2d"
    # rows
    for N in (256, 512, 1024, 2048):
        assert bm.rows_fwd_kernel(16, N, 1) == "split" and bm.rows_fwd_kernel(2048, N, 1) == "split" and bm.rows_fwd_kernel(4096, N, 1) == "packed"
        assert bm.rows_fwd_kernel(16, N, 2) == "packed"
        assert bm.rows_fwd_kernel(16, N, 8, full=True) == "packed"  # full spectrum: image by image, and no split kernel
    assert bm.rows_fwd_kernel(16, 128, 1) == "packed" and bm.rows_fwd_kernel(16, 4096, 1) == "packed"
    assert bm.rows_fwd_kernel(16, 8192, 1) == "persistent" and bm.rows_fwd_kernel(16, 8192, 8) == "persistent"


def test_loop_depths():
    assert bm.rows_pers_wg_per_cu(8192) == 1  # 512 threads, 144 KiB of LDS
    assert bm.tiles_per_workgroup(512, 8192, 8) == (4, 4)
    assert bm.tiles_per_workgroup(512, 8192, 5) == (2, 3)
    assert bm.tiles_per_workgroup(512, 8192, 4) == (2, 2)
    assert bm.tiles_per_workgroup(256, 8192, 8) == (2, 2)
    assert bm.tiles_per_workgroup(128, 8192, 8, True) == (2, 2) and bm.tiles_per_workgroup(128, 8192, 8, False) == (1, 1)
    assert bm.tiles_per_workgroup(512, 8192, 8, False, 64) == (16, 16)  # a smaller device loops deeper
    assert bm.tiles_per_workgroup(1024, 8192, 8) == (1, 1) and bm.tiles_per_workgroup(512, 8192, 1) == (1, 1)
    assert bm.rows_fwd_groups_per_workgroup(512, 8192, 8, 256) == (4, 4)
    assert bm.rows_fwd_groups_per_workgroup(512, 8192, 5, 256) == (2, 3)
    assert bm.rows_fwd_groups_per_workgroup(256, 8192, 8, 256) == (2, 2)
    assert bm.rows_fwd_groups_per_workgroup(128, 8192, 8, 256, full=True) == (1, 1)  # image by image: 32 groups
    assert bm.rows_fwd_groups_per_workgroup(2048, 8192, 1, 256) == (2, 2) and bm.rows_fwd_groups_per_workgroup(16, 4096, 8, 256) == (1, 1)
    # the plan heights of the older batch tests (M in {8, 128, 512, 1024, 2048}) on the half spectrum with rows up to 2048 points, or
    # up to 4096 in groups of at most 4, and their two full-spectrum shapes: one tile per workgroup, the loop body runs once
    for M in (8, 128, 512, 1024, 2048):
        for logn in range(5, 13):
            for n in range(1, 9 if logn < 12 else 5):
                assert bm.tiles_per_workgroup(M, 1 << logn, n) == (1, 1), (M, logn, n)
    for n in range(1, 9):
        assert bm.tiles_per_workgroup(8, 32, n, True) == (1, 1) and bm.tiles_per_workgroup(1024, 4096, n, True) == (1, 1)


def test_launches_and_chunks():
    assert bm.launches(11, 2) == [2, 2, 2, 2, 2, 1] and bm.launches(11, 3) == [3, 3, 3, 2] and bm.launches(11, 4) == [4, 4, 3]
    assert bm.launches(11, 5) == [5, 5, 1] and bm.launches(11, 8) == [8, 3] and bm.launches(9, 8) == [8, 1]
    assert bm.spectrum_bytes(128, 1024) == 540672 and bm.spectrum_bytes(256, 1024) == 1064960 and bm.spectrum_bytes(4096, 4096) == 4096 * 16400
    assert bm.ce_chunk(bm.spectrum_bytes(4096, 4096), bm.CHUNK_DEFAULT_MB, 4, 2) == 2   # the default: pairs at 4096^2 ...
    assert bm.ce_chunk(bm.spectrum_bytes(1024, 1024), bm.CHUNK_DEFAULT_MB, 8, 2) == 8   # ... the whole group below
    assert bm.ce_chunk(bm.spectrum_bytes(4096, 4096), bm.CHUNK_DEFAULT_MB, 4, 1) == 4   # one stream: never
    assert bm.ce_chunk(bm.spectrum_bytes(128, 1024), 0, 4, 2) == 4


# ---- coverage of the case lists ---------------------------------------------------------------------------------------------
def _launch_sizes(groupings, count):
    return {n for ns, g in groupings for n in bm.launches(count, g)}


def test_case_lists_cover_every_length_group_size_and_mapping():
    assert _launch_sizes(GROUPINGS, COUNT) == {1, 2, 3, 4, 5, 8}
    assert {ns for ns, g in GROUPINGS} == {1, 2}
    sizes = sorted(_launch_sizes(GROUPINGS, COUNT) - {1})
    for logm in range(3, 14):  # every LOGM with groups of 2, 3, 4, 5 and 8
        plans = [(M, N) for M, N in COLUMN_PLANS if M == 1 << logm]
        assert plans and sizes == [2, 3, 4, 5, 8]
        kinds = {bm.cols_kernel(M, n, N) for M, N in plans for n in sizes}
        if logm >= 10:
            assert kinds == {"fused16-flat", "fused16-2d"}
            assert {n for M, N in plans for n in sizes if bm.cols_kernel(M, n, N) == "fused16-flat"} == {2, 4, 8}
            assert all(bm.cols_kernel(M, n, N) == "fused16-2d" for M, N in plans for n in (2, 4, 8) if N == 32)  # 2, 4, 8 images on the 2-D grid too
        else:
            assert kinds == {"radix8-persistent"}
    assert {bm.log2(N) for M, N in ROW_PLANS} == set(range(5, 14))
    assert {bm.rows_fwd_kernel(M, N, 8) for M, N in ROW_PLANS} == {"packed", "persistent"}
    assert any(bm.rows4_use_split(N, M, 1, True) for M, N in ROW_PLANS)  # the image restored alone takes the split kernels there
    assert {M for M, N in COLUMN_PLANS} >= set(bm.ONE_SWEEP_M)
    for M, N in COLUMN_PLANS + ROW_PLANS:
        rows, cols = bm.short_window(M, N)
        assert rows % 4 == 3 and cols % 4 == 1 and 0 < rows < M and 0 < cols < N


def test_tile_cases_reach_the_loop():
    depth = [bm.tiles_per_workgroup(M, N, group, bool(flags & FLAG_FULL_SPECTRUM), 256) for M, N, flags, group, count, want in TILE_CASES]
    assert depth == [c[5] for c in TILE_CASES]
    assert {hi for lo, hi in depth} == {2, 3, 4} and min(lo for lo, hi in depth) == 2
    assert (2, 3) in depth  # odd and even exits in one launch, and sequences that cross image boundaries
    ns, group, count = TILE_SECOND
    for M, N, flags, _g, _c, _w in TILE_CASES:
        assert bm.tiles_per_workgroup(M, N, group, bool(flags & FLAG_FULL_SPECTRUM), 256)[0] >= 1
    rows = [bm.rows_fwd_groups_per_workgroup(M, N, group, 256, bool(flags & FLAG_FULL_SPECTRUM)) for M, N, flags, group, count, want in TILE_CASES]
    assert rows == [(4, 4), (2, 3), (2, 2), (1, 1)]
    assert all(count == group for _M, _N, _f, group, count, _w in TILE_CASES)


def test_pitch_and_chunk_cases():
    for M, N, rows, cols, flags, two in PITCH_CASES:
        lay = bm.loose_layout(rows, cols, PITCH_COUNT)
        assert lay.stride == cols + 7 and lay.out_stride == cols + 13 and lay.img_pitch == rows * lay.stride + 5 and lay.out_pitch == rows * lay.out_stride + 3
        assert rows <= M and cols <= N
    kinds = {bm.cols_kernel(M, n, N, bool(flags)) for M, N, _r, _c, flags, _t in PITCH_CASES for _ns, g in PITCH_GROUPINGS for n in bm.launches(PITCH_COUNT, g)}
    assert kinds == {"split", "radix8-persistent", "fused16-flat", "fused16-2d"}
    assert any(flags for *_x, flags, _t in PITCH_CASES) and any(two == 0 for *_x, two in PITCH_CASES)
    chunks = set()
    for M, N, mb, want in CHUNK_CASES:
        for ns, group in CHUNK_GROUPINGS:
            c = bm.ce_chunk(bm.spectrum_bytes(M, N), mb, group, ns)
            if want is None:
                assert c == group and bm.spectrum_bytes(M, N) > mb << 20
            else:
                assert c == want and 1 <= c < group
                chunks.add(c)
            assert bm.ce_chunk(bm.spectrum_bytes(M, N), bm.CHUNK_DEFAULT_MB, group, ns) == group  # the default does not split these
    assert chunks == {1, 2}
    assert all(ns >= 2 and COUNT > g for ns, g in CHUNK_GROUPINGS)  # (one group alone runs on one stream: no chunks)


# ---- inputs and reference ---------------------------------------------------------------------------------------------------
SMALL = [(M, N) for M, N in COLUMN_PLANS + ROW_PLANS if M * N <= 1 << 17]


@pytest.mark.parametrize("M,N", SMALL + [(256, 512)])
def test_batch_images_differ_in_range_and_in_where_their_extremes_sit(M, N):
    for rows, cols in ((M, N), bm.short_window(M, N)):
        imgs = bm.batch_images(M, N, rows, cols, COUNT, 17)
        assert imgs.dtype == np.float32 and imgs.shape == (COUNT, rows, cols) and np.all(np.isfinite(imgs))
        hi = [int(np.argmax(im)) for im in imgs]
        lo = [int(np.argmin(im)) for im in imgs]
        assert len(set(hi)) == COUNT and len(set(lo)) == COUNT, (hi, lo)
        span = [float(im.max() - im.min()) for im in imgs]
        assert all(abs(b - a) > 0.1 * a for a, b in zip(span, span[1:])), span  # (the tones' random phases move the range about its factor of 2)
        assert float(imgs.max()) < bm.GARBAGE / 10


def test_references_are_wiener_model(oracle):
    M, N, rows, cols = 16, 64, 15, 61
    psf = bm.fit_psf(oracle.motion_blur_kernel(15, 30.0), M, N)
    imgs = bm.batch_images(M, N, rows, cols, 3, 5)
    refs = bm.references(imgs, psf, K32, M, N)
    for area in AREAS:
        for i in range(3):
            assert np.array_equal(refs[area][i], wiener_model(imgs[i], psf, K32, M, N, norm_cropped=area == NORM_CROPPED))
    assert bm.fit_psf(oracle.motion_blur_kernel(15, 30.0), 8, 64).shape == (8, 15)
    assert abs(float(bm.fit_psf(oracle.motion_blur_kernel(15, 30.0), 8, 64).sum()) - 1.0) < 1e-6


def test_layouts_pack_and_unpack():
    imgs = bm.batch_images(8, 32, 7, 29, 3, 1)
    for lay in (bm.tight_layout(7, 29, 3), bm.loose_layout(7, 29, 3)):
        flat = bm.pack_inputs(imgs, lay)
        assert flat.size == 3 * lay.img_pitch and np.count_nonzero(flat != bm.GARBAGE) == imgs.size
        out = bm.new_output(lay)
        assert bm.outside_untouched(out, lay) and np.all(bm.unpack(out, lay) == SENTINEL)
        for i in range(3):
            for r in range(7):
                b = bm.out_base(lay, i) + r * lay.out_stride
                out[b:b + 29] = imgs[i, r]
        assert np.array_equal(bm.unpack(out, lay), imgs) and bm.outside_untouched(out, lay)
        for at in (0, lay.lead - 1, bm.out_base(lay, 2) + 6 * lay.out_stride + 29, out.size - 1):  # slack in front, behind the last window, the end
            poked = out.copy()
            poked[at] = 0.5
            assert not bm.outside_untouched(poked, lay), at
        if lay.out_stride > lay.cols:
            for at in (bm.out_base(lay, 0) + 29, bm.out_base(lay, 1) - 1, bm.out_base(lay, 1) + 3 * lay.out_stride - 1):  # stride padding, pitch gap
                poked = out.copy()
                poked[at] = 0.5
                assert not bm.outside_untouched(poked, lay), at


# ---- the judge against the fault models ---------------------------------------------------------------------------------------
# (M, N, flags, count, group, workgroups of pass B'): 16-point columns make tiles of 4 panels; 16 x 64 has 2 tiles per image, the
# full spectrum of 16 x 32 as well.  4 workgroups over the 10 tiles of 5 images: sequences of 3, 3, 2 and 2 tiles, every step over
# an image boundary; 3 workgroups over groups of 3 (6 tiles, then 4): sequences of 2, and of 2, 1, 1.
FAULT_SHAPES = [(16, 64, 0, 5, 5, 4), (16, 64, 0, 5, 3, 3), (16, 32, FLAG_FULL_SPECTRUM, 5, 5, 4)]
NEEDS_LOOP = ("boundary_reads_image0", "drop_last_tile")
NEEDS_LOOSE = ("ignore_img_pitch", "ignore_out_stride")


def _setup(oracle, M, N, count, loose):
    rows, cols = bm.short_window(M, N)
    psf = bm.fit_psf(oracle.motion_blur_kernel(15, 30.0), M, N)
    imgs = bm.batch_images(M, N, rows, cols, count, 29)
    lay = (bm.loose_layout if loose else bm.tight_layout)(rows, cols, count)
    return psf, imgs, lay, bm.pack_inputs(imgs.astype(np.float64), lay), bm.references(imgs, psf, K32, M, N)


def _ones(flat, lay, psf, M, N, area, full):
    """every image through the unfaulted operator alone (a batch of one)"""
    one = lay._replace(count=1)
    return np.stack([bm.unpack(bm.batched_operator(flat[i * lay.img_pitch:(i + 1) * lay.img_pitch], one, psf, K32, M, N, area, 1, 1, full), one)[0]
                     for i in range(lay.count)])


@pytest.mark.parametrize("M,N,flags,count,group,grid", FAULT_SHAPES)
@pytest.mark.parametrize("loose", (False, True), ids=("tight", "loose"))
def test_judge_passes_the_clean_operator_and_flags_every_fault(oracle, M, N, flags, count, group, grid, loose):
    full = bool(flags)
    psf, imgs, lay, flat, refs = _setup(oracle, M, N, count, loose)
    for area in AREAS:
        ones = _ones(flat, lay, psf, M, N, area, full)
        clean = bm.judge("clean", bm.batched_operator(flat, lay, psf, K32, M, N, area, group, grid, full), lay, ones, refs[area])
        assert not clean.bad and clean.worst < 1e-12, clean.bad
        for fault in FAULTS:
            v = bm.judge(fault, bm.batched_operator(flat, lay, psf, K32, M, N, area, group, grid, full, fault), lay, ones, refs[area])
            if fault in NEEDS_LOOSE and not loose:
                assert not v.bad, "tightly packed images cannot tell %s" % fault  # rows * stride == img_pitch, cols == out_stride
                continue
            # flagged by the comparison with the image restored alone AND, independently of it, by the model or the layout check:
            # a fault that the one-by-one path shared would still be seen
            assert "bits" in v.checks and v.checks & {"model", "layout"}, (fault, area, v.checks)
            assert v.worst != v.worst or v.worst > 100 * SPATIAL_TOL or "layout" in v.checks, (fault, v.worst)
        assert "layout" in bm.judge("x", bm.batched_operator(flat, lay, psf, K32, M, N, area, group, grid, full, "ignore_out_stride"), lay, ones,
                                    refs[area]).checks or not loose


def test_one_tile_per_workgroup_hides_the_loop_faults(oracle):
    """with at least as many workgroups as tiles -- every batch shape of the older tests -- the tile loop's faults do not exist"""
    M, N, count, group = 16, 64, 5, 5
    psf, imgs, lay, flat, refs = _setup(oracle, M, N, count, True)
    ones = _ones(flat, lay, psf, M, N, NORM_CROPPED, False)
    for fault in NEEDS_LOOP:
        assert not bm.judge(fault, bm.batched_operator(flat, lay, psf, K32, M, N, NORM_CROPPED, group, 10, False, fault), lay, ones, refs[NORM_CROPPED]).bad
        assert bm.judge(fault, bm.batched_operator(flat, lay, psf, K32, M, N, NORM_CROPPED, group, 5, False, fault), lay, ones, refs[NORM_CROPPED]).bad


def test_judge_flags_nan_inf_one_ulp_and_a_stray_store(oracle):
    M, N, count = 16, 64, 3
    psf, imgs, lay, flat, refs = _setup(oracle, M, N, count, True)
    out = bm.batched_operator(flat, lay, psf, K32, M, N, NORM_PADDED, 3, 2)
    ones = bm.unpack(out, lay)
    assert not bm.judge("clean", out, lay, ones, refs[NORM_PADDED]).bad
    at = bm.out_base(lay, 1) + 2 * lay.out_stride + 5
    for value, want in ((float("nan"), {"finite", "bits", "model"}), (float("inf"), {"finite", "bits", "model"}),
                        (np.nextafter(out[at], 2.0), {"bits"}), (out[at] + 4 * SPATIAL_TOL, {"bits", "model"})):
        bad = out.copy()
        bad[at] = value
        v = bm.judge("poke", bad, lay, ones, refs[NORM_PADDED])
        assert v.checks == want and v.bad, (value, v.checks)
    bad = out.copy()
    bad[at + lay.cols] = 0.25  # (row 2 of image 1, a column inside the stride padding)
    assert bm.judge("stray", bad, lay, ones, refs[NORM_PADDED]).checks == {"layout"}
