"""CPU pins of tests/_extremes.py: the transform-free delta reference against the float64 Wiener model and against the CPU oracle,
and the proof that the shared case table catches every fault model of the counted mask.  No GPU."""
import numpy as np
import pytest

from _extremes import (FAST_CASES, FAULTS, K, NORM_CROPPED, NORM_PADDED, PARITY_CASES, PARITY_EDGE_TOL, combos, delta_reference,
                       delta_references, edge_positions, oracle_reference, planted, position_pairs, seed_of, windows)
from _mixed_model import wiener_model
from _spectral import delta_psf, max_abs

WIENER_CASES = FAST_CASES + PARITY_CASES
BIG = 1 << 17  # plans above this many points: every 10th position against the transform model (rfft2 of 2^20 points)


def test_planted_and_positions():
    img = planted(5, 29, (4, 28), (0, 0), 1)
    assert img.dtype == np.float32 and img[4, 28] == 1.0 and img[0, 0] == 0.0625
    rest = np.delete(img.ravel(), [0, 5 * 29 - 1])
    assert rest.min() >= 0.375 and rest.max() < 0.625
    pos = edge_positions(8, 32, 5, 29)
    assert len(set(pos)) == len(pos)
    for want in ((0, 0), (0, 28), (4, 0), (4, 28), (4, 14), (2, 28), (0, 15), (0, 16), (0, 17), (2, 16), (4, 16)):
        assert want in pos
    assert all(0 <= r < 5 and 0 <= c < 29 for r, c in pos)
    assert (30, 2) in edge_positions(64, 4, 61, 3) and (0, 1) in edge_positions(64, 4, 61, 3)  # N/2 + 1 clipped to the window
    assert all(hi != lo for hi, lo in position_pairs(pos))
    rows4, cols4 = set(), set()
    for case in WIENER_CASES:
        for rows, cols in windows(case):
            assert 1 <= rows <= case[2] and 1 <= cols <= case[3] and (rows, cols) != (case[2], case[3])
            rows4.add(rows % 4)
            cols4.add(cols % 4)
    assert rows4 == {0, 1, 2, 3} and cols4 >= {0, 1, 3}


@pytest.mark.parametrize("case", WIENER_CASES, ids=[c[0] for c in WIENER_CASES])
def test_delta_reference_equals_wiener_model(case):
    M, N = case[2], case[3]
    worst, calls = 0.0, 0
    for i, (rows, cols, (r0, c0), hi_at, lo_at) in enumerate(combos(case)):
        if M * N > BIG and i % 10:
            continue
        img = planted(rows, cols, hi_at, lo_at, seed_of(rows, cols))
        both = delta_references(img, r0, c0, K, M, N)
        for area in (NORM_CROPPED, NORM_PADDED):
            ref = delta_reference(img, r0, c0, K, M, N, area == NORM_CROPPED)
            assert np.array_equal(ref, both[area])
            worst = max(worst, max_abs(ref, wiener_model(img, delta_psf(r0, c0), K, M, N, norm_cropped=area == NORM_CROPPED)))
            calls += 1
    print("EXTREMES-HOST\t%s\tdelta_reference vs wiener_model\tmax=%.3g\tcalls=%d" % (case[0], worst, calls))
    assert worst <= 1e-12


def test_flat_plane_rule():
    img = np.full((5, 7), 0.5, dtype=np.float32)
    assert not delta_reference(img, 0, 0, K, 5, 7, True).any()       # a flat window
    assert not delta_reference(np.zeros((5, 7), np.float32), 1, 1, K, 8, 8, False).any()
    assert delta_reference(img, 0, 0, K, 8, 8, False)[0, 0] == 1.0    # PADDED: the padding is the minimum


def test_every_fault_model_is_caught_by_the_table():
    """For each fault model at least one (case, delta, position, area) moves the reference by >= 0.05 max-abs: a device with
    that fault fails that call (the tolerances are below 1e-4).  The plans of up to 4096 points are enough, and every one of
    their combinations is a device call of test_extremes_gpu.py."""
    largest = dict.fromkeys(FAULTS, 0.0)
    where = dict.fromkeys(FAULTS, None)
    for case in WIENER_CASES:
        M, N = case[2], case[3]
        if M * N > 4096:
            continue
        for rows, cols, (r0, c0), hi_at, lo_at in combos(case):
            img = planted(rows, cols, hi_at, lo_at, seed_of(rows, cols))
            for cropped in (True, False):
                ref = delta_reference(img, r0, c0, K, M, N, cropped)
                for f in FAULTS:
                    d = max_abs(delta_reference(img, r0, c0, K, M, N, cropped, fault=f), ref)
                    if d > largest[f]:
                        largest[f] = d
                        where[f] = "%s window %dx%d delta (%d, %d) hi %s lo %s %s" % (case[0], rows, cols, r0, c0, hi_at, lo_at,
                                                                                      "CROPPED" if cropped else "PADDED")
    for f in FAULTS:
        print("EXTREMES-HOST\tfault %s\tlargest shift %.3g\t%s" % (f, largest[f], where[f]))
    missed = [f for f in FAULTS if not largest[f] >= 0.05]
    assert not missed, "fault models the table does not catch: %s" % missed


def test_unknown_fault_is_refused():
    with pytest.raises(ValueError):
        delta_reference(np.ones((3, 3), np.float32), 0, 0, K, 4, 4, True, fault="no_such_fault")


def test_oracle_against_delta_reference(oracle):
    """The CPU oracle on the parity cases: its result on the padded picture for the plan's area (the bits of oracle.serial_channel
    where the plan is the window's next power of two: compared here, on the long plan once per window and delta), its raw plane
    normalised over the window for the cropped area.  This measures PARITY_EDGE_TOL: 4x the largest value printed here."""
    overall, serial = 0.0, 0
    for case in PARITY_CASES:
        M, N = case[2], case[3]
        worst, calls = 0.0, 0
        for rows, cols, (r0, c0), hi_at, lo_at in combos(case):
            img = planted(rows, cols, hi_at, lo_at, seed_of(rows, cols))
            refs = delta_references(img, r0, c0, K, M, N)
            got = oracle_reference(oracle, img, delta_psf(r0, c0), K, M, N)
            if (M, N) == (oracle.next_pow2(rows), oracle.next_pow2(cols)) and (M * N <= 4096 or hi_at == (0, 0)):
                assert np.array_equal(oracle.serial_channel(img, delta_psf(r0, c0), K), got[NORM_PADDED])
                serial += 1
            for area in (NORM_CROPPED, NORM_PADDED):
                worst = max(worst, max_abs(got[area], refs[area]))
                calls += 1
        print("EXTREMES-HOST\t%s\toracle vs delta_reference\tmax=%.3g\tcalls=%d" % (case[0], worst, calls))
        overall = max(overall, worst)
    print("EXTREMES-HOST\toracle vs delta_reference, all parity cases\tmax=%.3g\tPARITY_EDGE_TOL=%.3g" % (overall, PARITY_EDGE_TOL))
    assert serial >= 500
    assert overall <= PARITY_EDGE_TOL and PARITY_EDGE_TOL <= 4 * overall * 1.01
