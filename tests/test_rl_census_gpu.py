"""The launch census of the Richardson-Lucy calls whose sequences no other test pins: the plain and the free-boundary batch (groups
and groups of one), the auto call and the plain blind call.  One 32 x 256 MODE_FAST plan, a 29 x 250 window, the motion PSF 15 / 30;
profile(True) afresh before each call, so pass_times() counts that call alone.  Every case asserts the whole {name: launches} table:
a name that is not in the table must not have been launched.  The tables follow from the host code (a step is pass A, B', C twice; a
group of n > 1 runs pass A under its group name) and were confirmed on a build from before the drivers were unified (DESIGN.md,
section 25)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, N, ROWS, COLS = 32, 256, 29, 250

FWD, FWD_N = "A op rows: pad+FFT (blur / RL)", "A op rows: pad+FFT (blur / RL), group"
COLS_H, COLS_C = "B' op cols: FFT*H*IFFT", "B' op cols: FFT*conj(H)*IFFT"
FREE = {"RLF setup: dw, W, sums": 3, "RLF start: wgt = 1/alpha, u": 3, "RLF out: crop": 3}  # per image, whatever the groups


@pytest.fixture(scope="module")
def bench(fdr):
    import torch
    rng = np.random.default_rng(11)
    imgs = torch.from_numpy((0.1 + rng.random((5, ROWS, COLS))).astype(np.float32)).cuda()
    mask = np.ones((ROWS, COLS), dtype=np.float32)
    mask[3:7, 40:90] = 0
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        p.set_operator_psf_motion(15, 30.0, stream=torch.cuda.current_stream().cuda_stream)
        yield fdr, p, imgs, torch.from_numpy(mask).cuda(), torch.zeros_like(imgs)


def census(p, call):
    """{name: launches} of one call"""
    import torch
    p.profile(True)
    call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = {}
    for name, _, c in p.pass_times():
        if c:
            got[name] = got.get(name, 0) + c
    p.profile(False)
    return got


def test_plain_batch(bench):
    fdr, p, imgs, _, out = bench
    p.set_batching(1, 2)  # 5 images: groups of 2, 2, 1
    got = census(p, lambda s: p.richardson_lucy_batch_dev(imgs.data_ptr(), ROWS * COLS, 5, ROWS, COLS, COLS, out.data_ptr(), ROWS * COLS, COLS, 3,
                                                          fdr.NORM_CROPPED, stream=s))
    assert got == {"RL init: u = max(d, 0)": 5, FWD_N: 12, FWD: 6, COLS_H: 9, COLS_C: 9, "C op rows: IFFT+RL ratio": 9,
                   "C op rows: IFFT+RL update": 9, "E RL minmax+normalize": 5}


@pytest.mark.parametrize("group", (2, 1))
def test_free_batch(bench, group):
    fdr, p, imgs, mask, out = bench
    p.set_batching(1, group)  # 3 images: groups of 2, 1, or the loop of three single calls
    got = census(p, lambda s: p.richardson_lucy_batch_dev(imgs.data_ptr(), ROWS * COLS, 3, ROWS, COLS, COLS, out.data_ptr(), ROWS * COLS, COLS, 2,
                                                          fdr.NORM_NONE, free_boundary=True, d_weights=mask.data_ptr(), wstride=COLS, stream=s))
    want = dict(FREE)
    if group == 2:
        want.update({FWD: 5, FWD_N: 4, COLS_H: 4, COLS_C: 5, "C op rows: IFFT+crop (blur)": 1, "C op rows: IFFT+RL ratio (free)": 4,
                     "C op rows: IFFT+RL update (weighted)": 4})
    else:
        want.update({FWD: 15, COLS_H: 6, COLS_C: 9, "C op rows: IFFT+crop (blur)": 3, "C op rows: IFFT+RL ratio (free)": 6,
                     "C op rows: IFFT+RL update (weighted)": 6})
    assert got == want


def test_auto_plain(bench):
    fdr, p, imgs, _, out = bench
    got = census(p, lambda s: p.richardson_lucy_auto_dev(imgs.data_ptr(), ROWS, COLS, COLS, out.data_ptr(), COLS, 3, rule=fdr.RL_STOP_NONE,
                                                         norm_area=fdr.NORM_CROPPED, stream=s))
    assert got == {"RL init: u = max(d, 0)": 1, FWD: 6, COLS_H: 3, COLS_C: 3, "C op rows: IFFT+RL ratio+fit": 3, "C op rows: IFFT+RL update": 3,
                   "RLS out: move": 1, "E RL minmax+normalize": 1}


def test_blind_plain(fdr):
    import torch
    rng = np.random.default_rng(12)
    img = torch.from_numpy((0.1 + rng.random((ROWS, COLS))).astype(np.float32)).cuda()
    psf = torch.from_numpy(fdr.psf_gaussian(7)).cuda()
    out = torch.zeros_like(img)
    with fdr.Plan(M, N, fdr.MODE_FAST) as p:
        got = census(p, lambda s: p.richardson_lucy_blind_dev(img.data_ptr(), ROWS, COLS, COLS, psf.data_ptr(), 7, 7, 7, out.data_ptr(), COLS, 3,
                                                              psf_hold=1, norm_area=fdr.NORM_CROPPED, stream=s))
        assert p.blind_status() == 0
    # iteration 0 holds the PSF; 1 and 2 add the table, the correlation (pass A, B', C) and the projection with its operator tables
    assert got == {"BL PSF: start / project / wgt": 3, "O rows: PSF pad+FFT (operator)": 3, "O cols: FFT -> H/MN, conj(H)/MN": 3,
                   "RL init: u = max(d, 0)": 1, FWD: 8, COLS_H: 3, COLS_C: 3, "C op rows: IFFT+RL ratio": 3, "C op rows: IFFT+RL update": 3,
                   "BL cols: FFT -> conj(U)/MN": 2, "B' op cols: FFT*conj(U)*IFFT": 2, "C op rows: IFFT+crop (PSF)": 2, "E RL minmax+normalize": 1}
