"""The stream fence (tests/_stream_fence.py) for fdr_tv_deconv_frames_f32_dev, whose stream travels in its
parameter struct (include/fdr.h says why): it has no `void* stream` parameter, so the case table of test_stream_order_gpu.py, which
test_stream_order_host.py holds against the declarations that have one, does not list it.  These are the cases that table would
hold; they move there when it can next be edited.

The sequence behind the fence, on a non-blocking side stream: fdr_set_frame_psfs_dev from poisoned PSF planes, then
fdr_tv_deconv_frames_f32_dev with params.stream = the side stream, K = 3 on the 64 x 128 plan in launch groups of 2 -- least squares
and Poisson, with and without per-frame weights.  Both verdicts must hold: ordered, and does not wait."""
import numpy as np
import pytest

import _stream_fence as sf
from _tvframes_model import LEAST_SQUARES, POISSON, short_frames, short_psfs, short_weights

pytestmark = pytest.mark.gpu

M, N, ROWS, COLS, STRIDE, WSTRIDE, OSTRIDE = 64, 128, 37, 101, 103, 101, 131
K = 3
PITCH, WPITCH = (ROWS + 1) * STRIDE, (ROWS + 1) * WSTRIDE
PR, PC, PSTRIDE = 5, 5, 8
PPITCH = PR * PSTRIDE + 3


def _pitched(planes, stride, pitch):
    h = np.zeros(len(planes) * pitch, dtype=np.float32)
    for k, a in enumerate(planes):
        for r in range(a.shape[0]):
            h[k * pitch + r * stride:k * pitch + r * stride + a.shape[1]] = a[r]
    return h


@pytest.mark.parametrize("with_weights", [False, True], ids=["no-weights", "per-frame-weights"])
@pytest.mark.parametrize("term,bg", [(LEAST_SQUARES, 0.0), (POISSON, 0.1)], ids=["least-squares", "poisson"])
def test_frames_tv_is_ordered_on_the_stream_of_its_struct_and_does_not_wait(fdr, term, bg, with_weights):
    assert hasattr(fdr.lib, "fdr_tv_deconv_frames_f32_dev"), "the library has no multi-frame TV deconvolution"
    import torch
    psfs = short_psfs("dense", K, M, N)
    ds = short_frames(M, N, ROWS, COLS, K, psfs, 17)
    inputs, outputs = [], []

    def inp(host):
        staging = torch.from_numpy(np.ascontiguousarray(host)).cuda()
        buf = torch.empty_like(staging)
        inputs.append((buf, staging))
        return buf

    d_psfs = inp(_pitched(psfs, PSTRIDE, PPITCH))
    d_imgs = inp(_pitched(ds, STRIDE, PITCH))
    d_w = inp(_pitched(list(short_weights("per_frame", K, ROWS, COLS, 17)), WSTRIDE, WPITCH)) if with_weights else None
    d_out = torch.empty(ROWS * OSTRIDE, dtype=torch.float32, device="cuda")
    outputs.append(d_out)
    p = fdr.Plan(M, N, fdr.MODE_FAST)
    try:
        p.set_batching(1, 2)

        def call(st):
            p.set_frame_psfs_dev(d_psfs.data_ptr(), PPITCH, K, PR, PC, PSTRIDE, stream=st)
            p.tv_deconv_frames_dev(d_imgs.data_ptr(), PITCH, K, ROWS, COLS, STRIDE, d_out.data_ptr(), OSTRIDE, 30.0, 3,
                                   d_weights=d_w.data_ptr() if with_weights else None, weight_pitch=WPITCH if with_weights else 0,
                                   wstride=WSTRIDE if with_weights else 0, data_term=term, background=bg, stream=st)

        name = "frames-tv-%s%s" % ("poisson" if term == POISSON else "ls", "-weights" if with_weights else "")
        v = sf.judge(fdr, name, call, inputs, outputs)
        assert v.ordered, "%s: the results behind the fence differ from the quiet run's: part of the call did not run in order on its stream" % name
        assert not v.waits, "%s: the call returned after the delay on its stream had ended: it waited for the stream" % name
        got = d_out.cpu().numpy().reshape(ROWS, OSTRIDE)[:, :COLS]
        assert np.all(np.isfinite(got)), "the fenced result is not finite: the poison was read"
    finally:
        torch.cuda.synchronize()
        p.close()
