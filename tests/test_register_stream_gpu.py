"""The stream fence (tests/_stream_fence.py) for fdr_register_frames_f32_dev and fdr_psf_shift_f32_dev, whose
streams travel in their parameter structs (include/fdr.h says why): they have no `void* stream` parameter, so the case table of
test_stream_order_gpu.py, which test_stream_order_host.py holds against the declarations that have one, does not list them.  These are
the cases that table would hold; they move there when it can next be edited.

The sequence behind the fence, on a non-blocking side stream: the estimate from poisoned frames and PSFs into a device array of
results (and the correlation planes), then the PSF shift that reads those results from device memory.  Both verdicts must hold:
ordered, and does not wait."""
import numpy as np
import pytest

import _register_model as rm
import _stream_fence as sf

pytestmark = pytest.mark.gpu

PAD = 6


@pytest.mark.parametrize("case,with_psfs", [(rm.GPU_CASES[1], True), (rm.GPU_CASES[5], True), (rm.GPU_CASES[1], False)],
                         ids=["pow2-psfs", "mixed-radix-psfs", "pow2-plain"])
def test_estimate_and_shift_are_ordered_on_the_stream_of_their_structs_and_do_not_wait(fdr, case, with_psfs):
    assert hasattr(fdr.lib, "fdr_register_frames_f32_dev") and hasattr(fdr.lib, "fdr_psf_shift_f32_dev"), "the library has no frame registration"
    import torch
    name, M, N, rows, cols, mixed, ref, max_shift = case[:8]
    frames, psfs = rm.short_case(M, N, rows, cols, len(case[9]), case[9], case[10])
    K = len(frames)
    inputs, outputs = [], []

    def inp(host):
        staging = torch.from_numpy(np.ascontiguousarray(host)).cuda()
        buf = torch.empty_like(staging)
        inputs.append((buf, staging))
        return buf

    def outp(shape):
        buf = torch.empty(shape, dtype=torch.float32, device="cuda")
        outputs.append(buf)
        return buf

    d_imgs = inp(np.stack(frames))
    d_psfs = inp(np.stack(psfs))
    d_shifts = outp(K * 6)  # 24 bytes per result
    d_corr = outp((K, M, N))
    d_out = outp((K, 5 + 2 * PAD, 5 + 2 * PAD))
    p = fdr.Plan(M, N, fdr.MODE_FAST, flags=fdr.FLAG_MIXED_RADIX if mixed else 0)
    try:
        def call(st):
            p.register_frames_dev(d_imgs.data_ptr(), rows * cols, K, rows, cols, cols, d_shifts.data_ptr(),
                                  d_psfs=d_psfs.data_ptr() if with_psfs else None, psf_pitch=25, prows=5, pcols=5, pstride=5, reference=ref,
                                  max_shift=max_shift, d_corr=d_corr.data_ptr(), stream=st)
            fdr.psf_shift_dev(d_psfs.data_ptr(), 25, K, 5, 5, 5, d_shifts.data_ptr(), PAD, PAD, d_out.data_ptr(), (5 + 2 * PAD) ** 2, 5 + 2 * PAD,
                              stream=st)

        tag = "register-%s%s" % (name, "" if with_psfs else "-plain")
        v = sf.judge(fdr, tag, call, inputs, outputs)
        assert v.ordered, "%s: the results behind the fence differ from the quiet run's: part of the calls did not run in order on their stream" % tag
        assert not v.waits, "%s: a call returned after the delay on its stream had ended: it waited for the stream" % tag
        assert np.all(np.isfinite(d_corr.cpu().numpy())) and np.all(np.isfinite(d_out.cpu().numpy())), "the fenced result is not finite: the poison was read"
        got = d_shifts.cpu().numpy().view(np.dtype([("dy", "<f8"), ("dx", "<f8"), ("peak", "<f4"), ("confidence", "<f4")]))
        assert (got[ref]["dy"], got[ref]["dx"], got[ref]["peak"]) == (0.0, 0.0, 1.0)
    finally:
        torch.cuda.synchronize()
        p.close()
