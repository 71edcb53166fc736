"""The stream fence: does an entry point with a `void* stream` parameter do ALL its device work on that stream,
in order, and does it return without waiting for it?

fenced() runs one call on a NON-BLOCKING side stream (a blocking one would order itself against the null stream and hide a launch
that dropped its stream argument) behind a delay the device is still spinning in when the call is made:

    1. every input buffer holds NaN, every output buffer the sentinel byte, the true inputs sit in staging buffers; synchronise
    2. side stream: delay (torch.cuda._sleep), event `delay_done`
    3. side stream: the true inputs device-to-device over the poison
    4. the call with stream = the side stream; then delay_done.query()
    5. side stream: the outputs into result buffers
    6. side.synchronize()

The side stream is chosen so that the null stream runs beside it (runs_beside: streams that share a hardware queue run in submission
order, and a misplaced launch would then look right).  A launch, memset or copy of the call that went to any other stream runs while the delay still holds the side stream back: it reads
the poison, or writes early and is overwritten, or its result is missing when step 5 copies -- the results then differ from those of
the quiet run (the same sequence without the delay, with a device synchronise before and after the call), which judge() compares bit
for bit.  A call that waited for its stream finds delay_done already true in step 4.  The delay is measured (event time) and must be
at least DELAY_FACTOR times the wall time of the quiet run's call-plus-synchronise -- which bounds the host's enqueue time -- and at
least MIN_DELAY_MS: judge() asserts that before it looks at a verdict, so a fence cannot pass because its delay ran out.

Buffers are torch device tensors.  `inputs` is a list of (buffer, staging) pairs of equal shape (float32: the poison is NaN),
`outputs` a list of buffers (a buffer that is both is poisoned, not filled with the sentinel); `call(stream_pointer)` makes the call and
returns its host values (or None).  Nothing here uses a bad pointer: a misplaced launch reads NaN from valid memory."""
import collections
import functools
import time

import numpy as np

MIN_DELAY_MS = 20.0
DELAY_FACTOR = 4.0
DELAY_MARGIN = 1.5     # the delay asked for is this much above the condition, so that the measured one meets it
SENTINEL = 0xA5
HIP_STREAM_NON_BLOCKING = 1

Fenced = collections.namedtuple("Fenced", "results host early call_ms delay_ms")
Verdict = collections.namedtuple("Verdict", "ordered waits call_ms quiet_ms delay_ms")


def stream_flags(fdr, stream):
    """hipStreamGetFlags of a torch stream, through the HIP runtime libfdr.so is bound to"""
    import ctypes
    flags = ctypes.c_uint(0xFFFFFFFF)
    fn = fdr.lib.hipStreamGetFlags
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
    rc = fn(ctypes.c_void_p(int(stream.cuda_stream)), ctypes.byref(flags))
    assert rc == 0, "hipStreamGetFlags failed with %d" % rc
    return flags.value


@functools.lru_cache(maxsize=None)
def _cycles_per_ms():
    """the rate of torch.cuda._sleep's counter, from the event time of a spin (second of two: the first loads the kernel)"""
    import torch
    ms = 0.0
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(2000000)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
    assert ms > 0
    return 2000000.0 / ms


def runs_beside(a, b):
    """True when work on stream b completes while a delay still holds stream a: the runtime maps streams onto a few hardware queues,
    and two streams on one queue run in submission order, which would hide from the fence a launch that went to b instead of a"""
    import torch
    x = torch.zeros(16, device="cuda")
    held, ran = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        torch.cuda._sleep(int(MIN_DELAY_MS * _cycles_per_ms()))
        held.record()
    with torch.cuda.stream(b):
        x.fill_(1.0)
        ran.record()
    ran.synchronize()
    beside = not held.query()
    torch.cuda.synchronize()
    return beside


def pick_stream(others):
    """a non-blocking torch stream that runs beside every stream of `others`"""
    import torch
    for _ in range(64):
        s = torch.cuda.Stream()
        if all(runs_beside(s, o) for o in others):
            return s
    raise AssertionError("no stream found that runs beside %r: the fence could not see a launch on them" % (others,))


@functools.lru_cache(maxsize=None)
def side_stream():
    """the side stream of the fence: one that the null stream does not queue behind"""
    import torch
    return pick_stream((torch.cuda.default_stream(),))


def _bytes(t):
    """a device tensor as its bytes on the host"""
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().copy()


def fenced(call, inputs, outputs, side, delay_ms=None, prepare=None):
    """One run of the sequence above; delay_ms None is the quiet run: no delay, torch.cuda.synchronize() before and after the call,
    and call_ms is then the wall time of call plus synchronise.  `prepare` (optional) runs first, outside the fence, and leaves the
    device idle: it puts a plan into the state the call is to find.  Returns Fenced(result bytes per output, host values, whether the delay
    was still running when the call returned, call wall time, the delay's event time)."""
    import torch
    quiet = delay_ms is None
    if prepare is not None:
        prepare()
    poisoned = {b.data_ptr() for b, _ in inputs}
    results = [torch.empty_like(o) for o in outputs]
    for b, s in inputs:
        assert b.dtype == torch.float32 and b.shape == s.shape and b.is_contiguous() and s.is_contiguous()
        b.fill_(float("nan"))
    for o in outputs:
        assert o.is_contiguous()
        if o.data_ptr() not in poisoned:
            o.view(torch.uint8).fill_(SENTINEL)
    start, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 0 if quiet else int(delay_ms * _cycles_per_ms())
    torch.cuda.synchronize()
    early = None
    with torch.cuda.stream(side):
        if not quiet:
            start.record()
            torch.cuda._sleep(cycles)
            done.record()
        for b, s in inputs:
            b.copy_(s, non_blocking=True)
        if quiet:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = call(int(side.cuda_stream))
        if quiet:
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        if not quiet:
            early = not done.query()
        for r, o in zip(results, outputs):
            r.copy_(o, non_blocking=True)
    side.synchronize()
    torch.cuda.synchronize()
    return Fenced([_bytes(r) for r in results], host, early, 1e3 * (t1 - t0), 0.0 if quiet else start.elapsed_time(done))


def _same_host(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def same(a, b):
    """bit for bit: every result buffer byte by byte (NaN guards and sentinels in the padding included), host values as numbers"""
    return len(a.results) == len(b.results) and all(np.array_equal(x, y) for x, y in zip(a.results, b.results)) and _same_host(a.host, b.host)


def judge(fdr, name, call, inputs, outputs, side=None, exempt=None, prepare=None):
    """The quiet run (twice when the first one, which makes the workspaces and loads the kernels, took long: the second is then the
    quiet run), the delay sized from it, the fenced run, the delay condition asserted, one STREAM line, the Verdict.  `exempt`: the
    sentence of fdr.h that lets this entry wait (printed; the caller then does not judge `waits`)."""
    import torch
    side = side or side_stream()
    assert stream_flags(fdr, side) & HIP_STREAM_NON_BLOCKING, "the side stream must be non-blocking"
    assert int(side.cuda_stream) != 0 and int(side.cuda_stream) != int(torch.cuda.default_stream().cuda_stream)
    quiet = fenced(call, inputs, outputs, side, prepare=prepare)
    if quiet.call_ms > 2.0:
        again = fenced(call, inputs, outputs, side, prepare=prepare)
        assert same(quiet, again), "%s: two quiet runs differ: the call does not repeat bit for bit" % name
        quiet = again
    need = max(MIN_DELAY_MS, DELAY_FACTOR * quiet.call_ms)
    run = fenced(call, inputs, outputs, side, delay_ms=DELAY_MARGIN * need, prepare=prepare)
    assert run.delay_ms >= need, ("%s: the delay ran %.2f ms, below max(%g ms, %g x the quiet run's %.3f ms): the fence cannot judge"
                                  % (name, run.delay_ms, MIN_DELAY_MS, DELAY_FACTOR, quiet.call_ms))
    v = Verdict(same(run, quiet), not run.early, run.call_ms, quiet.call_ms, run.delay_ms)
    print("STREAM %s: call %.3f ms, quiet run %.3f ms, delay %.1f ms (%.0f x the quiet run, %.0f x the call): %s, %s"
          % (name, v.call_ms, v.quiet_ms, v.delay_ms, v.delay_ms / max(v.quiet_ms, 1e-6), v.delay_ms / max(v.call_ms, 1e-6),
             "ordered" if v.ordered else "NOT ORDERED", ("waits" if v.waits else "does not wait") + (" (exempt)" if exempt else "")))
    return v
