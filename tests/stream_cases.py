"""The delayed producer with decoys: what tests/test_gpu_streams.py uses to make a stream-ordering mistake of an entry point deterministic.

Every entry of the C ABI takes a stream and the Python layer passes torch's current one.  On the default (null) stream everything is ordered implicitly, so a launch,
clear or copy of a call that goes to another stream than the caller's shows only under `with torch.cuda.stream(S):` - and then only if the timing is unlucky.  A case
here removes the luck:

    S = torch.cuda.Stream()                         (torch's pool streams do not synchronise with the null stream)
    with torch.cuda.stream(S):
        delay                                       a kernel that keeps the stream busy for DELAY_MS
        produce                                     buf.copy_(true_value) into a buffer that holds a DECOY, queued behind the delay
        out = call(buf)                             the entry point under test
        pending = not event_after_delay.query()     the self-check: the delay was still running when the call returned
        result = out.cpu()                          read inside the context, on S

    form "S":        the delay is on S.  Work of the call that went to another stream runs at once: it reads the decoy, or writes before the call's own clears.
    form "default":  the delay is on the default stream, the call on S.  Work of the call that went to the null stream lands late: after S's kernels and after the
                     result was read.

THE DECOY RULE.  A decoy is a valid input, only another one: the true array rolled along its first axis (other rays, another image, the same pixel ids in another
order), or for offsets another monotone list with the same total.  A stale read gives a wrong number, never an out-of-range access: no case can fault by construction.

THE DELAY.  Measured on an MI355X with the parent commit's library: the slowest single covered call that returns without a synchronisation is renderD of the
82-triangle BVH scene through the Python layer, 0.070 ms from call to return (median of 30; p90 0.078, max 0.086); a whole case - the delay's launch, up to three producer
copies, the call, the event query - takes 0.04 to 0.40 ms of host time once its kernels are loaded (ISSUE_MS below collects it; the slowest is the variance denoiser's apply
with its three producers).  ENQUEUE_MS is that slowest case, and the delay ten times it, so that scheduling jitter of a 16-CPU cgroup cannot outlast it: 4 ms, far below
0.2 s.  The FIRST call of a kind in a process is another matter - loading a kernel's code object took up to 93 ms, the first launch on a new stream 5 ms - which is why
run_on_stream makes every early-returning call once on the default stream before the case.  torch.cuda._sleep counts device clock ticks, whose rate is calibrated once
per process against HIP events; should it not hold a stream for the time asked (checked at calibration), a chain of 2048^2 matrix products of the same measured length
takes its place."""
import contextlib
import gc
import time

import numpy as np

ENQUEUE_MS = 0.4          # ms, measured: see the module docstring
DELAY_MS = 10.0 * ENQUEUE_MS
FORMS = ("S", "default")

_delay = None
ISSUE_MS = []          # host time of every case so far, from the delay's launch to the call's return: what ENQUEUE_MS was read from


def _calibrate(torch):
    """-> queue(): puts about DELAY_MS of work on the current stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ticks = 20_000_000
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(ticks)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    if ms > 1.0:
        n = max(1, int(ticks * DELAY_MS / ms))
        return lambda: torch.cuda._sleep(n)
    a = torch.randn((2048, 2048), device="cuda")
    b = torch.empty_like(a)
    torch.mm(a, a, out=b)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(8):
        torch.mm(a, a, out=b)
    e1.record()
    torch.cuda.synchronize()
    reps = max(1, int(np.ceil(DELAY_MS / (e0.elapsed_time(e1) / 8))))

    def chain():
        for _ in range(reps):
            torch.mm(a, a, out=b)
    return chain


def calibrate(torch):
    """once per process, outside every case (it synchronises)"""
    global _delay
    if _delay is None:
        _delay = _calibrate(torch)


def delay(torch):
    """queues the delay on the current stream; -> an event recorded behind it"""
    calibrate(torch)
    _delay()
    ev = torch.cuda.Event()
    ev.record()
    return ev


def decoy_of(a):
    """another valid input of the same kind: the rows of `a` in another order"""
    a = np.asarray(a)
    d = np.roll(a, len(a) // 3 + 1, axis=0)
    assert d.shape == a.shape and not np.array_equal(d, a), "the decoy must differ from the true input"
    return np.ascontiguousarray(d)


class Slot:
    """One device input of a call: `buf` holds the decoy until produce() copies the true value over it (on the current stream)."""

    def __init__(self, torch, true, decoy=None):
        true = np.ascontiguousarray(true)
        decoy = decoy_of(true) if decoy is None else np.ascontiguousarray(decoy)
        assert decoy.shape == true.shape and decoy.dtype == true.dtype and not np.array_equal(decoy, true)
        self.true_np = true
        self._true = torch.from_numpy(true).cuda()
        self._decoy = torch.from_numpy(decoy).cuda()
        self.buf = self._decoy.clone()

    def reset(self):
        self.buf.copy_(self._decoy)

    def produce(self):
        self.buf.copy_(self._true)


def run_on_stream(torch, stream, form, slots, call, fetch, returns_early=True, follows_at_once=False):
    """One case in one form -> what fetch(call()) returns, read on `stream` inside the context.

    form: "S" (delay on `stream`) or "default" (delay on the default stream).  slots: the inputs produced behind the delay.  returns_early: the entry point is documented
    to return without synchronising, so the delay must still be running when it does (entries that synchronise inside pass False and skip this self-check).  Such a call
    is first made once on the default stream with the true inputs: the first call of a kind loads its kernels and may grow scratch, for which the host or the stream
    waits, and the self-check is about the calls that follow.  follows_at_once: no warm-up, no reset and no device synchronisation ahead of the case - it follows
    whatever the test has just queued (a handle whose create was issued under another stream); the test has reset the slots before."""
    assert form in FORMS
    calibrate(torch)
    if not follows_at_once:
        if returns_early:
            run_plain(torch, slots, call, lambda out: None)
        for s in slots:
            s.reset()
        torch.cuda.synchronize()
    gc_was_on = gc.isenabled()
    gc.disable()          # (a collection of the whole suite's heap between the delay and the query would outlast the delay)
    try:
        with torch.cuda.stream(stream):
            t0 = time.perf_counter()
            if form == "S":
                ev = delay(torch)
            else:
                with torch.cuda.stream(torch.cuda.default_stream()):
                    ev = delay(torch)
            for s in slots:
                s.produce()
            out = call()
            pending = not ev.query()
            issue_ms = (time.perf_counter() - t0) * 1e3
            result = fetch(out)
    finally:
        if gc_was_on:
            gc.enable()
        torch.cuda.synchronize()          # (also after a failed call: nothing of this case is left running behind the next one)
    if returns_early:
        ISSUE_MS.append(issue_ms)
        print("issued in %.3f ms behind a delay of %g ms on %s" % (issue_ms, DELAY_MS, form))
        assert pending, "the delay had ended before the call returned: the case proves nothing (DELAY_MS = %g)" % DELAY_MS
    return result


def run_plain(torch, slots, call, fetch):
    """the same call on the default stream, no delay, inputs in place"""
    for s in slots:
        s.produce()
    torch.cuda.synchronize()
    result = fetch(call())
    torch.cuda.synchronize()
    return result


@contextlib.contextmanager
def env_var(monkeypatch, name, value):
    monkeypatch.setenv(name, value)
    try:
        yield
    finally:
        monkeypatch.delenv(name)
