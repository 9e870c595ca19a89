"""Holding one HIP stream back, for the stream-order tests (test_gpu_stream_order.py).

Ordering between streams, and between the host and the device, cannot be tested by running the same work twice: the kernels
are short, the host queues slowly, and a missing wait goes unnoticed because the other stream has long finished.  Here one
stream is held back by a spin kernel of ONE thread in ONE block (torch.cuda._sleep: it holds a stream, not the chip, and
always terminates) for longer than everything the other stream does in that window.  A missing wait then reads a stale
value on every run; correct ordering gives results that are bit-identical with and without the delay.

  calibrate()      once per process: cycles per millisecond of torch.cuda._sleep, from two HIP-event timings that must be
                   linear within a factor of two; a chain of plain torch kernels of measured duration when _sleep is missing
                   or does not delay.
  hold(stream, ms) one delay of `ms` on `stream`; more than CAP_MS is refused.
  delay_for(T)     the sizing rule, a property of the harness and not a tolerance on the code under test:
                   D = max(4 * T, 20 ms), T = the wall time (measured by the test on its undelayed run) of the span that must
                   fit inside the delay; the factor 4 covers the run-to-run jitter of that span.  A D above the cap is an
                   error: the test shrinks its shape, the cap stays.
  late_side(ops, D) context manager: ops.SIDE_LAUNCH_HOOK holds the side stream for D at the first side launch after every
                   join (= of every backward; after a data-parallel bucket's join as well), so everything queued on it
                   afterwards is behind the delay; counts the launches per kind.  D = 0: count only.
  late_main(D)     holds the current stream for D.
  independent_streams(n)  streams SEEN to run beside the current stream (two streams that share a hardware queue run one
                   behind the other: holding one holds both); the tests hold these.
  self_check()     the harness on torch alone: a copy behind a held stream is not seen by another stream before it waits.

Values seen on the MI355X (tests/test_gpu_stream_order.py prints them with -s): see that module's docstring.
"""
import contextlib
import time

import torch

CAP_MS = 500.0
MIN_MS = 20.0
FACTOR = 4.0

_CAL = None          # ("sleep", cycles per ms) or ("chain", tensor, ms per kernel)
_SELF = None


def _timed_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def calibrate():
    """What one millisecond of delay costs; measured once per process on the current device (synchronises it)."""
    global _CAL
    if _CAL is not None:
        return _CAL
    torch.cuda.synchronize()
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        sleep(1000)                                            # loads the kernel
        torch.cuda.synchronize()
        c, t1 = 100000, 0.0
        while c <= 10 ** 9:                                    # what a cycle is on this chip is measured, not assumed
            t1 = _timed_ms(lambda: sleep(c))
            if t1 >= 2.0:
                break
            c *= 10
        if t1 >= 2.0:
            t2 = _timed_ms(lambda: sleep(4 * c))
            assert 2.0 <= t2 / t1 <= 8.0, "torch.cuda._sleep is not linear: {} cycles {:.3f} ms, {} cycles {:.3f} ms".format(
                c, t1, 4 * c, t2)
            _CAL = ("sleep", 4 * c / t2)
            return _CAL
    # no _sleep, or one that does not delay: a chain of plain kernels (this one does occupy the chip)
    buf = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
    buf.add_(1.0)
    torch.cuda.synchronize()
    t1 = _timed_ms(lambda: [buf.add_(1.0) for _ in range(8)]) / 8.0
    t2 = _timed_ms(lambda: [buf.add_(1.0) for _ in range(32)]) / 32.0
    assert t1 > 0 and 0.5 <= t2 / t1 <= 2.0, "the fallback delay kernel is not linear: {:.4f} vs {:.4f} ms".format(t1, t2)
    _CAL = ("chain", buf, t2)
    return _CAL


def hold(stream, ms):
    """Queue one delay of `ms` milliseconds on `stream` (bounded: at most CAP_MS)."""
    ms = float(ms)
    if not 0.0 <= ms <= CAP_MS:
        raise ValueError("a delay of {} ms is refused: the cap is {} ms (shrink the test's shape instead)".format(ms, CAP_MS))
    if ms == 0.0:
        return
    cal = calibrate()
    with torch.cuda.stream(stream):
        if cal[0] == "sleep":
            torch.cuda._sleep(int(ms * cal[1]))
        else:
            for _ in range(int(ms / cal[2]) + 1):
                cal[1].add_(1.0)


def delay_for(t_ms, floor_ms=MIN_MS):
    """D for a span measured at `t_ms` on the undelayed run."""
    d = max(FACTOR * float(t_ms), float(floor_ms))
    assert d <= CAP_MS, "the span took {:.1f} ms: a delay of {:.1f} ms is above the cap of {} ms -- shrink the shape".format(
        t_ms, d, CAP_MS)
    return d


class Span(object):
    """Wall time of a span on the undelayed run, device idle at both ends: with Span() as s: ...; s.ms"""

    def __enter__(self):
        torch.cuda.synchronize()
        self._t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.ms = (time.perf_counter() - self._t0) * 1e3
        return False


KINDS = ("conv2d", "conv3d", "deconv")


@contextlib.contextmanager
def late_side(ops, ms):
    """Every side launch is counted per kind; the first one after a join first holds the side stream for `ms`."""
    counts = dict((k, 0) for k in KINDS)
    counts["holds"] = 0

    def hook(kind, side):
        if ms and not ops._Side.pending:
            hold(side, ms)
            counts["holds"] += 1
        counts[kind] += 1

    if ms:
        calibrate()                     # never from inside a backward: it synchronises
    prev = ops.SIDE_LAUNCH_HOOK
    ops.SIDE_LAUNCH_HOOK = hook
    try:
        yield counts
    finally:
        ops.SIDE_LAUNCH_HOOK = prev


def late_main(ms):
    """Hold the current stream for `ms`: what the host queues on it next waits, every other stream does not."""
    hold(torch.cuda.current_stream(), ms)


_INDEPENDENT = []
_PROBED = []


def _runs_beside(main, cand, ms=5.0):
    """Does work queued on `main` run while `cand` is held?"""
    a = torch.full((1 << 16,), 7.0, device="cuda")
    b = torch.zeros_like(a)
    torch.cuda.synchronize()
    cand.wait_stream(main)
    with torch.cuda.stream(cand):
        hold(cand, ms)
        b.copy_(a)
    with torch.cuda.stream(main):
        early = b.clone()
    torch.cuda.synchronize()
    return bool((early == 0).all())


def independent_streams(n=1):
    """`n` streams (cached per process) that were SEEN to run beside the current stream and beside each other.

    HIP maps its streams onto a few hardware queues (4 by default), torch hands out streams from a pool of 32, and two
    streams that share a queue run one behind the other: holding one holds both, and a test that delays such a stream
    proves nothing.  Which pool stream shares the current stream's queue depends on how many streams the process made
    before, so candidates are probed (a 5 ms hold each) until enough independent ones are found; None when the pool has
    none."""
    calibrate()
    main = torch.cuda.current_stream()
    while len(_INDEPENDENT) < n and len(_PROBED) < 32:
        cand = torch.cuda.Stream()
        _PROBED.append(cand)
        if all(_runs_beside(other, cand) and _runs_beside(cand, other) for other in [main] + _INDEPENDENT):
            _INDEPENDENT.append(cand)
    return list(_INDEPENDENT[:n]) if len(_INDEPENDENT) >= n else None


def self_check(ms=40.0):
    """(ok, text).  On a side stream: hold, then b.copy_(a).  The main stream reads b without waiting and must see the old
    value; after wait_stream it sees the new one; the delay measured with events is at least ms / 2."""
    global _SELF
    if _SELF is not None:
        return _SELF
    calibrate()
    found = independent_streams(1)
    if found is None:
        _SELF = (False, "none of {} pool streams runs beside the current stream".format(len(_PROBED)))
        return _SELF
    main, side = torch.cuda.current_stream(), found[0]
    a = torch.full((1 << 20,), 7.0, device="cuda")
    b = torch.zeros_like(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        e0.record()
        hold(side, ms)
        b.copy_(a)
        e1.record()
    early = b.clone()                   # the main stream, not waiting
    main.wait_stream(side)
    late = b.clone()
    torch.cuda.synchronize()
    measured = e0.elapsed_time(e1)
    stale, fresh = bool((early == 0).all()), bool((late == 7.0).all())
    ok = stale and fresh and measured >= ms / 2
    _SELF = (ok, "delay asked {:.1f} ms, measured {:.2f} ms ({}); unordered read saw the old value: {}; ordered read saw the "
                 "new value: {}; pool streams probed: {}".format(ms, measured, calibrate()[0], stale, fresh, len(_PROBED)))
    return _SELF
