"""Helpers of tests/test_gpu_stream_matrix.py and tests/test_gpu_threads.py: a calibrated delay on a stream, and a thin proxy around the
loaded library that runs a callback directly before and after each entry point of tests/stream_matrix.py's `LISTED`."""
import contextlib
import time

from tests import stream_matrix as st
from twisterl_amd import _lib

_CAL = {}
CAL_CYCLES = 20_000_000


def cycles_per_ms():
    """How many cycles of torch.cuda._sleep last one millisecond on this GPU: measured once per process with two events around a sleep
    of CAL_CYCLES (the median of three), after one sleep that pays for the kernel's load."""
    if "v" not in _CAL:
        import torch
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(CAL_CYCLES)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        mid = sorted(ms)[1]
        assert mid > 0.5, ms                               # (a sleep that does not sleep would make every delay of these tests empty)
        _CAL["v"], _CAL["ms"] = CAL_CYCLES / mid, ms
    return _CAL["v"]


def null_stream():
    import torch
    s = torch.cuda.default_stream()
    assert s.cuda_stream == 0, "torch's default stream is not the legacy null stream: the delays of these tests would go elsewhere"
    return s


def delay(stream, ms):
    """Enqueues a delay of `ms` milliseconds on `stream`, then an event -> the event (pending while the delay runs)."""
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms()))
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


PROBE_MS = 20.0


def independent_stream(others=(), candidates=12):
    """A non-blocking torch.cuda.Stream whose work does not queue behind the null stream's (nor behind that of `others`).

    The HIP runtime maps every stream onto one of a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) in turn, and two streams
    that share a hardware queue run in order, whatever their flags say: on such a stream "the call did not wait for unrelated
    null-stream work" is false for every call, the library's or anyone's.  That is the runtime's mapping and no property of the code
    under test, so the tests choose their stream: each candidate gets one small kernel while a short delay runs on the null stream
    (and on each of `others`), and the first whose kernel finishes under the delay is taken.  None among `candidates`: the test fails."""
    import torch
    x = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(candidates):
        s = torch.cuda.Stream()
        if s.cuda_stream == 0 or any(s.cuda_stream == o.cuda_stream for o in others):
            continue
        pending = [delay(b, PROBE_MS) for b in (null_stream(), *others)]
        with torch.cuda.stream(s):
            x.add_(1.0)
        done = torch.cuda.Event()
        done.record(s)
        done.synchronize()
        free = not any(z.query() for z in pending)                # every delay still runs: the kernel did not wait for any of them
        torch.cuda.synchronize()
        if free:
            return s
    raise AssertionError(f"none of {candidates} streams runs beside the null stream: every one shares its hardware queue")


class EntryProxy:
    """Stands in for the loaded library (`_lib.lib()`): every attribute is the library's, but a listed entry point is wrapped --
    before(name) -> token runs directly before the call, after(name, token, status) directly after it; `calls` keeps
    (name, wall milliseconds, status) of each."""

    def __init__(self, real, before=None, after=None):
        self._real, self._before, self._after, self.calls = real, before, after, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in st.LISTED:
            return fn

        def wrapped(*args):
            token = self._before(name) if self._before else None
            t0 = time.perf_counter()
            status = fn(*args)
            self.calls.append((name, (time.perf_counter() - t0) * 1e3, status))
            if self._after:
                self._after(name, token, status)
            return status
        return wrapped


@contextlib.contextmanager
def entry_proxy(before=None, after=None):
    real = _lib.lib()
    assert not isinstance(real, EntryProxy)
    proxy = EntryProxy(real, before, after)
    _lib._lib = proxy
    try:
        yield proxy
    finally:
        _lib._lib = real


@contextlib.contextmanager
def delayed_entries(stream, ms):
    """Mode 1: directly before each listed entry point a delay and an event m on `stream`.  m is pending immediately before the call;
    an entry point that waits for its stream (`WAITS`) returns with m complete -- it did not return sooner than the delay lasts --,
    unless it refused its arguments before it touched the device."""
    def before(name):
        m = delay(stream, ms)
        assert not m.query(), f"{name}: the delay of {ms:.1f} ms had ended before the call began"
        return m

    def after(name, m, status):
        if status == _lib.TW_OK and name in st.WAITS:
            assert m.query(), f"{name} returned while the delay in front of it on the caller's stream was still running: it did not wait for that stream"
    with entry_proxy(before, after) as proxy:
        yield proxy
