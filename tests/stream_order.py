"""Helpers of tests/_dist_gpu_worker_stream_order.py (not a conftest, no fixtures): what it takes to make every stream wait of the sequence-parallel
drivers decide a result on ONE GPU.

  Delay       a device-side delay on the current stream (`torch.cuda._sleep`, calibrated once with events; a calibrated chain of `torch.mm` where
              the sleep kernel proves unusable), never touching the host;
  StandIns    world-1 replacements of `dist.all_to_all_single` / `dist.all_gather_into_tensor` that run on the stream they are called under: in the
              slow-communication regime they fill the receive tensor with NaN, delay, then copy; otherwise they copy at once;
  WaitFilter  `torch.cuda.Stream.wait_stream` patched so that the waits of ONE role (which stream waits on which) become no-ops: the negative controls;
  HostSyncs   counts host synchronisations made inside watched driver calls, and times those calls with events.

Nothing here edits lightx2v_amd: every hook is a patch applied by the worker process to itself."""
import math

import torch
import torch.distributed as dist

NAN = float("nan")
ROLES = ("comm_waits_compute", "compute_waits_comm", "branch_waits_calling", "calling_waits_branch")


def timed_ms(fn):
    """Device time of what fn() enqueues on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Delay:
    """delay(ms): keep the current stream busy for about `ms` milliseconds, without a host synchronisation."""

    PROBE_CYCLES = 1 << 21

    def __init__(self):
        self.kind, self.per_ms = "torch.cuda._sleep", None
        try:
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
            ms = min(timed_ms(lambda: torch.cuda._sleep(self.PROBE_CYCLES)) for _ in range(3))
            self.per_ms = self.PROBE_CYCLES / max(ms, 1e-6)
            self.check_ms = timed_ms(lambda: self(2.0))
            usable = 1.5 <= self.check_ms <= 20.0
        except (AttributeError, RuntimeError):
            usable = False
        if not usable:  # a chain of 1024^3 fp32 products, each timed once
            self.kind = "torch.mm chain"
            self._a = torch.ones((1024, 1024), dtype=torch.float32, device="cuda")
            self._c = torch.empty_like(self._a)
            torch.mm(self._a, self._a, out=self._c)
            torch.cuda.synchronize()
            self.per_ms = 16 / timed_ms(lambda: [torch.mm(self._a, self._a, out=self._c) for _ in range(16)])  # products per millisecond
            self.check_ms = timed_ms(lambda: self(2.0))
        assert self.check_ms >= 1.5, f"a 2 ms delay ({self.kind}) measured {self.check_ms:.3f} ms: no usable device-side delay"

    def __call__(self, ms):
        if ms <= 0:
            return
        if self.kind == "torch.cuda._sleep":
            torch.cuda._sleep(int(ms * self.per_ms))
        else:
            for _ in range(max(1, math.ceil(ms * self.per_ms))):
                torch.mm(self._a, self._a, out=self._c)


def serialized_behind(x, y, delay, ms=5.0):
    """Does work enqueued on stream `y` behind a delay on stream `x`, with no wait between them, start only when the delay has ended?  Then the two
    share a hardware queue, the runtime orders them by itself, and no delay can make a missing wait between them show."""
    import time

    torch.cuda.synchronize()
    e = torch.cuda.Event()
    t0 = time.perf_counter()
    with torch.cuda.stream(x):
        delay(ms)
    with torch.cuda.stream(y):
        e.record()
    e.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return dt > ms / 2


class StandIns:
    """The collectives of a group of one, on the current stream, with no host access.  `comm_delay_ms` > 0 is the slow-communication regime.
    `calls` records (name, stream handle) of every call."""

    def __init__(self, delay):
        self.delay, self.comm_delay_ms, self.calls = delay, 0.0, []
        self._real = None

    def transfer(self, name, pairs):
        """pairs: (receive tensor, source tensor)...  One collective: NaN, delay, copy in the slow regime; the copy alone otherwise."""
        self.calls.append((name, torch.cuda.current_stream().cuda_stream))
        if self.comm_delay_ms > 0:
            for out, _ in pairs:
                out.fill_(NAN)
            self.delay(self.comm_delay_ms)
        for out, inp in pairs:
            assert out.shape == inp.shape and out.data_ptr() != inp.data_ptr(), (name, tuple(out.shape), tuple(inp.shape))
            out.copy_(inp)

    def all_to_all_single(self, out, inp, output_split_sizes=None, input_split_sizes=None, group=None, async_op=False):
        assert not async_op
        self.transfer("all_to_all_single", [(out, inp)])

    def all_gather_into_tensor(self, out, inp, group=None, async_op=False):
        assert not async_op
        self.transfer("all_gather_into_tensor", [(out, inp)])

    def install(self):
        self._real = (dist.all_to_all_single, dist.all_gather_into_tensor)
        dist.all_to_all_single, dist.all_gather_into_tensor = self.all_to_all_single, self.all_gather_into_tensor

    def restore(self):
        dist.all_to_all_single, dist.all_gather_into_tensor = self._real


class WaitFilter:
    """While `role` names one of ROLES, every `waiter.wait_stream(waited)` of that role returns without waiting.  A wait's role follows from the
    streams alone: the communication streams are what `comm_ids()` returns (stream handles), the calling stream is the default stream, every other
    stream is a CFG branch stream."""

    def __init__(self):
        self.role, self.skipped, self.seen = None, 0, {}
        self.comm_ids = lambda: set()
        self.calling = torch.cuda.default_stream().cuda_stream
        real = torch.cuda.Stream.wait_stream
        flt = self

        def wait_stream(self, other):
            role = flt.role_of(self, other)
            flt.seen[role] = flt.seen.get(role, 0) + 1
            if role is not None and role == flt.role:
                flt.skipped += 1
                return None
            return real(self, other)

        torch.cuda.Stream.wait_stream = wait_stream

    def role_of(self, waiter, waited):
        comm, w, o = self.comm_ids(), waiter.cuda_stream, waited.cuda_stream
        if w in comm:
            return ROLES[0]
        if o in comm:
            return ROLES[1]
        if o == self.calling and w != self.calling:
            return ROLES[2]
        if w == self.calling and o != self.calling:
            return ROLES[3]
        return None


class HostSyncs:
    """Host synchronisations inside watched calls: torch.cuda.synchronize, Stream.synchronize and Event.synchronize (what
    tests/_dist_gpu_worker_ring.py counts), and .item() / .cpu() / .tolist() of a device tensor.  With `timing` on, every watched call marked `timed`
    is bracketed by two events on the stream it is called under."""

    def __init__(self):
        self.depth, self.count, self.timing, self._events = 0, 0, False, []
        me = self

        def counted(fn, is_tensor=False):
            def wrapped(*a, **kw):
                if me.depth > 0 and (not is_tensor or a[0].is_cuda):
                    me.count += 1
                return fn(*a, **kw)

            return wrapped

        torch.cuda.synchronize = counted(torch.cuda.synchronize)
        torch.cuda.Stream.synchronize = counted(torch.cuda.Stream.synchronize)
        torch.cuda.Event.synchronize = counted(torch.cuda.Event.synchronize)
        for name in ("item", "cpu", "tolist"):
            setattr(torch.Tensor, name, counted(getattr(torch.Tensor, name), is_tensor=True))

    def watch(self, cls, name, timed=False):
        real, me = getattr(cls, name), self

        def wrapped(*a, **kw):
            ev = None
            if timed and me.timing:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            me.depth += 1
            try:
                return real(*a, **kw)
            finally:
                me.depth -= 1
                if ev is not None:
                    ev[1].record()
                    me._events.append(ev)

        setattr(cls, name, wrapped)

    def take_durations_ms(self):
        torch.cuda.synchronize()
        out, self._events = [a.elapsed_time(b) for a, b in self._events], []
        return out


def poison(obj, value=NAN):
    """`value` into every floating tensor of a driver's buffer table (dicts / lists / tuples of tensors): what a run reads without the wait that
    should have ordered it is then never the previous run's correct data."""
    if isinstance(obj, torch.Tensor):
        if obj.is_floating_point():
            obj.fill_(value)
    elif isinstance(obj, dict):
        for v in obj.values():
            poison(v, value)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            poison(v, value)


def differing(got, want):
    """How many elements of `got` are NaN or differ from `want`."""
    return int(((got != want) | torch.isnan(got)).sum())
