"""Stream-order harness for the GPU tests (not a test module, not a conftest).

Every `_device` entry point promises that its work is queued on the caller's
stream and that the call itself does not wait.  A test that synchronises
before and after one call cannot see a kernel, memset or copy queued on the
wrong stream, an event wait missing in one direction, scratch rewritten while
the previous call still reads it, or a hidden host wait.  `Sandwich` runs the
call between work that is still pending on the stream:

1. input buffers hold decoy bytes (seeded random, same size, never all zero),
   outputs hold the poison 0xA5, the real inputs wait in staging tensors; one
   device-wide wait;
2. `stall()` keeps the stream busy for a measured time and records `done`;
3. on the stream, staging is copied into the inputs and the outputs are
   poisoned once more (a fill or kernel that ran ahead of the stream is wiped
   out again);
4. the library call(s), with `hip_stream` = the stalled stream;
5. on the stream, every output is copied into a snapshot, then the inputs are
   overwritten with the decoy and the outputs with a second poison 0x5A;
6. for a call documented not to synchronise: `done.query()` must still be
   False — the call returned while the stream was stalled;
7. the stream is synchronised; the snapshots must equal the expected bytes and
   the live outputs must be all 0x5A.

A read that ran ahead of the stream sees the decoy, work left on a stream the
caller's does not wait for leaves 0xA5 in the snapshot (or lands after it, on
the 0x5A), a hidden host wait trips step 6.

The sequence is first run once without a stall and synchronised: that grows
every scratch buffer (no hipMalloc / hipFree under the stall), and the host
time from the first enqueue to the last sizes the stall.

Stall length (measured on the MI355X, profiles/stream_order/README.md):
torch.cuda._sleep spins about 2.39 million units per ms.  Behind a stall the
steps 3 to 5 of a case take the host 0.06 to 0.77 ms (the slowest: two deep
tiled batches on two streams, 0.51 - 0.77 ms; the whole pipeline, 0.43 -
0.59 ms).  The unstalled first run takes 0.08 to 2 ms where everything is
loaded, and 20 - 24 ms where it loads a kernel module for the first time in
the process.  Between runs the same case moved by up to 40%.
STALL_FLOOR_MS = 60 is about eighty times the slowest stalled enqueue seen,
so that a host thread
descheduled for several scheduler slices on a shared machine still returns
inside the stall; STALL_MULTIPLE = 20 only matters where the first run was
slow, and then errs long.  A stall never exceeds STALL_CAP_MS.  A stall too
short fails step 6; it cannot pass silently.
"""
import time

import numpy as np

from gpu_util import torch_cuda

POISON = 0xA5        # outputs before the call
LATE_POISON = 0x5A   # outputs after the snapshot

STALL_MULTIPLE = 20    # x the dry run's host enqueue time
STALL_FLOOR_MS = 60.0
STALL_CAP_MS = 2000.0  # every stall ends by itself, soon

_CAL = {}


def _sleep_fn(torch):
    return getattr(torch.cuda, "_sleep", None)


def cycles_per_ms():
    """Spin cycles of torch.cuda._sleep per millisecond, measured once a
    process with two timing events around a fixed sleep (or, without _sleep,
    the elementwise passes over a 64 MiB tensor per millisecond)."""
    if "cpm" in _CAL:
        return _CAL["cpm"]
    torch = torch_cuda()
    s = torch.cuda.Stream()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    sleep = _sleep_fn(torch)
    if sleep is None:
        _CAL["filler"] = torch.zeros(16 << 20, dtype=torch.float32, device="cuda")
    amount = 1_000_000 if sleep is not None else 8
    for _ in range(4):
        with torch.cuda.stream(s):
            _spin(torch, amount)  # warm: module load, clocks
            e0.record(s)
            _spin(torch, amount)
            e1.record(s)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 2.0:
            break
        amount *= 8
    assert ms > 0, "stall calibration measured no time"
    _CAL["cpm"] = amount / ms
    print(f"stream_order calibration: {_CAL['cpm']:.0f} spin units per ms "
          f"({amount} took {ms:.3f} ms)")
    return _CAL["cpm"]


def _spin(torch, amount):
    sleep = _sleep_fn(torch)
    if sleep is not None:
        sleep(int(amount))
    else:
        x = _CAL["filler"]
        for _ in range(int(amount)):
            x.add_(1.0)


def stall(stream, ms):
    """Keep `stream` busy for about `ms` milliseconds with a kernel that ends
    by itself, then record and return an event."""
    torch = torch_cuda()
    ms = min(float(ms), STALL_CAP_MS)
    amount = max(1, int(cycles_per_ms() * ms))
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        _spin(torch, amount)
        done.record(stream)
    return done


def decoy_like(arr, seed):
    """Seeded random bytes of arr's size that differ from it and are not all
    zero."""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    d = np.random.default_rng(seed).integers(1, 256, raw.size, dtype=np.uint8)
    same = d == raw
    d[same] ^= 0xFF
    d[d == 0] = 1
    return d


class _Buf:
    pass


class Sandwich:
    """One library call, or a sequence of calls, between pending work on a
    stream that is neither torch's current stream nor the null stream.

        sw = Sandwich("label")
        d_in = sw.input(frames)                     # device tensor (uint8)
        d_out = sw.output(nbytes, expect)           # device tensor, poisoned
        sw.run(lambda sw: lib_call(..., stream=sw.hip_stream))

    `expect` is a uint8 array the snapshot must equal byte for byte, or a
    function of the snapshot (a numpy uint8 array) that raises AssertionError,
    or a dict {"dry": ..., "stalled": ...} of those for a call whose handle
    carries state from the dry run into the stalled one.  Inside the call,
    `sw.snapshot(tensor, expect, name)` takes a snapshot between two calls and
    `sw.still_stalled(what)` is step 6 ahead of a call that blocks by contract.
    A second stream (n_streams=2) is idle: buffers made with stream=1 are
    loaded, snapshot and poisoned on it.
    """

    def __init__(self, label, n_streams=1, seed=0, repoison=True):
        torch = torch_cuda()
        self.torch = torch
        self.label = label
        self.streams = []
        for _ in range(n_streams):
            self.streams.append(self.new_stream())
        self.inputs, self.outputs, self.snaps = [], [], []
        self.seed = seed
        self.repoison = repoison  # step 3 poisons the outputs again on the stream
        self.phase = None
        self.done = None
        self.dry_ms = None
        self.stall_ms = None
        self.stalled_ms = None
        self.keep = []  # anything the stream may still use
        self._pending = []

    def new_stream(self):
        """A stream that is not the null stream, not torch's current stream
        (tests before this one may have made any pool stream current, and
        torch hands its pool out in turn) and none of this sandwich's."""
        torch = self.torch
        avoid = {0, torch.cuda.current_stream().cuda_stream}
        avoid |= {s.cuda_stream for s in self.streams}
        for _ in range(64):
            s = torch.cuda.Stream()
            if s.cuda_stream not in avoid:
                return s
        raise AssertionError("no stream apart from the current one")

    @property
    def stream(self):
        return self.streams[0]

    @property
    def hip_stream(self):
        return self.streams[0].cuda_stream

    def hip_stream_of(self, i):
        return self.streams[i].cuda_stream

    # ---- buffers -----------------------------------------------------------

    def input(self, arr, stream=0):
        torch = self.torch
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()
        b = _Buf()
        b.stream = stream
        b.staging = torch.from_numpy(raw).to("cuda")
        b.decoy = torch.from_numpy(decoy_like(raw, self.seed + 101 * len(self.inputs) + 7)).to("cuda")
        b.live = b.decoy.clone()
        self.inputs.append(b)
        return b.live

    def output(self, nbytes, expect, stream=0, name=None):
        torch = self.torch
        b = _Buf()
        b.stream = stream
        b.name = name or f"output {len(self.outputs)}"
        b.expect = expect
        b.live = torch.full((max(int(nbytes), 1),), POISON, dtype=torch.uint8, device="cuda")
        b.snap = torch.zeros_like(b.live)
        self.outputs.append(b)
        return b.live

    def snapshot(self, tensor, expect, name, stream=0):
        """Inside the call: copy `tensor` as it stands at this point of the
        stream.  The snapshot tensors are made in the dry run and reused, so
        nothing is allocated under the stall."""
        i = self._snap_i
        self._snap_i += 1
        if i == len(self.snaps):
            b = _Buf()
            b.snap = self.torch.zeros_like(tensor)
            self.snaps.append(b)
        b = self.snaps[i]
        b.name, b.expect, b.stream = name, expect, stream
        with self.torch.cuda.stream(self.streams[stream]):
            b.snap.copy_(tensor, non_blocking=True)

    def still_stalled(self, what):
        """Step 6: the calls so far returned while the stream was stalled."""
        if self.phase != "stalled":
            return
        assert not self.done.query(), (
            f"{self.label}: {what} returned only after the stall of {self.stall_ms:.0f} ms had "
            f"ended: a host wait in a call documented to have none (or a stall too short: the "
            f"dry run enqueued in {self.dry_ms:.3f} ms)")
        if self._pending:
            self._check_pending()
            self._pending = []

    def pending(self, stream, what):
        """The work queued on idle stream `stream` so far has not finished
        while the first stream is stalled: it waits for that stream."""
        if self.phase != "stalled":
            return
        ev = self.torch.cuda.Event()
        ev.record(self.streams[stream])
        self._pending.append((ev, what))

    def _check_pending(self):
        # looked at after the whole sequence is queued, so unordered work on
        # the idle stream has had the rest of the enqueue time to finish
        finished = [what for ev, what in self._pending if ev.query()]
        assert not self.done.query(), f"{self.label}: the stall ended before step 6"
        assert not finished, (f"{self.label}: {finished[0]} finished while the stream it must "
                              f"wait for was still stalled")

    # ---- the run -----------------------------------------------------------

    def _prepare(self, real):
        torch = self.torch
        for b in self.inputs:
            b.live.copy_(b.staging if real else b.decoy)
        for b in self.outputs:
            b.live.fill_(POISON)
            b.snap.zero_()
        for b in self.snaps:
            b.snap.zero_()
        torch.cuda.synchronize()

    def _sequence(self, call):
        """Steps 3 to 5; returns the host time from the first enqueue to the
        last, in ms."""
        torch = self.torch
        self._snap_i = 0
        t0 = time.perf_counter()
        for b in self.inputs:
            with torch.cuda.stream(self.streams[b.stream]):
                b.live.copy_(b.staging, non_blocking=True)
        if self.repoison:
            for b in self.outputs:
                with torch.cuda.stream(self.streams[b.stream]):
                    b.live.fill_(POISON)
        call(self)
        for b in self.outputs:
            with torch.cuda.stream(self.streams[b.stream]):
                b.snap.copy_(b.live, non_blocking=True)
        for b in self.inputs:
            with torch.cuda.stream(self.streams[b.stream]):
                b.live.copy_(b.decoy, non_blocking=True)
        for b in self.outputs:
            with torch.cuda.stream(self.streams[b.stream]):
                b.live.fill_(LATE_POISON)
        return (time.perf_counter() - t0) * 1e3

    def _check(self, phase):
        for b in self.outputs + self.snaps[:self._snap_i]:
            expect = b.expect[phase] if isinstance(b.expect, dict) else b.expect
            got = b.snap.cpu().numpy()
            where = f"{self.label} ({phase} run): snapshot of {b.name}"
            if callable(expect):
                try:
                    expect(got)
                except AssertionError as e:
                    raise AssertionError(f"{where}: {e}") from None
                continue
            want = np.ascontiguousarray(expect).view(np.uint8).reshape(-1)
            assert got.size == want.size, f"{where}: {got.size} bytes, expected {want.size}"
            bad = np.flatnonzero(got != want)
            if bad.size == 0:
                continue
            poisoned = int((got[bad] == POISON).sum())
            if poisoned == bad.size:
                raise AssertionError(
                    f"{where}: {bad.size} of {got.size} bytes still hold the poison 0xA5, first "
                    f"at {bad[0]}: they were written after the snapshot, never, or before the "
                    f"stream reached the call")
            raise AssertionError(
                f"{where}: wrong bytes at {bad.size} of {got.size} places, first at {bad[0]} "
                f"({got[bad[0]]:#x}, expected {want[bad[0]]:#x}); {poisoned} of them hold the "
                f"poison 0xA5 (a read ahead of the stream sees the decoy input)")
        for b in self.outputs:
            live = b.live.cpu().numpy()
            late = np.flatnonzero(live != LATE_POISON)
            assert late.size == 0, (
                f"{self.label} ({phase} run): {late.size} bytes of {b.name} were written after "
                f"the snapshot, first at {late[0]}: work left on a stream the caller's does not "
                f"wait for")

    def run(self, call, blocks=False, check_dry=True, stall_ms=None):
        """Dry run, then the stalled run.  `blocks`: the sequence ends with a
        call that waits by contract, so step 6 is skipped after it (use
        still_stalled() ahead of that call for the calls that must not)."""
        torch = self.torch
        cycles_per_ms()
        self.phase = "dry"
        self._prepare(real=True)
        self.dry_ms = self._sequence(call)
        torch.cuda.synchronize()
        if check_dry:
            self._check("dry")
        self.phase = "stalled"
        self._prepare(real=False)
        self.stall_ms = stall_ms if stall_ms is not None else min(
            STALL_CAP_MS, max(STALL_FLOOR_MS, STALL_MULTIPLE * self.dry_ms))
        self.done = stall(self.stream, self.stall_ms)
        self.stalled_ms = self._sequence(call)
        if not blocks:
            self.still_stalled("the sequence")
        if self._pending:
            self._check_pending()
        for s in self.streams:
            s.synchronize()
        torch.cuda.synchronize()
        self._check("stalled")
        print(f"stream_order {self.label}: dry enqueue {self.dry_ms:.3f} ms, stalled enqueue "
              f"{self.stalled_ms:.3f} ms, stall {self.stall_ms:.0f} ms")
        return self
