"""GPU: aqz_ds_run_device_volume_tiled and aqz_ds_run_device_volume_chunked
between pending work on the caller's stream (tests/stream_order.py, imported
as it is).  The unstalled first run takes the scratch growth; the stalled run
must return while the stall runs, read its inputs and write its outputs in
stream order, and leave nothing on another stream.  The chunked form's third
call in flight may wait, as aqz_ds_run_device_batch_chunked's does."""
import numpy as np
import pytest

import volume_tiled_cases as vc
from gpu_util import random_frames
from stream_order import Sandwich

pytestmark = pytest.mark.gpu

MEAN = 1


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def flags_expect(want_nz):
    def check(got):
        raw = got.reshape(want_nz.shape)
        assert np.isin(raw, (0, 1)).all(), "a flag byte is neither 0 nor 1"
        assert np.array_equal(raw.astype(bool), want_nz), "zero scan differs"
    return check


class TiledRig:
    """Inputs, poisoned outputs and oracle expectations of one tiled batch."""

    def __init__(self, sw, oracle, case, stream=0):
        w, h, planes, levels, dtype, tr, tc, _ = case
        self.geo = vc.volume_geo(w, h, planes, levels)
        frames = vc.case_frames(case)
        self.n = len(frames)
        self.tiles = [None] + [(tr, tc)] * (levels - 1)
        want = vc.expected_tiled(oracle, vc.oracle_planes(oracle, self.geo, dtype, MEAN, frames),
                                 self.tiles)
        self.d_in = sw.input(frames, stream=stream)
        self.outs, self.flags = [None], [None]
        for L in range(1, levels):
            t, nz = want[L]
            self.outs.append(sw.output(t.nbytes, as_bytes(t), stream=stream,
                                       name=f"level {L} tiles"))
            self.flags.append(sw.output(nz.size, flags_expect(nz), stream=stream,
                                        name=f"level {L} flags"))

    def run(self, ds, hip_stream):
        return ds.run_device_volume_tiled(
            self.d_in.data_ptr(), self.n, self.tiles, [0] + [o.data_ptr() for o in self.outs[1:]],
            [0] + [f.data_ptr() for f in self.flags[1:]], hip_stream)


@pytest.mark.parametrize("case", [vc.CASES[3], vc.CASES[6]], ids=["one_run", "chained_runs"])
def test_run_device_volume_tiled(aqz, oracle, case):
    """One run of two levels, and the 5-level pyramid whose runs chain through
    handle scratch (grown by the unstalled run)."""
    sw = Sandwich(f"run_device_volume_tiled {vc.case_id(case)}")
    rig = TiledRig(sw, oracle, case)
    ds = aqz.Downsampler(rig.geo, case[4], MEAN)
    sw.run(lambda sw: rig.run(ds, sw.hip_stream))
    assert ds.last_batch_kind() == 5
    ds.close()


def test_deep_volume_batches_on_two_streams_share_the_chain(aqz, oracle):
    """Two deep batches of one handle, the first on the stalled stream, the
    second straight after it on an idle one: the second waits for the first
    (chain_done) and cannot finish while the first stream is stalled."""
    case = vc.CASES[6]
    sw = Sandwich("deep volume batches on two streams", n_streams=2)
    first = TiledRig(sw, oracle, case, stream=0)
    second = TiledRig(sw, oracle, case, stream=1)
    ds = aqz.Downsampler(first.geo, case[4], MEAN)

    def call(sw):
        first.run(ds, sw.hip_stream_of(0))
        second.run(ds, sw.hip_stream_of(1))
        sw.pending(1, "the second deep batch")

    sw.run(call)
    ds.close()


class ChunkedRig:
    """One chunked batch of 8 planes starting at plane `first`: its own
    lattice buffers, expected from the oracle pyramid at the oracle's places."""

    def __init__(self, sw, oracle, first, seed):
        w, h, _ = vc.CHUNK_GEO[0]
        frames = random_frames(np.random.default_rng(seed), np.uint16, (8, h, w))
        want = vc.expected_chunked(
            oracle, vc.oracle_planes(oracle, vc.CHUNK_GEO, np.uint16, MEAN, frames), first,
            np.uint16)
        self.d_in = sw.input(frames)
        self.offsets = [None] + [want[L][1] for L in (1, 2)]
        self.lats = [None]
        for L in (1, 2):
            buf, offs, cb, _, cap = want[L]
            _, cy, cx = vc.CHUNK_SHAPES[L]
            d = sw.output(cap, buf, name=f"first {first} level {L} lattice")
            self.lats.append((d.data_ptr(), cap, cy, cx, cb, offs))

    def run(self, ds, hip_stream):
        return ds.run_device_volume_chunked(self.d_in.data_ptr(), 8, self.lats, stream=hip_stream)


def test_two_volume_chunked_batches_keep_their_own_offsets(aqz, oracle):
    """Two batches with different plane offsets back to back on the stalled
    stream: each offset table crosses through its own pinned half."""
    ds = aqz.Downsampler(vc.CHUNK_GEO, np.uint16, MEAN, device=0)
    sw = Sandwich("two volume chunked batches")
    a = ChunkedRig(sw, oracle, 0, seed=1)
    b = ChunkedRig(sw, oracle, 4, seed=2)
    assert a.offsets[2] != b.offsets[2]

    def call(sw):
        a.run(ds, sw.hip_stream)
        b.run(ds, sw.hip_stream)

    sw.run(call)
    ds.close()


def test_third_volume_chunked_batch_may_wait_for_the_first(aqz, oracle):
    """At most two chunked batches of a handle are in flight: the first two
    return while the stream is stalled; the third needs the pinned half of the
    first and waits for it by contract.  All three land at their own places."""
    ds = aqz.Downsampler(vc.CHUNK_GEO, np.uint16, MEAN, device=0)
    sw = Sandwich("three volume chunked batches")
    rigs = [ChunkedRig(sw, oracle, first, seed=10 + first) for first in (0, 4, 8)]
    blocked = {}

    def call(sw):
        rigs[0].run(ds, sw.hip_stream)
        rigs[1].run(ds, sw.hip_stream)
        sw.still_stalled("two volume chunked batches in a row")
        rigs[2].run(ds, sw.hip_stream)
        if sw.phase == "stalled":
            blocked["third"] = sw.done.query()

    sw.run(call, blocks=True)  # the third call waits by contract
    assert blocked["third"], "the third chunked batch returned with the first still pending"
    ds.close()
