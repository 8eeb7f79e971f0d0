"""GPU: aqz_ds_run_device_batch_tiled_base and aqz_ds_run_device_batch_chunked_base
between pending work on the caller's stream (tests/stream_order.py, imported
as it is).  The unstalled first run takes the scratch growth; the stalled run
must return while the stall runs, read its inputs and write its outputs —
level 0's tiles and flags among them — in stream order, and leave nothing on
another stream.  The chunked form's third call in flight may wait, as
aqz_ds_run_device_batch_chunked's does."""
import numpy as np
import pytest

import tiled_base_cases as tb
from gpu_util import random_frames
from stream_order import Sandwich

pytestmark = pytest.mark.gpu

MEAN = 1


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def flags_expect(want_nz, slots):
    def check(got):
        raw = got.reshape(want_nz.shape + (slots,))
        assert np.isin(raw, (0, 1)).all(), "a flag byte is neither 0 nor 1"
        assert np.array_equal(raw.any(axis=-1), want_nz), "zero scan differs"
    return check


class TiledRig:
    """Inputs, poisoned outputs and oracle expectations of one batch, level 0
    included."""

    def __init__(self, sw, oracle, ds, c):
        self.geo = tb.halving(c["w"], c["h"], c["levels"])
        frames = tb.case_frames(c)
        self.n, self.tiles = len(frames), c["tiles"]
        want = tb.expected(oracle, frames, c["levels"], MEAN, self.tiles)
        self.d_in = sw.input(frames)
        self.outs, self.flags = [], []
        for L in range(c["levels"]):
            t, nz = want[L]
            slots = ds.tiled_flag_slots(L, *self.tiles[L]) if L else \
                ds.tiled_base_flag_slots(*self.tiles[0])
            self.outs.append(sw.output(t.nbytes, as_bytes(t), name=f"level {L} tiles"))
            self.flags.append(sw.output(nz.size * slots, flags_expect(nz, slots),
                                        name=f"level {L} flags"))

    def run(self, ds, hip_stream):
        return ds.run_device_batch_tiled_base(
            self.d_in.data_ptr(), self.n, self.tiles, [o.data_ptr() for o in self.outs],
            [f.data_ptr() for f in self.flags], hip_stream)


@pytest.mark.parametrize("name", ["rowfill", "slots_none_l2gen", "chain2_big"])
def test_run_device_batch_tiled_base(aqz, oracle, name):
    """One run with zero-fill waves and a cleared base flag byte, one with
    two flag clears queued ahead of the kernel, and the 7-level pyramid whose
    runs chain through handle scratch (grown by the unstalled run)."""
    c = tb.CASE[name]
    sw = Sandwich(f"run_device_batch_tiled_base {name}")
    ds = aqz.Downsampler(tb.halving(c["w"], c["h"], c["levels"]), c["dtype"], MEAN)
    rig = TiledRig(sw, oracle, ds, c)
    sw.run(lambda sw: rig.run(ds, sw.hip_stream))
    assert ds.last_batch_kind() == 6
    ds.close()


CHUNK_GEO = tb.halving(64, 48, 3)
CHUNK_SHAPES = [(3, 32, 48), (3, 16, 16), (3, 8, 16)]  # (t, y, x) chunk per level, ragged


class ChunkedRig:
    """One chunked batch of 5 frames starting at frame `first` of the stream:
    its own lattice buffers, expected from the oracle at the oracle's places."""

    def __init__(self, sw, oracle, first, seed):
        w, h, _ = CHUNK_GEO[0]
        frames = random_frames(np.random.default_rng(seed), np.uint16, (5, h, w))
        tiles = [s[1:] for s in CHUNK_SHAPES]
        want = tb.expected(oracle, frames, 3, MEAN, tiles)
        self.d_in = sw.input(frames)
        self.offsets, self.lats = [], []
        for L in range(3):
            offs, cb, lb = oracle.chunk_frame_offsets(tb.chunk_dims(CHUNK_GEO, L, CHUNK_SHAPES[L]),
                                                      2, first, 5)
            cap = (max(offs) // lb + 1) * lb
            buf = np.full(cap, tb.POISON, np.uint8)
            tbytes = tiles[L][0] * tiles[L][1] * 2
            for k in range(5):
                t = want[L][0][k]
                at = offs[k] + np.arange(t.shape[0], dtype=np.int64)[:, None] * cb
                buf[at + np.arange(tbytes, dtype=np.int64)[None, :]] = \
                    t.view(np.uint8).reshape(t.shape[0], tbytes)
            d = sw.output(cap, buf, name=f"first {first} level {L} lattice")
            self.offsets.append(offs)
            self.lats.append((d.data_ptr(), cap, tiles[L][0], tiles[L][1], cb, offs))

    def run(self, ds, hip_stream):
        return ds.run_device_batch_chunked_base(self.d_in.data_ptr(), 5, self.lats,
                                                stream=hip_stream)


def test_run_device_batch_chunked_base(aqz, oracle):
    ds = aqz.Downsampler(CHUNK_GEO, np.uint16, MEAN, device=0)
    sw = Sandwich("run_device_batch_chunked_base")
    rig = ChunkedRig(sw, oracle, 2, seed=3)
    sw.run(lambda sw: rig.run(ds, sw.hip_stream))
    assert ds.last_batch_kind() == 6
    ds.close()


def test_third_chunked_base_batch_may_wait_for_the_first(aqz, oracle):
    """At most two chunked batches of a handle are in flight: the first two
    return while the stream is stalled; the third needs the pinned half of the
    first and waits for it by contract.  All three offset tables — level 0's
    in slot 0 of each half — land their frames at their own places."""
    ds = aqz.Downsampler(CHUNK_GEO, np.uint16, MEAN, device=0)
    sw = Sandwich("three chunked base batches")
    rigs = [ChunkedRig(sw, oracle, first, seed=10 + first) for first in (0, 1, 2)]
    assert rigs[0].offsets[0] != rigs[1].offsets[0] != rigs[2].offsets[0]
    blocked = {}

    def call(sw):
        rigs[0].run(ds, sw.hip_stream)
        rigs[1].run(ds, sw.hip_stream)
        sw.still_stalled("two chunked base batches in a row")
        rigs[2].run(ds, sw.hip_stream)
        if sw.phase == "stalled":
            blocked["third"] = sw.done.query()

    sw.run(call, blocks=True)  # the third call waits by contract
    assert blocked["third"], "the third chunked batch returned with the first still pending"
    ds.close()
