"""GPU: stream ordering of every queued call with work in flight.

Every `_device` entry point promises that its work is queued on the caller's
`hip_stream` and that the call does not synchronise (aqz_downsampler.h,
aqz_codec.h, aqz_blosc.h, aqz_shard.h).  The rest of the suite makes its
inputs, waits for the device, makes one call and waits again, so it cannot see
work queued on the wrong stream, a missing event wait, reused scratch or a
hidden host wait.  Here every call runs inside a `Sandwich`
(tests/stream_order.py): the inputs arrive on the stream behind a stall, the
outputs are read on the stream right behind the call, and the call must
return while the stall still runs.

Expected bytes come from what the suite already trusts (the oracle, the
shard model, the host blosc path that tests/test_gpu_blosc.py pins to
c-blosc), never from the call under test run a second time.

Which case fails if a mechanism is taken out (argued from the code):

* StreamSwap::join, handle's stream -> caller's: without it the handle's
  stream runs add_frame ahead of the stalled batch, so its frame meets no
  stored plane: test_run_device_batch_per_frame_joins_handle_stream (the
  take and the next batch differ from the oracle).  Caller's -> handle's:
  batch B on the idle stream runs before batch A and the added frame:
  test_per_frame_batch_on_an_idle_stream_waits_for_the_handle_stream.
* chain_done: the second deep batch, on an idle stream, would finish while
  the first is stalled, which the `pending` check refuses (behind a stall the
  two never overlap, so the bytes alone would not show it):
  test_deep_tiled_batches_on_two_streams_share_the_chain.
* lattice_done and the two pinned halves: with one half, or no wait, the
  second (third) batch's host writes change the offsets the first batch's
  upload has not read yet, and its tiles land at the other batch's offsets:
  test_two_chunked_batches_keep_their_own_offsets,
  test_third_chunked_batch_waits_for_the_first.
* the fills in front of the S == 1 flag kernel, in aqz_tile_frame_device and
  in aqz_zarr_shard_set_begin: a fill on another stream runs ahead, step 3
  poisons the flags again and the zero tiles keep 0xA5
  (test_run_device_batch_tiled[one_slot], test_tile_frame_device); a begin
  that runs ahead leaves the first shards' layers in the second tables
  (test_shard_layers_and_tables_back_to_back).
* the node's events: without `ready` the pulls copy the decoy; without the
  wait for `done` the snapshot holds 0xA5; without `pulled` / `ran` the
  pyramid reads an empty slot or the push copies early
  (test_node_run_device_batch[stage_all]).
* ctx scratch and shard-set scratch: both are ordered by the stream alone;
  a kernel of the second call queued elsewhere rewrites d_filtered / d_comp /
  d_rows, or chunk_rel and the pairs, under the first
  (test_two_lz4_frames_calls_share_the_scratch,
  test_shard_layers_and_tables_back_to_back, test_pipeline_on_one_stalled_stream).
"""
import re

import numpy as np
import pytest

import lz4_cases as lc
import zarr_shard_model as zm
from gpu_util import random_frames, to_device, torch_cuda
from stream_order import POISON, Sandwich, stall
from test_gpu_lattice import expected_lattices, level_dims
from test_gpu_parity import BATCH_GEOMETRIES

pytestmark = pytest.mark.gpu

SPACE, TIME = 0, 2
MEAN = 1


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def halving(w, h, n):
    geo = [(w, h, 1)]
    for _ in range(1, n):
        w, h = (w + 1) // 2, (h + 1) // 2
        geo.append((w, h, 1))
    return geo


# ---- 1. the harness has teeth ------------------------------------------------

def fake_io(sw, seed):
    """A fake call's input and output: the output must become the input."""
    real = np.random.default_rng(seed).integers(0, 256, 1 << 16, dtype=np.uint8)
    d_in = sw.input(real)
    d_out = sw.output(real.size, real, name="copy")
    return d_in, d_out


@pytest.mark.parametrize("repoison,message", [
    (False, "wrong bytes"),                    # the snapshot holds the decoy
    (True, "still hold the poison 0xA5"),      # the early write is wiped out again
], ids=["decoy_seen", "early_write_wiped"])
def test_teeth_early_reader(repoison, message):
    """A copy queued on a second stream that never waits for the caller's:
    it reads the decoy, and it writes before the stream reaches the call."""
    torch = torch_cuda()
    sw = Sandwich("early reader", repoison=repoison)
    d_in, d_out = fake_io(sw, 1)
    other = sw.new_stream()

    def call(sw):
        with torch.cuda.stream(other):
            d_out.copy_(d_in, non_blocking=True)

    with pytest.raises(AssertionError, match=message):
        sw.run(call, check_dry=False)
    torch.cuda.synchronize()


def test_teeth_unjoined_writer():
    """The second stream waits for the caller's, but the caller's never waits
    back: the snapshot is taken before the write."""
    torch = torch_cuda()
    sw = Sandwich("unjoined writer")
    d_in, d_out = fake_io(sw, 2)
    other = sw.new_stream()

    def call(sw):
        ev = torch.cuda.Event()
        ev.record(sw.stream)
        other.wait_event(ev)
        stall(other, 5)
        with torch.cuda.stream(other):
            d_out.copy_(d_in, non_blocking=True)
        sw.keep.append(ev)

    with pytest.raises(AssertionError, match="still hold the poison 0xA5"):
        sw.run(call, check_dry=False)
    torch.cuda.synchronize()


def test_teeth_hidden_host_wait():
    torch = torch_cuda()
    sw = Sandwich("hidden host wait")
    d_in, d_out = fake_io(sw, 3)

    def call(sw):
        sw.stream.synchronize()
        with torch.cuda.stream(sw.stream):
            d_out.copy_(d_in, non_blocking=True)

    with pytest.raises(AssertionError, match="returned only after the stall"):
        sw.run(call)
    torch.cuda.synchronize()


def test_control_joined_both_ways():
    """The same second-stream copy, joined both ways: passes."""
    torch = torch_cuda()
    sw = Sandwich("joined both ways")
    d_in, d_out = fake_io(sw, 4)
    other = sw.new_stream()

    def call(sw):
        ev = torch.cuda.Event()
        ev.record(sw.stream)
        other.wait_event(ev)
        with torch.cuda.stream(other):
            d_out.copy_(d_in, non_blocking=True)
        back = torch.cuda.Event()
        back.record(other)
        sw.stream.wait_event(back)
        sw.keep += [ev, back]

    sw.run(call)
    assert sw.stall_ms >= 60


# ---- 2. aqz_ds_run_device_batch ---------------------------------------------

def oracle_stream(ref, frames, n_levels):
    """Frames emitted per level when `ref` is fed `frames` in order and every
    level is taken after every frame."""
    out = {L: [] for L in range(1, n_levels)}
    for f in frames:
        ref.add_frame(f)
        for L in out:
            r = ref.take_frame(L)
            if r is not None:
                out[L].append(r)
    return out


def level_expect(emitted, capacity):
    """The output buffer of one level: the emitted frames back to back, the
    rest untouched."""
    want = np.full(capacity, POISON, np.uint8)
    if emitted:
        raw = np.concatenate([as_bytes(e) for e in emitted])
        want[:raw.size] = raw
    return want


ROW_MAJOR = {
    # name: (geometry, frames, dtype, batch kind)
    "fused": BATCH_GEOMETRIES["2d_narrow_odd"][:2] + (np.uint16, 1),
    "band": BATCH_GEOMETRIES["2d_band_staged"][:2] + (np.uint16, 1),
    "volume": BATCH_GEOMETRIES["3d_fused_one_level"][:2] + (np.uint16, 2),
    # rows of 7 bytes: under one 16-byte load, batched single-level kernels
    "narrow": (halving(7, 33, 3), 5, np.uint8, 3),
}


@pytest.mark.parametrize("name", list(ROW_MAJOR))
def test_run_device_batch(aqz, oracle, name):
    geo, n, dtype, kind = ROW_MAJOR[name]
    w, h, _ = geo[0]
    bpp = np.dtype(dtype).itemsize
    frames = random_frames(np.random.default_rng(len(name)), dtype, (n, h, w))
    emitted = oracle_stream(oracle.OracleDownsampler(geo, dtype, MEAN), frames, len(geo))
    sw = Sandwich(f"run_device_batch {name}")
    d_in = sw.input(frames)
    outs = [None] + [sw.output(n * gw * gh * bpp, level_expect(emitted[L], n * gw * gh * bpp),
                               name=f"level {L}") for L, (gw, gh, _) in enumerate(geo[1:], 1)]
    ds = aqz.Downsampler(geo, dtype, MEAN)
    seen = {}

    def call(sw):
        seen["counts"] = ds.run_device_batch(d_in.data_ptr(), n,
                                             [0] + [o.data_ptr() for o in outs[1:]],
                                             sw.hip_stream)

    sw.run(call)
    assert ds.last_batch_kind() == kind
    assert seen["counts"][1:] == [len(emitted[L]) for L in range(1, len(geo))]
    ds.close()


def test_run_device_batch_per_frame_joins_handle_stream(aqz, oracle):
    """Kind 0 (the per-frame state machine) on the stalled caller's stream,
    followed at once by add_frame and take_frame, which run on the handle's
    own stream: they must see the stored Z plane the batch left (the join back
    from the caller's stream), and the batch the state the earlier add left
    (the join towards it).  The batch returns while the stream is stalled;
    add_frame and take_frame wait by contract.  The handle carries its state
    from the dry run into the stalled one, so one oracle is fed both."""
    geo, n, kind = BATCH_GEOMETRIES["3d_odd_stack"]
    assert kind == 0 and n % geo[0][2] == 1  # one plane of the next stack is stored
    dtype = np.uint16
    w, h, _ = geo[0]
    rng = np.random.default_rng(5)
    frames = random_frames(rng, dtype, (n, h, w))
    extra = random_frames(rng, dtype, (h, w))
    ref = oracle.OracleDownsampler(geo, dtype, MEAN)
    levels = range(1, len(geo))
    emitted, taken = {}, {}
    for phase in ("dry", "stalled"):
        emitted[phase] = oracle_stream(ref, frames, len(geo))
        ref.add_frame(extra)
        taken[phase] = {L: ref.take_frame(L) for L in levels}
    assert taken["dry"][1] is not None  # the stored plane found its pair
    sw = Sandwich("run_device_batch per-frame")
    d_in = sw.input(frames)
    outs = [None]
    for L in levels:
        gw, gh, _ = geo[L]
        cap = n * gw * gh * 2
        outs.append(sw.output(cap, {p: level_expect(emitted[p][L], cap) for p in emitted},
                              name=f"level {L}"))
    ds = aqz.Downsampler(geo, dtype, MEAN)
    got = {}

    def call(sw):
        ds.run_device_batch(d_in.data_ptr(), n, [0] + [o.data_ptr() for o in outs[1:]],
                            sw.hip_stream)
        sw.still_stalled("aqz_ds_run_device_batch (per-frame fallback)")
        ds.add_frame(extra)
        got[sw.phase] = {L: ds.take_frame(L) for L in levels}

    sw.run(call, blocks=True)  # add_frame / take_frame wait for the upload and the levels
    assert ds.last_batch_kind() == 0
    for phase in ("dry", "stalled"):
        for L in levels:
            want = taken[phase][L]
            if want is None:
                assert got[phase][L] is None, (phase, L)
            else:
                assert got[phase][L] is not None and \
                    np.array_equal(got[phase][L], want), (phase, L)
    ds.close()


def test_per_frame_batch_on_an_idle_stream_waits_for_the_handle_stream(aqz, oracle):
    """The join towards the caller's stream.  Batch A runs on the stalled
    stream; aqz_ds_add_device_frame then queues a frame on the handle's own
    stream, which the join back holds behind A; batch B follows at once on an
    idle second stream.  B reads the Z state A and the frame leave, so it must
    wait for the handle's stream — and cannot finish while the first stream
    is stalled.  One oracle is fed A, the frame and B, for both runs."""
    torch = torch_cuda()
    geo, n, kind = BATCH_GEOMETRIES["3d_odd_stack"]
    dtype = np.uint16
    w, h, _ = geo[0]
    rng = np.random.default_rng(6)
    frames_a = random_frames(rng, dtype, (n, h, w))
    extra = random_frames(rng, dtype, (h, w))
    frames_b = random_frames(rng, dtype, (n, h, w))
    ref = oracle.OracleDownsampler(geo, dtype, MEAN)
    levels = range(1, len(geo))
    want_a, want_b, taken = {}, {}, {}
    for phase in ("dry", "stalled"):
        want_a[phase] = oracle_stream(ref, frames_a, len(geo))
        ref.add_frame(extra)
        taken[phase] = {L: ref.take_frame(L) for L in levels}
        want_b[phase] = oracle_stream(ref, frames_b, len(geo))
    assert taken["dry"][1] is not None
    sw = Sandwich("per-frame batches on two streams", n_streams=2)
    d_a = sw.input(frames_a)
    d_extra = sw.input(extra)
    d_b = sw.input(frames_b, stream=1)
    outs_a, outs_b = [None], [None]
    for L in levels:
        gw, gh, _ = geo[L]
        cap = n * gw * gh * 2
        outs_a.append(sw.output(cap, {p: level_expect(want_a[p][L], cap) for p in want_a},
                                name=f"batch A level {L}"))
        outs_b.append(sw.output(cap, {p: level_expect(want_b[p][L], cap) for p in want_b},
                                stream=1, name=f"batch B level {L}"))
    ds = aqz.Downsampler(geo, dtype, MEAN)
    got = {}

    def call(sw):
        ds.run_device_batch(d_a.data_ptr(), n, [0] + [o.data_ptr() for o in outs_a[1:]],
                            sw.hip_stream_of(0))
        ds.add_device_frame(d_extra.data_ptr(), extra.nbytes)
        ds.run_device_batch(d_b.data_ptr(), n, [0] + [o.data_ptr() for o in outs_b[1:]],
                            sw.hip_stream_of(1))
        sw.pending(1, "batch B")
        # the frame must stay valid until the next call on the handle: B is
        # that call, so the first stream may reuse the frame once B has run
        ev = torch.cuda.Event()
        ev.record(sw.streams[1])
        sw.streams[0].wait_event(ev)
        sw.keep.append(ev)
        sw.still_stalled("two per-frame batches and aqz_ds_add_device_frame")
        got[sw.phase] = {L: ds.take_frame(L) for L in levels}  # waits by contract

    sw.run(call, blocks=True)
    assert ds.last_batch_kind() == 0
    for phase in ("dry", "stalled"):
        for L in levels:
            want = taken[phase][L]
            if want is None:
                assert got[phase][L] is None, (phase, L)
            else:
                assert got[phase][L] is not None and \
                    np.array_equal(got[phase][L], want), (phase, L)
    ds.close()


# ---- 3. aqz_ds_run_device_batch_tiled ----------------------------------------

def flags_expect(want_nz, slots):
    """Zero-scan flags: `slots` bytes a tile, each 0 or 1, any of them set
    exactly where the oracle's tile holds a nonzero byte."""
    def check(got):
        raw = got.reshape(want_nz.shape + (slots,))
        assert np.isin(raw, (0, 1)).all(), "a flag byte is neither 0 nor 1"
        assert np.array_equal(raw.any(axis=-1), want_nz), "zero scan differs"
    return check


class TiledRig:
    """Inputs, poisoned outputs and oracle expectations of one tiled batch."""

    def __init__(self, sw, ds, oracle, geo, dtype, tile, frames, stream=0, flags=True):
        tr, tc = tile
        n = len(frames)
        bpp = np.dtype(dtype).itemsize
        self.n = n
        self.tiles = [None] + [tile] * (len(geo) - 1)
        self.d_in = sw.input(frames, stream=stream)
        self.slots = [None]
        tiles_want = {L: [] for L in range(1, len(geo))}
        nz_want = {L: [] for L in range(1, len(geo))}
        for fr in frames:
            ref = oracle.cascade_2d(fr, len(geo), MEAN)
            for L in range(1, len(geo)):
                t, nz = oracle.tile_frame(ref[L - 1], tr, tc)
                tiles_want[L].append(t)
                nz_want[L].append(nz)
        self.outs, self.flags = [None], [None]
        for L, (w, h, _) in enumerate(geo[1:], 1):
            nt = (-(-h // tr)) * (-(-w // tc))
            S = ds.tiled_flag_slots(L, tr, tc)
            self.slots.append(S)
            self.outs.append(sw.output(n * nt * tr * tc * bpp, as_bytes(np.stack(tiles_want[L])),
                                       stream=stream, name=f"level {L} tiles"))
            self.flags.append(sw.output(n * nt * S, flags_expect(np.stack(nz_want[L]), S),
                                        stream=stream, name=f"level {L} flags")
                              if flags else None)

    def run(self, ds, hip_stream):
        return ds.run_device_batch_tiled(
            self.d_in.data_ptr(), self.n, self.tiles, [0] + [o.data_ptr() for o in self.outs[1:]],
            [0] + [f.data_ptr() for f in self.flags[1:]] if self.flags[1] is not None else None,
            hip_stream)


def tiled_frames(seed, dtype, n, h, w):
    frames = random_frames(np.random.default_rng(seed), dtype, (n, h, w), specials=False)
    frames[0][: h // 2, : w // 2] = 0  # zero tiles at every level
    return frames


@pytest.mark.parametrize("case", [
    # one flag byte a tile: cleared by a fill queued in front of the kernel
    ("one_slot", 320, 48, 3, (10, 60), lambda s: s == 1),
    # several flag bytes a tile, each written by the wave that owns it
    ("many_slots", 512, 64, 3, (16, 128), lambda s: s > 1),
], ids=lambda c: c[0])
def test_run_device_batch_tiled(aqz, oracle, case):
    name, w, h, nl, tile, slots_ok = case
    geo = halving(w, h, nl)
    ds = aqz.Downsampler(geo, np.uint16, MEAN)
    sw = Sandwich(f"run_device_batch_tiled {name}")
    rig = TiledRig(sw, ds, oracle, geo, np.uint16, tile, tiled_frames(w, np.uint16, 2, h, w))
    assert all(slots_ok(s) for s in rig.slots[1:]), rig.slots
    sw.run(lambda sw: rig.run(ds, sw.hip_stream))
    assert ds.last_batch_kind() == 4
    ds.close()


DEEP = (512, 256, 6, np.uint8, (8, 16))  # level 4 is 32 bytes wide: a second fused run


def test_run_device_batch_tiled_deep(aqz, oracle):
    w, h, nl, dtype, tile = DEEP
    geo = halving(w, h, nl)
    ds = aqz.Downsampler(geo, dtype, MEAN)
    sw = Sandwich("run_device_batch_tiled deep")
    rig = TiledRig(sw, ds, oracle, geo, dtype, tile, tiled_frames(6, dtype, 2, h, w))
    sw.run(lambda sw: rig.run(ds, sw.hip_stream))
    ds.close()


def test_deep_tiled_batches_on_two_streams_share_the_chain(aqz, oracle):
    """Two deep batches of one handle, the first on the stalled stream, the
    second straight after it on an idle one: both chain their runs through the
    handle's scratch, so the second must wait for the first (chain_done) and
    cannot finish while the first stream is stalled."""
    w, h, nl, dtype, tile = DEEP
    geo = halving(w, h, nl)
    ds = aqz.Downsampler(geo, dtype, MEAN)
    sw = Sandwich("deep tiled batches on two streams", n_streams=2)
    first = TiledRig(sw, ds, oracle, geo, dtype, tile, tiled_frames(11, dtype, 2, h, w), stream=0)
    second = TiledRig(sw, ds, oracle, geo, dtype, tile, tiled_frames(12, dtype, 2, h, w), stream=1)

    def call(sw):
        first.run(ds, sw.hip_stream_of(0))
        second.run(ds, sw.hip_stream_of(1))
        sw.pending(1, "the second deep batch")

    sw.run(call)
    ds.close()


# ---- 4. aqz_ds_run_device_batch_chunked --------------------------------------

CHUNK_DIMS = [(TIME, 0, 3, 1), (SPACE, 96, 32, 1), (SPACE, 160, 32, 1)]


class ChunkedRig:
    """One chunked batch of `n` frames starting at frame `first`: its own
    lattice buffers, expected from the oracle pyramid placed by the oracle's
    addressing."""

    def __init__(self, sw, aqz, oracle, geo, first, n, seed):
        dtype = np.uint16
        H, W = CHUNK_DIMS[-2][1], CHUNK_DIMS[-1][1]
        frames = random_frames(np.random.default_rng(seed), dtype, (n, H, W))
        cap = [0]
        for L in range(1, len(geo)):
            o, cb, lb = oracle.chunk_frame_offsets(level_dims(CHUNK_DIMS, geo, L), 2, first, n)
            cap.append((max(o) // lb + 1) * lb)
        want, offs = expected_lattices(oracle, CHUNK_DIMS, geo, list(frames), dtype, MEAN, first,
                                       cap)
        self.n = n
        self.d_in = sw.input(frames)
        self.bufs = [None] + [sw.output(cap[L], want[L], name=f"first {first} level {L} lattice")
                              for L in range(1, len(geo))]
        self.lats = [None] + [(self.bufs[L].data_ptr(), cap[L], 32, 32, offs[L][1], offs[L][0])
                              for L in range(1, len(geo))]
        self.offsets = offs

    def run(self, ds, hip_stream):
        return ds.run_device_batch_chunked(self.d_in.data_ptr(), self.n, self.lats,
                                           stream=hip_stream)


def test_two_chunked_batches_keep_their_own_offsets(aqz, oracle):
    """Two batches with different frame offsets back to back on the stalled
    stream: each offset table crosses through its own pinned half."""
    geo = aqz.level_geometry(aqz.plan_levels(CHUNK_DIMS))
    ds = aqz.Downsampler(geo, np.uint16, MEAN, device=0)
    sw = Sandwich("two chunked batches")
    a = ChunkedRig(sw, aqz, oracle, geo, 0, 4, seed=1)
    b = ChunkedRig(sw, aqz, oracle, geo, 2, 4, seed=2)
    assert a.offsets[1][0] != b.offsets[1][0]

    def call(sw):
        a.run(ds, sw.hip_stream)
        b.run(ds, sw.hip_stream)

    sw.run(call)
    ds.close()


def test_third_chunked_batch_waits_for_the_first(aqz, oracle):
    """At most two chunked batches are in flight (aqz_downsampler.h): the
    first two return while the stream is stalled, the third needs the pinned
    half of the first and returns only once that batch has finished.  All
    three land at their own offsets."""
    geo = aqz.level_geometry(aqz.plan_levels(CHUNK_DIMS))
    ds = aqz.Downsampler(geo, np.uint16, MEAN, device=0)
    sw = Sandwich("three chunked batches")
    rigs = [ChunkedRig(sw, aqz, oracle, geo, first, 3, seed=10 + first) for first in (0, 1, 2)]
    blocked = {}

    def call(sw):
        rigs[0].run(ds, sw.hip_stream)
        rigs[1].run(ds, sw.hip_stream)
        sw.still_stalled("two chunked batches in a row")
        rigs[2].run(ds, sw.hip_stream)
        if sw.phase == "stalled":
            blocked["third"] = sw.done.query()

    sw.run(call, blocks=True)  # the third call waits by contract
    assert blocked["third"], "the third chunked batch returned with the first still pending"
    ds.close()


# ---- 5. free functions -------------------------------------------------------

def test_tile_frame_device(aqz, oracle):
    """A fill of the flags and a kernel, both on the caller's stream."""
    w, h, tr, tc = 300, 70, 32, 64
    frame = random_frames(np.random.default_rng(3), np.uint16, (h, w))
    frame[:tr, :tc] = 0
    tiles, nz = oracle.tile_frame(frame, tr, tc)
    assert not nz[0] and nz[1:].all()

    def flags(got):
        assert np.array_equal(got.view(np.uint32) != 0, nz), "zero scan differs"

    sw = Sandwich("tile_frame_device")
    d_in = sw.input(frame)
    d_tiles = sw.output(tiles.nbytes, as_bytes(tiles), name="tiles")
    d_nz = sw.output(4 * nz.size, flags, name="flags")
    sw.run(lambda sw: aqz.tile_frame_device(np.uint16, d_in.data_ptr(), w, h, tr, tc,
                                            d_tiles.data_ptr(), d_nz.data_ptr(), sw.hip_stream))


def test_tile_frame_device_sliced(aqz, oracle):
    w, h, tr, tc = 300, 70, 32, 64
    frame = random_frames(np.random.default_rng(4), np.uint16, (h, w))
    frame[:tr, :tc] = 0
    tiles, nz = oracle.tile_frame(frame, tr, tc)
    sl = aqz.tile_slices(tr, tc)
    sw = Sandwich("tile_frame_device_sliced")
    d_in = sw.input(frame)
    d_tiles = sw.output(tiles.nbytes, as_bytes(tiles), name="tiles")
    d_sl = sw.output(nz.size * sl, flags_expect(nz, sl), name="slice flags")
    sw.run(lambda sw: aqz.tile_frame_device_sliced(np.uint16, d_in.data_ptr(), w, h, tr, tc,
                                                   d_tiles.data_ptr(), d_sl.data_ptr(),
                                                   sw.hip_stream))


def test_transpose_frame_device(aqz, oracle):
    rows, cols = 70, 301
    frame = random_frames(np.random.default_rng(5), np.float32, (rows, cols))
    sw = Sandwich("transpose_frame_device")
    d_in = sw.input(frame)
    d_out = sw.output(frame.nbytes, as_bytes(oracle.transpose_frame(frame)), name="transposed")
    sw.run(lambda sw: aqz.transpose_frame_device(np.float32, d_in.data_ptr(), rows, cols,
                                                 d_out.data_ptr(), sw.hip_stream))


# ---- 6. codecs ---------------------------------------------------------------

@pytest.mark.parametrize("shuffle,ts,bs,nbytes,nbuf", [
    (1, 2, 65536, 65536 * 3 + 4096, 2),  # byte shuffle, a leftover block
    (2, 4, 16384, 16384 * 4, 3),         # bit shuffle
], ids=["shuffle", "bitshuffle"])
def test_blosc_filter_device(aqz, oracle, shuffle, ts, bs, nbytes, nbuf):
    host = np.random.default_rng(ts + shuffle).integers(0, 256, nbytes * nbuf, dtype=np.uint8)
    host[: nbytes // 3] = 0
    want = np.concatenate([oracle.blosc_filter(host[k * nbytes:(k + 1) * nbytes], shuffle, ts, bs)
                           for k in range(nbuf)])
    sw = Sandwich(f"blosc_filter_device shuffle {shuffle}")
    d_src = sw.input(host)
    d_dst = sw.output(host.size, want, name="filtered")
    sw.run(lambda sw: aqz.blosc_filter_device(shuffle, ts, bs, d_src.data_ptr(), nbytes, nbuf,
                                              d_dst.data_ptr(), sw.hip_stream))


@pytest.mark.parametrize("n,nbuf", [(1000, 37), (1 << 20, 3)], ids=["packed_tables", "large"])
def test_crc32c_device(aqz, oracle, n, nbuf):
    stride = n + 5
    host = np.random.default_rng(n).integers(0, 256, nbuf * stride, dtype=np.uint8)
    want = np.full(nbuf + 8, 0xA5A5A5A5, np.uint32)  # the words behind the last stay untouched
    for k in range(nbuf):
        want[k] = oracle.crc32c(host[k * stride:k * stride + n])
    sw = Sandwich(f"crc32c_device {n}")
    d = sw.input(host)
    out = sw.output(4 * (nbuf + 8), as_bytes(want), name="crcs")
    sw.run(lambda sw: aqz.crc32c_device(d.data_ptr(), n, stride, nbuf, out.data_ptr(),
                                        sw.hip_stream))


@pytest.fixture(scope="module")
def ctx(aqz):
    c = aqz.BloscContext(0, 2)
    yield c
    c.close()


def test_debug_lz4_splits_device(aqz, ctx):
    """Five splits of 4097 bytes against the serial encoder on the host."""
    case = next(c for c in lc.cases("unaligned") if c[0] == "unaligned-n4097")
    name, n, accel, bufs = case
    want = lc.expected(aqz, case)
    nb = len(bufs)

    def rows(got):
        r = got.view(np.uint32).reshape(nb, 2)
        assert [tuple(int(x) for x in row) for row in r] == [(c, need) for c, _, need in want]

    def comp(got):
        for k, (csize, block, _) in enumerate(want):
            slot = got[k * n:(k + 1) * n]
            assert slot[:csize].tobytes() == block, f"split {k}"
            if csize:
                assert (slot[csize:] == POISON).all(), f"split {k}: written past its size"
        assert (got[nb * n:] == POISON).all(), "guard written"

    sw = Sandwich("debug_lz4_splits_device")
    d_src = sw.input(np.concatenate(bufs))
    d_comp = sw.output(nb * n + 256, comp, name="compressed splits")
    d_rows = sw.output(8 * nb, rows, name="rows")
    sw.run(lambda sw: ctx.debug_lz4_splits_device(d_src.data_ptr(), n, nb, accel,
                                                  d_comp.data_ptr(), d_rows.data_ptr(),
                                                  sw.hip_stream, 0))


def need_lz4(aqz):
    if not re.match(r"lz4 \S+ \(", aqz.blosc_codec_info()):
        pytest.skip("no liblz4 loaded: " + aqz.blosc_codec_info())


def smooth_chunks(seed, n_chunks, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n_chunks, h, w), np.uint16)
    for k in range(n_chunks):
        base = 2000 + 500 * np.sin((xx + 13 * k + seed) / 17.0) * np.cos((yy - 5 * k) / 23.0)
        out[k] = (base + rng.normal(0, 4, (h, w))).astype(np.uint16)
    return out


def host_frames(ctx, raw, nbytes, n, clevel, shuffle, ts):
    """The host path's frames (aqz_blosc_compress_device, pinned to c-blosc by
    tests/test_gpu_blosc.py) of chunks given on the host."""
    d = to_device(raw)
    torch_cuda().cuda.synchronize()
    return ctx.compress_device(clevel, shuffle, ts, "lz4", d.data_ptr(), nbytes, n)


def frames_expect(frames, nbytes, stride):
    def check(got):
        out = got.reshape(len(frames), stride)
        for k, fr in enumerate(frames):
            assert out[k, :len(fr)].tobytes() == fr, f"frame {k}"
            assert (out[k, nbytes + 16:] == POISON).all(), f"frame {k}: written past its slot"
    return check


def test_two_lz4_frames_calls_share_the_scratch(aqz, ctx):
    """aqz_blosc_lz4_frames_device twice back to back on the stalled stream,
    different chunks and destinations: the second call's filter rewrites the
    ctx's scratch only after the first call's frame kernel has read it."""
    need_lz4(aqz)
    n, nbytes = 4, 128 * 256 * 2
    stride = nbytes + 16 + 48
    sw = Sandwich("two lz4_frames_device calls")
    jobs = []
    for seed, shuffle in ((1, 1), (2, 2)):
        raw = as_bytes(smooth_chunks(seed, n, 128, 256))
        want = host_frames(ctx, raw, nbytes, n, 5, shuffle, 2)
        d_src = sw.input(raw)
        d_dst = sw.output(n * stride, frames_expect(want, nbytes, stride), name=f"frames {seed}")
        d_sizes = sw.output(4 * n, as_bytes(np.array([len(f) for f in want], np.uint32)),
                            name=f"sizes {seed}")
        jobs.append((shuffle, d_src, d_dst, d_sizes))

    def call(sw):
        for shuffle, d_src, d_dst, d_sizes in jobs:
            ctx.lz4_frames_device(5, shuffle, 2, d_src.data_ptr(), nbytes, n, d_dst.data_ptr(),
                                  stride, d_sizes.data_ptr(), sw.hip_stream)

    sw.run(call)


# ---- 7. shards ---------------------------------------------------------------

def placed(frames_host, stride, sizes, place, capacity, base=None):
    want = np.full(capacity, POISON, np.uint8) if base is None else base.copy()
    for c, at in enumerate(place):
        if at is not None:
            want[at:at + sizes[c]] = frames_host[c * stride:c * stride + sizes[c]]
    return want


def segments_expect(rows, total):
    return as_bytes(np.array([v for r in rows for v in r] + [total], np.uint64))


def tables_expect(oracle, m):
    return np.concatenate([oracle.shard_index_table(m.offsets[s], m.extents[s])
                           for s in range(m.n_shards)])


def test_shard_layers_and_tables_back_to_back(aqz, oracle):
    """begin, two layers and the tables queued on the stalled stream with no
    wait between them; both layers go through the same device_out and segment
    table, read on the stream after each.  Then begin again, one layer and
    the tables: the fills of the second begin must land behind the first
    shards' layers, or the second tables keep their entries."""
    dims = [(TIME, 0, 1, 2), (SPACE, 1, 1, 1), (SPACE, 6, 1, 3)]  # 2 shards, 3 slots, 2 layers
    stride = 1000
    st = aqz.ZarrShardSet(dims, 0)
    m = zm.ShardModel(dims)
    n = m.cpl
    assert (m.n_shards, m.cps, n, m.lps) == (2, 6, 6, 2)
    rng = np.random.default_rng(8)
    sw = Sandwich("shard layers and tables")
    cap = n * stride
    layers, want_out = [], None
    for layer in range(2):
        sizes = [int(v) for v in rng.integers(0, stride + 1, n)]
        has = [int(v) for v in rng.integers(0, 4, n) > 0]
        host = rng.integers(0, 256, n * stride, dtype=np.uint8)
        rows, total, place = m.append(sizes, has)
        want_out = placed(host, stride, sizes, place, cap, want_out)
        layers.append((sw.input(host), sw.input(np.asarray(sizes, np.uint32)),
                       sw.input(np.asarray(has, np.uint8)), want_out, segments_expect(rows, total)))
        if layer == 0:
            first = (host, sizes, has)
    d_out = sw.output(cap, layers[1][3], name="device_out")
    d_seg = sw.output(8 * st.segment_words, layers[1][4], name="segments")
    d_tab = sw.output(st.table_bytes * m.n_shards, tables_expect(oracle, m), name="tables")
    d_off = sw.output(8 * m.n_shards, as_bytes(np.array(m.file_off, np.uint64)),
                      name="table offsets")
    # fresh shards: the first layer's frames once more
    m.begin()
    rows, total, place = m.append(first[1], first[2])
    d_out2 = sw.output(cap, placed(first[0], stride, first[1], place, cap),
                       name="device_out of the fresh shards")
    d_seg2 = sw.output(8 * st.segment_words, segments_expect(rows, total),
                       name="segments of the fresh shards")
    d_tab2 = sw.output(st.table_bytes * m.n_shards, tables_expect(oracle, m),
                       name="tables of the fresh shards")
    d_off2 = sw.output(8 * m.n_shards, as_bytes(np.array(m.file_off, np.uint64)),
                       name="table offsets of the fresh shards")

    def call(sw):
        s = sw.hip_stream
        st.begin(s)
        for layer, (d_frames, d_sizes, d_has, out_want, seg_want) in enumerate(layers):
            st.append_layer_device(d_frames.data_ptr(), stride, d_out.data_ptr(), cap,
                                   d_seg.data_ptr(), d_sizes.data_ptr(), d_has.data_ptr(), s)
            sw.snapshot(d_out, out_want, f"device_out after layer {layer}")
            sw.snapshot(d_seg, seg_want, f"segments after layer {layer}")
        st.tables_device(d_tab.data_ptr(), d_off.data_ptr(), s)
        st.begin(s)
        d_frames, d_sizes, d_has = layers[0][:3]
        st.append_layer_device(d_frames.data_ptr(), stride, d_out2.data_ptr(), cap,
                               d_seg2.data_ptr(), d_sizes.data_ptr(), d_has.data_ptr(), s)
        st.tables_device(d_tab2.data_ptr(), d_off2.data_ptr(), s)

    sw.run(call)
    st.close()


def test_chunk_has_data_device_two_launches(aqz):
    """70 frames: a launch of 64 and one of 6, behind the caller's clear."""
    torch = torch_cuda()
    n_frames, n_tiles, S = 70, 300, 2
    rng = np.random.default_rng(7)
    flags = (rng.integers(0, 40, (n_frames, n_tiles, S)) == 0).astype(np.uint8)
    base = [int(b) for b in rng.integers(0, 5, n_frames) * n_tiles]
    want = np.zeros(5 * n_tiles, np.uint8)
    for k in range(n_frames):
        want[base[k]:base[k] + n_tiles] |= flags[k].any(axis=1)
    sw = Sandwich("chunk_has_data_device")
    d_flags = sw.input(flags)
    d_has = sw.output(want.size, want, name="has_data")

    def call(sw):
        with torch.cuda.stream(sw.stream):
            d_has.zero_()
        aqz.zarr_shard_chunk_has_data_device(d_flags.data_ptr(), n_frames, n_tiles, S, base,
                                             d_has.data_ptr(), sw.hip_stream)

    sw.run(call)


# ---- 8. the whole pipeline ---------------------------------------------------

def test_pipeline_on_one_stalled_stream(aqz, oracle, ctx):
    """The integration's sequence with no host wait: a batch into its chunk
    lattice, then per layer has_data from the zero scan, LZ4 frames and the
    shard layer, then the tables — test_pyramid_level_to_shards' geometry
    (512x512 u16, 128-pixel chunks, 4 frames a chunk, 8 frames), all on one
    stalled stream.  Frames, sizes and has_data go through one set of buffers
    for both layers, as a writer would reuse them."""
    need_lz4(aqz)
    torch = torch_cuda()
    dims = [(TIME, 0, 4, 1), (SPACE, 512, 128, 1), (SPACE, 512, 128, 1)]
    geo = aqz.level_geometry(aqz.plan_levels(dims))
    n_frames, tile = 8, 128
    frames = np.random.default_rng(9).integers(0, 65536, (n_frames, 512, 512), dtype=np.uint16)
    frames[:, :256, 256:] = 0   # level-1 tile 1 of every frame: chunk 1 empty in both layers
    frames[4:, 256:, :256] = 0  # and tile 2 in the second layer
    ds = aqz.Downsampler(geo, np.uint16, MEAN, device=0)
    sw = Sandwich("pipeline")
    d_in = sw.input(frames)
    # the oracle's lattices of every level
    cap, info = [0], [None]
    for L in range(1, len(geo)):
        o, cb, lb = oracle.chunk_frame_offsets(level_dims(dims, geo, L), 2, 0, n_frames)
        cap.append((max(o) // lb + 1) * lb)
        info.append((cb, lb))
    want_lat, offs = expected_lattices(oracle, dims, geo, list(frames), np.uint16, MEAN, 0, cap)
    bufs, flags, lats = [None], [None], [None]
    for L in range(1, len(geo)):
        w, h, _ = geo[L]
        S = ds.tiled_flag_slots(L, tile, tile)
        nt = (-(-h // tile)) * (-(-w // tile))
        bufs.append(sw.output(cap[L], want_lat[L], name=f"level {L} lattice"))
        flags.append(sw.output(n_frames * nt * S, lambda got: None, name=f"level {L} flags"))
        lats.append((bufs[L].data_ptr(), cap[L], tile, tile, offs[L][1], offs[L][0]))
        if L == 1:
            nt1, S1 = nt, S
    cb, lb = info[1]
    nt = nt1
    assert nt == 4 and lb == 4 * cb and cap[1] == 2 * lb
    assert not (want_lat[1] == POISON).all()
    # level 1 as 2 x 2 chunks a layer, two layers to a shard, shards of 2 x 1 chunks
    sdims = [(TIME, 0, 4, 2), (SPACE, 256, tile, 2), (SPACE, 256, tile, 1)]
    st = aqz.ZarrShardSet(sdims, 0)
    m = zm.ShardModel(sdims)
    assert (st.n_shards, st.chunks_per_shard, st.chunks_per_layer, st.layers_per_shard) == \
        (2, 4, 4, 2)
    stride = cb + aqz.BLOSC_MAX_OVERHEAD
    out_cap = nt * stride
    # expected: the host path's frames of the oracle's chunks, packed by the model
    ref, has_want, per_layer = [], [], []
    for layer in range(2):
        chunks = want_lat[1][layer * lb:(layer + 1) * lb]
        fr = host_frames(ctx, chunks, cb, nt, 1, 1, 2)
        has = [int(chunks[c * cb:(c + 1) * cb].any()) for c in range(nt)]
        sizes = [len(f) for f in fr]
        packed = np.zeros(nt * stride, np.uint8)
        for c, f in enumerate(fr):
            packed[c * stride:c * stride + len(f)] = np.frombuffer(f, np.uint8)
        rows, total, place = m.append(sizes, has)
        per_layer.append((placed(packed, stride, sizes, place, out_cap),
                          segments_expect(rows, total), rows, total))
        ref.append(fr)
        has_want.append(has)
    assert has_want == [[1, 0, 1, 1], [1, 0, 0, 1]]
    got = {}

    def keep(name, want):
        def check(snap):
            got[name] = snap.copy()
            assert np.array_equal(snap, want), "differs from the model's bytes"
        return check

    d_frames = sw.output(nt * stride, lambda g: None, name="lz4 frames")
    d_sizes = sw.output(4 * nt, lambda g: None, name="frame sizes")
    d_has = sw.output(nt, lambda g: None, name="has_data")
    d_out = [sw.output(out_cap, keep(f"out{k}", per_layer[k][0]), name=f"device_out layer {k}")
             for k in range(2)]
    d_seg = [sw.output(8 * st.segment_words, keep(f"seg{k}", per_layer[k][1]),
                       name=f"segments layer {k}") for k in range(2)]
    d_tab = sw.output(st.table_bytes * 2, keep("tab", tables_expect(oracle, m)), name="tables")
    d_off = sw.output(16, keep("off", as_bytes(np.array(m.file_off, np.uint64))),
                      name="table offsets")

    def call(sw):
        s = sw.hip_stream
        ds.run_device_batch_chunked(d_in.data_ptr(), n_frames, lats,
                                    device_nonzero=[None] + [f.data_ptr() for f in flags[1:]],
                                    stream=s)
        st.begin(s)
        for layer in range(2):
            src = bufs[1].data_ptr() + layer * lb
            with torch.cuda.stream(sw.stream):
                d_has.zero_()
            # 3-D dims: tile_group_offset is 0 for every frame
            aqz.zarr_shard_chunk_has_data_device(flags[1].data_ptr() + layer * 4 * nt * S1, 4, nt,
                                                 S1, [0] * 4, d_has.data_ptr(), s)
            ctx.lz4_frames_device(1, 1, 2, src, cb, nt, d_frames.data_ptr(), stride,
                                  d_sizes.data_ptr(), s)
            st.append_layer_device(d_frames.data_ptr(), stride, d_out[layer].data_ptr(), out_cap,
                                   d_seg[layer].data_ptr(), d_sizes.data_ptr(), d_has.data_ptr(),
                                   s)
            sw.snapshot(d_has, np.asarray(has_want[layer], np.uint8), f"has_data layer {layer}")
        st.tables_device(d_tab.data_ptr(), d_off.data_ptr(), s)

    sw.run(call)
    # walk each shard's image by its own table, as test_pyramid_level_to_shards does
    images = [bytearray() for _ in range(st.n_shards)]
    for layer in range(2):
        seg = got[f"seg{layer}"].view(np.uint64)
        for s_ in range(st.n_shards):
            start, nbytes, file_off = (int(v) for v in seg[3 * s_:3 * s_ + 3])
            assert file_off == len(images[s_])
            images[s_] += got[f"out{layer}"][start:start + nbytes].tobytes()
    tab = got["tab"].reshape(st.n_shards, st.table_bytes)
    tab_off = got["off"].view(np.uint64)
    for s_ in range(st.n_shards):
        assert int(tab_off[s_]) == len(images[s_])
        pairs = tab[s_, :-4].copy().view(np.uint64).reshape(st.chunks_per_shard, 2)
        assert int(tab[s_, -4:].copy().view(np.uint32)[0]) == oracle.crc32c(tab[s_, :-4])
        used = 0
        for layer in range(2):
            for c in range(nt):
                if m.shard_of[c] != s_:
                    continue
                off, ext = (int(v) for v in pairs[layer * m.spl + int(m.slot_of[c])])
                if not has_want[layer][c]:
                    assert (off, ext) == (zm.SENTINEL, zm.SENTINEL)
                    continue
                assert bytes(images[s_][off:off + ext]) == ref[layer][c], (s_, layer, c)
                used += ext
        assert used == len(images[s_])
    st.close()
    ds.close()


# ---- 9. aqz_node_run_device_batch --------------------------------------------

@pytest.mark.parametrize("stage_all", [False, True], ids=["in_place", "stage_all"])
def test_node_run_device_batch(aqz, oracle, stage_all):
    """Handles [0, 0] on a stalled caller's stream: in place the blocks run on
    that stream; staged, the pull streams wait for `ready` and the caller's
    stream for every block's `done`.  Read on the caller's stream only."""
    geo = halving(256, 128, 3)
    n, dtype = 6, np.uint16
    frames = random_frames(np.random.default_rng(13), dtype, (n, 128, 256))
    emitted = oracle_stream(oracle.OracleDownsampler(geo, dtype, MEAN), frames, len(geo))
    sw = Sandwich(f"node_run_device_batch stage_all={stage_all}")
    d_in = sw.input(frames)
    outs = [None] + [sw.output(n * w * h * 2, level_expect(emitted[L], n * w * h * 2),
                               name=f"level {L}") for L, (w, h, _) in enumerate(geo[1:], 1)]
    node = aqz.Node(geo, dtype, MEAN, [0, 0])
    seen = {}
    try:
        def call(sw):
            seen["counts"] = node.run_device_batch(d_in.data_ptr(), 0, n,
                                                   [0] + [o.data_ptr() for o in outs[1:]],
                                                   sw.hip_stream, stage_all=stage_all)
        sw.run(call)
        assert seen["counts"] == [n] * len(geo)
    finally:
        node.close()
