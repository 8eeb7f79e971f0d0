"""GPU: aqz_ds_run_device_mixed_tiled and aqz_ds_run_device_mixed_chunked
between pending work on the caller's stream (tests/stream_order.py, imported
as it is).  The unstalled run is the handle's first use (or, on a handle that
has run a smaller batch, the call that grows the chain scratch and the offset
staging) and is checked like the stalled one — the steady state — which must
return while the stall runs, read its inputs and write its outputs in stream
order."""
import numpy as np
import pytest

import mixed_batch_cases as mc
import mixed_tiled_cases as tc
from stream_order import Sandwich

pytestmark = pytest.mark.gpu

# two runs chained through handle scratch: XYZ x 2 then XY x 2; Z x 3 then Z x 2
SHAPES = [("volume2_cascade2", (32, 64)), ("zrun3_zrun2_851", (8, 5))]


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def flags_expect(want_nz, slots):
    def check(got):
        raw = got.reshape(want_nz.shape + (slots,))
        assert np.isin(raw, (0, 1)).all(), "a flag byte is neither 0 nor 1"
        assert np.array_equal(raw.any(axis=-1), want_nz), "zero scan differs"
    return check


class Rig:
    """Inputs, poisoned outputs and oracle expectations of one batch of
    `units` x 2^zcount frames, tiled or (chunks of 2 planes) chunked."""

    def __init__(self, sw, oracle, ds, name, spec, units, chunked, seed=1):
        geo, _, dtype, _ = mc.FIXED[name]
        self.geo, self.n = geo, units << mc.zcount(geo, len(geo) - 1)
        rng = np.random.default_rng(seed)
        frames = mc.random_frames(rng, dtype, (self.n, geo[0][1], geo[0][0]))
        frames[: self.n // 2, :, : geo[0][0] // 2] = 0
        levels = mc.oracle_levels(oracle, geo, dtype, mc.MEAN, frames)
        self.tiles = tc.tiles_for(geo, spec)
        self.d_in = sw.input(frames)
        self.chunked = chunked
        self.outs, self.flags, self.lats = [None], [None], [None]
        want_t = tc.expected_tiled(oracle, levels, self.tiles)
        shapes = [None] + [(2,) + t for t in self.tiles[1:]]
        want_c = tc.expected_chunked(oracle, geo, levels, shapes, [0] * len(geo), dtype)
        for L in range(1, len(geo)):
            t, nz = want_t[L]
            slots = ds.mixed_flag_slots(L, *self.tiles[L])
            if chunked:
                buf, offs, cb, cap = want_c[L]
                d = sw.output(cap, buf, name=f"level {L} lattice")
                self.lats.append((d.data_ptr(), cap) + self.tiles[L] + (cb, offs))
            else:
                self.outs.append(sw.output(t.nbytes, as_bytes(t), name=f"level {L} tiles"))
            self.flags.append(sw.output(nz.size * slots, flags_expect(nz, slots),
                                        name=f"level {L} flags"))

    def run(self, ds, hip_stream):
        flags = [0] + [f.data_ptr() for f in self.flags[1:]]
        if self.chunked:
            return ds.run_device_mixed_chunked(self.d_in.data_ptr(), self.n, self.lats, flags,
                                               hip_stream)
        return ds.run_device_mixed_tiled(self.d_in.data_ptr(), self.n, self.tiles,
                                         [0] + [o.data_ptr() for o in self.outs[1:]], flags,
                                         hip_stream)


@pytest.mark.parametrize("chunked", [False, True], ids=["tiled", "chunked"])
@pytest.mark.parametrize("name,spec", SHAPES, ids=[s[0] for s in SHAPES])
def test_first_use_then_steady_state(aqz, oracle, name, spec, chunked):
    geo, _, dtype, _ = mc.FIXED[name]
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    sw = Sandwich(f"run_device_mixed_{'chunked' if chunked else 'tiled'} {name}")
    rig = Rig(sw, oracle, ds, name, spec, 2, chunked)
    counts = []
    try:
        sw.run(lambda sw: counts.append(rig.run(ds, sw.hip_stream)))
        assert counts == [mc.emitted(geo, rig.n)] * 2 and ds.last_batch_kind() == 8
    finally:
        ds.close()


@pytest.mark.parametrize("chunked", [False, True], ids=["tiled", "chunked"])
def test_grown_scratch_then_steady_state(aqz, oracle, chunked):
    """A batch of one unit first; the Sandwich's batch of four then grows the
    chain scratch (and the offset staging) in its unstalled run."""
    name, spec = SHAPES[0]
    geo, _, dtype, _ = mc.FIXED[name]
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        small = Sandwich(f"mixed {name} one unit")
        first = Rig(small, oracle, ds, name, spec, 1, chunked, seed=2)
        small.run(lambda sw: first.run(ds, sw.hip_stream))
        sw = Sandwich(f"mixed {name} four units")
        rig = Rig(sw, oracle, ds, name, spec, 4, chunked, seed=3)
        sw.run(lambda sw: rig.run(ds, sw.hip_stream))
        assert ds.last_batch_kind() == 8
    finally:
        ds.close()
