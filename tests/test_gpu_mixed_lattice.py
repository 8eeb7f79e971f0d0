"""GPU: aqz_ds_run_device_mixed_chunked — every tile of every frame a mixed
pyramid emits straight into its chunk of a lattice of chunk buffers
(aqz_ds_last_batch_kind 8).  Chunks hold 2 planes in Z, so consecutive emitted
frames share a chunk at different internal offsets; expected bytes are the
oracle's levels tiled by oracle.tile_frame at oracle.chunk_frame_offsets'
places; every byte no frame owns keeps the poison; flags are exactly 0 or 1."""
import numpy as np
import pytest

import mixed_batch_cases as mc
import mixed_tiled_cases as tc
from gpu_util import empty_device, from_device, launch_stream, random_frames, to_device, torch_cuda
from stream_order import Sandwich

pytestmark = pytest.mark.gpu

# name, stacks-of-2^zcount in the batch, chunk shapes (z, y, x) per level,
# T/Z/Y/X or Z/Y/X, the batch's lead in units of 2^zcount frames
CASES = [
    # u8 37 x 23 under 2 x 8 x 5: ragged both ways; level 5 emits frames 1..4
    # of its stack: from inside chunk 0 through chunks 1 and 2 (three layers)
    ("zrun3_zrun2_851", 4, [None] + [(2, 8, 5)] * 5, False, 1),
    # f32, ragged in Y and X; level 4 emits frames 1..4
    ("volume1_zrun3", 4, [None, (2, 16, 12), (2, 16, 12), (2, 5, 32), (2, 24, 7)], False, 1),
    # T/Z/Y/X: three time points, each a stack; 2 planes a chunk in Z
    ("volume1_zrun3", 3, [None, (2, 16, 12), (2, 16, 16), (2, 8, 32), (2, 24, 20)], True, 2),
    ("xy_xyz_z", 3, [None, (2, 8, 8), (2, 8, 8), (2, 8, 8)], True, 0),
]
IDS = [f"{c[0]}-{'tzyx' if c[3] else 'zyx'}" for c in CASES]


def build(oracle, case, seed=0):
    name, units, shapes, four_d, lead = case
    geo, _, dtype, _ = mc.FIXED[name]
    zc = mc.zcount(geo, len(geo) - 1)
    n = units << zc
    frames = random_frames(np.random.default_rng(seed), dtype, (n, geo[0][1], geo[0][0]))
    frames[: n // 2, :, : max(1, geo[0][0] // 2)] = 0       # zero tiles exist
    levels = mc.oracle_levels(oracle, geo, dtype, mc.MEAN, frames)
    firsts = [(lead << zc) >> mc.zcount(geo, L) for L in range(len(geo))]
    want = tc.expected_chunked(oracle, geo, levels, shapes, firsts, dtype, four_d)
    return geo, dtype, n, frames, levels, want


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lattice(aqz, oracle, case):
    geo, dtype, n, frames, levels, want = build(oracle, case)
    shapes = case[2]
    for L in range(1, len(geo)):
        offs = want[L][1]
        assert len(offs) == mc.emitted(geo, n)[L]
        if len(offs) > 1 and geo[L][2] > 1:   # two planes share a chunk
            assert any(b - a == shapes[L][1] * shapes[L][2] * np.dtype(dtype).itemsize
                       for a, b in zip(offs, offs[1:])), (L, offs)
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        slots = [None] + [ds.mixed_flag_slots(L, *shapes[L][1:]) for L in range(1, len(geo))]
        lat = tc.Lattice(geo, dtype, shapes, n, want, slots)
        d_in, src = tc.device_input(frames, 3)
        assert lat.run(ds, src) == mc.emitted(geo, n)
        torch_cuda().cuda.synchronize()
        assert ds.last_batch_kind() == 8
    finally:
        ds.close()
    lat.check(oracle, levels, case[0])


def test_bad_lattices_are_refused(aqz, oracle):
    """Out of the buffer, misaligned and short-stride lattices: status 1 with a
    message naming the level, nothing written."""
    case = CASES[1]
    geo, dtype, n, frames, levels, want = build(oracle, case)
    shapes = case[2]
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        lat = tc.Lattice(geo, dtype, shapes, n, want, [None] + [1] * (len(geo) - 1))
        d_in, src = tc.device_input(frames)
        good = lat.lattices()

        def refused(L, change, match):
            lats = list(good)
            base, cap, cy, cx, cb, offs = lats[L]
            lats[L] = change(base, cap, cy, cx, cb, list(offs))
            with pytest.raises(aqz.AqzError, match=match) as e:
                ds.run_device_mixed_chunked(src, n, lats, lat.flag_ptrs(), launch_stream())
            assert e.value.status == 1
        last = len(geo) - 1
        refused(last, lambda b, cap, cy, cx, cb, o: (b, o[-1] + 4, cy, cx, cb, o),
                f"level {last} frame 3.*outside the lattice buffer")
        refused(2, lambda b, cap, cy, cx, cb, o: (b, cap, cy, cx, cb, o[:-1] + [cap]),
                "level 2 frame 15.*outside the lattice buffer")
        refused(3, lambda b, cap, cy, cx, cb, o: (b, cap, cy, cx, cb, [o[0] + 2] + o[1:]),
                "level 3 frame 0")
        refused(1, lambda b, cap, cy, cx, cb, o: (b, cap, cy, cx, cy * cx * 4 - 4, o),
                "level 1: chunk stride")
        refused(1, lambda b, cap, cy, cx, cb, o: (b, cap, cy, cx, cb + 2, o),
                "level 1: chunk stride")
        refused(4, lambda b, cap, cy, cx, cb, o: (0, cap, cy, cx, cb, o), "level 4 needs an output")
        torch_cuda().cuda.synchronize()
        assert ds.last_batch_kind() == -1
        for b in lat.bufs[1:] + lat.flags[1:]:
            assert (from_device(b, np.uint8, (-1,)) == tc.POISON).all()
        # and the good one goes through
        assert lat.run(ds, src) == mc.emitted(geo, n)
    finally:
        ds.close()
    lat.check(oracle, levels, "after the refusals")


@pytest.mark.parametrize("i", range(tc.N_FUZZ_CHUNKED))
def test_fuzz_chunked(aqz, oracle, i):
    c = tc.fuzz_chunked_case(i)
    geo, dtype, method = c["geo"], c["dtype"], c["method"]
    frames = random_frames(c["rng"], dtype, (c["n"], geo[0][1], geo[0][0]))
    frames[: max(1, c["n"] // 2), :, : max(1, geo[0][0] // 2)] = 0
    levels = mc.oracle_levels(oracle, geo, dtype, method, frames)
    want = tc.expected_chunked(oracle, geo, levels, c["shapes"], c["firsts"], dtype)
    ds = aqz.Downsampler(geo, dtype, method)
    ctx = f"fuzz {i} {geo} x {c['n']} {np.dtype(dtype).name} m{method} {c['shapes'][1:]}"
    try:
        slots = [None] + [ds.mixed_flag_slots(L, *c["tiles"][L]) for L in range(1, len(geo))]
        lat = tc.Lattice(geo, dtype, c["shapes"], c["n"], want, slots, c["flags"])
        d_in, src = tc.device_input(frames, c["offs"][0])
        assert lat.run(ds, src) == mc.emitted(geo, c["n"]), ctx
        torch_cuda().cuda.synchronize()
        assert ds.last_batch_kind() == 8, ctx
    finally:
        ds.close()
    lat.check(oracle, levels, ctx)


# ---- the pinned halves of the offset tables ----------------------------------------

class Rig:
    """One chunked batch of `n` frames of z_then_xy starting `lead` pairs into
    the stack (an odd lead starts levels 1 and 2 inside a chunk)."""

    GEO, _, DTYPE, _ = mc.FIXED["z_then_xy"]
    SHAPES = [None, (2, 16, 12), (2, 16, 16)]

    def __init__(self, sw, oracle, lead, seed, n=8):
        geo, self.n = self.GEO, n
        frames = random_frames(np.random.default_rng(seed), self.DTYPE, (n, geo[0][1], geo[0][0]))
        levels = mc.oracle_levels(oracle, geo, self.DTYPE, mc.MEAN, frames)
        firsts = [2 * lead, lead, lead]
        want = tc.expected_chunked(oracle, geo, levels, self.SHAPES, firsts, self.DTYPE)
        self.d_in = sw.input(frames)
        self.offsets = [None] + [want[L][1] for L in (1, 2)]
        self.lats = [None]
        for L in (1, 2):
            buf, offs, cb, cap = want[L]
            _, cy, cx = self.SHAPES[L]
            d = sw.output(cap, buf, name=f"lead {lead} level {L} lattice")
            self.lats.append((d.data_ptr(), cap, cy, cx, cb, offs))

    def run(self, ds, hip_stream):
        return ds.run_device_mixed_chunked(self.d_in.data_ptr(), self.n, self.lats,
                                           stream=hip_stream)


def test_three_chunked_batches_behind_a_stall(aqz, oracle):
    """Three calls with three offset tables: the first two return while the
    stream is stalled, each table through its own pinned half; the third needs
    the first's half and waits for it by contract.  All three land at their
    own places."""
    ds = aqz.Downsampler(Rig.GEO, Rig.DTYPE, mc.MEAN, device=0)
    sw = Sandwich("three mixed chunked batches")
    rigs = [Rig(sw, oracle, lead, seed=20 + lead + n, n=n) for lead, n in ((0, 8), (1, 8), (0, 4))]
    assert len({tuple(r.offsets[1]) for r in rigs}) == 3
    blocked = {}

    def call(sw):
        rigs[0].run(ds, sw.hip_stream)
        rigs[1].run(ds, sw.hip_stream)
        sw.still_stalled("two mixed chunked batches in a row")
        rigs[2].run(ds, sw.hip_stream)
        if sw.phase == "stalled":
            blocked["third"] = sw.done.query()

    sw.run(call, blocks=True)  # the third call waits by contract
    assert blocked["third"], "the third chunked batch returned with the first still pending"
    assert ds.last_batch_kind() == 8
    ds.close()


# ---- frames -> shards -> frames ------------------------------------------------------

def test_round_trip_frames_shards_frames(aqz, oracle):
    """Levels 1 and 2 of volume1_zrun3 (an XYZ level and a Z level, f32): the
    chunked batch, has_data from its flags, LZ4 frames, shards and tables,
    every shard decoded through its own table, the gather back into frames —
    which must be the oracle's level frames.  One chunk layer a level: T/Y/X
    with the level's 16 / 8 emitted frames a chunk, ragged 16 x 12 chunks in
    2 x 2-chunk shards."""
    from test_gpu_chunk_gather import Dest
    torch = torch_cuda()
    geo, n, dtype, _ = mc.FIXED["volume1_zrun3"]
    counts = mc.emitted(geo, n)
    frames = random_frames(np.random.default_rng(3), dtype, (n, geo[0][1], geo[0][0]),
                           specials=False)
    frames[frames == 0] = 1
    frames[:, 0:32, 24:48] = 0      # levels 1..4: the chunk at rows 0-15, columns 12-23
    levels = mc.oracle_levels(oracle, geo, dtype, mc.MEAN, frames)
    shapes = [None] + [(counts[L], 16, 12) for L in range(1, len(geo))]
    dims_of = lambda L: [(tc.TIME, 0, counts[L], 1), (tc.SPACE, geo[L][1], 16, 2),
                         (tc.SPACE, geo[L][0], 12, 2)]
    bpp = 4
    want = [None]
    for L in range(1, len(geo)):
        offs, cb, lb = oracle.chunk_frame_offsets(dims_of(L), bpp, 0, counts[L])
        want.append((None, offs, cb, lb))
    ds = aqz.Downsampler(geo, dtype, mc.MEAN, device=0)
    slots = [None] + [ds.mixed_flag_slots(L, 16, 12) for L in range(1, len(geo))]
    assert slots[1:] == [1] * 4
    lat = tc.Lattice(geo, dtype, shapes, n, want, slots)
    d_in, src = tc.device_input(frames)
    s = launch_stream()
    assert lat.run(ds, src, s) == counts and ds.last_batch_kind() == 8          # step 1
    ctx = aqz.BloscContext(0, 0)
    after = []
    for L in (1, 2):
        lw, lh, _ = geo[L]
        nt, cb = lat.nt[L], want[L][2]
        base, internal, pcb, cpl = aqz.chunk_frame_places(dims_of(L), bpp, 0, counts[L])
        assert (pcb, cpl) == (cb, nt) and not base.any()
        d_has = empty_device(nt)
        d_has.fill_(0)
        aqz.zarr_shard_chunk_has_data_device(lat.flags[L].data_ptr() + tc.GUARD, counts[L], nt, 1,
                                             base, d_has.data_ptr(), s)          # step 2
        stride = cb + aqz.BLOSC_MAX_OVERHEAD
        d_frames, d_sizes = empty_device(nt * stride), empty_device(4 * nt)
        ctx.lz4_frames_device(5, 1, bpp, lat.bufs[L].data_ptr() + tc.GUARD, cb, nt,
                              d_frames.data_ptr(), stride, d_sizes.data_ptr(), s)  # step 3
        st = aqz.ZarrShardSet(dims_of(L), 0)
        assert st.chunks_per_layer == nt and st.chunks_per_shard == 4
        st.begin(s)
        d_out = empty_device(nt * stride)
        d_seg = empty_device(8 * st.segment_words)
        st.append_layer_device(d_frames.data_ptr(), stride, d_out.data_ptr(), nt * stride,
                               d_seg.data_ptr(), d_sizes.data_ptr(), d_has.data_ptr(), s)
        d_tab = empty_device(st.n_shards * st.table_bytes)
        d_taboff = empty_device(8 * st.n_shards)
        st.tables_device(d_tab.data_ptr(), d_taboff.data_ptr(), s)               # step 4
        seg = from_device(d_seg, np.uint64, (-1,))[:-1].reshape(-1, 3)
        k = st.chunks_per_shard
        d_chunks = empty_device(st.n_shards * k * cb)
        d_chunks.fill_(tc.POISON)
        d_st = empty_device(4 * st.n_shards * k)
        for sh in range(st.n_shards):
            start, nbytes, file_off = (int(v) for v in seg[sh])
            ctx.zarr_shard_decompress_device(bpp, cb, d_out.data_ptr() + start, nbytes, file_off,
                                             d_tab.data_ptr() + sh * st.table_bytes, k,
                                             d_chunks.data_ptr() + sh * k * cb, cb,
                                             d_st.data_ptr() + 4 * sh * k, s)     # step 5
        _, shard_of, internal_of = aqz.zarr_shard_layout(dims_of(L))
        table = (shard_of.astype(np.uint32) * k + internal_of).astype(np.uint32)
        d_table = to_device(table)
        fb = lw * lh * bpp
        dst = Dest(counts[L], fb, fb)
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        aqz.chunk_gather_frames_device(dtype, lw, lh, 16, 12, d_chunks.data_ptr(), cb,
                                       st.n_shards * k, d_table.data_ptr(), nt, base, internal,
                                       dst.ptr, fb, d_bad.data_ptr(), s)         # step 6
        got = dst.frames(dtype, lh, lw, f"level {L}")   # and the guards
        mc.assert_parity(got, levels[L], f"level {L}: the frames did not come back")
        has = from_device(d_has, np.uint8, (-1,))
        assert np.flatnonzero(has == 0).tolist() == [1], (L, has)
        assert int(d_bad.cpu()[0]) == 0
        after.append(st)
    for st in after:
        st.close()
    ctx.close()
    ds.close()
