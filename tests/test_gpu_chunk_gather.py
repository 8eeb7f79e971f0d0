"""GPU: aqz_chunk_gather_frames_device and aqz_untile_frame_device — chunk
buffers back into row-major frames (csrc/gather_kernels.hip).

Every comparison is byte for byte.  The chunk buffers are built on the CPU
from the frames by the oracle's tiling and addressing
(tests/chunk_gather_cases.py) and the result must be the frames themselves.
Every chunk byte no in-frame pixel owns is poison, so a read outside a frame
shows; every destination is poisoned, with 64 guard bytes on each side that
must survive, as must the bytes between two frames.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chunk_gather_cases as cg
import kat_runner
import tiled_base_cases as tb
from gpu_util import empty_device, from_device, launch_stream, to_device, torch_cuda

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = cg.GUARD


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Dest:
    """n frames of fb bytes, `stride` apart, `off` bytes past a 64-byte
    boundary, in a poisoned buffer with GUARD bytes on each side."""

    def __init__(self, n, fb, stride, off=0):
        torch = torch_cuda()
        self.n, self.fb, self.stride = n, fb, stride
        self.lead = GUARD + off
        self.buf = torch.full((self.lead + (n - 1) * stride + fb + GUARD,), cg.DST_POISON,
                              dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + self.lead

    def frames(self, dtype, h, w, ctx=""):
        """The frames; everything around them must still be poison."""
        got = from_device(self.buf, np.uint8, (-1,))
        own = np.zeros(got.size, bool)
        for k in range(self.n):
            own[self.lead + k * self.stride:self.lead + k * self.stride + self.fb] = True
        touched = np.flatnonzero(~own & (got != cg.DST_POISON))
        assert touched.size == 0, f"{ctx}: byte {touched[0]} outside the frames written"
        return got[own].view(dtype).reshape(self.n, h, w)

    def untouched(self):
        return bool((from_device(self.buf, np.uint8, (-1,)) == cg.DST_POISON).all())


def device_chunks(src, off=0):
    """The source on the device, `off` bytes past a 64-byte boundary, poison
    in front: (tensor, pointer)."""
    raw = np.full(GUARD + off + src.chunks.size, cg.POISON, np.uint8)
    raw[GUARD + off:] = src.chunks.reshape(-1)
    t = to_device(raw)
    return t, t.data_ptr() + GUARD + off


def gather(aqz, src, dst_off=0, src_off=0, gap=0, with_bad=True, ctx=""):
    """Runs the call on a Source; returns (frames, bad_slot or None)."""
    torch = torch_cuda()
    n, fb = len(src.frames), src.w * src.h * src.bpp
    keep, p_src = device_chunks(src, src_off * src.bpp)
    dst = Dest(n, fb, fb + gap * src.bpp, dst_off * src.bpp)
    d_tab = to_device(src.table) if src.table is not None else None
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda") if with_bad else None
    aqz.chunk_gather_frames_device(
        src.dtype, src.w, src.h, src.tr, src.tc, p_src, src.stride, src.n_slots,
        d_tab.data_ptr() if d_tab is not None else 0, src.n_chunks, src.base, src.internal,
        dst.ptr, dst.stride, d_bad.data_ptr() if with_bad else 0, launch_stream())
    got = dst.frames(src.dtype, src.h, src.w, ctx)
    del keep
    return got, (int(d_bad.cpu()[0]) if with_bad else None)


def check(aqz, src, ctx, **kw):
    got, bad = gather(aqz, src, ctx=ctx, **kw)
    want = src.expected()
    diff = np.flatnonzero((bits(got) != bits(want)).reshape(-1))
    assert diff.size == 0, (f"{ctx}: {diff.size} bytes differ, first at byte {diff[0]} "
                            f"({bits(got).reshape(-1)[diff[0]]:#x}, expected "
                            f"{bits(want).reshape(-1)[diff[0]]:#x})")
    if bad is not None:
        assert bad == src.bad(), f"{ctx}: bad_slot {bad}"


# ---- the fixed shapes --------------------------------------------------------------

@pytest.mark.parametrize("case", cg.FIXED, ids=lambda c: c[0])
def test_fixed_shapes(aqz, oracle, case):
    name, w, h, tile, dtype, _ = case
    rng = np.random.default_rng(w * 31 + h)
    frames = cg.random_bytes_frames(rng, dtype, (3, h, w))
    # 2 frames a chunk, the batch starts at frame 1: inside a chunk, two layers
    check(aqz, cg.Source(oracle, cg.tyx(w, h, tile, 2), frames, 1), name)


@pytest.mark.parametrize("dtype", cg.DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_dtype_keeps_its_bits(aqz, oracle, dtype):
    """1031 x 517, tiles of 128 x 256: random bytes, and for the float types
    every bit pattern of tests/float_cases.py's catalogue (signalling NaNs,
    payloads, -0.0, subnormals) sown over the frame, its ends included."""
    w, h, tile = 1031, 517, (128, 256)
    rng = np.random.default_rng(np.dtype(dtype).itemsize * 7 + np.dtype(dtype).kind.encode()[0])
    frames = cg.random_bytes_frames(rng, dtype, (2, h, w)).copy()
    if np.dtype(dtype).kind == "f":
        pats = cg.float_patterns(dtype)
        ut = np.dtype(f"u{np.dtype(dtype).itemsize}")
        flat = frames.view(ut).reshape(2, -1)
        for k in range(2):
            at = rng.choice(flat.shape[1], 40 * len(pats), replace=False)
            flat[k, at] = np.tile(pats.view(ut), 40)
            flat[k, :len(pats)] = pats.view(ut)       # the frame's head
            flat[k, -len(pats):] = pats.view(ut)[::-1]  # and its tail
    check(aqz, cg.Source(oracle, cg.tyx(w, h, tile), frames, 0), np.dtype(dtype).name)


@pytest.mark.parametrize("dtype,shape", [(np.uint8, (21, 37, (5, 20))), (np.uint16, (13, 43, (4, 16))),
                                         (np.float32, (9, 29, (3, 8))), (np.int64, (7, 11, (2, 4))),
                                         (np.uint16, (6, 19, (4, 3)))],
                         ids=["u8", "u16", "f32", "i64", "u16_elem"])
def test_pointers_and_stride_at_element_offsets(aqz, oracle, dtype, shape):
    """Source, destination and frame stride 1 to 7 elements off a 16-byte
    boundary: heads and tails of every length, vectors loaded at every
    misalignment."""
    h, w, tile = shape
    rng = np.random.default_rng(h * w)
    frames = cg.random_bytes_frames(rng, dtype, (3, h, w))
    src = cg.Source(oracle, cg.tyx(w, h, tile, 2), frames, 1, stride_extra=np.dtype(dtype).itemsize)
    for off in range(1, 8):
        check(aqz, src, f"offset {off}", dst_off=off, src_off=8 - off, gap=off)
        check(aqz, src, f"dst offset {off}", dst_off=off)


@pytest.mark.parametrize("geo", cg.TILING_GEOMETRIES,
                         ids=lambda g: f"{g[0]}x{g[1]}_{np.dtype(g[2]).name}_{g[3]}x{g[4]}")
def test_untile_inverts_tile_frame_device(aqz, oracle, geo):
    """aqz_tile_frame_device, then aqz_untile_frame_device on its output: the
    frame again.  And on the oracle's tiles with poison in the overhang."""
    torch = torch_cuda()
    w, h, dtype, tr, tc = geo
    bpp = np.dtype(dtype).itemsize
    rng = np.random.default_rng(w + h)
    frame = cg.random_bytes_frames(rng, dtype, (1, h, w))
    nt = -(-h // tr) * -(-w // tc)
    d_in = to_device(frame)
    d_tiles = empty_device(nt * tr * tc * bpp)
    d_nz = torch.zeros(nt, dtype=torch.int32, device="cuda")
    s = launch_stream()
    aqz.tile_frame_device(dtype, d_in.data_ptr(), w, h, tr, tc, d_tiles.data_ptr(),
                          d_nz.data_ptr(), s)
    dst = Dest(1, w * h * bpp, w * h * bpp)
    aqz.untile_frame_device(dtype, d_tiles.data_ptr(), w, h, tr, tc, dst.ptr, s)
    assert np.array_equal(bits(dst.frames(dtype, h, w, "after tile_frame_device")), bits(frame))
    src = cg.Source(oracle, cg.tyx(w, h, (tr, tc)), frame, 0)
    assert src.n_chunks == nt and src.stride == tr * tc * bpp
    keep, p = device_chunks(src)
    dst = Dest(1, w * h * bpp, w * h * bpp)
    aqz.untile_frame_device(dtype, p, w, h, tr, tc, dst.ptr, launch_stream())
    assert np.array_equal(bits(dst.frames(dtype, h, w, "oracle tiles")), bits(frame))


# ---- lattices ------------------------------------------------------------------------

def test_time_lattice_from_both_sources(aqz, oracle):
    """tests/test_gpu_lattice.py's T/Y/X geometry read backwards: 3 frames a
    chunk, frames 2 .. 8 (inside a chunk, three layers), level 0 and level 1.
    Once from the CPU-built lattice and once from the one
    aqz_ds_run_device_batch_chunked_base wrote."""
    torch = torch_cuda()
    w, h, n, first = 520, 384, 7, 2
    geo = tb.halving(w, h, 2)
    shapes = [(3, 128, 96), (3, 64, 48)]
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    levels = [frames, np.stack([oracle.cascade_2d(f, 2, aqz.MEAN)[0] for f in frames])]
    ds = aqz.Downsampler(geo, np.uint16, aqz.MEAN, device=0)
    lat = tb.Lattice(oracle, ds, geo, shapes, np.uint16, aqz.MEAN, frames, first)
    s = launch_stream()
    assert lat.run(ds, s) == [n, n]
    for L, want in enumerate(levels):
        lw, lh, _ = geo[L]
        dims = tb.chunk_dims(geo, L, shapes[L])
        src = cg.Source(oracle, dims, want, first)
        assert src.n_chunks * src.chunk_bytes == lat.want[L][4]
        check(aqz, src, f"L{L} CPU lattice")
        s = launch_stream()
        dst = Dest(n, lw * lh * 2, lw * lh * 2)
        aqz.chunk_gather_frames_device(np.uint16, lw, lh, shapes[L][1], shapes[L][2],
                                       lat.bufs[L].data_ptr(), src.chunk_bytes, src.n_chunks, 0,
                                       src.n_chunks, src.base, src.internal, dst.ptr,
                                       lw * lh * 2, 0, s)
        assert np.array_equal(dst.frames(np.uint16, lh, lw, f"L{L}"), want), f"L{L} device lattice"
    torch.cuda.synchronize()
    ds.close()


def test_channel_lattice(aqz, oracle):
    """T/C/Y/X, channels chunked 2 of 3: a frame's chunk depends on its
    channel, and the second channel chunk is half empty."""
    dims = [(cg.TIME, 0, 2, 1), (cg.CHANNEL, 3, 2, 1), (cg.SPACE, 50, 16, 1),
            (cg.SPACE, 77, 24, 1)]
    frames = cg.random_bytes_frames(np.random.default_rng(8), np.int16, (11, 50, 77))
    check(aqz, cg.Source(oracle, dims, frames, 4), "t/c/y/x")


def test_kat_dims_all_76_frames_take_two_launches(aqz, oracle):
    dims = [tuple(d) for d in kat_runner.load()["addressing"][0]["dims"]]
    assert [d[1:3] for d in dims] == [(0, 5), (3, 2), (5, 2), (48, 16), (64, 16)]
    frames = cg.random_bytes_frames(np.random.default_rng(76), np.uint16, (76, 48, 64))
    assert 76 > cg.FRAMES_PER_LAUNCH == aqz.CHUNK_GATHER_FRAMES
    check(aqz, cg.Source(oracle, dims, frames, 0), "kat dims")
    check(aqz, cg.Source(oracle, dims, frames[:70], 3), "kat dims from frame 3", dst_off=3)


# ---- slot tables ---------------------------------------------------------------------

SLOT_SHAPES = [(1031, 517, (128, 250), np.float32), (11, 7, (4, 3), np.uint8),
               (40, 9, (4, 8), np.uint16)]


@pytest.mark.parametrize("shape", SLOT_SHAPES, ids=["straddle", "elem", "vec"])
def test_slot_tables(aqz, oracle, shape):
    w, h, tile, dtype = shape
    rng = np.random.default_rng(w)
    frames = cg.random_bytes_frames(rng, dtype, (3, h, w)).copy()
    frames.view(np.uint8)[frames.view(np.uint8) == 0] = 1  # a zero is a missing chunk
    dims = cg.tyx(w, h, tile, 2)
    n_chunks = cg.Source(oracle, dims, frames, 1).n_chunks
    n_slots = n_chunks + 5
    perm = rng.permutation(n_slots)[:n_chunks].astype(np.uint32)
    check(aqz, cg.Source(oracle, dims, frames, 1, perm, n_slots), "permutation")
    absent = perm.copy()
    absent[rng.choice(n_chunks, max(2, n_chunks // 4), replace=False)] = cg.ABSENT
    src = cg.Source(oracle, dims, frames, 1, absent, n_slots)
    assert src.bad() == 0 and not np.array_equal(src.expected(), frames)
    check(aqz, src, "absent chunks")
    bad = absent.copy()
    victim = int(np.flatnonzero(bad != cg.ABSENT)[1])
    bad[victim] = n_slots  # the first value that is no slot
    src = cg.Source(oracle, dims, frames, 1, bad, n_slots)
    assert src.bad() == 1
    check(aqz, src, "a slot past n_slots")
    check(aqz, src, "a slot past n_slots, no flag", with_bad=False)


# ---- the launch log ------------------------------------------------------------------

def test_launch_log_pins_the_form(aqz):
    """One fresh process with the launch log on: each fixed shape records one
    line of the family `gather` with the form it is named for."""
    env = dict(os.environ)
    env["AQZ_LAUNCH_LOG"] = "1"
    r = subprocess.run([sys.executable, "-u",
                        os.path.join(ROOT, "tests", "chunk_gather_launch_child.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for name, w, h, tile, dtype, form in cg.FIXED:
        lines = rec[name]
        assert len(lines) == 1, (name, lines)
        ln = lines[0]
        assert ln["family"] == "gather" and ln["form"] == cg.log_form(form), (name, ln)
        assert (ln["frames_per_launch"], ln["launches"], ln["frames"]) == (64, 1, 3), (name, ln)
        assert ln["block"] == 256
        if ln["form"] == "elem":
            assert ln["grid"] == -(-w * h // 256) and ln["band_rows"] == 0
        else:
            row = w * np.dtype(dtype).itemsize
            rows = min(h, -(-(64 << 10) // row))
            assert ln["band_rows"] == rows and ln["grid"] == -(-h // rows), (name, ln)
    assert [(ln["form"], ln["launches"], ln["frames"]) for ln in rec["kat_76"]] == [("vec", 2, 76)]
    assert [(ln["form"], ln["launches"]) for ln in rec["untile"]] == [("vec", 1)]
    assert rec["refused"] == []


# ---- refusals ------------------------------------------------------------------------

def test_refusals_leave_the_destination_untouched(aqz, oracle):
    torch = torch_cuda()
    w, h, tile, dtype = 40, 9, (4, 8), np.uint16
    frames = cg.random_bytes_frames(np.random.default_rng(5), dtype, (2, h, w))
    src = cg.Source(oracle, cg.tyx(w, h, tile), frames, 0)
    keep, p_src = device_chunks(src)
    fb = w * h * 2
    dst = Dest(2, fb, fb)
    d_tab = to_device(np.arange(src.n_chunks, dtype=np.uint32))
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = aqz.lib()
    code = aqz.dtype_code(dtype)
    good = dict(dtype=code, w=w, h=h, tr=tile[0], tc=tile[1], chunks=p_src, cstride=src.stride,
                n_slots=src.n_slots, table=d_tab.data_ptr(), n_chunks=src.n_chunks,
                base=src.base.copy(), internal=src.internal.copy(), n=2, frames=dst.ptr,
                fstride=fb, bad=d_bad.data_ptr())

    def call(**change):
        a = dict(good, **change)
        base = np.ascontiguousarray(a["base"], np.uint32) if a["base"] is not None else None
        internal = (np.ascontiguousarray(a["internal"], np.uint64)
                    if a["internal"] is not None else None)
        return L.aqz_chunk_gather_frames_device(
            a["dtype"], a["w"], a["h"], a["tr"], a["tc"], a["chunks"] or None, a["cstride"],
            a["n_slots"], a["table"] or None, a["n_chunks"],
            base.ctypes.data if base is not None else None,
            internal.ctypes.data if internal is not None else None, a["n"],
            a["frames"] or None, a["fstride"], a["bad"] or None, None)

    refused = {
        "null chunks": dict(chunks=0), "null frames": dict(frames=0),
        "null base": dict(base=None), "null internal": dict(internal=None),
        "zero width": dict(w=0), "zero height": dict(h=0), "zero tile rows": dict(tr=0),
        "zero tile cols": dict(tc=0), "zero slots": dict(n_slots=0),
        "zero chunks": dict(n_chunks=0), "zero frames": dict(n=0),
        "zero chunk stride": dict(cstride=0), "zero frame stride": dict(fstride=0),
        "bad dtype": dict(dtype=10), "negative dtype": dict(dtype=-1),
        "tile of 2^31 elements": dict(tr=1 << 16, tc=1 << 15),
        "2^31 tiles": dict(w=(1 << 32) - 1, h=(1 << 32) - 1, tr=1, tc=2),
        "odd chunk stride": dict(cstride=src.stride + 1),
        "odd internal offset": dict(internal=[0, 1]),
        "odd frame stride": dict(fstride=fb + 1),
        "tile past the chunk stride": dict(internal=[0, 2]),
        "chunk stride below a tile": dict(cstride=src.stride - 2),
        "base past n_chunks": dict(base=[0, src.n_chunks - 14]),
        "n_chunks below a frame's tiles": dict(n_chunks=14, table=d_tab.data_ptr()),
        "frame stride below a frame": dict(fstride=fb - 2),
        "identity with n_chunks != n_slots": dict(table=0, n_slots=src.n_slots + 1),
        # 2^25 bands of 128 rows x 64 frames
        "vector grid of 2^31 workgroups": dict(w=256, h=(1 << 32) - 1, tr=1 << 20, tc=256, n=64,
                                                base=[0] * 64, internal=[0] * 64, table=0,
                                                n_chunks=4096, n_slots=4096, cstride=1 << 29,
                                                fstride=1 << 41),
        # 2^40 pixels, 256 a workgroup
        "element grid of 2^31 workgroups": dict(w=1 << 20, h=1 << 20, tr=1 << 20, tc=7, n=1,
                                                 base=[0], internal=[0], table=0,
                                                 n_chunks=1 << 18, n_slots=1 << 18,
                                                 cstride=7 << 21, fstride=1 << 41),
    }
    torch.cuda.synchronize()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst.frames(dtype, h, w), frames)
    dst.buf.fill_(cg.DST_POISON)
    for what, change in refused.items():
        assert call(**change) == 1, what  # AQZ_INVALID_ARGUMENT
        assert L.aqz_last_error().decode().startswith("zarr_shard: chunk_gather_frames_device"), \
            (what, L.aqz_last_error())
    # the optional pointers
    torch.cuda.synchronize()
    assert dst.untouched()
    assert int(d_bad.cpu()[0]) == 0
    assert call(bad=0) == 0 and call(table=0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst.frames(dtype, h, w), frames)
    with pytest.raises(aqz.AqzError):
        aqz.untile_frame_device(dtype, p_src, w, h, 0, 8, dst.ptr)
    with pytest.raises(aqz.AqzError):
        aqz.untile_frame_device(dtype, 0, w, h, 4, 8, dst.ptr)
    torch.cuda.synchronize()


# ---- seeded fuzz ---------------------------------------------------------------------

@pytest.mark.parametrize("i", range(cg.N_FUZZ))
def test_fuzz(aqz, oracle, i):
    c = cg.fuzz_case(i)
    src = cg.fuzz_source(oracle, c)
    bpp = src.bpp
    check(aqz, src, f"fuzz {i} {c['form']}", dst_off=i % (16 // bpp), src_off=(i // 3) % 4,
          gap=(i // 2) % 5)


# ---- frames -> shards -> frames ------------------------------------------------------

def test_round_trip_frames_shards_frames(aqz, oracle):
    """The stream of tests/test_gpu_blosc_decode.py's shard round trip — 96 x
    128 u16, T/Y/X, 3 frames a chunk, one chunk all zero, ragged 2 x 2-chunk
    shards with seeded file offsets — at level 0 and level 1, and all the way
    back: chunked batch, has_data, LZ4 frames, shards and tables, every shard
    decoded through its own table, the gather with slots from
    aqz_zarr_shard_layout.  Level 0 must be the input frames, level 1 the
    oracle's cascade, the skipped chunk zeros.  No pixel leaves the device
    before the comparison, which torch makes there: the host reads each
    layer's segment table (where a shard's bytes begin, as a writer must) and,
    after the comparison, has_data and the statuses."""
    torch = torch_cuda()
    geo = tb.halving(128, 96, 2)
    shapes = [(3, 32, 48), (3, 16, 16)]
    rng = np.random.default_rng(12)
    frames = rng.integers(1, 65536, (3, 96, 128), dtype=np.uint16)
    frames[:, 32:64, 48:96] = 0  # level 0's chunk (1, 1); level 1's chunk (1, 2)
    want = [frames, np.stack([oracle.cascade_2d(f, 2, aqz.MEAN)[0] for f in frames])]
    assert not want[1][:, 16:32, 32:48].any() and want[1][:, 16:32, 23].all()
    d_want = [to_device(x) for x in want]
    ctx = aqz.BloscContext(0, 0)
    ds = aqz.Downsampler(geo, np.uint16, aqz.MEAN, device=0)
    lat = tb.Lattice(oracle, ds, geo, shapes, np.uint16, aqz.MEAN, frames, 0)
    s = launch_stream()
    assert lat.run(ds, s) == [3, 3]                                               # step 1
    after = []
    for L in (0, 1):
        lw, lh, _ = geo[L]
        nt, slots = lat.nt[L], lat.slots[L]
        cb = lat.want[L][2]
        dims = tb.chunk_dims(geo, L, shapes[L])
        base, internal, pcb, cpl = aqz.chunk_frame_places(dims, 2, 0, 3)
        assert (pcb, cpl) == (cb, nt) and base.tolist() == [0, 0, 0]
        d_has = empty_device(nt)
        d_has.fill_(0)
        aqz.zarr_shard_chunk_has_data_device(lat.flags[L].data_ptr(), 3, nt, slots, base,
                                             d_has.data_ptr(), s)                # step 2
        stride = cb + aqz.BLOSC_MAX_OVERHEAD
        d_frames, d_sizes = empty_device(nt * stride), empty_device(4 * nt)
        ctx.lz4_frames_device(5, 1, 2, lat.bufs[L].data_ptr(), cb, nt, d_frames.data_ptr(),
                              stride, d_sizes.data_ptr(), s)                     # step 3
        sdims = [(tb.TIME, 0, 3, 1), (tb.SPACE, lh, shapes[L][1], 2),
                 (tb.SPACE, lw, shapes[L][2], 2)]
        st = aqz.ZarrShardSet(sdims, 0)
        assert st.chunks_per_layer == nt and st.chunks_per_shard == 4
        st.begin(s)
        seeds = [int(v) for v in rng.integers(0, 1 << 34, st.n_shards)]
        st.debug_set_file_offsets(seeds, s)
        d_out = empty_device(nt * stride)
        d_seg = empty_device(8 * st.segment_words)
        st.append_layer_device(d_frames.data_ptr(), stride, d_out.data_ptr(), nt * stride,
                               d_seg.data_ptr(), d_sizes.data_ptr(), d_has.data_ptr(), s)
        d_tab = empty_device(st.n_shards * st.table_bytes)
        d_taboff = empty_device(8 * st.n_shards)
        st.tables_device(d_tab.data_ptr(), d_taboff.data_ptr(), s)               # step 4
        seg = from_device(d_seg, np.uint64, (-1,))[:-1].reshape(-1, 3)  # the segment table only
        n = st.chunks_per_shard
        d_chunks = empty_device(st.n_shards * n * cb)
        d_chunks.fill_(cg.POISON)
        d_st = empty_device(4 * st.n_shards * n)
        for sh in range(st.n_shards):
            start, nbytes, file_off = (int(v) for v in seg[sh])
            assert file_off == seeds[sh]
            ctx.zarr_shard_decompress_device(2, cb, d_out.data_ptr() + start, nbytes, file_off,
                                             d_tab.data_ptr() + sh * st.table_bytes, n,
                                             d_chunks.data_ptr() + sh * n * cb, cb,
                                             d_st.data_ptr() + 4 * sh * n, s)     # step 5
        _, shard_of, internal_of = aqz.zarr_shard_layout(sdims)
        table = (shard_of.astype(np.uint32) * n + internal_of).astype(np.uint32)
        assert len(set(table.tolist())) == nt and table.max() < st.n_shards * n
        d_table = to_device(table)
        fb = lw * lh * 2
        dst = Dest(3, fb, fb)
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        aqz.chunk_gather_frames_device(np.uint16, lw, lh, shapes[L][1], shapes[L][2],
                                       d_chunks.data_ptr(), cb, st.n_shards * n,
                                       d_table.data_ptr(), nt, base, internal, dst.ptr, fb,
                                       d_bad.data_ptr(), s)                      # step 6
        got = dst.buf[dst.lead:dst.lead + 3 * fb]
        assert torch.equal(got, d_want[L]), f"level {L}: the frames did not come back"
        after.append((d_has, d_st, d_bad, dst, st, shard_of, internal_of, n))
    for L, (d_has, d_st, d_bad, dst, st, shard_of, internal_of, n) in enumerate(after):
        has = from_device(d_has, np.uint8, (-1,))
        skipped = [4] if L == 0 else [6]
        assert np.flatnonzero(has == 0).tolist() == skipped, (L, has)
        status = from_device(d_st, np.uint32, (-1,))
        present = {int(shard_of[c]) * n + int(internal_of[c]) for c in range(len(has)) if has[c]}
        for i, v in enumerate(status):
            assert v == (aqz.FRAME_OK if i in present else aqz.FRAME_ABSENT), (L, i, v)
        assert int(d_bad.cpu()[0]) == 0
        lw, lh, _ = geo[L]
        dst.frames(np.uint16, lh, lw, f"level {L}")  # the guards
        st.close()
    ds.close()
    ctx.close()
