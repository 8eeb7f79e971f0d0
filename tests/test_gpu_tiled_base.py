"""GPU: aqz_ds_run_device_batch_tiled_base / _chunked_base — the fused 2-D
cascade writing level 0's chunk tiles as well, from the block every wave has
loaded.  Expectations are the oracle's: oracle.tile_frame of the frame itself
for level 0, of oracle.cascade_2d for the rest, placed by
oracle.chunk_frame_offsets for the lattice.  Every output and flag buffer is
poisoned first; the guard bytes behind each and the offset bytes in front must
still be poison afterwards, and every flag byte 0 or 1."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import tiled_base_cases as tb
from gpu_util import (assert_parity, empty_device, from_device, launch_stream, random_frames,
                      to_device, torch_cuda)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN = 1


def run_case(aqz, oracle, c, method=MEAN, frames=None, with_flags=True, in_off=0, offs=None,
             want=None):
    """One batch through the new call, checked against the oracle; returns
    (Outputs, expectation) for what a test compares further."""
    geo = tb.halving(c["w"], c["h"], c["levels"])
    frames = tb.case_frames(c) if frames is None else frames
    ds = aqz.Downsampler(geo, c["dtype"], method)
    out = tb.Outputs(ds, geo, c["dtype"], c["tiles"], len(frames), with_flags, offs)
    d_in, src = tb.offset_input(frames, in_off)
    counts = out.run(ds, src)
    torch_cuda().cuda.synchronize()
    assert counts == [len(frames)] * len(geo)
    assert ds.last_batch_kind() == 6
    ds.close()
    if want is None:
        want = tb.expected(oracle, frames, c["levels"], method, c["tiles"])
    out.check(want, f"{c['name']} m{method}")
    tail = from_device(d_in, np.uint8, (-1,))[-tb.GUARD:]
    assert (tail == tb.POISON).all()
    return out, want


@pytest.mark.parametrize("name", ["stale", "colfill_base", "colfill_level1", "rowfill"])
def test_named_shapes(aqz, oracle, name):
    """Stale lane columns past the row end and the shifted last row; column
    zero-fill at the base alone and at level 1 alone; row zero-fill with lane
    columns across tile edges."""
    c = tb.CASE[name]
    out, want = run_case(aqz, oracle, c)
    if name == "stale":
        # the padded base's columns 1031..1087 of every row, spelled out
        tiles = want[0][0].reshape(c["n"], 9, 17, 64, 64)
        assert not tiles[:, :, 16, :, 1031 - 1024:].any()
        _, body, _ = out.tile_bytes(0)
        got = body.view(c["dtype"]).reshape(c["n"], 9, 17, 64, 64)
        assert not got[:, :, 16, :, 1031 - 1024:].any() and not got[:, 8, :, 517 - 512:, :].any()


@pytest.mark.parametrize("name", list(tb.SLOT_CASES) + ["slots_f32"])
def test_flag_slots(aqz, oracle, name):
    """Clear-free slots where blocks and tiles nest (two per tile here), one
    cleared byte elsewhere; an all-zero frame, a frame with one nonzero pixel,
    and for f32 a tile of -0.0 (nonzero bytes)."""
    c = tb.CASE[name]
    geo = tb.halving(c["w"], c["h"], c["levels"])
    ds = aqz.Downsampler(geo, c["dtype"], MEAN)
    slots = ds.tiled_base_flag_slots(*c["tiles"][0])
    assert ds.tiled_flag_slots(0, *c["tiles"][0]) == 0
    assert ds.tiled_base_flag_slots(0, 64) == 0 and ds.tiled_base_flag_slots(64, 0) == 0
    ds.close()
    if name in tb.SLOT_CASES:
        assert slots == tb.SLOT_CASES[name]
    frames = tb.case_frames(c)
    frames[2][:] = 0
    if np.dtype(c["dtype"]).kind == "f":
        frames[2][: c["tiles"][0][0], : c["tiles"][0][1]] = -0.0
    out, want = run_case(aqz, oracle, c, frames=frames)
    assert want[0][1][1].sum() == 1  # the one-pixel frame: one base tile with data
    if np.dtype(c["dtype"]).kind == "f":
        assert want[0][1][2].tolist() == [True] + [False] * (out.nt[0] - 1)
    else:
        assert not want[0][1][2].any()
    if name == "slots_rowfill":
        raw, _ = out.flag_bytes(0)
        # tile row 1 (rows 32..63): slot row 1 covers rows 48..63, which no wave owns
        assert not raw.reshape(c["n"], 2, 4, 2)[:, 1, :, 1].any()


@pytest.mark.parametrize("name", ["chain2_small", "chain2_big", "chain3_small", "chain3_big"])
def test_chains(aqz, oracle, name):
    """Two and three fused runs: the base and every level exact; the later
    runs, which read chain scratch, leave level 0 alone."""
    run_case(aqz, oracle, tb.CASE[name])


_SWEEP = {}


def sweep_frames(dtype):
    key = np.dtype(dtype).name
    if key not in _SWEEP:
        rng = np.random.default_rng(zlib.crc32(key.encode()))
        frames = random_frames(rng, dtype, (2, tb.SWEEP["h"], tb.SWEEP["w"]))
        frames[1][:] = 0
        if np.dtype(dtype).kind == "f":
            frames[1][-40:, -40:] = -0.0  # nonzero bytes, zero value
        frames.setflags(write=False)
        _SWEEP[key] = frames
    return _SWEEP[key]


@pytest.mark.parametrize("dtype", tb.DTYPES, ids=lambda d: np.dtype(d).name)
def test_dtypes_and_methods(aqz, oracle, dtype):
    """All four methods over NaN, inf, -0.0 and subnormals, ragged tiles: every
    level bit for bit, and the base tiles the same bytes under every method."""
    c = tb.case("sweep", tb.SWEEP["w"], tb.SWEEP["h"], tb.SWEEP["levels"], dtype,
                [tb.SWEEP["tile"]])
    frames = sweep_frames(dtype)
    base = None
    for method in range(4):
        out, _ = run_case(aqz, oracle, c, method=method, frames=frames)
        body = out.tile_bytes(0)[1].copy()
        flags = out.flag_bytes(0)[0].copy()
        if base is None:
            base = (body, flags)
        assert np.array_equal(body, base[0]) and np.array_equal(flags, base[1]), method


@pytest.mark.parametrize("dtype,w,cols", tb.COLS_CASES,
                         ids=[f"{np.dtype(d).name}_{w}" for d, w, _ in tb.COLS_CASES])
def test_full_and_half_width_tiles(aqz, oracle, dtype, w, cols):
    """4- and 8-byte types at 32 and at 16 bytes a lane (a lane's base store is
    two 16-byte accesses or one), float edge values in the frames; the launch
    log's cols= for these shapes is the next test's."""
    c = tb.case(f"cols{w}", w, tb.SWEEP["h"], tb.SWEEP["levels"], dtype, [tb.SWEEP["tile"]])
    run_case(aqz, oracle, c,
             frames=random_frames(np.random.default_rng(w), dtype, (2, tb.SWEEP["h"], w)))


def test_launch_log_shows_full_and_half_width_tiles():
    """The launch log is switched on by the environment at the library's first
    use: a process of its own, one for the four shapes."""
    env = dict(os.environ, AQZ_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tiled_base_launch_child.py")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(recs) == len(tb.COLS_CASES)
    for rec, (dtype, w, cols) in zip(recs, tb.COLS_CASES):
        log = [l for l in rec["log"] if l.get("family") == "tiled"]
        assert rec["kind"] == 6 and len(log) == 1, rec
        assert (log[0]["cols"], log[0]["base"], log[0]["n_out"]) == (cols, 1, 3), rec
        assert log[0]["dtype"] == np.dtype(dtype).itemsize


@pytest.mark.parametrize("name", ["stale", "rowfill"])
@pytest.mark.parametrize("off", range(1, 8))
def test_element_offsets(aqz, oracle, name, off):
    """Input and every output `off` (+ level) elements into their buffers."""
    c = tb.CASE[name]
    offs = [1 + (off + L - 1) % 7 for L in range(c["levels"])]
    key = ("want", name)
    frames = tb.case_frames(c)
    if key not in _SWEEP:
        _SWEEP[key] = tb.expected(oracle, frames, c["levels"], MEAN, c["tiles"])
    run_case(aqz, oracle, c, frames=frames, in_off=off, offs=offs, want=_SWEEP[key])


@pytest.mark.parametrize("name", ["stale", "rowfill", "chain2_big"])
def test_levels_are_those_of_the_call_without_the_base(aqz, oracle, name):
    c = tb.CASE[name]
    geo = tb.halving(c["w"], c["h"], c["levels"])
    frames = tb.case_frames(c)
    d_in, src = tb.offset_input(frames)
    got = {}
    for base in (True, False):
        ds = aqz.Downsampler(geo, c["dtype"], MEAN)
        out = tb.Outputs(ds, geo, c["dtype"], c["tiles"], len(frames), base=base)
        counts = out.run(ds, src)
        torch_cuda().cuda.synchronize()
        assert ds.last_batch_kind() == (6 if base else 4)
        got[base] = (out, counts)
        ds.close()
    assert got[True][1:] == got[False][1:]
    for L in range(1, c["levels"]):
        assert np.array_equal(got[True][0].tile_bytes(L)[1], got[False][0].tile_bytes(L)[1]), L
        assert np.array_equal(got[True][0].flag_bytes(L)[0], got[False][0].flag_bytes(L)[0]), L


# ---- lattice ------------------------------------------------------------------------

LATTICE_GEO = tb.halving(200, 70, 3)
LATTICE_SHAPES = [(3, 32, 48), (3, 16, 40), (3, 8, 16)]  # ragged in X and Y at every level


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32],
                         ids=lambda d: np.dtype(d).name)
def test_lattice(aqz, oracle, dtype):
    """T/Y/X with 3 frames a chunk: frames 2..6 start inside a chunk and span
    three layers; level 0's offsets come from its own dimensions."""
    rng = np.random.default_rng(np.dtype(dtype).itemsize)
    frames = random_frames(rng, dtype, (5, 70, 200))
    ds = aqz.Downsampler(LATTICE_GEO, dtype, MEAN)
    lat = tb.Lattice(oracle, ds, LATTICE_GEO, LATTICE_SHAPES, dtype, MEAN, frames, first=2,
                     in_off=3)
    bpp = np.dtype(dtype).itemsize
    for L in range(3):
        assert lat.want[L][1] == aqz.chunk_frame_offsets(
            tb.chunk_dims(LATTICE_GEO, L, LATTICE_SHAPES[L]), bpp, 2, 5)[0]
        assert lat.want[L][1][1] // lat.want[L][3] == 1 and lat.want[L][1][4] // lat.want[L][3] == 2
    assert lat.run(ds, launch_stream()) == [5, 5, 5]
    torch_cuda().cuda.synchronize()
    assert ds.last_batch_kind() == 6
    lat.check(np.dtype(dtype).name)
    # the completed middle layer: every level-0 chunk is one contiguous span
    # holding frames 3, 4, 5 of one tile
    buf, offs, cb, lb, _ = lat.want[0]
    got = from_device(lat.bufs[0], np.uint8, (-1,))
    tiles = lat.want_tiles[0][0]
    for t in range(lat.nt[0]):
        chunk = got[lb + t * cb: lb + (t + 1) * cb]
        want = np.stack([tiles[k][t] for k in (1, 2, 3)])
        assert np.array_equal(chunk, want.view(np.uint8).reshape(-1)), t
    ds.close()


def test_lattice_refusals_leave_everything_poisoned(aqz, oracle):
    frames = random_frames(np.random.default_rng(5), np.uint16, (5, 70, 200))
    ds = aqz.Downsampler(LATTICE_GEO, np.uint16, MEAN)
    lat = tb.Lattice(oracle, ds, LATTICE_GEO, LATTICE_SHAPES, np.uint16, MEAN, frames, first=2)
    cap, cb, offs = lat.want[0][4], lat.want[0][2], lat.want[0][1]
    tile_bytes = 32 * 48 * 2
    bad = {
        "an offset that leaves the buffer": {"offs": offs[:4] + [cap - tile_bytes + 2]},
        "an offset past the buffer": {"offs": offs[:4] + [cap + 2]},
        "a misaligned offset": {"offs": [offs[0] + 1] + offs[1:]},
        "a misaligned stride": {"stride": cb + 1},
        "a stride below one tile": {"stride": tile_bytes - 2},
        "a null lattice buffer": {"base": 0},
        "a zero tile side": {"tr": 0},
    }
    for what, change in bad.items():
        with pytest.raises(aqz.AqzError, match="level 0") as e:
            lat.run(ds, launch_stream(), L0=change)
        assert e.value.status == 1, what
        torch_cuda().cuda.synchronize()
        assert lat.still_poison(), what
    # ... and the same call with the arguments as they should be runs
    assert lat.run(ds, launch_stream()) == [5, 5, 5]
    lat.check("after the refusals")
    ds.close()


# ---- refusals ---------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(aqz, oracle):
    c = tb.CASE["rowfill"]
    geo = tb.halving(c["w"], c["h"], c["levels"])
    frames = tb.case_frames(c)
    d_in, src = tb.offset_input(frames)
    ds = aqz.Downsampler(geo, c["dtype"], MEAN)
    out = tb.Outputs(ds, geo, c["dtype"], c["tiles"], c["n"])

    def refused(handle, tiles, ptrs, what, n=c["n"], match="level 0"):
        with pytest.raises(aqz.AqzError, match=match) as e:
            handle.run_device_batch_tiled_base(src, n, tiles, ptrs,
                                               out.flag_ptrs()[: len(tiles)], launch_stream())
        assert e.value.status == 1, what
        torch_cuda().cuda.synchronize()
        assert out.still_poison(), what

    ptrs = out.out_ptrs()
    refused(ds, c["tiles"], [0] + ptrs[1:], "null base output")
    refused(ds, [(0, 60)] + c["tiles"][1:], ptrs, "zero base tile rows")
    refused(ds, [(48, 0)] + c["tiles"][1:], ptrs, "zero base tile columns")
    refused(ds, [None] + c["tiles"][1:], ptrs, "no base tile shape")
    refused(ds, c["tiles"], ptrs, "no frames", n=0)
    ds.set_input_transpose(True)
    refused(ds, c["tiles"], ptrs, "input transposition")
    ds.set_input_transpose(False)
    ds.close()
    vol = aqz.Downsampler([(640, 40, 4), (320, 20, 2), (160, 10, 1)], c["dtype"], MEAN)
    refused(vol, c["tiles"], ptrs, "a volume pyramid")
    vol.close()
    one = aqz.Downsampler(geo[:1], c["dtype"], MEAN)
    assert one.tiled_base_flag_slots(48, 60) == 0
    refused(one, c["tiles"][:1], ptrs[:1], "a one-level handle")
    one.close()
    # u16 frames of 3 px: below the half-width tile's 8-byte load (4 px; 7 px would run)
    narrow = aqz.Downsampler(tb.halving(3, 40, 2), np.uint16, MEAN)
    refused(narrow, c["tiles"][:2], ptrs[:2], "narrower than one vector load")
    narrow.close()
    # a later run refused: u8 100 px, six levels, level 4 (7 px) feeds the second
    # run and is below its 8-byte load; nothing of the first run may be written
    geo6 = tb.halving(100, 40, 6)
    deep = aqz.Downsampler(geo6, np.uint8, MEAN)
    out6 = tb.Outputs(deep, geo6, np.uint8, [(8, 16)] * 6, 2)
    d6, src6 = tb.offset_input(np.ones((2, 40, 100), np.uint8))
    with pytest.raises(aqz.AqzError, match="level 4 is narrower.*level 0 is not written") as e:
        out6.run(deep, src6)
    assert e.value.status == 1
    torch_cuda().cuda.synchronize()
    assert out6.still_poison()
    deep.close()


# ---- seeded fuzz --------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(tb.N_FUZZ_TILED))
def test_fuzz_tiled(aqz, oracle, i):
    c = tb.fuzz_tiled_params(i)
    run_case(aqz, oracle, c, method=c["method"], frames=tb.fuzz_frames(c),
             with_flags=c["flags"], in_off=c["in_off"], offs=c["out_off"])


@pytest.mark.parametrize("i", range(tb.N_FUZZ_CHUNKED))
def test_fuzz_chunked(aqz, oracle, i):
    c = tb.fuzz_chunked_params(i)
    ds = aqz.Downsampler(c["geo"], c["dtype"], c["method"])
    lat = tb.Lattice(oracle, ds, c["geo"], c["shapes"], c["dtype"], c["method"],
                     tb.fuzz_frames(c), c["first"], c["flags"], c["in_off"])
    assert lat.run(ds, launch_stream()) == [c["n"]] * c["levels"]
    torch_cuda().cuda.synchronize()
    assert ds.last_batch_kind() == 6
    ds.close()
    lat.check(c["name"])


# ---- shard glue ---------------------------------------------------------------------------

def test_base_flags_feed_the_shard_call(aqz, oracle):
    """u16 256 x 256, 64 x 64 base tiles, 8 frames: the base flags with the
    reported slot count through aqz_zarr_shard_chunk_has_data_device; chunk j
    has data iff any frame's tile j does (every frame in chunk layer 0)."""
    c = tb.case("shard", 256, 256, 3, np.uint16, [(64, 64), (32, 32)], 8)
    frames = tb.case_frames(c)
    frames[2:, :64, 64:128] = 0  # tile 1: data in no frame but 0 and 1 ...
    frames[:2, :64, 64:128] = 0  # ... nor there
    geo = tb.halving(256, 256, 3)
    ds = aqz.Downsampler(geo, np.uint16, MEAN)
    out = tb.Outputs(ds, geo, np.uint16, c["tiles"], 8)
    d_in, src = tb.offset_input(frames)
    out.run(ds, src)
    want = tb.expected(oracle, frames, 3, MEAN, c["tiles"])
    out.check(want, "shard")
    has = empty_device(16 + tb.GUARD)
    has.fill_(tb.POISON)
    has[:16] = 0  # the caller clears has_data at the layer's start
    aqz.zarr_shard_chunk_has_data_device(out.flags[0].data_ptr(), 8, 16, out.slots[0], [0] * 8,
                                         has.data_ptr(), launch_stream())
    got = from_device(has, np.uint8, (-1,))
    assert (got[16:] == tb.POISON).all()
    assert np.array_equal(got[:16].astype(bool), want[0][1].any(axis=0))
    assert not got[1] and got[:16].sum() == 15
    ds.close()


# ---- past 4 GiB ---------------------------------------------------------------------------

def test_past_4_gib(aqz, oracle):
    """u8 1024 x 64, 3 levels, base tile 32 x 256 (no overhang), 65,538 frames:
    the input and level 0's tiles pass 2^32 bytes.  Frame k is base + k mod 251
    (251 the largest prime under 255 - 4; 65,536 mod 251 = 25, so a 32-bit
    truncated frame offset finds another tag); every frame of every level is
    compared on the device against one oracle run shifted by its tag."""
    import large_batch as lb
    torch = torch_cuda()
    w, h, n = 1024, 64, 65538
    tiles = [(32, 256), (16, 128), (8, 64)]
    geo = tb.halving(w, h, 3)
    M = lb.modulus(np.uint8)
    assert M == 251 and 65536 % M == 25 and n * w * h > 1 << 32
    base = np.random.default_rng(13).integers(0, lb.BASE_MAX["uint8"] + 1, (h, w), dtype=np.uint8)
    tags = (torch.arange(n, device="cuda", dtype=torch.int64) % M).to(torch.uint8)
    raw = torch.empty(n * w * h, dtype=torch.uint8, device="cuda")
    torch.add(torch.from_numpy(base).to("cuda").view(1, h, w), tags.view(-1, 1, 1),
              out=raw.view(n, h, w))
    want = tb.expected(oracle, base[None], 3, MEAN, tiles)
    ds = aqz.Downsampler(geo, np.uint8, MEAN)
    nbytes = [n * (geo[L][0] * geo[L][1]) for L in range(3)]  # no overhang: the level's bytes
    outs = [lb.poisoned(torch, b) for b in nbytes]
    counts = ds.run_device_batch_tiled_base(raw.data_ptr(), n, tiles, [o.data_ptr() for o in outs],
                                            None, launch_stream())
    torch.cuda.synchronize()
    assert counts == [n] * 3 and ds.last_batch_kind() == 6
    ds.close()
    for L in range(3):
        assert bool((outs[L][nbytes[L]:] == lb.POISON).all()), f"L{L}: guard bytes written"
        want0 = torch.from_numpy(want[L][0][0].copy()).to("cuda")
        got = outs[L][: nbytes[L]].view(n, *want0.shape)
        lb.compare_frames(torch, got, want0, None, tags, 1, f"past 4 GiB level {L}")
