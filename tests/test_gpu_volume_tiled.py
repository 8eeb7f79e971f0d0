"""GPU parity of aqz_ds_run_device_volume_tiled / _chunked: the fused volume
kernel (levels halving X, Y and Z) writes every emitted plane straight into
chunk-tile order, or into a chunk lattice.

The expected bytes never come from the product: the planes go through
oracle.OracleDownsampler, every emitted plane is tiled by oracle.tile_frame,
and lattice places come from oracle.chunk_frame_offsets.  Outputs and flags
are poisoned with 0xA5 first; every output byte and every flag byte must be
written, and in a lattice every byte no plane owns must keep the poison."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import volume_tiled_cases as vc
from gpu_util import (assert_parity, empty_device, from_device, launch_stream, random_frames,
                      to_device, torch_cuda)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON, GUARD = vc.POISON, vc.GUARD
Outputs, Lattice, offset_input = vc.Outputs, vc.Lattice, vc.offset_input
MEAN = 1


_WANT = {}


def case_setup(oracle, case, method=MEAN):
    """Frames, geometry and the oracle's tiles of a table case: computed once,
    shared, never changed."""
    key = (vc.case_id(case), method)
    if key not in _WANT:
        w, h, planes, levels, dtype, tr, tc, _ = case
        geo = vc.volume_geo(w, h, planes, levels)
        frames = vc.case_frames(case)
        frames.setflags(write=False)
        tiles = [None] + [(tr, tc)] * (levels - 1)
        lv = vc.oracle_planes(oracle, geo, dtype, method, frames)
        _WANT[key] = (geo, frames, tiles, lv, vc.expected_tiled(oracle, lv, tiles))
    return _WANT[key]


@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_volume_tiled_matches_oracle(aqz, oracle, case):
    dtype = case[4]
    geo, frames, tiles, _, want = case_setup(oracle, case)
    n = len(frames)
    for L in range(1, len(geo)):
        nz = want[L][1]
        assert nz.any(), f"L{L}: no nonzero tile"
        if -(-geo[L][0] // tiles[L][1]) > 1:  # more than one tile column
            assert not nz.all(), f"L{L}: no zero tile"
    ds = aqz.Downsampler(geo, dtype, MEAN)
    out = Outputs(geo, dtype, tiles, n)
    counts = out.run(ds, to_device(frames))
    torch_cuda().cuda.synchronize()
    assert ds.last_batch_kind() == 5
    assert counts == [n >> L for L in range(len(geo))]
    out.check(want, vc.case_id(case))
    ds.close()


def run_case(aqz, oracle, case, method, in_off=0, offs=None):
    """A table case through the call: every tile byte, flag and guard."""
    dtype = case[4]
    geo, frames, tiles, _, want = case_setup(oracle, case, method)
    n = len(frames)
    ds = aqz.Downsampler(geo, dtype, method)
    out = Outputs(geo, dtype, tiles, n, offs=offs)
    d_in, src = offset_input(frames, in_off)
    counts = out.run(ds, src)
    torch_cuda().cuda.synchronize()
    assert ds.last_batch_kind() == 5
    assert counts == [n >> L for L in range(len(geo))]
    out.check(want, f"{vc.case_id(case)} m{method} in+{in_off} out+{offs}")
    raw = from_device(d_in, np.uint8, (-1,))
    assert (raw[-GUARD:] == POISON).all() and (raw[:in_off * frames.dtype.itemsize] == POISON).all()
    ds.close()
    return want


BRANCH_RUNS = [(c, m) for c, methods, _ in vc.BRANCH_CASES for m in methods]


@pytest.mark.parametrize("case,method", BRANCH_RUNS,
                         ids=[f"{vc.case_id(c)}-m{m}" for c, m in BRANCH_RUNS])
def test_volume_tiled_branch_cases(aqz, oracle, case, method):
    """The shapes of volume_tiled_cases.BRANCH_CASES: column zero-fill at one
    level and at both, lane columns across tile edges for 1- and 2-byte types,
    three chained runs, one tile a level, one-pixel tiles.  What each reaches
    is asserted on the CPU (test_volume_tiled_fuzz_cases.py)."""
    want = run_case(aqz, oracle, case, method)
    for L in range(1, case[3]):
        assert want[L][1].any(), f"L{L}: no nonzero tile"


@pytest.mark.parametrize("case", vc.OFFSET_CASES, ids=vc.case_id)
@pytest.mark.parametrize("in_off", [1, 3, 7])
def test_volume_tiled_element_offsets(aqz, oracle, case, in_off):
    """The input `in_off` elements past its allocation and every level's tiles
    at an element offset of its own (1-7): the misaligned load path with its
    last-row shift, and vector stores to odd addresses."""
    offs = [0] + [1 + (in_off + 2 * L) % 7 for L in range(1, case[3])]
    assert len(set(offs[1:])) == len(offs) - 1 and all(1 <= o <= 7 for o in offs[1:])
    run_case(aqz, oracle, case, MEAN, in_off, offs)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16,
                                   np.int32, np.int64, np.float32, np.float64],
                         ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_volume_tiled_dtypes_methods(aqz, oracle, dtype, method):
    """Every method over the signed and float edge values (NaN, +-inf, -0.0,
    subnormals) through interior and edge units of the new instantiations: one
    all-zero plane group, and a -0.0 patch, whose bytes are nonzero, so its
    flag is 1."""
    w, h, levels, tile = 520, 21, 3, (6, 40)
    geo = vc.volume_geo(w, h, 4, levels)
    rng = np.random.default_rng(zlib.crc32(f"{np.dtype(dtype).name}/{method}".encode()))
    frames = random_frames(rng, dtype, (8, h, w))
    frames[4:] = 0
    if np.dtype(dtype).kind == "f":
        frames[4:, -8:, -40:] = -0.0
    tiles = [None] + [tile] * (levels - 1)
    lv = vc.oracle_planes(oracle, geo, dtype, method, frames)
    want = vc.expected_tiled(oracle, lv, tiles)
    if np.dtype(dtype).kind == "f":
        # the patch's planes: value zero everywhere, flags set where the patch lies
        assert want[1][1][2:].any() and not want[1][1][2:].all()
    else:
        assert not want[1][1][2:].any()
    ds = aqz.Downsampler(geo, dtype, method)
    out = Outputs(geo, dtype, tiles, 8)
    out.run(ds, to_device(frames))
    torch_cuda().cuda.synchronize()
    out.check(want, f"{np.dtype(dtype).name} m{method}")
    ds.close()


def test_row_major_batch_tiles_to_the_same_bytes(aqz, oracle):
    """run_device_batch on a fresh handle takes the fused volume path (kind 2);
    its row-major planes, tiled, are the new call's bytes."""
    case = vc.CASES[3]
    dtype = case[4]
    geo, frames, tiles, _, want = case_setup(oracle, case)
    n = len(frames)
    bpp = np.dtype(dtype).itemsize
    d_in = to_device(frames)
    ds = aqz.Downsampler(geo, dtype, MEAN)
    rows = [None] + [empty_device((n >> L) * w * h * bpp) for L, (w, h, _) in enumerate(geo)][1:]
    counts = ds.run_device_batch(d_in.data_ptr(), n, [0] + [r.data_ptr() for r in rows[1:]],
                                 launch_stream())
    assert ds.last_batch_kind() == 2
    assert counts == [n >> L for L in range(len(geo))]
    ds.close()
    ds = aqz.Downsampler(geo, dtype, MEAN)
    out = Outputs(geo, dtype, tiles, n, with_flags=False)
    out.run(ds, d_in)
    for L in range(1, len(geo)):
        w, h, _ = geo[L]
        tr, tc = tiles[L]
        planes = from_device(rows[L], dtype, (n >> L, h, w))
        tiled = np.stack([oracle.tile_frame(p, tr, tc)[0] for p in planes])
        got = from_device(out.outs[L], np.uint8, (-1,))[:tiled.nbytes].view(dtype) \
            .reshape(tiled.shape)
        assert_parity(got, tiled, f"L{L} against the row-major batch")
    out.check(want, "no flags")  # device_tile_nonzero NULL
    ds.close()


def test_launch_log_names_both_families():
    """Both launches record their family= line (the log is switched on by the
    environment at the library's first use: a process of its own)."""
    env = dict(os.environ, AQZ_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "volume_tiled_launch_child.py")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert [l["family"] for l in rec["row_major"]] == ["volume"]
    assert [l["family"] for l in rec["tiled"]] == ["volume_tiled"]
    t = rec["tiled"][0]
    # 520x22x8 f32, tiles 5x25: 3 x 6 units a group, 2 groups; level 1 is 260x11 -> 11 x 3 tiles
    assert (t["units"], t["units_x"], t["units_y"], t["n_out"]) == (36, 3, 6, 2)
    assert (t["ntx1"], t["nty1"], t["pw1"], t["ph1"]) == (11, 3, 275, 15)
    assert rec["kinds"] == [2, 5]


def test_repeat_call_on_another_stream(aqz, oracle):
    """The 5-level case twice on one handle, on two streams: the second call's
    chained runs are ordered behind the first's through chain_done."""
    torch = torch_cuda()
    case = vc.CASES[6]
    dtype = case[4]
    geo, frames, tiles, _, want = case_setup(oracle, case)
    n = len(frames)
    d_in = to_device(frames)
    ds = aqz.Downsampler(geo, dtype, MEAN)
    a = Outputs(geo, dtype, tiles, n)
    b = Outputs(geo, dtype, tiles, n)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a.run(ds, d_in, s1.cuda_stream)
    b.run(ds, d_in, s2.cuda_stream)
    torch.cuda.synchronize()
    a.check(want, "first call")
    b.check(want, "second call")
    assert ds.last_batch_kind() == 5
    ds.close()


# ---- chunk lattice -----------------------------------------------------------

def chunk_frames(seed):
    w, h, _ = vc.CHUNK_GEO[0]
    frames = random_frames(np.random.default_rng(seed), np.uint16, (8, h, w), specials=False)
    frames[:4, : h // 2, : w // 2] = 0
    return frames


def lattices_of(want, bufs):
    lats = [None]
    for L in range(1, len(vc.CHUNK_GEO)):
        _, offs, cb, _, cap = want[L]
        _, cy, cx = vc.CHUNK_SHAPES[L]
        lats.append((bufs[L].data_ptr(), cap, cy, cx, cb, offs))
    return lats


@pytest.mark.parametrize("first", [0, 4], ids=lambda f: f"first{f}")
def test_volume_chunked_places_every_tile(aqz, oracle, first):
    """Level 1 = 4 x 24 x 32 in chunks of 2 x 16 x 16 (ragged in Y, two layers),
    level 2 = 2 x 12 x 16 in chunks of 2 x 8 x 16.  The batch starts at plane 0,
    then at plane 4: level 2's plane 1, the middle of its layer."""
    torch = torch_cuda()
    geo = vc.CHUNK_GEO
    frames = chunk_frames(first + 1)
    lv = vc.oracle_planes(oracle, geo, np.uint16, MEAN, frames)
    want = vc.expected_chunked(oracle, lv, first, np.uint16)
    if first:
        assert want[2][1][0] != 0, "level 2 starts inside its chunk"
    for L in (1, 2):  # aqz_chunk_frame_offsets gives the oracle's places
        o, cb, lb = aqz.chunk_frame_offsets(vc.chunk_dims(L), 2, first >> L, 8 >> L)
        assert (list(o), cb, lb) == (list(want[L][1]), want[L][2], want[L][3])
    if first:  # plane 0 of level 2's first chunk layer belongs to no plane of this batch
        assert (want[2][0][:want[2][1][0]] == POISON).all()
    bufs = [None] + [empty_device(want[L][4]) for L in (1, 2)]
    flags = [None] + [empty_device((8 >> L) * vc.n_tiles(geo, L, vc.CHUNK_SHAPES[L][1:]))
                      for L in (1, 2)]
    for b in bufs[1:] + flags[1:]:
        b.fill_(POISON)
    ds = aqz.Downsampler(geo, np.uint16, MEAN)
    counts = ds.run_device_volume_chunked(to_device(frames).data_ptr(), 8, lattices_of(want, bufs),
                                          [0] + [f.data_ptr() for f in flags[1:]],
                                          launch_stream())
    torch.cuda.synchronize()
    assert counts == [8, 4, 2] and ds.last_batch_kind() == 5
    for L in (1, 2):
        got = bufs[L].cpu().numpy()
        bad = np.flatnonzero(got != want[L][0])
        assert bad.size == 0, f"level {L}: {bad.size} bytes differ, first at {bad[0]}"
        nz = np.stack([oracle.tile_frame(p, *vc.CHUNK_SHAPES[L][1:])[1] for p in lv[L]])
        raw = from_device(flags[L], np.uint8, nz.shape)
        assert np.isin(raw, (0, 1)).all() and np.array_equal(raw.astype(bool), nz), f"L{L} flags"
    ds.close()


# Five levels: runs 1-2 and 3-4 chained through the handle's scratch, level 4's
# offsets read from the staged table by the second run.  Level 1 is 100 x 12
# (ragged in X and Y), level 4 is 13 x 2 under one 2 x 16 tile; a batch that
# starts at plane 16 starts level 4 in the middle of its 2-plane chunk.
DEEP_GEO = vc.volume_geo(200, 24, 16, 5)
DEEP_SHAPES = [None, (2, 8, 32), (2, 4, 16), (1, 2, 8), (2, 2, 16)]


def deep_frames(dtype, seed):
    frames = random_frames(np.random.default_rng(seed), dtype, (32, 24, 200))
    frames[:16, :, :64] = 0  # zero tiles down to level 3
    return frames


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("first", [0, 16], ids=lambda f: f"first{f}")
def test_volume_chunked_chained_runs(aqz, oracle, dtype, first):
    lat = Lattice(oracle, DEEP_GEO, DEEP_SHAPES, dtype, MEAN, deep_frames(dtype, first + 5), first)
    if first:
        assert lat.want[4][1][0] != 0, "level 4 starts inside its chunk"
    for L in range(1, 5):
        nz = np.stack([oracle.tile_frame(p, *DEEP_SHAPES[L][1:])[1] for p in lat.lv[L]])
        assert nz.any() and (L == 4 or not nz.all()), f"L{L}: zero and nonzero tiles"
    ds = aqz.Downsampler(DEEP_GEO, dtype, MEAN)
    counts = lat.run(ds, launch_stream())
    torch_cuda().cuda.synchronize()
    assert counts == [32 >> L for L in range(5)] and ds.last_batch_kind() == 5
    lat.check(oracle, f"{np.dtype(dtype).name} first {first}")
    ds.close()


# chunks three planes deep: batches that start 0, 1 and 2 planes into the last
# level's chunk get three different offset tables
THREE_DEEP = [(vc.CHUNK_GEO, [None, (3, 16, 16), (3, 8, 16)], 8),
              (DEEP_GEO, [None, (3, 8, 32), (3, 4, 16), (3, 2, 8), (3, 2, 16)], 32)]


@pytest.mark.parametrize("geo,shapes,n", THREE_DEEP, ids=["one_run", "chained"])
def test_three_chunked_calls_queued_keep_their_own_offsets(aqz, oracle, geo, shapes, n):
    """Three calls on one stream with nothing between them, each at its own
    place in the stack with its own buffers, queued behind a stall
    (stream_order.stall: a kernel that ends by itself), so that the first two
    batches are certainly still pending when the third call stages its table.
    The offset tables cross through two pinned halves: the third call must not
    overwrite the half a pending batch still has to read (it waits for the
    first, by contract).  Checked by where the bytes landed: a batch that ran
    with another call's table puts its tiles at that call's places.  Every
    lattice buffer has room for the largest of the three capacities, so such
    a batch would still write inside its own buffer."""
    from stream_order import STALL_FLOOR_MS, stall

    torch = torch_cuda()
    w, h, _ = geo[0]
    last = len(geo) - 1
    ds = aqz.Downsampler(geo, np.uint16, MEAN)

    def batch(seed, first, room=None):
        frames = random_frames(np.random.default_rng(seed), np.uint16, (n, h, w), specials=False)
        return Lattice(oracle, geo, shapes, np.uint16, MEAN, frames, first, room=room)

    # an unstalled call first: it grows the handle's scratch and the staging
    # (and takes the first pinned half; the three below take the second, the
    # first, the second)
    warm = batch(39, 0)
    warm.run(ds, launch_stream())
    torch.cuda.synchronize()
    warm.check(oracle, "unstalled call")
    caps = [[batch(40 + i, i << last).want[L][4] for i in range(3)] for L in range(1, len(geo))]
    room = [None] + [max(c) for c in caps]
    lats = [batch(40 + i, i << last, room) for i in range(3)]
    assert len({tuple(b.want[last][1]) for b in lats}) == 3, "three different offset tables"
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    done = stall(s, STALL_FLOOR_MS)
    lats[0].run(ds, s.cuda_stream)
    lats[1].run(ds, s.cuda_stream)
    assert not done.query(), "the stall ended before two calls were queued: nothing was pending"
    lats[2].run(ds, s.cuda_stream)  # may wait for the first batch
    torch.cuda.synchronize()
    assert ds.last_batch_kind() == 5
    for i, b in enumerate(lats):
        b.check(oracle, f"call {i}")
    ds.close()


# ---- refusals ----------------------------------------------------------------

def refused(aqz, call):
    with pytest.raises(aqz.AqzError) as e:
        call()
    assert e.value.status == 1, e.value
    return str(e.value)


def test_refusals_write_nothing(aqz, oracle):
    torch = torch_cuda()
    d_in = empty_device(64 * 48 * 2 * 8)
    out = [None] + [empty_device(1 << 16) for _ in range(2)]
    for o in out[1:]:
        o.fill_(POISON)
    ptrs = [0] + [o.data_ptr() for o in out[1:]]
    tiles = [None, (16, 16), (16, 16)]
    u16 = np.uint16

    def tiled(geo, n, t=tiles, transpose=False):
        ds = aqz.Downsampler(geo, u16, MEAN)
        if transpose:
            ds.set_input_transpose(True)
        try:
            return refused(aqz, lambda: ds.run_device_volume_tiled(
                d_in.data_ptr(), n, t[:len(geo)], ptrs[:len(geo)], None, launch_stream()))
        finally:
            ds.close()

    vol = vc.volume_geo(64, 48, 8, 3)
    assert "level 1" in tiled([(64, 48, 1), (32, 24, 1), (16, 12, 1)], 4)   # pure XY
    assert "level 1" in tiled([(64, 48, 8), (64, 48, 4)], 4)               # Z-only level
    assert "level 1" in tiled([(64, 48, 6), (32, 24, 3), (16, 12, 2)], 4)  # odd planes at level 1
    assert "level 2" in tiled(vol, 6)                                      # not a multiple of 4
    tiled(vol, 0)
    assert "level 2" in tiled(vol, 8, [None, (16, 16), (0, 16)])           # zero tile shape
    tiled(vol, 8, transpose=True)                                          # transposition on
    # lattices: out of the buffer, misaligned, stride below one tile
    frames = chunk_frames(3)
    want = vc.expected_chunked(oracle, vc.oracle_planes(oracle, vc.CHUNK_GEO, u16, MEAN, frames),
                               0, u16)
    bufs = [None] + [empty_device(want[L][4]) for L in (1, 2)]
    for b in bufs[1:]:
        b.fill_(POISON)
    good = lattices_of(want, bufs)
    ds = aqz.Downsampler(vc.CHUNK_GEO, u16, MEAN)
    base, cap, cy, cx, cb, offs = good[2]
    for bad in ((base, cap - 2, cy, cx, cb, offs),                      # short by a pixel
                (base, cap, cy, cx, cb, [offs[0], offs[1] + 1]),       # misaligned offset
                (base, cap, cy, cx, cy * cx * 2 - 2, offs)):           # stride below a tile
        msg = refused(aqz, lambda: ds.run_device_volume_chunked(
            d_in.data_ptr(), 8, [None, good[1], bad], None, launch_stream()))
        assert "level 2" in msg, msg
    ds.close()
    torch.cuda.synchronize()
    for b in out[1:] + bufs[1:]:
        assert bool((b == POISON).all()), "a refused call wrote to an output"
