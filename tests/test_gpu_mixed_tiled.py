"""GPU: aqz_ds_run_device_mixed_tiled — mixed 3-D pyramids (levels that halve
XY and Z, XY alone or Z alone) written as chunk tiles by a chain of fused runs
on the caller's stream (aqz_ds_last_batch_kind 8): the tiled volume kernel,
the tiled cascade and the tiled Z run.

Expected tiles are oracle.tile_frame of oracle.OracleDownsampler's levels for
the same frames, bit for bit (floats with their NaN payloads); the fixed
shapes are also held, on the device, to the same handle type's kind-7
row-major output tiled plane by plane with aqz_tile_frame_device.  Every batch
runs into poisoned tile and flag buffers with 64 guard bytes on both sides;
every byte is compared and every flag byte is exactly 0 or 1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mixed_batch_cases as mc
import mixed_tiled_cases as tc
from gpu_util import (empty_device, from_device, launch_stream, random_frames, to_device,
                      torch_cuda)
from test_gpu_float_classes import edge_stack
from test_gpu_parity import BATCH_GEOMETRIES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WANT = {}


def name_of(dtype):
    return np.dtype(dtype).name


def fixed_levels(oracle, name, dtype=None, method=mc.MEAN):
    """(geo, n, dtype, frames, oracle levels) of a fixed shape: one oracle run
    per (shape, dtype, method), shared and left unchanged."""
    geo, n, dt, _ = mc.FIXED[name]
    dtype = dt if dtype is None else dtype
    key = (name, name_of(dtype), method)
    if key not in _WANT:
        frames = mc.fixed_frames(name, dtype)
        want = mc.oracle_levels(oracle, geo, dtype, method, frames)
        for a in [frames] + want[1:]:
            a.setflags(write=False)
        _WANT[key] = (frames, want)
    return (geo, n, dtype) + _WANT[key]


def slots_of(ds, geo, tiles):
    return [None] + [ds.mixed_flag_slots(L, *tiles[L]) for L in range(1, len(geo))]


def run_checked(aqz, oracle, geo, dtype, method, frames, levels, tiles, ctx, offs=None,
                with_flags=True):
    """One batch on a fresh handle into poisoned buffers: kind 8, counts, every
    byte of tiles and flags.  Returns the tiles read back."""
    n = len(frames)
    want = tc.expected_tiled(oracle, levels, tiles)
    ds = aqz.Downsampler(geo, dtype, method)
    try:
        slots = slots_of(ds, geo, tiles)
        assert all(s >= 1 for s in slots[1:]), f"{ctx}: slots {slots}"
        out = tc.Outputs(geo, dtype, tiles, n, slots, with_flags, offs)
        d_in, src = tc.device_input(frames, offs[0] if offs else 0)
        counts = out.run(ds, src)
        torch_cuda().cuda.synchronize()
        assert ds.last_batch_kind() == 8, f"{ctx}: kind {ds.last_batch_kind()}"
    finally:
        ds.close()
    assert counts == mc.emitted(geo, n), f"{ctx}: counts {counts}"
    assert (from_device(d_in, np.uint8, (-1,))[:tc.GUARD] == tc.POISON).all()
    return out.check(want, ctx)


@pytest.mark.parametrize("name,spec", tc.FIXED_CASES, ids=tc.FIXED_IDS)
def test_fixed_shapes(aqz, oracle, name, spec):
    geo, n, dtype, frames, levels = fixed_levels(oracle, name)
    tiles = tc.tiles_for(geo, spec)
    got = run_checked(aqz, oracle, geo, dtype, mc.MEAN, frames, levels, tiles, f"{name} {spec}")
    # the same handle type's kind-7 row-major output, tiled plane by plane on
    # the device with aqz_tile_frame_device, holds the same bytes
    counts = mc.emitted(geo, n)
    b = mc.Batch(geo, dtype, frames, counts)
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        assert b.run(ds) == counts and ds.last_batch_kind() == 7
    finally:
        ds.close()
    bpp = np.dtype(dtype).itemsize
    stream = launch_stream()
    for L in range(1, len(geo)):
        w, h, _ = geo[L]
        tr, tcol = tiles[L]
        nt = tc.n_tiles(geo, L, tiles[L])
        d_t = empty_device(counts[L] * nt * tr * tcol * bpp)
        d_nz = empty_device(counts[L] * nt * 4)
        for k in range(counts[L]):
            aqz.tile_frame_device(dtype, b.ptrs()[L] + k * w * h * bpp, w, h, tr, tcol,
                                  d_t.data_ptr() + k * nt * tr * tcol * bpp,
                                  d_nz.data_ptr() + k * nt * 4, stream)
        two_pass = from_device(d_t, np.dtype(dtype), (counts[L], nt, tr, tcol))
        assert two_pass.tobytes() == got[L].tobytes(), f"{name} {spec} L{L}: tile pass differs"


@pytest.mark.parametrize("method", mc.METHODS)
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=name_of)
@pytest.mark.parametrize("name", mc.SWEEP_SHAPES)
def test_every_dtype_and_method(aqz, oracle, name, dtype, method):
    geo, n, dtype, frames, levels = fixed_levels(oracle, name, dtype, method)
    tiles = tc.tiles_for(geo, tc.FIXED_TILES[name][0])
    run_checked(aqz, oracle, geo, dtype, method, frames, levels, tiles,
                f"{name} {name_of(dtype)} m{method}")


@pytest.mark.parametrize("off", range(1, 8))
@pytest.mark.parametrize("name", mc.OFFSET_SHAPES)
def test_element_offsets(aqz, oracle, name, off):
    """The input `off` elements off its buffer's start, every tile output at
    an offset of its own (1-7 elements, in turn)."""
    geo, n, dtype, frames, levels = fixed_levels(oracle, name)
    offs = [off] + [1 + (off + L) % 7 for L in range(1, len(geo))]
    tiles = tc.tiles_for(geo, tc.FIXED_TILES[name][-2])
    run_checked(aqz, oracle, geo, dtype, mc.MEAN, frames, levels, tiles,
                f"{name} offsets {offs}", offs=offs)


@pytest.mark.parametrize("method", mc.METHODS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=name_of)
@pytest.mark.parametrize("name", mc.FLOAT_SHAPES)
def test_float_classes(aqz, oracle, name, dtype, method):
    """Stacks built from float_cases: every planted class of every level, the
    tiles bit for bit (gpu_util.assert_parity compares floats as bits, NaN
    payloads included)."""
    geo, n, _, _ = mc.FIXED[name]
    frames = edge_stack(dtype, geo, n)
    levels = mc.oracle_levels(oracle, geo, dtype, method, frames)
    tiles = tc.tiles_for(geo, tc.FIXED_TILES[name][0])
    run_checked(aqz, oracle, geo, dtype, method, frames, levels, tiles,
                f"{name} {name_of(dtype)} m{method}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=name_of)
def test_zero_tiles_by_sign(aqz, oracle, dtype):
    """On the Z levels of volume1_zrun3 under 8 x 8 tiles: a tile of +0.0 has
    flag 0, a tile of -0.0 flag 1 (the scan is on bits), and so has a tile
    whose one nonzero pattern is a single -0.0."""
    geo, n, _, _ = mc.FIXED["volume1_zrun3"]
    frames = np.ones((n, geo[0][1], geo[0][0]), dtype)
    frames[:, 0:16, 0:16] = 0.0           # level-1.. tile (0, 0): +0.0
    frames[:, 0:16, 16:32] = -0.0         # tile (0, 1): -0.0
    frames[:, 16:32, 0:16] = 0.0          # tile (1, 0): +0.0 but for one -0.0
    frames[:, 18:20, 6:8] = -0.0
    tiles = tc.tiles_for(geo, (8, 8))
    for method in (mc.MEAN, mc.MIN):
        levels = mc.oracle_levels(oracle, geo, dtype, method, frames)
        want = tc.expected_tiled(oracle, levels, tiles)
        for L in (2, 3, 4):               # the Z levels: 32 x 24, 4 tiles across
            t, nz = want[L]
            bits = t.view(f"u{np.dtype(dtype).itemsize}")
            assert not nz[:, 0].any() and not bits[:, 0].any()
            assert nz[:, 1].all() and (bits[:, 1] != 0).all()
            assert nz[:, 4].all() and (bits[:, 4] != 0).sum() == len(t), (L, method)
        run_checked(aqz, oracle, geo, dtype, method, frames, levels, tiles,
                    f"zero tiles {name_of(dtype)} m{method}")


def test_decimate_reads_even_planes_only(aqz, oracle):
    """A Decimate stack whose odd planes alone are nonzero: every Z-level
    output is zero and every flag 0."""
    name = "zrun3_zrun2_851"
    geo, n, dtype, _ = mc.FIXED[name]
    frames = np.zeros((n, geo[0][1], geo[0][0]), dtype)
    frames[1::2] = 0xFF
    levels = mc.oracle_levels(oracle, geo, dtype, mc.DECIMATE, frames)
    assert not any(l.any() for l in levels[1:])
    tiles = tc.tiles_for(geo, (8, 5))
    run_checked(aqz, oracle, geo, dtype, mc.DECIMATE, frames, levels, tiles, "odd planes")


@pytest.mark.parametrize("name", ["volume2_cascade2", "xy_xyz_z", "z_then_xy"])
def test_flag_slots(aqz, oracle, name):
    """1 on XYZ and Z levels; on XY levels the tiled cascade's count for the
    level's place in its own run, which the bytes written bear out (run_checked
    sizes the flag buffers by it, guards on both sides)."""
    geo, n, dtype, frames, levels = fixed_levels(oracle, name)
    # 32 x 64 tiles nest in the cascade's wave blocks at 64 x 32 u16 input
    for spec in [tc.FIXED_TILES[name][0], (2, 16), (4, 32)]:
        tiles = tc.tiles_for(geo, spec)
        ds = aqz.Downsampler(geo, dtype, mc.MEAN)
        try:
            slots = slots_of(ds, geo, tiles)
            assert ds.mixed_flag_slots(0, *spec) == 0
            assert ds.mixed_flag_slots(len(geo), *spec) == 0
            assert ds.mixed_flag_slots(1, 0, 8) == 0 and ds.mixed_flag_slots(1, 8, 0) == 0
        finally:
            ds.close()
        for L, cls in enumerate(mc.classes(geo)):
            if cls in ("XYZ", "Z"):
                assert slots[L] == 1, (name, L, slots)
            elif cls == "XY":
                # the same level as level j of a pure-XY pyramid of its run's
                # length has aqz_ds_tiled_flag_slots' value there
                _, first, k = tc.run_of_level(geo, L)
                g2 = [(geo[first - 1][0], geo[first - 1][1], 1)] + \
                     [(geo[l][0], geo[l][1], 1) for l in range(first, first + k)]
                ref = aqz.Downsampler(g2, dtype, mc.MEAN)
                try:
                    assert slots[L] == ref.tiled_flag_slots(L - first + 1, *tiles[L]), (name, L)
                finally:
                    ref.close()
        run_checked(aqz, oracle, geo, dtype, mc.MEAN, frames, levels, tiles, f"{name} {spec}")
    odd = aqz.Downsampler([(64, 32, 3), (64, 32, 1)], np.uint16, mc.MEAN)
    try:
        assert odd.mixed_flag_slots(1, 8, 8) == 0
    finally:
        odd.close()


@pytest.mark.parametrize("name,kind", [("2d_odd", 4), ("3d_fused", 5)])
def test_pure_pyramids(aqz, oracle, name, kind):
    """A pure-XY and a pure-XYZ pyramid are one-class run lists: the new call
    takes them (kind 8) and writes what run_device_batch_tiled /
    run_device_volume_tiled (kinds 4 / 5) write."""
    geo, n, _ = BATCH_GEOMETRIES[name]
    dtype = np.uint16
    frames = random_frames(np.random.default_rng(5), dtype, (n, geo[0][1], geo[0][0]))
    levels = mc.oracle_levels(oracle, geo, dtype, mc.MEAN, frames)
    tiles = tc.tiles_for(geo, (16, 24))
    got = run_checked(aqz, oracle, geo, dtype, mc.MEAN, frames, levels, tiles, name)
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        slots = [None] + [ds.tiled_flag_slots(L, *tiles[L]) if kind == 4 else 1
                          for L in range(1, len(geo))]
        out = tc.Outputs(geo, dtype, tiles, n, slots)
        d_in, src = tc.device_input(frames)
        call = ds.run_device_batch_tiled if kind == 4 else ds.run_device_volume_tiled
        counts = call(src, n, tiles, out.out_ptrs(), out.flag_ptrs(), launch_stream())
        torch_cuda().cuda.synchronize()
        assert ds.last_batch_kind() == kind and counts == mc.emitted(geo, n)
    finally:
        ds.close()
    for L in range(1, len(geo)):
        assert out.tile_bytes(L, name).tobytes() == got[L].tobytes(), f"{name} L{L}"


def refused(aqz, call, match):
    with pytest.raises(aqz.AqzError, match=match) as e:
        call()
    assert e.value.status == 1, e.value


def test_refusals_leave_everything_untouched(aqz, oracle):
    """An odd stack, frames off the multiple, a held plane, a zero tile side,
    a null level, an XY run narrower than one load and transposition: status
    1 with a message naming the level, outputs and flags still poisoned, the
    kind and the counts where they were — the accepted batch that follows on
    the same handle gives the oracle's bytes and counts."""
    name = "volume2_cascade2"
    geo, n, dtype, frames, levels = fixed_levels(oracle, name)
    tiles = tc.tiles_for(geo, (32, 64))
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        out = tc.Outputs(geo, dtype, tiles, n, slots_of(ds, geo, tiles))
        d_in, src = tc.device_input(frames)

        def call(n_frames=n, t=tiles, ptrs=None):
            return lambda: ds.run_device_mixed_tiled(src, n_frames, t, ptrs or out.out_ptrs(),
                                                     out.flag_ptrs(), launch_stream())
        refused(aqz, call(n_frames=6), "multiple of 4")
        refused(aqz, call(n_frames=0), "multiple of 4")
        zero = list(tiles)
        zero[3] = (32, 0)
        refused(aqz, call(t=zero), "level 3")
        null = out.out_ptrs()
        null[2] = 0
        refused(aqz, call(ptrs=null), "level 2")
        ds.set_input_transpose(True)
        refused(aqz, call(), "transposition")
        ds.set_input_transpose(False)
        assert ds.last_batch_kind() == -1
        out.untouched("refused calls")
        assert out.run(ds, src) == mc.emitted(geo, n) and ds.last_batch_kind() == 8
        out.check(tc.expected_tiled(oracle, levels, tiles), "after the refusals")
        out.poison()
        # one add_frame: level 1 holds the earlier plane of its first pair
        ds.add_frame(frames[0])
        refused(aqz, call(), "level 1 holds an earlier plane")
        assert ds.last_batch_kind() == 8
        out.untouched("held plane")
    finally:
        ds.close()
    # an odd stack
    geo, n, _ = BATCH_GEOMETRIES["3d_odd_stack"]
    ds = aqz.Downsampler(geo, np.uint16, mc.MEAN)
    try:
        t = tc.tiles_for(geo, (8, 8))
        o = tc.Outputs(geo, np.uint16, t, n, [None] + [1] * (len(geo) - 1))
        d_in, src = tc.device_input(np.ones((n, geo[0][1], geo[0][0]), np.uint16))
        refused(aqz, lambda: o.run(ds, src), "odd plane count")
        assert ds.last_batch_kind() == -1
        o.untouched("odd stack")
    finally:
        ds.close()
    # an XY run whose source is narrower than any vector load (3 bytes)
    geo = [(3, 8, 4), (3, 8, 2), (2, 4, 2)]
    ds = aqz.Downsampler(geo, np.uint8, mc.MEAN)
    try:
        t = tc.tiles_for(geo, (4, 4))
        o = tc.Outputs(geo, np.uint8, t, 4, [None, 1, 1])
        d_in, src = tc.device_input(np.ones((4, 8, 3), np.uint8))
        refused(aqz, lambda: o.run(ds, src), "level 1 is narrower than one vector load")
        assert ds.last_batch_kind() == -1
        o.untouched("narrow XY run")   # the Z run in front of it was not queued
    finally:
        ds.close()


def test_existing_calls_keep_refusing_mixed_pyramids(aqz, oracle):
    geo, n, dtype, frames, _ = fixed_levels(oracle, "volume2_cascade2")
    tiles = tc.tiles_for(geo, (32, 64))
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        out = tc.Outputs(geo, dtype, tiles, n, [None] + [4] * (len(geo) - 1))
        d_in, src = tc.device_input(frames)
        args = (src, n, tiles, out.out_ptrs(), out.flag_ptrs())
        refused(aqz, lambda: ds.run_device_batch_tiled(*args, launch_stream()), "pure-XY")
        refused(aqz, lambda: ds.run_device_volume_tiled(*args, launch_stream()), "volume pyramids")
        refused(aqz, lambda: ds.run_device_batch_tiled_base(*args, launch_stream()), "pure-XY")
        lats = [None] + [(out.out_ptrs()[L], out.nbytes[L], 32, 64, 32 * 64 * 2,
                          [0] * n) for L in range(1, len(geo))]
        refused(aqz, lambda: ds.run_device_batch_chunked(src, n, lats, None, launch_stream()),
                "pure-XY")
        vlats = [None] + [l[:5] + ([0] * (n >> L),) for L, l in enumerate(lats) if L]
        refused(aqz, lambda: ds.run_device_volume_chunked(src, n, vlats, None, launch_stream()),
                "volume pyramids")
        assert ds.last_batch_kind() == -1
        out.untouched("existing calls")
    finally:
        ds.close()


def test_state_after_a_tiled_mixed_batch(aqz, oracle):
    """A kind-8 batch, one more stack streamed through add_frame / take_frame
    on the same handle, then a second kind-8 batch: the oracle fed the same
    frames in the same order gives every level of all three."""
    name = "volume1_zrun3"
    geo, n, dtype, _ = mc.FIXED[name]
    rng = np.random.default_rng(7)
    first, streamed, second = (random_frames(rng, dtype, (k, geo[0][1], geo[0][0]))
                               for k in (n, geo[0][2], n))
    ref = oracle.OracleDownsampler(geo, dtype, mc.MEAN)
    wants = [mc.oracle_levels(oracle, geo, dtype, mc.MEAN, f, ref=ref)
             for f in (first, streamed, second)]
    tiles = tc.tiles_for(geo, (16, 16))
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        slots = slots_of(ds, geo, tiles)
        a = tc.Outputs(geo, dtype, tiles, n, slots)
        d_a, src_a = tc.device_input(first)
        assert a.run(ds, src_a) == mc.emitted(geo, n) and ds.last_batch_kind() == 8
        a.check(tc.expected_tiled(oracle, wants[0], tiles), "first batch")
        got = [[] for _ in geo]
        for fr in streamed:
            ds.add_frame(fr)
            for L in range(1, len(geo)):
                p = ds.take_frame(L)
                if p is not None:
                    got[L].append(p)
        for L in range(1, len(geo)):
            assert len(got[L]) == len(wants[1][L]), f"streamed L{L}: {len(got[L])} frames"
            mc.assert_parity(np.stack(got[L]), wants[1][L], f"streamed L{L}")
        b = tc.Outputs(geo, dtype, tiles, n, slots)
        d_b, src_b = tc.device_input(second)
        assert b.run(ds, src_b) == mc.emitted(geo, n) and ds.last_batch_kind() == 8
        b.check(tc.expected_tiled(oracle, wants[2], tiles), "second batch")
    finally:
        ds.close()


@pytest.mark.parametrize("i", range(tc.N_FUZZ_TILED))
def test_fuzz(aqz, oracle, i):
    c = tc.fuzz_tiled_case(i)
    geo, dtype, method = c["geo"], c["dtype"], c["method"]
    frames = random_frames(c["rng"], dtype, (c["n"], geo[0][1], geo[0][0]))
    frames[: max(1, c["n"] // 2), :, : max(1, geo[0][0] // 2)] = 0   # zero tiles exist
    levels = mc.oracle_levels(oracle, geo, dtype, method, frames)
    run_checked(aqz, oracle, geo, dtype, method, frames, levels, c["tiles"],
                f"fuzz {i} {geo} x {c['n']} {name_of(dtype)} m{method} tiles {c['tiles'][1:]} "
                f"offs {c['offs']}", offs=c["offs"], with_flags=c["flags"])


def test_launch_log_names_the_runs():
    """In one fresh process with the log on: each fixed shape records the
    families of its runs in order, each zrun_tiled line the planned shape; a
    refused call records no line."""
    env = dict(os.environ, AQZ_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mixed_tiled_launch_child.py")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    family = {"XYZ": "volume_tiled", "XY": "tiled", "Z": "zrun_tiled"}
    for name, spec in tc.FIXED_CASES:
        geo, n, dtype, runs = mc.FIXED[name]
        tiles = tc.tiles_for(geo, spec)
        got = rec[f"{name}-{tc.tiles_id(spec)}"]
        lines = got["log"]
        assert got["kind"] == 8, name
        assert [l["family"] for l in lines] == [family[c] for c, _, _, _ in runs], (name, lines)
        bpp = np.dtype(dtype).itemsize
        for line, (cls, first, k, frames) in zip(lines, runs):
            assert line["n_out"] == k, (name, line)
            if cls != "Z":
                continue
            w, h, _ = geo[first - 1]
            groups, spans, main = mc.zrun_shape(w * h, bpp, k, frames)
            zitems = zbytes = 0
            for j in range(k):
                tr, tcol = tiles[first + j]
                pw, ph = -(-w // tcol) * tcol, -(-h // tr) * tr
                per = 1 << (k - 1 - j)
                zitems += (ph if w < pw else ph - h) * per
                zbytes += (pw * ph - w * h) * bpp * per
            zw = (zbytes * groups >> 17) + 1
            if bpp == 1:
                zw = max(zw, -(-zitems * groups // 32))
            zblocks = (-(-(min(max(zw, 64), 4096) if zitems else 0) // 4) + 7) // 8 * 8
            assert (line["dtype"], line["method"], line["planes"], line["groups"], line["spans"],
                    line["zitems"], line["zwaves"], line["grid"], line["block"]) == \
                (bpp, 1, frames, groups, spans, zitems, zblocks * 4, zblocks + main, 256), \
                (name, line)
    for name in ("refused_odd_stack", "refused_six_frames"):
        assert rec[name] == {"kind": -1, "log": [], "status": 1}, (name, rec[name])
