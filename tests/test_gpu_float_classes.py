"""GPU: the float result classes of tests/float_cases.py, bit for bit, through
every kernel path.

float32 and float64, the four methods, tests/float_cases.py's edge frames
(the sign of a zero, subnormal rounding, overflow from finite operands, sums
whose order matters, first-NaN and default-NaN payloads, zero ties and
signalling NaNs through Min / Max / Decimate; tests/test_float_cases.py shows
on the CPU that the frames reach each of them at every level).  The oracle's
output is compared as uint32 / uint64: bit equality and nothing else.  Device
outputs are filled with 0xA5 first and carry 64 poisoned bytes behind them
(and the offset elements in front), which must still be poison afterwards.  A
mismatch names the level, the element, the class planted there and both bit
patterns.

Paths, at the suite's own smallest shape per scheme (BATCH_GEOMETRIES of
tests/test_gpu_parity.py; float64's schemes there are pinned on the planner
by tests/test_float_cases.py), two frames or one stack each:
* the row-major batch (kind 1), every buffer aligned and again with the input
  and each level at an element offset of 1-7, which turns aligned rows into
  misaligned ones;
* the stream (add_frame / take_frame): two fused runs, and odd widths;
* the chunk-tiled batch with zero-scan flags, one frame holding whole tiles of
  +0.0 (flag 0), whole tiles of -0.0 (flag 1: the scan is byte-wise) and a
  tile whose only nonzero bytes are one -0.0;
* the fused volume kernel (kind 2) and the Z state machine (kind 0, and a
  Z-only stack through add_frame);
* the fused volume kernel writing chunk tiles (kind 5), with the same three
  kinds of zero tile on a plane of level 1 and on one of level 2.
"""
import numpy as np
import pytest

import float_cases as fc
from gpu_util import empty_device, from_device, launch_stream, to_device, torch_cuda
from test_gpu_fuzz import oracle_stream
from test_gpu_parity import BATCH_GEOMETRIES, halving_geometry, run_both, seed_of

pytestmark = pytest.mark.gpu

FLOATS = [np.float32, np.float64]
METHODS = [0, 1, 2, 3]
POISON, PAD = 0xA5, 64

BATCH_2D = ["2d", "2d_generic", "2d_narrow", "2d_oddw_deep", "2d_six", "2d_band_staged",
            "2d_wide_misaligned", "2d_band8_aligned", "2d_band6_edge_rows", "2d_band_segments",
            "2d_complete_8tile", "2d_complete_short_last", "2d_mis_segments"]
VOLUMES = ["3d_fused", "3d_fused_edge", "3d_fused_oddw", "3d_fused_one_level"]
Z_ONLY = [(40, 30, 6), (40, 30, 3), (40, 30, 2)]
STREAMS = [(1000, 600, 6), (37, 1023, 4)]   # (w, h, levels)
# (w, h, levels, tile_rows, tile_cols): test_gpu_tiled's float shapes
TILED = [(520, 301, 4, 64, 96), (1000, 600, 4, 64, 128), (512, 512, 4, 3, 5)]


def _name(dtype):
    return np.dtype(dtype).name


def _cases(names):
    # geometry outermost: float_cases caches the frames of the last few
    return [pytest.param(g, d, m, id=f"{g if isinstance(g, str) else 'x'.join(map(str, g))}-"
                                     f"{_name(d)}-m{m}")
            for g in names for d in FLOATS for m in METHODS]


def edge_stack(dtype, geo, n):
    w, h, planes = geo[0]
    return fc.edge_frames(dtype, n, h, w, len(geo), planes, geometry=geo)


def assert_bits(got, want, dtype, geo, n, method, level, ctx, first=0):
    """Bit equality of one level's frames (n_level, h, w), the level's frames
    from number `first` on; on a mismatch the first differing element, its
    planted class and both patterns."""
    ut = np.dtype(f"u{np.dtype(dtype).itemsize}")
    g, w = np.ascontiguousarray(got).view(ut), np.ascontiguousarray(want).view(ut)
    assert g.shape == w.shape, f"{ctx} level {level}: shape {g.shape} vs {w.shape}"
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    k, y, x = (int(v) for v in bad[0])
    fw, fh, planes = geo[0]
    cls = fc.class_map(dtype, n, fh, fw, len(geo), method, level, planes,
                       geometry=geo)[first + k, y, x]
    raise AssertionError(
        f"{ctx} level {level}: {len(bad)} of {g.size} elements differ in bits; first at frame "
        f"{first + k} element ({y}, {x}), planted class {cls}: got {int(g[k, y, x]):#x}, oracle "
        f"{int(w[k, y, x]):#x}")


def run_batch(aqz, geo, dtype, method, frames, offs, kind, expected):
    """One aqz_ds_run_device_batch into poisoned outputs, `offs[L]` elements
    in front of the input (L = 0) and of level L, PAD bytes behind each."""
    torch = torch_cuda()
    bpp = np.dtype(dtype).itemsize
    n = frames.shape[0]
    raw = np.zeros(offs[0] * bpp + frames.nbytes, dtype=np.uint8)
    raw[offs[0] * bpp:] = frames.view(np.uint8).reshape(-1)
    d_in = to_device(raw)
    sizes = [0] + [len(expected[L]) * gw * gh * bpp for L, (gw, gh, _) in enumerate(geo) if L]
    outs = [None]
    for L in range(1, len(geo)):
        o = empty_device(offs[L] * bpp + sizes[L] + PAD)
        o.fill_(POISON)
        outs.append(o)
    ptrs = [0] + [outs[L].data_ptr() + offs[L] * bpp for L in range(1, len(geo))]
    ds = aqz.Downsampler(geo, dtype, method)
    try:
        counts = ds.run_device_batch(d_in.data_ptr() + offs[0] * bpp, n, ptrs, launch_stream())
        torch.cuda.synchronize()
        assert ds.last_batch_kind() == kind
    finally:
        ds.close()
    got = {}
    for L in range(1, len(geo)):
        gw, gh, _ = geo[L]
        assert counts[L] == len(expected[L]), f"level {L}: {counts[L]} frames"
        raw = from_device(outs[L], np.uint8, (-1,))
        a = offs[L] * bpp
        assert (raw[:a] == POISON).all() and (raw[a + sizes[L]:] == POISON).all(), \
            f"level {L}: bytes outside the output were written"
        got[L] = raw[a:a + sizes[L]].view(dtype).reshape(len(expected[L]), gh, gw)
    return got


def check_batch(aqz, oracle, geo, dtype, method, frames, kind, passes, ctx):
    expected = oracle_stream(oracle, geo, dtype, method, frames)
    for tag, offs in passes:
        got = run_batch(aqz, geo, dtype, method, frames, offs, kind, expected)
        for L in range(1, len(geo)):
            assert_bits(got[L], np.stack(expected[L]), dtype, geo, frames.shape[0], method, L,
                        f"{ctx} {tag}")


@pytest.mark.parametrize("name,dtype,method", _cases(BATCH_2D))
def test_row_major_batch(aqz, oracle, name, dtype, method):
    geo, _, kind = BATCH_GEOMETRIES[name]
    assert kind == 1
    frames = edge_stack(dtype, geo, 2)
    rng = np.random.default_rng(seed_of("float-classes", name, _name(dtype)))
    offs = [int(x) for x in rng.integers(1, 8, len(geo))]
    check_batch(aqz, oracle, geo, dtype, method, frames, 1,
                [("aligned", [0] * len(geo)), ("offset", offs)], f"{name} {_name(dtype)} m{method}")


@pytest.mark.parametrize("name,dtype,method", _cases(VOLUMES))
def test_volume_batch(aqz, oracle, name, dtype, method):
    geo, n, kind = BATCH_GEOMETRIES[name]
    assert kind == 2 and n == geo[0][2]
    check_batch(aqz, oracle, geo, dtype, method, edge_stack(dtype, geo, n), 2,
                [("aligned", [0] * len(geo))], f"{name} {_name(dtype)} m{method}")


@pytest.mark.parametrize("name,dtype,method", _cases(["3d_odd_stack"]))
def test_z_state_machine_batch(aqz, oracle, name, dtype, method):
    geo, _, kind = BATCH_GEOMETRIES[name]
    assert kind == 0
    check_batch(aqz, oracle, geo, dtype, method, edge_stack(dtype, geo, 2 * geo[0][2]), 0,
                [("aligned", [0] * len(geo))], f"{name} {_name(dtype)} m{method}")


def check_stream(aqz, oracle, geo, dtype, method, frames, ctx):
    got, want = run_both(aqz, oracle, geo, dtype, method, frames)
    assert len(got) == len(want) > 0
    seen = {L: 0 for L in range(1, len(geo))}
    for (i, L, a), (_, _, b) in zip(got, want):
        assert_bits(a[None], b[None], dtype, geo, len(frames), method, L,
                    f"{ctx} input frame {i}", first=seen[L])
        seen[L] += 1
    return seen


@pytest.mark.parametrize("shape,dtype,method", _cases(STREAMS))
def test_stream(aqz, oracle, shape, dtype, method):
    w, h, nl = shape
    geo = halving_geometry(w, h, nl)
    seen = check_stream(aqz, oracle, geo, dtype, method, edge_stack(dtype, geo, 2),
                        f"stream {w}x{h} {_name(dtype)} m{method}")
    assert all(v == 2 for v in seen.values())


@pytest.mark.parametrize("dtype", FLOATS, ids=_name)
@pytest.mark.parametrize("method", METHODS)
def test_z_only_stack_stream(aqz, oracle, dtype, method):
    """Z halves alone: the pair reducers on raw operands, signalling NaNs and
    max + max included; the last plane of the odd level passes through."""
    seen = check_stream(aqz, oracle, Z_ONLY, dtype, method, edge_stack(dtype, Z_ONLY, 12),
                        f"z-only {_name(dtype)} m{method}")
    assert seen == {1: 6, 2: 4}


def run_tiled_poisoned(aqz, geo, dtype, method, frames, tr, tc):
    """aqz_ds_run_device_batch_tiled with flags into poisoned tiles and flag
    slots, PAD poisoned bytes behind each: (tiles (n, nt, tr, tc), flags
    (n, nt)) per level."""
    torch = torch_cuda()
    n = len(frames)
    bpp = np.dtype(dtype).itemsize
    d_in = to_device(np.stack(frames))
    ds = aqz.Downsampler(geo, dtype, method)
    outs, flags, dims = [None], [None], [None]
    for L, (w, h, _) in enumerate(geo[1:], 1):
        nt = (-(-h // tr)) * (-(-w // tc))
        slots = ds.tiled_flag_slots(L, tr, tc)
        assert slots >= 1
        outs.append(empty_device(n * nt * tr * tc * bpp + PAD))
        flags.append(empty_device(n * nt * slots + PAD))
        dims.append((nt, slots))
        outs[L].fill_(POISON)
        flags[L].fill_(POISON)
    try:
        counts = ds.run_device_batch_tiled(
            d_in.data_ptr(), n, [None] + [(tr, tc)] * (len(geo) - 1),
            [0] + [o.data_ptr() for o in outs[1:]], [0] + [f.data_ptr() for f in flags[1:]],
            launch_stream())
        torch.cuda.synchronize()
        assert ds.last_batch_kind() == 4
        assert counts == [n] * len(geo)
    finally:
        ds.close()
    got = [None]
    for L in range(1, len(geo)):
        nt, slots = dims[L]
        raw = from_device(outs[L], np.uint8, (-1,))
        fraw = from_device(flags[L], np.uint8, (-1,))
        assert (raw[-PAD:] == POISON).all() and (fraw[-PAD:] == POISON).all(), \
            f"level {L}: bytes behind the output were written"
        fl = fraw[:-PAD].reshape(n, nt, slots)
        assert np.isin(fl, (0, 1)).all(), f"level {L}: flag slot left unwritten"
        got.append((raw[:-PAD].view(dtype).reshape(n, nt, tr, tc), fl.any(axis=-1)))
    return got


def zero_region_frame(frame):
    """The top half +0.0 but for one 2x2 window of -0.0 (one -0.0 output at
    level 1), the bottom left quarter -0.0; the classes stay bottom right."""
    f = np.array(frame)
    h, w = f.shape
    f[: h // 2] = 0.0
    f[h // 2:, : w // 2] = -0.0
    f[2:4, 2:4] = -0.0
    return f


@pytest.mark.parametrize("case,dtype,method", _cases(TILED))
def test_tiled_batch(aqz, oracle, case, dtype, method):
    w, h, nl, tr, tc = case
    geo = halving_geometry(w, h, nl)
    edge = edge_stack(dtype, geo, 2)
    frames = [np.array(edge[0]), zero_region_frame(edge[1])]
    got = run_tiled_poisoned(aqz, geo, dtype, method, frames, tr, tc)
    ut = np.dtype(f"u{np.dtype(dtype).itemsize}")
    ctx = f"tiled {w}x{h} {tr}x{tc} {_name(dtype)} m{method}"
    for k, fr in enumerate(frames):
        ref = oracle.cascade_2d(fr, nl, method)
        for L in range(1, nl):
            want_t, want_nz = oracle.tile_frame(ref[L - 1], tr, tc)
            t, fl = got[L]
            if not np.array_equal(t[k].view(ut), want_t.view(ut)):
                # name the element in frame coordinates: compare untiled too
                bad = np.argwhere(t[k].view(ut) != want_t.view(ut))[0]
                ti, r, c = (int(v) for v in bad)
                ntx = -(-geo[L][0] // tc)
                y, x = ti // ntx * tr + r, ti % ntx * tc + c
                inside = y < geo[L][1] and x < geo[L][0]
                # frame 1 keeps its classes in the bottom right quarter only
                kept = k == 0 or (y << L >= h // 2 and x << L >= w // 2)
                cls = (fc.class_map(dtype, 2, h, w, nl, method, L)[k, y, x]
                       if inside and kept else None)
                raise AssertionError(
                    f"{ctx} level {L} frame {k}: tile {ti} element ({r}, {c}) = frame element "
                    f"({y}, {x}), planted class {cls}: got {int(t[k].view(ut)[ti, r, c]):#x}, "
                    f"oracle {int(want_t.view(ut)[ti, r, c]):#x}")
            assert np.array_equal(fl[k], want_nz), f"{ctx} level {L} frame {k}: zero scan"
            if k == 1 and L == 1:
                # the frame holds what it was built for: tiles of +0.0 alone
                # (flag 0), tiles of -0.0 alone and a tile whose only nonzero
                # bytes are one -0.0 (flag 1)
                bits = want_t.view(ut).reshape(want_t.shape[0], -1)
                nz_bit = ut.type(1 << (8 * ut.itemsize - 1))
                assert (~want_nz).any()
                assert want_nz[0] and (bits[0] != 0).sum() == 1 and bits[0, tc + 1] == nz_bit
                ntx = -(-geo[1][0] // tc)
                last_row_left = (-(-geo[1][1] // tr) - 1) * ntx
                inside = oracle.tile_frame(np.ones_like(ref[0]), tr, tc)[0][last_row_left] != 0
                assert want_nz[last_row_left] and \
                    (want_t.view(ut)[last_row_left][inside] == nz_bit).all()


# ---- the tiled volume call -------------------------------------------------------

# tile rows x columns per geometry: level edges inside tiles (200 / 201 x 61
# gives 100 / 101 x 31 and 50 / 51 x 16), lane columns across tile edges (25),
# and float_cases' zero-region shape on 3d_fused
VOLUME_TILES = {"3d_fused": fc.ZERO_TILE, "3d_fused_edge": (5, 25), "3d_fused_oddw": (16, 48),
                "3d_fused_one_level": (3, 40)}


def run_volume_tiled_poisoned(aqz, geo, dtype, method, frames, tr, tc):
    """aqz_ds_run_device_volume_tiled with flags into poisoned tiles and flag
    bytes, PAD poisoned bytes behind each: (tiles (planes, nt, tr, tc), flags
    (planes, nt)) per level."""
    torch = torch_cuda()
    n = len(frames)
    bpp = np.dtype(dtype).itemsize
    d_in = to_device(frames)
    outs, flags, nts = [None], [None], [None]
    for L, (w, h, _) in enumerate(geo[1:], 1):
        nt = (-(-h // tr)) * (-(-w // tc))
        outs.append(empty_device((n >> L) * nt * tr * tc * bpp + PAD))
        flags.append(empty_device((n >> L) * nt + PAD))
        nts.append(nt)
        outs[L].fill_(POISON)
        flags[L].fill_(POISON)
    ds = aqz.Downsampler(geo, dtype, method)
    try:
        counts = ds.run_device_volume_tiled(
            d_in.data_ptr(), n, [None] + [(tr, tc)] * (len(geo) - 1),
            [0] + [o.data_ptr() for o in outs[1:]], [0] + [f.data_ptr() for f in flags[1:]],
            launch_stream())
        torch.cuda.synchronize()
        assert ds.last_batch_kind() == 5
        assert counts == [n >> L for L in range(len(geo))]
    finally:
        ds.close()
    got = [None]
    for L in range(1, len(geo)):
        raw = from_device(outs[L], np.uint8, (-1,))
        fraw = from_device(flags[L], np.uint8, (-1,))
        assert (raw[-PAD:] == POISON).all() and (fraw[-PAD:] == POISON).all(), \
            f"level {L}: bytes behind the output were written"
        fl = fraw[:-PAD].reshape(n >> L, nts[L])
        assert np.isin(fl, (0, 1)).all(), f"level {L}: a flag byte is neither 0 nor 1"
        got.append((raw[:-PAD].view(dtype).reshape(n >> L, nts[L], tr, tc), fl.astype(bool)))
    return got


def check_volume_tiled(aqz, oracle, geo, dtype, method, frames, tr, tc, ctx, kept=None):
    """Tiles as unsigned integers against the oracle's planes tiled by
    oracle.tile_frame; a mismatch is named untiled, with its planted class
    (`kept(level, y, x)`: whether the element still holds the edge stack's)."""
    n = len(frames)
    w, h, planes = geo[0]
    expected = oracle_stream(oracle, geo, dtype, method, frames)
    got = run_volume_tiled_poisoned(aqz, geo, dtype, method, frames, tr, tc)
    ut = np.dtype(f"u{np.dtype(dtype).itemsize}")
    want = [None]
    for L in range(1, len(geo)):
        assert len(expected[L]) == n >> L
        t = [oracle.tile_frame(p, tr, tc) for p in expected[L]]
        want_t, want_nz = np.stack([a for a, _ in t]), np.stack([b for _, b in t])
        want.append((want_t, want_nz))
        g, fl = got[L]
        if not np.array_equal(g.view(ut), want_t.view(ut)):
            k, ti, r, c = (int(v) for v in np.argwhere(g.view(ut) != want_t.view(ut))[0])
            ntx = -(-geo[L][0] // tc)
            y, x = ti // ntx * tr + r, ti % ntx * tc + c
            inside = y < geo[L][1] and x < geo[L][0]
            cls = (fc.class_map(dtype, n, h, w, len(geo), method, L, planes, geometry=geo)[k, y, x]
                   if inside and (kept is None or kept(L, y, x)) else None)
            raise AssertionError(
                f"{ctx} level {L} plane {k}: tile {ti} element ({r}, {c}) = plane element "
                f"({y}, {x}), planted class {cls}: got {int(g.view(ut)[k, ti, r, c]):#x}, "
                f"oracle {int(want_t.view(ut)[k, ti, r, c]):#x}")
        assert np.array_equal(fl, want_nz), f"{ctx} level {L}: zero scan"
    return want


@pytest.mark.parametrize("name,dtype,method", _cases(VOLUMES))
def test_volume_tiled_batch(aqz, oracle, name, dtype, method):
    geo, n, kind = BATCH_GEOMETRIES[name]
    assert kind == 2 and n == geo[0][2]
    tr, tc = VOLUME_TILES[name]
    check_volume_tiled(aqz, oracle, geo, dtype, method, edge_stack(dtype, geo, n), tr, tc,
                       f"volume tiled {name} {tr}x{tc} {_name(dtype)} m{method}")


@pytest.mark.parametrize("dtype", FLOATS, ids=_name)
def test_volume_tiled_zero_tiles(aqz, oracle, dtype):
    """float_cases.zero_region_stack under Mean: whole tiles of +0.0 (flag 0),
    whole tiles of -0.0 (flag 1) and a tile whose only nonzero bytes are one
    -0.0, on a plane emitted at level 1 and on one emitted at level 2."""
    geo, n, _ = BATCH_GEOMETRIES["3d_fused"]
    w, h, _ = geo[0]
    tr, tc = fc.ZERO_TILE
    frames = fc.zero_region_stack(edge_stack(dtype, geo, n))
    want = check_volume_tiled(
        aqz, oracle, geo, dtype, fc.MEAN, frames, tr, tc, f"volume tiled zero tiles {_name(dtype)}",
        kept=lambda L, y, x: y > h // 2 >> L and x > w // 2 >> L)
    for L in (1, 2):
        fc.check_zero_region_tiles(dtype, L, want[L][0], want[L][1], geo[L][1], geo[L][0])
