"""GPU: every grow-on-demand scratch buffer of the streaming handle walked
through small -> larger -> smaller on ONE handle, each result against the
oracle.  The rest of the suite mostly grows each scratch once; here every
site sees a first allocation, a second growth and then a call that must reuse
what is there:

  * the on-demand tiling scratch of aqz_ds_take_frame_tiled;
  * the tiled slots of aqz_ds_set_level_tiling, changed while a frame is
    cached and untaken;
  * the chunk-lattice staging of aqz_ds_run_device_batch_chunked;
  * the chain scratch of aqz_ds_run_device_batch_tiled (deep pyramids);
  * the pipeline buffers of aqz_ds_run_host_batch.
"""
import numpy as np
import pytest

from gpu_util import (assert_parity, empty_device, from_device, launch_stream, random_frames,
                      to_device, torch_cuda)
from test_gpu_lattice import POISON, SPACE, TIME, expected_lattices, level_dims
from test_gpu_tiled import halving

pytestmark = pytest.mark.gpu

MEAN = 1


def check_tiled_take(ds, oracle, level_frame, L, tile, ctx):
    got = ds.take_frame_tiled(L, *tile)
    assert got is not None, ctx
    want_t, want_nz = oracle.tile_frame(level_frame, *tile)
    assert_parity(got[0], want_t, f"{ctx}: tiles")
    assert np.array_equal(got[1], want_nz), f"{ctx}: zero scan"


def test_on_demand_tiling_scratch(aqz, oracle):
    """Level 1 (32x24) taken tiled on demand: 768 elements, then 1024 (padded,
    grows), then 875 (ragged, fits what is there)."""
    geo = halving(64, 48, 2)
    ds = aqz.Downsampler(geo, np.uint16, MEAN)
    rng = np.random.default_rng(41)
    sizes = []
    for tile in ((4, 4), (16, 16), (5, 7)):
        frame = random_frames(rng, np.uint16, (48, 64))
        frame[:24, :32] = 0  # zero tiles, so the flags carry both values
        ds.add_frame(frame)
        level = oracle.cascade_2d(frame, 2, MEAN)[0]
        sizes.append(oracle.tile_frame(level, *tile)[0].size)
        check_tiled_take(ds, oracle, level, 1, tile, f"tile {tile}")
        assert ds.take_frame(1) is None
    assert sizes == [768, 1024, 875]
    ds.close()


def test_level_tiling_changed_under_a_cached_frame(aqz, oracle):
    """aqz_ds_set_level_tiling (8,8) -> (16,16) -> off -> (4,4), every change
    made while a frame is cached and untaken: that frame lost its tiles with
    the old slots and must come back right through the on-demand path; the
    frame added after the change is tiled as it is emitted."""
    nl = 3
    geo = halving(64, 48, nl)
    ds = aqz.Downsampler(geo, np.uint16, MEAN)
    rng = np.random.default_rng(43)

    def new_frame():
        f = random_frames(rng, np.uint16, (48, 64))
        f[24:, 32:] = 0
        return f

    cached = None  # the frame every level still holds from before the change
    for step, tiling in enumerate(((8, 8), (16, 16), None, (4, 4))):
        for L in range(1, nl):
            ds.set_level_tiling(L, *(tiling or (0, 0)))
        tile = tiling or (8, 8)  # tiling off: every take is on demand
        if cached is not None:
            ref = oracle.cascade_2d(cached, nl, MEAN)
            for L in range(1, nl):
                check_tiled_take(ds, oracle, ref[L - 1], L, tile,
                                 f"step {step} L{L} frame cached before the change")
        frame = new_frame()
        ds.add_frame(frame)
        ref = oracle.cascade_2d(frame, nl, MEAN)
        for L in range(1, nl):
            check_tiled_take(ds, oracle, ref[L - 1], L, tile, f"step {step} L{L} new frame")
        cached = new_frame()
        ds.add_frame(cached)
    ref = oracle.cascade_2d(cached, nl, MEAN)
    for L in range(1, nl):
        check_tiled_take(ds, oracle, ref[L - 1], L, (4, 4), f"last frame L{L}")
    ds.close()


def test_lattice_staging(aqz, oracle):
    """aqz_ds_run_device_batch_chunked with 2, then 5, then 3 frames on one
    handle and one stream: the offset staging is allocated, grows, then serves
    a smaller batch from the half the first call used.  Poison outside the
    tiles must survive."""
    torch = torch_cuda()
    dims = [(TIME, 0, 3, 1), (SPACE, 384, 128, 1), (SPACE, 520, 96, 1)]
    dtype, bpp = np.uint16, 2
    geo = aqz.level_geometry(aqz.plan_levels(dims))
    assert len(geo) >= 2
    ds = aqz.Downsampler(geo, dtype, MEAN, device=0)
    rng = np.random.default_rng(47)
    stream = launch_stream()
    first = 0
    for n in (2, 5, 3):
        frames = random_frames(rng, dtype, (n, 384, 520))
        cap = [0]
        for L in range(1, len(geo)):
            o, _, lb = oracle.chunk_frame_offsets(level_dims(dims, geo, L), bpp, first, n)
            cap.append((max(o) // lb + 1) * lb)  # the layers this batch touches
        want, offs = expected_lattices(oracle, dims, geo, list(frames), dtype, MEAN, first, cap)
        d_in = to_device(frames)
        bufs = [None] + [empty_device(cap[L]) for L in range(1, len(geo))]
        for b in bufs[1:]:
            b.fill_(POISON)
        lats = [None] + [(bufs[L].data_ptr(), cap[L], dims[-2][2], dims[-1][2], offs[L][1],
                          offs[L][0]) for L in range(1, len(geo))]
        counts = ds.run_device_batch_chunked(d_in.data_ptr(), n, lats, None, stream)
        torch.cuda.synchronize()
        assert counts == [n] * len(geo)
        for L in range(1, len(geo)):
            got = bufs[L].cpu().numpy()
            if not np.array_equal(got, want[L]):
                bad = np.flatnonzero(got != want[L])
                raise AssertionError(f"{n} frames from {first}, level {L}: {bad.size} bytes "
                                     f"differ, first at {bad[0]}")
        first += n
    ds.close()


def test_chain_scratch(aqz, oracle):
    """The 7-level pyramid of test_gpu_lattice.py (two fused runs, the second
    fed from the chain scratch) through the tiled batch with 1, then 3, then 2
    frames on one handle."""
    torch = torch_cuda()
    nl, tr, tc = 7, 16, 16
    geo = halving(1024, 1024, nl)
    ds = aqz.Downsampler(geo, np.uint16, MEAN)
    rng = np.random.default_rng(53)
    n_tiles = [None] + [(-(-h // tr)) * (-(-w // tc)) for w, h, _ in geo[1:]]
    for n in (1, 3, 2):
        frames = random_frames(rng, np.uint16, (n, 1024, 1024))
        frames[0, :512, :512] = 0
        d_in = to_device(frames)
        outs = [None] + [empty_device(n * n_tiles[L] * tr * tc * 2) for L in range(1, nl)]
        for o in outs[1:]:
            o.fill_(POISON)
        counts = ds.run_device_batch_tiled(d_in.data_ptr(), n, [None] + [(tr, tc)] * (nl - 1),
                                           [0] + [o.data_ptr() for o in outs[1:]], None,
                                           launch_stream())
        torch.cuda.synchronize()
        assert ds.last_batch_kind() == 4 and counts == [n] * nl
        for k in range(n):
            ref = oracle.cascade_2d(frames[k], nl, MEAN)
            for L in range(1, nl):
                got = from_device(outs[L], np.uint16, (n, n_tiles[L], tr, tc))
                assert_parity(got[k], oracle.tile_frame(ref[L - 1], tr, tc)[0],
                              f"{n} frames: frame {k} L{L}")
    ds.close()


def test_host_pipeline_buffers(aqz, oracle):
    """aqz_ds_run_host_batch with 2, then 5, then 3 frames: the group is
    min(..., n_frames), so the pipeline buffers are made for 2 frames, grow to
    5 and then serve 3."""
    nl = 3
    geo = halving(64, 48, nl)
    ds = aqz.Downsampler(geo, np.uint16, MEAN)
    rng = np.random.default_rng(59)
    for n in (2, 5, 3):
        frames = random_frames(rng, np.uint16, (n, 48, 64))
        views = [None] + [np.full(n * w * h, 0xA5A5, np.uint16) for w, h, _ in geo[1:]]
        counts = ds.run_host_batch(frames.ctypes.data, n,
                                   [0] + [v.ctypes.data for v in views[1:]])
        assert counts == [n] * nl
        for k in range(n):
            ref = oracle.cascade_2d(frames[k], nl, MEAN)
            for L in range(1, nl):
                w, h, _ = geo[L]
                assert_parity(views[L].reshape(n, h, w)[k], ref[L - 1],
                              f"{n} frames: frame {k} L{L}")
    ds.close()
