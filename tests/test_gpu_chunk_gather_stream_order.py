"""GPU: aqz_chunk_gather_frames_device and aqz_untile_frame_device between
pending work on the caller's stream (tests/stream_order.py, imported as it
is).  The chunks and the slot table arrive on the stream, the frames are read
on it right behind the call, and the call must return while the stall runs:
it owns no scratch, so this holds on its very first use as well.
"""
import numpy as np
import pytest

import chunk_gather_cases as cg
from gpu_util import torch_cuda
from stream_order import Sandwich

pytestmark = pytest.mark.gpu

W, H, TILE, DTYPE = 1031, 517, (128, 250), np.float32   # straddling vectors, a ragged last tile
FB = W * H * 4


def source(oracle, seed, n=5, first=1):
    frames = cg.random_bytes_frames(np.random.default_rng(seed), DTYPE, (n, H, W)).copy()
    frames.view(np.uint8)[frames.view(np.uint8) == 0] = 1
    dims = cg.tyx(W, H, TILE, 2)
    n_chunks = cg.frame_places(oracle, dims, 4, first, n)[3]
    rng = np.random.default_rng(seed + 1)
    table = rng.permutation(n_chunks + 3)[:n_chunks].astype(np.uint32)
    table[int(rng.integers(0, 15))] = cg.ABSENT  # a chunk of the first frame
    return cg.Source(oracle, dims, frames, first, table, n_chunks + 3)


def gather(aqz, src, d_chunks, d_table, d_frames, d_bad, stream):
    aqz.chunk_gather_frames_device(DTYPE, W, H, TILE[0], TILE[1], d_chunks.data_ptr(), src.stride,
                                   src.n_slots, d_table.data_ptr(), src.n_chunks, src.base,
                                   src.internal, d_frames.data_ptr(), FB, d_bad.data_ptr(), stream)


def warm_the_library(aqz):
    """Another kernel of the library, so that loading its code is not what the
    first gather of a process waits for."""
    torch = torch_cuda()
    a = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    b, nz = torch.zeros_like(a), torch.zeros(16, dtype=torch.int32, device="cuda")
    aqz.tile_frame_device(np.uint8, a.data_ptr(), 64, 64, 16, 16, b.data_ptr(), nz.data_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("first_use", [True, False], ids=["first_use", "second_use"])
def test_gather_does_not_wait(aqz, oracle, first_use):
    """first_use: the unstalled run makes no call at all, so the stalled call
    is the first this rig's buffers ever see — there is no scratch a dry run
    could have grown."""
    warm_the_library(aqz)
    src = source(oracle, 31)
    sw = Sandwich(f"chunk_gather_frames_device first_use={first_use}")
    d_chunks = sw.input(src.chunks)
    d_table = sw.input(src.table)
    want = src.expected()
    assert not np.array_equal(want, src.frames) and src.bad() == 0
    skipped = first_use

    def frames_or_poison(got):  # the dry run of first_use makes no call
        if sw.phase == "dry" and skipped:
            assert (got == 0xA5).all()
        else:
            assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint8).reshape(-1))

    d_frames = sw.output(len(want) * FB, frames_or_poison, name="frames")
    d_bad = sw.output(4, lambda got: None if (sw.phase == "dry" and skipped) else
                      np.testing.assert_array_equal(got, [0xA5] * 4), name="bad_slot")

    def call(sw):
        if sw.phase == "dry" and skipped:
            return
        gather(aqz, src, d_chunks, d_table, d_frames, d_bad, sw.hip_stream)

    sw.run(call)


def test_bad_slot_is_written_in_stream_order(aqz, oracle):
    src = source(oracle, 47)
    table = src.table.copy()
    table[3 if table[3] != cg.ABSENT else 4] = src.n_slots + 9
    src = cg.Source(oracle, src.dims, src.frames, src.first, table, src.n_slots)
    assert src.bad() == 1
    sw = Sandwich("chunk_gather_frames_device bad slot")
    d_chunks, d_table = sw.input(src.chunks), sw.input(src.table)
    d_frames = sw.output(len(src.frames) * FB, src.expected(), name="frames")
    d_bad = sw.output(4, np.array([1], np.uint32), name="bad_slot")
    sw.run(lambda sw: gather(aqz, src, d_chunks, d_table, d_frames, d_bad, sw.hip_stream))


def test_untile_does_not_wait(aqz, oracle):
    warm_the_library(aqz)
    frame = cg.random_bytes_frames(np.random.default_rng(2), DTYPE, (1, H, W))
    src = cg.Source(oracle, cg.tyx(W, H, TILE), frame, 0)
    sw = Sandwich("untile_frame_device")
    d_tiles = sw.input(src.chunks)
    d_frame = sw.output(FB, frame, name="frame")
    sw.run(lambda sw: aqz.untile_frame_device(DTYPE, d_tiles.data_ptr(), W, H, TILE[0], TILE[1],
                                              d_frame.data_ptr(), sw.hip_stream))


def test_two_gathers_back_to_back(aqz, oracle):
    """The second gather reads the lattice after a copy, queued between the
    two, has replaced what the first one read: each must see its own."""
    torch = torch_cuda()
    a, b = source(oracle, 5), source(oracle, 6)
    b = cg.Source(oracle, a.dims, b.frames, a.first, a.table, a.n_slots)
    assert a.chunks.shape == b.chunks.shape and not np.array_equal(a.frames, b.frames)
    sw = Sandwich("two gathers on one stream")
    d_chunks, d_table = sw.input(a.chunks), sw.input(a.table)
    second = torch.from_numpy(b.chunks.reshape(-1).copy()).to("cuda")
    sw.keep.append(second)
    d_a = sw.output(len(a.frames) * FB, a.expected(), name="first frames")
    d_b = sw.output(len(b.frames) * FB, b.expected(), name="second frames")
    d_bad = sw.output(4, np.full(4, 0xA5, np.uint8), name="bad_slot")

    def call(sw):
        gather(aqz, a, d_chunks, d_table, d_a, d_bad, sw.hip_stream)
        with torch.cuda.stream(sw.stream):
            d_chunks.copy_(second, non_blocking=True)
        gather(aqz, b, d_chunks, d_table, d_b, d_bad, sw.hip_stream)

    sw.run(call)
