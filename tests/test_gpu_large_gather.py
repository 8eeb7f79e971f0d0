"""GPU: aqz_chunk_gather_frames_device past 4 GiB.

u8 frames of 1024 x 1024 from 256 x 256 tiles, T/Y/X with 2 frames a chunk,
ceil(2^32 / frame bytes) + 2 frames: k * frame_stride and slot * chunk_stride
both pass 2^32, so an offset computed in 32 bits lands on another frame or
chunk.  The batch is base + k mod M with tests/large_batch.py's prime M, so
that a frame 2^32 bytes away never holds the same pixels.  Everything divides,
so the lattice is made on the device by torch's own reshape and permute,
independent of the library, and the result is compared there in slabs.
"""
import numpy as np
import pytest

import large_batch as lb
from gpu_util import launch_stream, torch_cuda

pytestmark = pytest.mark.gpu

W = H = 1024
TILE = 256
T_CHUNK = 2
FB = W * H
N = -(-(1 << 32) // FB) + 2          # 4098 frames
LAYERS = N // T_CHUNK
TILES = (H // TILE) * (W // TILE)    # chunks of one layer
CHUNK_BYTES = T_CHUNK * TILE * TILE
N_CHUNKS = LAYERS * TILES
SLAB = 256                           # frames a slab: 256 MiB
GUARD = 64
POISON = 0x5A


def base_frame():
    rng = np.random.default_rng(4098)
    return rng.integers(0, lb.BASE_MAX["uint8"], (H, W), endpoint=True).astype(np.uint8)


def frames_slab(torch, d_base, k0, k1):
    m = lb.modulus(np.uint8)
    tags = (torch.arange(k0, k1, device="cuda", dtype=torch.int64) % m).to(torch.uint8)
    return d_base[None] + tags[:, None, None]   # at most 4 + 250: no wrap


@pytest.fixture(scope="module")
def lattice():
    """(lattice [N_CHUNKS, CHUNK_BYTES], base frame), on the device: chunk
    (layer, ty, tx) holds, for each of its 2 frames, tile (ty, tx) row-major."""
    torch = torch_cuda()
    assert N % T_CHUNK == 0 and N * FB > 1 << 32 and N_CHUNKS * CHUNK_BYTES > 1 << 32
    assert lb.modulus(np.uint8) == 251 and FB % lb.modulus(np.uint8) != 0
    d_base = torch.from_numpy(base_frame()).to("cuda")
    lat = torch.empty((LAYERS, H // TILE, W // TILE, T_CHUNK, TILE, TILE), dtype=torch.uint8,
                      device="cuda")
    for k0 in range(0, N, SLAB):
        k1 = min(N, k0 + SLAB)
        f = frames_slab(torch, d_base, k0, k1)
        f = f.reshape((k1 - k0) // T_CHUNK, T_CHUNK, H // TILE, TILE, W // TILE, TILE)
        lat[k0 // T_CHUNK:k1 // T_CHUNK] = f.permute(0, 2, 4, 1, 3, 5)
    torch.cuda.synchronize()
    yield lat.reshape(N_CHUNKS, CHUNK_BYTES), d_base
    del lat
    torch.cuda.empty_cache()


@pytest.mark.parametrize("table", ["identity", "reversed"])
def test_gather_past_4_gib(aqz, lattice, table):
    torch = torch_cuda()
    lat, d_base = lattice
    k = np.arange(N)
    base = (k // T_CHUNK * TILES).astype(np.uint32)
    internal = (k % T_CHUNK * TILE * TILE).astype(np.uint64)
    d_table = None
    if table == "reversed":
        lat = lat.flip(0)  # chunk c now lies in slot N_CHUNKS - 1 - c
        d_table = torch.arange(N_CHUNKS - 1, -1, -1, device="cuda", dtype=torch.int64) \
            .to(torch.int32)
    out = torch.full((GUARD + N * FB + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    aqz.chunk_gather_frames_device(np.uint8, W, H, TILE, TILE, lat.data_ptr(), CHUNK_BYTES,
                                   N_CHUNKS, d_table.data_ptr() if d_table is not None else 0,
                                   N_CHUNKS, base, internal, out.data_ptr() + GUARD, FB,
                                   d_bad.data_ptr(), launch_stream())
    torch.cuda.synchronize()
    assert bool((out[:GUARD] == POISON).all()) and bool((out[-GUARD:] == POISON).all())
    got = out[GUARD:GUARD + N * FB].reshape(N, H, W)
    for k0 in range(0, N, SLAB):
        k1 = min(N, k0 + SLAB)
        want = frames_slab(torch, d_base, k0, k1)
        if not torch.equal(got[k0:k1], want):
            bad = (got[k0:k1] != want).reshape(k1 - k0, -1).any(dim=1).nonzero().reshape(-1)
            raise AssertionError(f"{table}: frames {[k0 + int(i) for i in bad[:8]]} differ "
                                 f"({bad.numel()} in frames {k0}..{k1 - 1})")
    assert int(d_bad.cpu()[0]) == 0
