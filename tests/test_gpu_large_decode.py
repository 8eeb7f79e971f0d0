"""GPU: the device round trip past 4 GiB.  ceil(2^32 / 128 KiB) + 5 = 32,773
chunks of 128 KiB (the size tests/test_gpu_large_codecs.py uses) are encoded
by aqz_blosc_lz4_frames_device, decoded by aqz_blosc_lz4_decompress_device and
compared on the device; nothing but a few words crosses to the host.

Chunks cycle 5 smooth u16 prototypes, and every chunk carries its own index in
its first and last four bytes, so a frame or chunk offset truncated to 32 bits
lands on a chunk with other bytes there.
"""
import numpy as np
import pytest

from gpu_util import torch_cuda

pytestmark = pytest.mark.gpu

CHUNK = 131072
PROTOS = 5


def test_round_trip_past_4gib(aqz):
    torch = torch_cuda()
    n = -(-(1 << 32) // CHUNK) + 5
    assert n == 32773 and n * CHUNK > 1 << 32 and n % PROTOS
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:256, 0:256]
    protos = np.stack([(1000 + 300 * np.sin(xx / (7.0 + p)) * np.cos(yy / (5.0 + p)) +
                        rng.normal(0, 2, (256, 256))).astype(np.uint16) for p in range(PROTOS)])
    protos = torch.from_numpy(protos.view(np.uint8).reshape(PROTOS, CHUNK)).to("cuda")
    src = torch.empty((n, CHUNK), dtype=torch.uint8, device="cuda")
    for p in range(PROTOS):
        src[p::PROTOS] = protos[p]
    index = torch.arange(n, dtype=torch.int32, device="cuda")
    words = src.view(torch.int32)
    words[:, 0] = index
    words[:, -1] = index ^ 0x5A5A5A5A
    stride = CHUNK + aqz.BLOSC_MAX_OVERHEAD
    frames = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n, dtype=torch.int32, device="cuda")
    dst = torch.full((n, CHUNK), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx = aqz.BloscContext(0, 0)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.lz4_frames_device(5, 1, 2, src.data_ptr(), CHUNK, n, frames.data_ptr(), stride,
                          sizes.data_ptr(), stream)
    ctx.lz4_decompress_device(2, CHUNK, frames.data_ptr(), stride, sizes.data_ptr(), n,
                              dst.data_ptr(), CHUNK, status.data_ptr(), stream)
    torch.cuda.synchronize()
    assert int(sizes.max()) < CHUNK, "the prototypes no longer compress"
    assert bool((status == 0).all()), f"first bad status at chunk {int(torch.nonzero(status)[0])}"
    got = dst.view(torch.int32)
    assert bool((got[:, 0] == index).all()) and bool((got[:, -1] == (index ^ 0x5A5A5A5A)).all())
    assert torch.equal(dst, src)
    ctx.close()
