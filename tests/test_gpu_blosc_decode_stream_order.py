"""GPU: aqz_blosc_lz4_decompress_device and aqz_zarr_shard_decompress_device
between pending work on the caller's stream (tests/stream_order.py, imported
as it is).  The status clear, the decode kernel and the unfilter must all be
queued on that stream: frames and tables are read, and chunks and statuses
written, in stream order, and nothing is left on another stream.

Each call is made twice.  With a ctx whose scratch the unstalled first run
has grown, the stalled call needs no more of it and must return while the
stall runs.  With a ctx that is new when the stalled run begins, the call
grows the scratch under the stall: it may wait by contract, and its results
must still be right.
"""
import numpy as np
import pytest

import blosc_decode_cases as bd
from stream_order import Sandwich

pytestmark = pytest.mark.gpu


def golden_group(prefix):
    items = [g for g in bd.golden() if g[0].startswith(prefix) and "__lz4__" in g[0]]
    assert len(items) >= 4
    frames = [fr for _, fr, _, _ in items]
    return frames, np.frombuffer(items[0][2], np.uint8), items[0][3]


class Rig:
    """Four LZ4 frames of one input (byte shuffle twice, bit shuffle, memcpy):
    through the scratch and the unfilter, and straight to the destination."""

    def __init__(self, sw, shard):
        frames, src, self.ts = golden_group("smooth_u16_128x128")
        self.n, self.nbytes, self.shard = len(frames), src.size, shard
        if shard:
            self.base = (1 << 36) + 3
            image = bytearray(b"\x77" * 5)
            pairs = []
            for fr in frames:
                pairs += [self.base + len(image), len(fr)]
                image += fr
            self.image_bytes = len(image)
            self.d_frames = sw.input(np.frombuffer(bytes(image), np.uint8))
            self.d_table = sw.input(np.array(pairs, np.uint64))
        else:
            self.stride = max(len(f) for f in frames) + 3
            packed = np.zeros(self.n * self.stride, np.uint8)
            for k, fr in enumerate(frames):
                packed[k * self.stride:k * self.stride + len(fr)] = np.frombuffer(fr, np.uint8)
            self.d_frames = sw.input(packed)
            self.d_sizes = sw.input(np.array([len(f) for f in frames], np.uint32))
        self.d_dst = sw.output(self.n * self.nbytes, np.tile(src, self.n), name="chunks")
        self.d_status = sw.output(4 * self.n, np.zeros(self.n, np.uint32), name="statuses")

    def run(self, ctx, hip_stream):
        if self.shard:
            ctx.zarr_shard_decompress_device(
                self.ts, self.nbytes, self.d_frames.data_ptr(), self.image_bytes, self.base,
                self.d_table.data_ptr(), self.n, self.d_dst.data_ptr(), self.nbytes,
                self.d_status.data_ptr(), hip_stream)
        else:
            ctx.lz4_decompress_device(
                self.ts, self.nbytes, self.d_frames.data_ptr(), self.stride,
                self.d_sizes.data_ptr(), self.n, self.d_dst.data_ptr(), self.nbytes,
                self.d_status.data_ptr(), hip_stream)


@pytest.mark.parametrize("shard", [False, True], ids=["frames", "shard"])
def test_decompress_with_grown_scratch_does_not_wait(aqz, shard):
    ctx = aqz.BloscContext(0, 0)
    sw = Sandwich(f"decompress_device shard={shard}")
    rig = Rig(sw, shard)
    sw.run(lambda sw: rig.run(ctx, sw.hip_stream))
    ctx.close()


@pytest.mark.parametrize("shard", [False, True], ids=["frames", "shard"])
def test_decompress_that_grows_scratch_may_wait(aqz, shard):
    ctxs = {"dry": aqz.BloscContext(0, 0), "stalled": aqz.BloscContext(0, 0)}
    sw = Sandwich(f"decompress_device growing shard={shard}")
    rig = Rig(sw, shard)
    # the stalled run's ctx has no scratch yet: this call allocates it
    sw.run(lambda sw: rig.run(ctxs[sw.phase], sw.hip_stream), blocks=True)
    for c in ctxs.values():
        c.close()
