"""GPU, end to end: a volume pyramid level from the fused volume kernel into
its chunk lattice (run_device_volume_chunked), has_data from the zero scan
(aqz_zarr_shard_chunk_has_data_device, flag_slots = 1), LZ4 frames on the
device (aqz_blosc_lz4_frames_device), and the shards
(aqz_zarr_shard_set_append_layer and the tables).

Expected: the oracle pyramid placed by the oracle's addressing, its chunks
compressed by aqz_blosc_compress_device, laid out by tests/zarr_shard_model.py.
The geometry is the chunked case of tests/test_gpu_volume_tiled.py widened to
two shards: level 1 is Z/Y/X = 4 x 24 x 64 u16 in chunks of 2 x 16 x 16 — two
layers of 2 x 4 chunks, ragged in Y — in shards of 2 layers x 2 x 2 chunks."""
import re

import numpy as np
import pytest

import volume_tiled_cases as vc
import zarr_shard_model as zm
from gpu_util import empty_device, to_device, torch_cuda

pytestmark = pytest.mark.gpu

MEAN = 1
GEO = vc.volume_geo(128, 48, 8, 3)
SHAPES = [None, (2, 16, 16), (2, 8, 16)]


def test_volume_level_to_shards(aqz, oracle):
    if not re.match(r"lz4 \S+ \(", aqz.blosc_codec_info()):
        pytest.skip("no liblz4 loaded: " + aqz.blosc_codec_info())
    torch = torch_cuda()
    rng = np.random.default_rng(17)
    frames = rng.integers(1, 65536, (8, 48, 128), dtype=np.uint16)
    frames[:4, :32, 32:64] = 0  # level 1, layer 0, chunk (0, 1): all zero
    lv = vc.oracle_planes(oracle, GEO, np.uint16, MEAN, frames)
    want = vc.expected_chunked(oracle, lv, 0, np.uint16, GEO, SHAPES)
    bufs, flags, lats = [None], [None], [None]
    for L in (1, 2):
        _, offs, cb, _, cap = want[L]
        _, cy, cx = SHAPES[L]
        bufs.append(empty_device(cap))
        flags.append(empty_device((8 >> L) * vc.n_tiles(GEO, L, (cy, cx))))
        bufs[L].fill_(vc.POISON)
        flags[L].fill_(vc.POISON)
        lats.append((bufs[L].data_ptr(), cap, cy, cx, cb, offs))
    ds = aqz.Downsampler(GEO, np.uint16, MEAN, device=0)
    ds.run_device_volume_chunked(to_device(frames).data_ptr(), 8, lats,
                                 [0] + [f.data_ptr() for f in flags[1:]])
    torch.cuda.synchronize()
    assert ds.last_batch_kind() == 5
    ds.close()

    lattice, _, cb, lb, cap = want[1]
    nt = vc.n_tiles(GEO, 1, SHAPES[1][1:])
    assert (nt, lb, cap) == (8, 8 * cb, 2 * lb)
    assert np.array_equal(bufs[1].cpu().numpy(), lattice)  # every plane owns its bytes here
    sdims = [(zm.TIME, 0, 2, 2), (zm.SPACE, 24, 16, 2), (zm.SPACE, 64, 16, 2)]
    st = aqz.ZarrShardSet(sdims, 0)
    m = zm.ShardModel(sdims)
    assert (st.n_shards, st.chunks_per_shard, st.chunks_per_layer, st.layers_per_shard) == \
        (m.n_shards, m.cps, m.cpl, m.lps) == (2, 8, 8, 2)
    ctx = aqz.BloscContext(0, 2)
    # the model's input: aqz_blosc_compress_device's frames of the oracle-placed chunks
    d_want = to_device(lattice)
    ref = ctx.compress_device(1, 1, 2, "lz4", d_want.data_ptr(), cb, 2 * nt)
    stride = cb + aqz.BLOSC_MAX_OVERHEAD
    d_frames = empty_device(nt * stride)
    d_sizes = empty_device(4 * nt)
    d_has = empty_device(nt)
    images = [bytearray() for _ in range(st.n_shards)]
    for layer in range(2):
        chunks = lattice[layer * lb:(layer + 1) * lb].reshape(nt, cb)
        has_want = [int(c.any()) for c in chunks]
        assert has_want == ([1, 0, 1, 1, 1, 1, 1, 1] if layer == 0 else [1] * 8)
        d_has.fill_(0)
        # two planes a layer, one flag byte per tile and plane; 3-D dims: every
        # plane's tiles start at the layer's chunk 0
        aqz.zarr_shard_chunk_has_data_device(flags[1].data_ptr() + layer * 2 * nt, 2, nt, 1,
                                             [0, 0], d_has.data_ptr())
        ctx.lz4_frames_device(1, 1, 2, bufs[1].data_ptr() + layer * lb, cb, nt,
                              d_frames.data_ptr(), stride, d_sizes.data_ptr())
        rows, total, data = st.append_layer(d_frames.data_ptr(), stride, d_sizes.data_ptr(),
                                            d_has.data_ptr())
        assert list(d_has.cpu().numpy()) == has_want
        sizes = [len(ref[layer * nt + c]) for c in range(nt)]
        m_rows, m_total, place = m.append(sizes, has_want)
        assert [tuple(int(v) for v in r) for r in rows] == [tuple(r) for r in m_rows]
        assert total == m_total == data.size
        for c in range(nt):
            if place[c] is not None:
                assert data[place[c]:place[c] + sizes[c]].tobytes() == ref[layer * nt + c], \
                    (layer, c)
        for s in range(st.n_shards):
            start, nbytes, file_off = (int(v) for v in rows[s])
            assert file_off == len(images[s])
            images[s] += data[start:start + nbytes].tobytes()
    tab, tab_off = st.tables()
    for s in range(st.n_shards):
        assert int(tab_off[s]) == len(images[s]) == m.file_off[s]
        assert np.array_equal(tab[s], oracle.shard_index_table(m.offsets[s], m.extents[s]))
    assert m.offsets[0].count(zm.SENTINEL) == 1  # the all-zero chunk occupies no bytes
    ctx.close()
    st.close()
