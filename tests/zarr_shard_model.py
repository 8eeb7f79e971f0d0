"""Plain-Python model of Shard::write_chunk / skip_chunk (shard.cpp:53-133)
driven layer by layer like Array::compress_and_flush_data_ (array.cpp:762-811)
with one thread, for tests/test_gpu_zarr_shards.py (not a test module).

Nothing here calls the product: the chunk -> (shard, internal index) map is
the numpy statement of tests/test_zarr_shard_layout.py (which the CPU suite
pins to the reference's assertions), the offsets are Python sums."""
import numpy as np

SENTINEL = 0xFFFFFFFFFFFFFFFF
SPACE, CHANNEL, TIME = 0, 1, 2


def one_shard_dims(n_slots, layers=1):
    """One shard whose layer has `n_slots` chunks."""
    return [(TIME, 0, 1, layers), (SPACE, 1, 1, 1), (SPACE, n_slots, 1, n_slots)]


def many_shard_dims(n_shards, n_slots):
    """`n_shards` shards of `n_slots` chunks a layer."""
    return [(TIME, 0, 1, 1), (SPACE, 1, 1, 1), (SPACE, n_shards * n_slots, 1, n_slots)]


def layout(dims):
    """(n_shards, chunks_per_shard, chunks_per_layer, layers_per_shard,
    shard_of, slot_of) — slot = internal index within layer 0."""
    chunks = [-(-d[1] // d[2]) for d in dims[1:]]
    shard = [d[3] for d in dims[1:]]
    n_sh = [-(-c // s) for c, s in zip(chunks, shard)]
    lat = np.array(np.unravel_index(np.arange(int(np.prod(chunks))), chunks))
    sh = np.array(shard)[:, None]
    shard_of = np.ravel_multi_index(tuple(lat // sh), n_sh)
    slot_of = np.ravel_multi_index(tuple(lat % sh), shard)
    lps = dims[0][3]
    return (int(np.prod(n_sh)), int(np.prod(shard)) * lps, int(np.prod(chunks)), lps,
            shard_of, slot_of)


class ShardModel:
    def __init__(self, dims):
        (self.n_shards, self.cps, self.cpl, self.lps, self.shard_of,
         self.slot_of) = layout(dims)
        self.spl = self.cps // self.lps
        self.begin()

    def begin(self):
        self.file_off = [0] * self.n_shards
        self.offsets = [[SENTINEL] * self.cps for _ in range(self.n_shards)]
        self.extents = [[SENTINEL] * self.cps for _ in range(self.n_shards)]
        self.layer = 0

    def append(self, sizes, has):
        """sizes[c], has[c] per chunk of the layer.  Returns (rows, total,
        place): rows[s] = (start, bytes, file offset), place[c] = start of
        chunk c in the packed output, or None when it is skipped."""
        rows, place, start = [], [None] * self.cpl, 0
        for s in range(self.n_shards):
            mine = [c for c in range(self.cpl) if self.shard_of[c] == s]
            mine.sort(key=lambda c: self.slot_of[c])
            first, at = self.file_off[s], 0
            for c in mine:
                i = self.layer * self.spl + int(self.slot_of[c])
                if has[c]:
                    self.offsets[s][i] = first + at
                    self.extents[s][i] = int(sizes[c])
                    place[c] = start + at
                    at += int(sizes[c])
            rows.append((start, at, first))
            self.file_off[s] = first + at
            start += at
        self.layer += 1
        return rows, start, place
