"""CPU: aqz_zarr_shard_layout (csrc/shard_layout.cpp, host only) against the
reference's own assertions (tests/golden/reference_shard_kats.json, written by
make_shard_kats.py from array-dimensions-shard-index-for-chunk.cpp and
array-dimensions-shard-internal-index.cpp) and against an independent numpy
statement of the chunk -> (shard, internal index) map on random dimension
sets with ragged shards.  No GPU is touched."""
import json
import os

import numpy as np
import pytest

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                   "reference_shard_kats.json")))


@pytest.mark.parametrize("case", KATS["addressing"], ids=lambda c: c["name"])
def test_reference_assertions(aqz, case):
    """Every EXPECT_EQ of the two reference tests: chunk index =
    layer * chunks_per_layer + c."""
    dims = [tuple(d) for d in case["dims"]]
    geo, _, _ = aqz.zarr_shard_layout(dims, 0)
    per_layer = {L: aqz.zarr_shard_layout(dims, L)
                 for L in range(geo["layers_per_shard"])}
    assert len(case["asserts"]) >= 24
    for a in case["asserts"]:
        layer, c = divmod(a["chunk"], geo["chunks_per_layer"])
        _, shard_of, internal_of = per_layer[layer]
        got = {"shard_index_for_chunk": shard_of, "shard_internal_index": internal_of}[
            a["function"]][c]
        assert int(got) == a["expect"], (case["name"], a["line"])


def test_reference_geometry(aqz):
    """The counts the two files' comments state: 18 shards of 8 chunks, two
    layers; four ragged shards of 6 chunks."""
    five, three = [[tuple(d) for d in c["dims"]] for c in KATS["addressing"]]
    assert aqz.zarr_shard_layout(five)[0] == {
        "n_shards": 18, "chunks_per_shard": 8, "chunks_per_layer": 72, "layers_per_shard": 2}
    assert aqz.zarr_shard_layout(three)[0] == {
        "n_shards": 4, "chunks_per_shard": 6, "chunks_per_layer": 12, "layers_per_shard": 1}


def numpy_layout(dims, layer):
    """unravel_index on the chunk lattice, divide and modulo by
    shard_size_chunks, ravel_multi_index; dimension 0 enters the internal
    index only (through the layer)."""
    chunks = [-(-d[1] // d[2]) for d in dims[1:]]
    shard = [d[3] for d in dims[1:]]
    n_shards = [-(-c // s) for c, s in zip(chunks, shard)]
    lat = np.array(np.unravel_index(np.arange(int(np.prod(chunks))), chunks))
    sh = np.array(shard)[:, None]
    shard_of = np.ravel_multi_index(tuple(lat // sh), n_shards)
    internal = np.ravel_multi_index(tuple(lat % sh), shard) + layer * int(np.prod(shard))
    return chunks, n_shards, shard_of, internal


def random_dims(rng):
    nd = int(rng.integers(3, 6))
    dims = []
    for i in range(nd):
        chunk = int(rng.integers(1, 9))
        n_chunks = int(rng.integers(1, 6))
        # a size that is not a multiple of the chunk, a shard that does not
        # divide the chunk count: ragged on both counts
        size = 0 if i == 0 and rng.integers(0, 2) else \
            max(1, n_chunks * chunk - int(rng.integers(0, chunk)))
        dims.append((int(rng.integers(0, 4)), size, chunk, int(rng.integers(1, 5))))
    return dims


def test_matches_numpy_on_random_dims(aqz):
    rng = np.random.default_rng(20)
    ragged = 0
    for _ in range(500):
        dims = random_dims(rng)
        lps = dims[0][3]
        layer = int(rng.integers(0, lps))
        geo, shard_of, internal_of = aqz.zarr_shard_layout(dims, layer)
        chunks, n_shards, want_shard, want_internal = numpy_layout(dims, layer)
        cps = int(np.prod([d[3] for d in dims]))
        assert geo == {"n_shards": int(np.prod(n_shards)), "chunks_per_shard": cps,
                       "chunks_per_layer": int(np.prod(chunks)), "layers_per_shard": lps}, dims
        assert np.array_equal(shard_of, want_shard), dims
        assert np.array_equal(internal_of, want_internal), dims
        # per shard and layer: real chunks' internal indices plus the skipped
        # ones (skipped_internal_indices_for_shard_layer) are exactly the
        # layer's range, each once; ascending chunk gives ascending internal
        spl = cps // lps
        for s in range(geo["n_shards"]):
            mine = internal_of[shard_of == s].astype(np.int64)
            assert np.all(np.diff(mine) > 0), dims
            layer_range = np.arange(layer * spl, (layer + 1) * spl)
            skipped = np.setdiff1d(layer_range, mine)
            assert np.all(np.isin(mine, layer_range)), dims
            assert mine.size + skipped.size == spl and np.unique(mine).size == mine.size
            ragged += skipped.size > 0
    assert ragged > 500  # the sweep does visit ragged shards


def test_refusals(aqz):
    ok = [(2, 0, 4, 2), (0, 64, 16, 2), (0, 64, 16, 2)]
    aqz.zarr_shard_layout(ok, 1)
    bad = [
        (ok[:2], 0),                                           # fewer than 3 dimensions
        (ok + [(0, 4, 2, 1)] * 30, 0),                         # more than AQZ_MAX_DIMS
        (ok, 2),                                               # layer >= layers_per_shard
        ([ok[0], (0, 64, 0, 2), ok[2]], 0),                    # zero chunk size
        ([ok[0], (0, 64, 16, 0), ok[2]], 0),                   # zero shard size
        ([ok[0], (0, 0, 16, 2), ok[2]], 0),                    # unbounded inner dimension
    ]
    for dims, layer in bad:
        with pytest.raises(aqz.AqzError) as e:
            aqz.zarr_shard_layout(dims, layer)
        assert e.value.status == 1, (dims, layer)
    big = 1 << 16
    over = [
        [ok[0], (0, big, 1, 1), (0, big, 1, 1)],               # chunks_per_layer = 2^32
        [ok[0], (0, 1 << 15, 1, 1), (0, big, 1, 1)],           # chunks_per_layer = 2^31
        [ok[0], (0, 4, 1, big), (0, 4, 1, big)],               # chunks_per_shard = 2^32
        [(2, 0, 1, 1 << 15), (0, 4, 1, big), (0, 4, 1, 1)],    # chunks_per_shard = 2^31
    ]
    for dims in over:
        with pytest.raises(aqz.AqzError) as e:
            aqz.zarr_shard_layout(dims, 0)
        assert e.value.status == 2, dims
    # just below the limit is a geometry query that answers
    lib = aqz.lib()
    import ctypes
    arr = (aqz.Dimension * 3)(*[aqz.Dimension(*d, 1.0) for d in
                                [ok[0], (0, (1 << 15) - 1, 1, 1), (0, big, 1, 1)]])
    geo = aqz.ZarrShardGeometry()
    assert lib.aqz_zarr_shard_layout(arr, 3, 0, ctypes.byref(geo), None, None) == 0
    assert geo.chunks_per_layer == ((1 << 15) - 1) * big
    assert lib.aqz_zarr_shard_layout(None, 3, 0, ctypes.byref(geo), None, None) == 1
    assert lib.aqz_zarr_shard_layout(arr, 3, 0, None, None, None) == 1


def test_set_create_refuses_without_gpu(aqz):
    """Argument validation happens before any device call."""
    with pytest.raises(aqz.AqzError) as e:
        aqz.ZarrShardSet([(2, 0, 4, 2), (0, 64, 0, 2), (0, 64, 16, 2)])
    assert e.value.status == 1
    with pytest.raises(aqz.AqzError) as e:  # a 1 GiB index table
        aqz.ZarrShardSet([(2, 0, 1, 1 << 10), (0, 4, 1, 1 << 8), (0, 4, 1, 1 << 8)])
    assert e.value.status == 2
