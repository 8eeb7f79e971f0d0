"""CPU: aqz_chunk_frame_places — aqz_chunk_frame_offsets with its sum kept in
parts (which chunk a frame's tile 0 lies in, and where inside it), for a gather
that finds chunks through a placement table.

Against the oracle's restatement of ArrayDimensions::chunk_lattice_index /
tile_group_offset / chunk_internal_offset (array.dimensions.cpp:232-314): on
the frames the reference's own unit tests assert on
(tests/golden/reference_kats.json, `addressing`) and on random N-D dimension
sets with batches that start inside a layer and span layers.  Its identity
with aqz_chunk_frame_offsets, its refusals and its overflow.
"""
import ctypes

import numpy as np
import pytest

import kat_runner

KATS = kat_runner.load()
KAT_DIMS = [tuple(d) for d in KATS["addressing"][0]["dims"]]
KAT_FRAMES = max(a["args"][0] for c in KATS["addressing"] for a in c["asserts"]) + 1

TIME, CHANNEL, SPACE = 2, 1, 0
UINT32_MAX = 0xFFFFFFFF


def oracle_places(oracle, dims, bpp, first, n):
    counts = [-(-d[1] // d[2]) for d in dims]
    per_layer = int(np.prod(counts[1:], dtype=np.uint64))
    layer0 = oracle.chunk_lattice_index(dims, first, 0)
    base = [(oracle.chunk_lattice_index(dims, k, 0) - layer0) * per_layer +
            oracle.tile_group_offset(dims, k) for k in range(first, first + n)]
    internal = [oracle.chunk_internal_offset(dims, bpp, k) for k in range(first, first + n)]
    chunk_bytes = bpp * int(np.prod([d[2] for d in dims], dtype=np.uint64))
    return base, internal, chunk_bytes, per_layer


def random_dims(rng):
    nd = int(rng.integers(3, 7))
    dims = [(TIME, 0, int(rng.integers(1, 6)), 1)]
    for _ in range(nd - 3):
        size = int(rng.integers(1, 8))
        dims.append((CHANNEL, size, int(rng.integers(1, size + 1)), 1))
    for _ in range(2):
        size = int(rng.integers(1, 400))
        dims.append((SPACE, size, int(rng.integers(1, 100)), 1))
    return dims


def test_kat_frames_are_76():
    assert KAT_FRAMES == 76


@pytest.mark.parametrize("bpp", [1, 2, 4, 8])
def test_places_on_the_reference_kat_frames(aqz, oracle, bpp):
    base, internal, cb, cpl = aqz.chunk_frame_places(KAT_DIMS, bpp, 0, KAT_FRAMES)
    wb, wi, wcb, wcpl = oracle_places(oracle, KAT_DIMS, bpp, 0, KAT_FRAMES)
    assert (cb, cpl) == (wcb, wcpl) == (bpp * 5 * 2 * 2 * 16 * 16, 2 * 3 * 3 * 4)
    assert base.dtype == np.uint32 and internal.dtype == np.uint64
    assert base.tolist() == wb
    assert internal.tolist() == wi


def test_places_pin_the_kat_values(aqz):
    """The reference's asserted values themselves, not only the oracle's
    restatement of its loops: chunk_internal_offset and tile_group_offset."""
    by = {c["function"]: c for c in KATS["addressing"]}
    bpp = np.dtype(kat_runner.NP_DTYPES[by["chunk_internal_offset"]["dtype"]]).itemsize
    base, internal, _, cpl = aqz.chunk_frame_places(KAT_DIMS, bpp, 0, KAT_FRAMES)
    for a in by["chunk_internal_offset"]["asserts"]:
        assert int(internal[a["args"][0]]) == a["expect"], a
    for a in by["tile_group_offset"]["asserts"]:
        assert int(base[a["args"][0]]) % cpl == a["expect"], a
    for a in by["chunk_lattice_index"]["asserts"]:
        if a["args"][1] == 0:
            assert int(base[a["args"][0]]) // cpl == a["expect"], a


def test_places_on_random_dimension_sets(aqz, oracle):
    rng = np.random.default_rng(1214)
    mid_layer = spans = 0
    for _ in range(200):
        dims = random_dims(rng)
        bpp = int(rng.choice([1, 2, 4, 8]))
        first = int(rng.integers(0, 300))
        n = 30
        base, internal, cb, cpl = aqz.chunk_frame_places(dims, bpp, first, n)
        wb, wi, wcb, wcpl = oracle_places(oracle, dims, bpp, first, n)
        assert (cb, cpl) == (wcb, wcpl), dims
        assert base.tolist() == wb, (dims, first)
        assert internal.tolist() == wi, (dims, first)
        layer_frames = dims[0][2] * int(np.prod([d[1] for d in dims[1:-2]], dtype=np.uint64))
        mid_layer += first % layer_frames != 0
        spans += (first + n - 1) // layer_frames > first // layer_frames
    assert mid_layer >= 50 and spans >= 50  # the generator reaches both


def test_identity_with_chunk_frame_offsets(aqz):
    rng = np.random.default_rng(77)
    for _ in range(200):
        dims = random_dims(rng)
        bpp = int(rng.choice([1, 2, 4, 8]))
        first = int(rng.integers(0, 10 ** 6))
        n = int(rng.integers(1, 40))
        offs, cb, lb = aqz.chunk_frame_offsets(dims, bpp, first, n)
        base, internal, pcb, cpl = aqz.chunk_frame_places(dims, bpp, first, n)
        assert pcb == cb and cpl * cb == lb
        assert [int(b) * cb + int(i) for b, i in zip(base, internal)] == offs, dims
        assert all(int(i) < cb for i in internal)


def test_zero_frames(aqz):
    dims = [(TIME, 0, 3, 1), (SPACE, 48, 16, 1), (SPACE, 64, 16, 1)]
    base, internal, cb, cpl = aqz.chunk_frame_places(dims, 2, 5, 0)
    assert len(base) == len(internal) == 0 and cb == 3 * 16 * 16 * 2 and cpl == 12


def _raw(aqz, dims, bpp, first, n, base=True, internal=True):
    L = aqz.lib()
    arr = (aqz.Dimension * max(len(dims), 1))(*[aqz.Dimension(*d, 1.0) for d in dims])
    b = np.zeros(max(n, 1), np.uint32)
    i = np.zeros(max(n, 1), np.uint64)
    return L.aqz_chunk_frame_places(arr if dims is not None else None,
                                    len(dims) if dims is not None else 3, bpp, first, n,
                                    b.ctypes.data if base else None,
                                    i.ctypes.data if internal else None, None, None)


def test_refusals_are_those_of_chunk_frame_offsets(aqz):
    INVALID = 1
    good = [(TIME, 0, 1, 1), (SPACE, 10, 5, 1), (SPACE, 10, 5, 1)]
    bad = [
        [(SPACE, 10, 5, 1), (SPACE, 10, 5, 1)],                              # two dimensions
        [(TIME, 0, 0, 1), (SPACE, 10, 5, 1), (SPACE, 10, 5, 1)],             # chunk size 0
        [(TIME, 0, 1, 1), (CHANNEL, 0, 1, 1), (SPACE, 10, 5, 1), (SPACE, 10, 5, 1)],
        [(TIME, 0, 1, 1), (SPACE, 10, 0, 1), (SPACE, 10, 5, 1)],
    ]
    assert _raw(aqz, good, 2, 0, 4) == 0
    assert _raw(aqz, good, 2, 0, 0, base=False, internal=False) == 0  # as offsets: none needed
    for dims in bad:
        assert _raw(aqz, dims, 2, 0, 1) == INVALID, dims
        with pytest.raises(aqz.AqzError):
            aqz.chunk_frame_offsets(dims, 2, 0, 1)
        with pytest.raises(aqz.AqzError):
            aqz.chunk_frame_places(dims, 2, 0, 1)
    assert _raw(aqz, good, 0, 0, 1) == INVALID           # bytes_per_px 0
    assert _raw(aqz, good, 2, 0, 1, base=False) == INVALID
    assert _raw(aqz, good, 2, 0, 1, internal=False) == INVALID
    L = aqz.lib()
    assert L.aqz_chunk_frame_places(None, 3, 2, 0, 0, None, None, None, None) == INVALID


def test_overflow_where_a_base_reaches_the_reserved_slot(aqz):
    """UINT32_MAX is AQZ_CHUNK_SLOT_ABSENT: no frame's tiles may reach it.
    65536 x 65535 one-pixel chunks a frame are UINT32_MAX - 65535 tiles: the
    first layer fits, a batch that reaches into the second does not; one more
    chunk row and not even the first does."""
    OVERFLOW = 2  # AQZ_OVERFLOW
    dims = [(TIME, 0, 1, 1), (SPACE, 65535, 1, 1), (SPACE, 65536, 1, 1)]
    base, _, _, cpl = aqz.chunk_frame_places(dims, 1, 7, 1)
    assert base.tolist() == [0] and cpl == 65535 * 65536
    assert _raw(aqz, dims, 1, 7, 2) == OVERFLOW
    with pytest.raises(aqz.AqzError) as e:
        aqz.chunk_frame_places(dims, 1, 7, 2)
    assert e.value.status == OVERFLOW
    full = [(TIME, 0, 1, 1), (SPACE, 65536, 1, 1), (SPACE, 65536, 1, 1)]
    assert _raw(aqz, full, 1, 0, 1) == OVERFLOW
    # base + tiles == UINT32_MAX - 1 is the last that fits
    edge = [(TIME, 0, 1, 1), (SPACE, 2, 1, 1), (SPACE, (UINT32_MAX - 1) // 2, 1, 1)]
    assert _raw(aqz, edge, 1, 0, 1) == 0
