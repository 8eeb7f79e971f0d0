"""CPU: the tables of tests/mixed_tiled_cases.py hold what the GPU tests of
aqz_ds_run_device_mixed_tiled / _chunked rely on: every store branch of the
tiled Z run is reached by a fixed shape named for it, from geometry alone; the
fuzz cases are accepted pyramids spread over the pyramid categories and the
store branches (a condition on the generator, checked here); the restated run
cut of aqz_ds_mixed_flag_slots agrees with mixed_batch_cases.runs_of; expected
tiles are oracle.tile_frame of the oracle's levels."""
import numpy as np
import pytest

import mixed_batch_cases as mc
import mixed_tiled_cases as tc


def fixed_branches(name, spec):
    geo, _, dtype, _ = mc.FIXED[name]
    return tc.branches_of(geo, dtype, tc.tiles_for(geo, spec))


# shape, tile spec -> the branch the issue names it for
NAMED = [
    ("volume1_zrun3", (16, 16), "vector_in_tile_row"),
    ("z_then_xy", (16, 12), "vector_across_tile_edge"),
    ("zrun3_zrun2_851", (8, 5), "vector_across_row_end"),
    ("zrun3_zrun2_851", (23, 37), "plane_tail"),
    ("zrun3_zrun2_851", (8, 5), "column_fill"),
    ("zrun3_zrun2_851", (8, 5), "row_fill"),
    ("volume1_zrun3", (64, 64), "tile_larger_than_frame"),
    ("zrun3_zrun2_851", (64, 64), "tile_larger_than_frame"),
    ("span_plus_1", (1, 512), "plane_tail"),
    ("span_minus_1", (1, 512), "plane_tail"),
    ("one_element", (4, 4), "tile_larger_than_frame"),
]


@pytest.mark.parametrize("name,spec,branch", NAMED)
def test_fixed_shapes_reach_their_branch(name, spec, branch):
    assert spec in tc.FIXED_TILES[name]
    assert branch in fixed_branches(name, spec), (name, spec, fixed_branches(name, spec))


def test_every_branch_has_a_fixed_shape():
    reached = set()
    for name, spec in tc.FIXED_CASES:
        reached |= fixed_branches(name, spec)
    assert reached == set(tc.BRANCHES)


def test_branches_from_geometry():
    # 32 x 24 f32 (4 a vector) under 16 x 16: every vector inside one tile row
    assert tc.z_level_branches(32, 24, 4, (16, 16)) == {"vector_in_tile_row", "row_fill"}
    # 64 x 32 u16 (8 a vector) under 12-column tiles: vectors at 8 cross 12
    assert tc.z_level_branches(64, 32, 2, (16, 12)) == {
        "vector_in_tile_row", "vector_across_tile_edge", "column_fill"}
    # 37-byte rows: vectors cross row ends; 851 = 53 * 16 + 3
    b = tc.z_level_branches(37, 23, 1, (23, 37))
    assert {"vector_across_row_end", "plane_tail"} <= b and "column_fill" not in b
    # one element: no vector at all
    assert tc.z_level_branches(1, 1, 2, (1, 1)) == {"plane_tail"}
    # a different tile shape per Z level of one run
    geo = mc.FIXED["volume1_zrun3"][0]
    per_level = tc.FIXED_TILES["volume1_zrun3"][1]
    assert len({per_level[L] for L in (2, 3, 4)}) == 3 and mc.classes(geo)[2:] == ["Z"] * 3


def test_fixed_shapes_are_accepted_pyramids():
    for name, (geo, n, _, runs) in mc.FIXED.items():
        assert mc.runs_of(geo, n) == runs, name


def all_geos():
    out = [(geo, n) for geo, n, _, _ in mc.FIXED.values()]
    out += [(c["geo"], c["n"]) for c in map(tc.fuzz_tiled_case, range(tc.N_FUZZ_TILED))]
    out += [(c["geo"], c["n"]) for c in map(tc.fuzz_chunked_case, range(tc.N_FUZZ_CHUNKED))]
    out += [(mc.fuzz_case(i)["geo"], mc.fuzz_case(i)["n"]) for i in range(mc.N_FUZZ)]
    return out


def test_run_cut_agrees_with_runs_of():
    for geo, n in all_geos():
        runs = mc.runs_of(geo, n)
        assert runs is not None
        for L in range(1, len(geo)):
            cls, first, k = tc.run_of_level(geo, L)
            match = [r for r in runs if r[1] <= L < r[1] + r[2]]
            assert len(match) == 1 and match[0][:3] == (cls, first, k), (geo, L, runs)
    # refused pyramids: a classless level, an odd plane count in front of a pair
    assert tc.run_of_level([(8, 8, 2), (8, 8, 2)], 1) is None
    assert tc.run_of_level([(8, 8, 3), (8, 8, 1)], 1) is None
    assert mc.runs_of([(8, 8, 3), (8, 8, 1)], 3) is None


def accepted(c):
    """What the tiled call accepts on top of runs_of: an XYZ or XY run starts
    at a level one 16-byte load wide."""
    bpp = np.dtype(c["dtype"]).itemsize
    runs = mc.runs_of(c["geo"], c["n"])
    return runs is not None and all(cls == "Z" or c["geo"][first - 1][0] * bpp >= 16
                                    for cls, first, _, _ in runs)


@pytest.mark.parametrize("make,count,least", [(tc.fuzz_tiled_case, tc.N_FUZZ_TILED, 4),
                                              (tc.fuzz_chunked_case, tc.N_FUZZ_CHUNKED, 2)],
                         ids=["tiled", "chunked"])
def test_fuzz_cases_are_accepted_and_spread(make, count, least):
    cats = {k: 0 for k in mc.CATEGORIES}
    branches = {k: 0 for k in tc.BRANCHES}
    for i in range(count):
        c = make(i)
        assert accepted(c), (i, c["geo"])
        assert make(i)["geo"] == c["geo"] and make(i)["tiles"] == c["tiles"]   # seeded
        assert all(r >= 1 and cc >= 1 for r, cc in c["tiles"][1:])
        for k in mc.fuzz_categories(c):
            cats[k] += 1
        for k in tc.branches_of(c["geo"], c["dtype"], c["tiles"]):
            branches[k] += 1
    assert min(cats.values()) >= least, cats
    assert min(branches.values()) >= least, branches


def test_expected_tiles_are_the_oracles(oracle):
    geo, n, dtype, _ = mc.FIXED["z_then_xy"]
    frames = mc.fixed_frames("z_then_xy")
    levels = mc.oracle_levels(oracle, geo, dtype, mc.MEAN, frames)
    tiles = tc.tiles_for(geo, (16, 12))
    want = tc.expected_tiled(oracle, levels, tiles)
    for L in range(1, len(geo)):
        w, h, _ = geo[L]
        t, nz = want[L]
        assert t.shape == (mc.emitted(geo, n)[L], tc.n_tiles(geo, L, tiles[L]), 16, 12)
        # tile 0's first row is the level's, and the overhang is zero
        assert np.array_equal(t[:, 0, 0, :min(12, w)], levels[L][:, 0, :min(12, w)])
        ntx = -(-w // 12)
        last = t[:, ntx - 1]
        assert not last[:, :, w - (ntx - 1) * 12:].any()
        assert nz.shape == t.shape[:2]
    # lattice places are oracle.chunk_frame_offsets'
    shapes = [None, (2, 16, 12), (2, 16, 12)]
    ch = tc.expected_chunked(oracle, geo, levels, shapes, [0, 0, 0], dtype)
    for L in (1, 2):
        offs, cb, _ = oracle.chunk_frame_offsets(tc.chunk_dims(geo, L, shapes[L]), 2, 0,
                                                 len(levels[L]))
        assert ch[L][1] == offs and ch[L][2] == cb
        assert offs[1] - offs[0] == 16 * 12 * 2   # two planes share a chunk
