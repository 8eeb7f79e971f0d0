"""CPU: what the tiled volume tests' shapes reach, from the geometry arithmetic
of plan_volume_tiled alone (volume_tiled_cases.level_geometry):

    units_x = ceil(W / (64 * 16 / bpp)),  cov_w = units_x * ((64 * 16 / bpp) >> j)
    units_y = ceil(H / 2^k),              cov_h = units_y * (2^k >> j)
    pw = ntx * tc,  ph = nty * tr,        CO = max((16 / bpp) >> j, 1)

for level j (1 or 2) of a run of k levels.  Every row of BRANCH_CASES has the
property it was chosen for, and the seeded fuzz generators construct only
pyramids the calls accept and fall into every class often enough."""
import numpy as np
import pytest

import volume_tiled_cases as vc


def geometry_of(case):
    w, h, _, levels, dtype, _, _, _ = case
    return vc.level_geometry(w, h, levels, dtype, vc.case_tiles(case))


def check_property(case, name):
    g = geometry_of(case)
    props = vc.case_properties(case)
    if name == "column_fill_both_levels":
        assert [(q["cov_w"], q["pw"]) for q in g[1:]] == [(256, 384), (128, 384)]
        assert props >= {"interior_units_only", "column_fill_many_rows", "runs_1"}
        assert all(q["ph"] > 1 for q in g[1:])  # zz / f split with zrows == ph > 1
        assert case[7] * case[2] >> 2 >= 2      # several plane groups
    elif name == "column_fill_second_level_only":
        assert g[1]["cov_w"] >= g[1]["pw"] and g[1]["cov_h"] >= g[1]["ph"]  # no items at level 1
        assert g[2]["cov_w"] < g[2]["pw"]
    elif name == "crossing_co_8_4":
        assert [q["co"] for q in g[1:]] == [8, 4]
        assert all(q["tc"] % q["co"] for q in g[1:])
        assert "interior_and_edge_units" in props
        # ragged rows: the last unit row passes the frame, the level its tiles
        assert all(q["src_h"] % (1 << q["k"]) for q in g[1:]) and g[1]["h"] % g[1]["tr"]
    elif name == "crossing_co_4_2":
        assert [q["co"] for q in g[1:]] == [4, 2]
        assert all(q["tc"] % q["co"] for q in g[1:])
    elif name == "three_runs":
        assert "runs_3" in props and all(q["k"] == 2 for q in g[1:])
        bpp = np.dtype(case[4]).itemsize
        assert all(q["src_w"] >= 16 // bpp for q in g[1:])
    elif name == "one_tile_a_level":
        assert all(q["tr"] > q["h"] and q["tc"] > q["w"] for q in g[1:])
    elif name == "one_pixel_tiles":
        assert all((q["tr"], q["tc"]) == (1, 1) for q in g[1:])
    else:
        raise AssertionError(f"unknown property {name}")


@pytest.mark.parametrize("row", vc.BRANCH_CASES, ids=lambda r: f"{vc.case_id(r[0])}-{r[2]}")
def test_branch_case_has_its_property(row):
    case, methods, name = row
    assert vc.MEAN in methods
    check_property(case, name)


def test_branch_cases_differ_from_the_first_table():
    """No volume-tiled shape of the first table reaches column zero-fill, and
    only f32 crosses a tile edge there: what BRANCH_CASES was added for."""
    old = set()
    for c in vc.CASES:
        old |= vc.case_properties(c)
    assert not any(p.startswith("column_fill") for p in old), old
    assert {p for p in old if p.startswith("crossing")} == {"crossing_co_2"}
    assert "runs_3" not in old
    new = set()
    for c, _, _ in vc.BRANCH_CASES:
        new |= vc.case_properties(c)
    assert new >= {"column_fill_level_1_of_run", "column_fill_level_2_of_run", "crossing_co_8",
                   "crossing_co_4", "crossing_co_2", "runs_3", "tile_wider_than_level"}
    # the element-offset test's cases: 260x12x4 f32, 520x22x8 u16 5x25, the 7-level pyramid
    assert [vc.case_id(c) for c in vc.OFFSET_CASES] == [
        "260x12x4_L3_float32_3x200", "520x22x8_L3_uint16_5x25", "600x40x64_L7_uint16_8x32"]
    for c in vc.OFFSET_CASES:  # 1 + (in_off + 2 L) % 7: a different offset at every level
        for in_off in (1, 3, 7):
            offs = [1 + (in_off + 2 * L) % 7 for L in range(1, c[3])]
            assert len(set(offs)) == len(offs) <= 6 and all(1 <= o <= 7 for o in offs)


def check_pyramid(c):
    bpp = np.dtype(c["dtype"]).itemsize
    levels = c["levels"]
    ws = [g[0] for g in c["geo"]]
    assert ws[0] == c["w"] and 1 <= c["h"] <= 48
    assert vc.fuzz_wmin(bpp, levels) <= c["w"] <= 2500
    for L in (0, 2, 4):  # the sources of the runs the pyramid has
        if L < levels - 1:
            assert ws[L] >= 16 // bpp, (L, ws)
    assert all(ws[L] < ws[L - 1] for L in range(1, levels)), ws
    assert c["planes"] in [(1 << (levels - 1)) * m for m in (1, 2, 3)]
    assert c["stacks"] in (1, 2) and c["n"] == c["planes"] * c["stacks"]
    assert all(g[2] % 2 == 0 for g in c["geo"][:-1])  # no level passes a plane through
    assert c["n"] * c["h"] * c["w"] * bpp <= 16 << 20
    assert 0 <= c["in_off"] <= 7


def test_wmin_is_the_smallest_width():
    # u8, 7 levels: level 4 holds 16 px from 241 px on (241 -> 121 -> 61 -> 31 -> 16)
    assert vc.fuzz_wmin(1, 7) == 241
    assert vc.fuzz_wmin(1, 5) == 61     # level 2 holds 16 px; level 4 is no source
    assert vc.fuzz_wmin(2, 3) == 8 and vc.fuzz_wmin(8, 2) == 2
    assert vc.fuzz_wmin(8, 7) == 33     # every level narrower: 33 17 9 5 3 2 1


TILED_CLASSES = ["column_fill_level_1_of_run", "column_fill_level_2_of_run", "row_fill",
                 "crossing_co_8", "crossing_co_4", "crossing_co_2", "edge_units_only",
                 "interior_and_edge_units", "runs_2", "runs_3", "input_offset", "no_flags",
                 "tile_wider_than_level"]
CHUNKED_CLASSES = ["chained", "first_nonzero", "ragged_x", "ragged_y"]


def test_tiled_fuzz_cases_are_accepted_and_cover_every_class():
    assert vc.N_FUZZ_TILED == 96
    count = dict.fromkeys(TILED_CLASSES, 0)
    for i in range(vc.N_FUZZ_TILED):
        c = vc.fuzz_tiled_params(i)
        check_pyramid(c)
        bpp = np.dtype(c["dtype"]).itemsize
        assert len(c["tiles"]) == c["levels"] and len(c["out_off"]) == c["levels"]
        for L in range(1, c["levels"]):
            tr, tc = c["tiles"][L]
            assert tr >= 1 and tc >= 1 and 0 <= c["out_off"][L] <= 7
            lw, lh, _ = c["geo"][L]
            assert (c["n"] >> L) * (-(-lh // tr) * tr) * (-(-lw // tc) * tc) * bpp <= \
                vc.FUZZ_LEVEL_BYTES
        for p in vc.fuzz_tiled_classes(c):
            if p in count:
                count[p] += 1
    short = {k: v for k, v in count.items() if v < 4}
    assert not short, f"classes with fewer than 4 of 96 cases: {short} (all: {count})"


def test_chunked_fuzz_cases_are_accepted_and_cover_every_class():
    assert vc.N_FUZZ_CHUNKED == 32
    count = dict.fromkeys(CHUNKED_CLASSES, 0)
    for i in range(vc.N_FUZZ_CHUNKED):
        c = vc.fuzz_chunked_params(i)
        check_pyramid(c)
        assert 2 <= c["levels"] <= 5
        assert c["first"] % (1 << (c["levels"] - 1)) == 0
        assert all(min(s) >= 1 for s in c["shapes"][1:])
        for p in vc.fuzz_chunked_classes(c):
            count[p] += 1
    short = {k: v for k, v in count.items() if v < 2}
    assert not short, f"classes with fewer than 2 of 32 cases: {short} (all: {count})"


def test_generators_are_deterministic():
    a, b = vc.fuzz_tiled_params(7), vc.fuzz_tiled_params(7)
    assert (a["w"], a["h"], a["tiles"], a["out_off"]) == (b["w"], b["h"], b["tiles"], b["out_off"])
