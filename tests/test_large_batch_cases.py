"""CPU: what tests/test_gpu_large_batch.py rests on, for every case of
tests/large_batch.py's table.

* The shift rule on the oracle, for the case's geometry, dtype and method, at
  tags 0, 1, M / 2 and M - 1, at every level (one plane group per tag, all in
  one stream, so groups are shown not to leak into each other either).
* What each case crosses: shallow cases hold at least 2 whole input frames
  wholly past byte offset 2^32, deep cases at least 2 whole level-1 output
  frames (for u8 that is element 2^32 too) and an input of more than 2^32
  elements.
* Aliasing: a frame 2^31 or 2^32 bytes or elements away, at the input and at
  every level, never carries the same tag.
* The planner's limits: the planner itself (tests/cpp/plan_probe.cpp) takes
  every case at its full frame count with units under its limit, volumes are
  whole stacks, and the generic case is one the cascade planner refuses.
* Chunk-tiled cases: the tiles and zero-scan flags of E + tag are those of
  tag 0 plus tag on the level's own elements, for every tag above 0.
"""
import numpy as np
import pytest

import large_batch as lb

IDS = [c.id for c in lb.CASES]


def test_table_is_what_the_issue_lists():
    fam = lambda f, d=None: len(lb.select(f, d))
    assert fam("row", "shallow") == 13 * 3 * 2
    assert fam("volume", "shallow") == 4 * 3 * 2
    assert fam("row", "deep") + fam("volume", "deep") == 5
    assert [c.kind for c in lb.CASES].count(3) == 1
    assert fam("zpath") == 1 and fam("tiled") == 4 and fam("lattice") == 1
    # tiled volumes: two shapes x (u8, u16, f32 Mean; u16 Decimate), one deep, one lattice
    assert fam("volume_tiled", "shallow") == 2 * 4 and fam("volume_tiled", "deep") == 1
    assert sorted((np.dtype(c.dtype).name, c.method) for c in lb.select("volume_tiled", "shallow")
                  if c.tile == lb.COLUMN_FILL_TILE) == \
        [("float32", 1), ("uint16", 0), ("uint16", 1), ("uint8", 1)]
    assert fam("volume_lattice") == 1 and all(c.kind == 5 for c in lb.select("volume_tiled"))
    assert len(set(IDS)) == len(IDS)


def test_moduli_are_the_largest_primes():
    assert lb.modulus(np.uint8) == 251
    assert lb.modulus(np.float32) == 1021
    m = lb.modulus(np.uint16)
    assert m <= 65535 - 4095 and m == lb.largest_prime_at_most(61440) == 61417
    for dt in (np.uint8, np.uint16):
        name = np.dtype(dt).name
        assert lb.BASE_MAX[name] + lb.modulus(dt) - 1 <= lb.DTYPE_MAX[name]
    # float32: every intermediate of a Mean over up to 6 levels is an integer
    # sum of 4 values below 1024 + 1021, far under 2^24
    assert 4 * (lb.BASE_MAX["float32"] + lb.modulus(np.float32)) < 1 << 24


def test_lattice_geometry_is_the_planners(oracle):
    assert lb.LATTICE_GEO == oracle.level_geometry(oracle.plan_levels(lb.LATTICE_DIMS))


_SHIFT_DONE = {}


@pytest.mark.parametrize("cid", IDS)
def test_shift_rule_on_the_oracle(oracle, cid):
    case = lb.BY_ID[cid]
    key = (case.family, case.name, np.dtype(case.dtype).name, case.method)
    if key in _SHIFT_DONE:      # a deep case shares its shallow twin's run
        assert _SHIFT_DONE[key]
        return
    _SHIFT_DONE[key] = False
    base = lb.base_group(case)
    assert base.max() <= lb.BASE_MAX[np.dtype(case.dtype).name] and base.min() >= 0
    if np.dtype(case.dtype).kind == "f":
        assert np.array_equal(base, np.floor(base))
    e = lb.expected_levels(oracle, case)
    tags = lb.cpu_tags(case)
    assert tags[0] == 0 and tags[1] == 1 and tags[-1] == lb.modulus(case.dtype) - 1
    got = lb.oracle_levels(oracle, case, [base + np.asarray(t, case.dtype) for t in tags])
    ut = np.dtype(f"u{np.dtype(case.dtype).itemsize}")
    for L in range(1, len(case.geo)):
        per = lb.per_group(case, L)
        assert got[L].shape[0] == per * len(tags)
        for i, t in enumerate(tags):
            want = e[L] + np.asarray(t, case.dtype)
            assert np.array_equal(got[L][i * per:(i + 1) * per].view(ut), want.view(ut)), \
                f"{cid} level {L} tag {t}"
    _SHIFT_DONE[key] = True


@pytest.mark.parametrize("cid", IDS)
def test_what_the_case_crosses(cid):
    case = lb.BY_ID[cid]
    n = lb.frames_for(case)
    four = 1 << 32
    assert n % max(1, case.geo[0][2]) == 0 and n % lb.group_planes(case) == 0

    def whole_frames_past(level, size):
        """Frames of the level that start at or past `size` bytes."""
        fb = lb.frame_bytes(case, level)
        return lb.level_frames(case, level, n) - -(-size // fb)

    if case.depth == "shallow":
        assert whole_frames_past(0, four) >= 2
    else:
        assert whole_frames_past(1, four) >= 2
        if lb.bpp(case) == 1:
            assert lb.level_frames(case, 1, n) * lb.frame_elems(case, 1) > four
        assert n * lb.frame_elems(case, 0) > four
    if case.family == "lattice":
        assert n % lb.LATTICE_DIMS[0][2] == 0          # whole chunk layers: no byte unowned
        assert n * lb.frame_bytes(case, 1) > four      # level 1's capacity
    if case.family == "volume_lattice":
        for L in range(1, len(case.geo)):              # whole chunk layers at every level
            assert (n >> L) % lb.VOLUME_LATTICE_SHAPES[L][0] == 0
        assert (n >> 1) * lb.frame_bytes(case, 1) > four   # level 1's capacity
    if case.family in ("volume_tiled", "volume_lattice"):
        assert [lb.level_frames(case, L, n) for L in range(len(case.geo))] == \
            [n >> L for L in range(len(case.geo))]
    assert lb.need_bytes(case) > n * lb.frame_bytes(case, 0)


@pytest.mark.parametrize("cid", IDS)
def test_truncated_offsets_never_alias(cid):
    """A frame `size / frame_size` frames away carries another tag: the
    distance is not whole, or not whole plane groups (another plane of the
    base group then), or not a multiple of M groups."""
    case = lb.BY_ID[cid]
    m = lb.modulus(case.dtype)
    assert m > 2 and lb.largest_prime_at_most(m) == m
    for L in range(len(case.geo)):
        per = lb.group_planes(case) if L == 0 else lb.per_group(case, L)
        for size in (1 << 31, 1 << 32):
            for fs in (lb.frame_bytes(case, L), lb.frame_elems(case, L)):
                d, r = divmod(size, fs)
                assert r != 0 or d % per != 0 or (d // per) % m != 0, (cid, L, size, fs)


DTYPE_CODE = {"uint8": 0, "uint16": 1, "float32": 8}


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    from test_launch_plan_limits import build_probe
    return build_probe(tmp_path_factory.mktemp("plan_probe_large"))


def plan_request(case, n):
    """The first fused run of the case at n frames, as tests/cpp/plan_probe.cpp
    reads it (tests/test_launch_plan.py asks for the small cases the same way)."""
    w, h, _ = case.geo[0]
    code, nl = DTYPE_CODE[np.dtype(case.dtype).name], len(case.geo)
    if case.family == "volume":
        return f"volume {code} {case.method} {w} {h} {min(2, nl - 1)} {n}"
    if case.tile:
        tr, tc = case.tile
        return (f"tiled {code} {case.method} {w} {h} {min(4, nl - 1)} {n} tile={tr}x{tc} "
                f"flags={int(case.family == 'tiled')}")
    return f"cascade {code} {case.method} {w} {h} {min(4, nl - 1)} {n}"


VOLUME_TILED_IDS = [c.id for c in lb.CASES if c.family in ("volume_tiled", "volume_lattice")]


@pytest.mark.parametrize("cid", [i for i in IDS if i not in VOLUME_TILED_IDS])
def test_units_stay_under_the_planner_limits(ask, cid):
    """The planner (ds_plan.cpp, through plan_probe) takes each case at its
    full frame count: the plan is valid, its units are the one-frame units
    times the frames (plane groups) and stay under the limit it refuses at,
    and its grid covers them.  The generic case is the one the cascade
    planner refuses, at every level; the per-frame Z path plans one frame at
    a time."""
    import launch_rule_child as child
    case = lb.BY_ID[cid]
    n = lb.frames_for(case)
    assert n < 1 << 32
    if case.family == "zpath":
        assert case.kind == 0
        return
    if case.kind == 3:
        code = DTYPE_CODE[np.dtype(case.dtype).name]
        reqs = [plan_request(case, 1), plan_request(case, n)]
        for (w, h, _) in case.geo[:-1]:       # level by level too: no run of any length fits
            reqs.append(f"cascade {code} {case.method} {w} {h} 1 {n}")
        assert ask(reqs) == [None] * len(reqs)
        return
    step = lb.group_planes(case)
    one, full = ask([plan_request(case, step), plan_request(case, n)])
    assert one is not None and full is not None, (cid, one, full)
    limit = 1 << 30 if case.tile else 1 << 31
    assert full["units"] == one["units"] * (n // step) < limit
    assert full["dtype"] == lb.bpp(case)
    assert not child.check_launch(full), (child.check_launch(full), full)
    if case.family == "volume":
        assert n % (1 << (len(case.geo) - 1)) == 0 and n % case.geo[0][2] == 0


@pytest.fixture(scope="module")
def ask_volume_tiled():
    """plan_volume_tiled through tests/cpp/volume_tiled_plan_probe.cpp."""
    import volume_tiled_cases as vc
    return vc.plan_probe()


@pytest.mark.parametrize("cid", VOLUME_TILED_IDS)
def test_volume_tiled_plans_at_full_length(ask_volume_tiled, cid):
    """plan_volume_tiled takes each case at its full plane count: units are
    the one-group units times the plane groups, under 2^31; the zero-fill
    items, zitems x groups, which the kernel multiplies in 32 bits, stay under
    2^32; every case has padding the units do not reach."""
    import launch_rule_child as child
    case = lb.BY_ID[cid]
    n = lb.frames_for(case)
    gp = lb.group_planes(case)
    assert len(case.geo) == 3 and gp == 4 and n % gp == 0 and n < 1 << 32
    w, h, _ = case.geo[0]
    (r1, c1), (r2, c2) = lb.tile_of(case, 1), lb.tile_of(case, 2)
    extra = ""
    if case.family == "volume_lattice":
        extra = f" stride={lb.VOLUME_LATTICE_SHAPES[1][0] * r1 * c1} flags=0"
        assert lb.VOLUME_LATTICE_SHAPES[1][0] * r1 * c1 >= lb.VOLUME_LATTICE_SHAPES[2][0] * r2 * c2
    req = (f"{DTYPE_CODE[np.dtype(case.dtype).name]} {case.method} {w} {h} 2 {{}} "
           f"tile={r1}x{c1} tile2={r2}x{c2}{extra}")
    one, full = ask_volume_tiled([req.format(gp), req.format(n)])
    assert one is not None and full is not None, (cid, one, full)
    groups = n // gp
    assert full["units"] == one["units"] * groups < 1 << 31
    assert full["zitems"] == one["zitems"] > 0 and full["zitems"] * groups < 1 << 32
    assert full["zwaves"] > 0 and full["dtype"] == lb.bpp(case)
    assert not child.check_launch(full), (child.check_launch(full), full)
    for L in (1, 2):
        assert full[f"pw{L}"] * full[f"ph{L}"] == lb.frame_elems(case, L)
    if case.tile == lb.COLUMN_FILL_TILE:    # columns past cov_w, at level 2 for every dtype
        assert full["cov_w2"] < full["pw2"] and full["zrows2"] == full["ph2"]
        assert (full["cov_w1"] < full["pw1"]) == (lb.bpp(case) > 1)
    else:                                   # rows past cov_h
        assert full["cov_w1"] >= full["pw1"] and full["cov_h1"] < full["ph1"]
    if case.depth == "deep" and case.family == "volume_tiled":
        assert lb.frame_bytes(case, 1) == 4096 and 2 * lb.frame_bytes(case, 0) == 2 * 2880


@pytest.mark.parametrize("cid", [c.id for c in lb.CASES if c.tile])
def test_tiles_of_a_tagged_frame(oracle, cid):
    """tile_frame(E + t) = tile_frame(E) + t on the level's own elements and 0
    on the overhang, with every tile flagged nonzero, for every t > 0: shown
    for the tag the GPU test computes (1) against two more; tag 0 keeps whole
    zero tiles.  For float32 both sides come from the same float addition, so
    the values prove little there (that E + t is exact in float32 is
    test_shift_rule_on_the_oracle's to show); what this still holds for floats
    is the tiling: which elements of the padded tiles are the level's own
    (`inside`), that the overhang stays zero, and the flags."""
    case = lb.BY_ID[cid]
    e = lb.expected_levels(oracle, case)
    m = lb.modulus(case.dtype)
    for L in range(1, len(case.geo)):
        for j in range(lb.per_group(case, L)):    # every plane a group emits at the level
            t0, f0 = lb.tiled_expectation(oracle, case, L, e[L][j], 0)
            t1, f1 = lb.tiled_expectation(oracle, case, L, e[L][j], 1)
            inside = t1 != t0
            assert f1.all(), f"{cid} level {L}: a tile without an element of the level"
            # (one 64 x 64 or 2 x 384 tile holds more than the zero quarter)
            if L == 1 and (case.family == "tiled" or case.tile == lb.VOLUME_TILED_TILE):
                assert (~f0).any() and f0.any(), f"{cid}: no whole zero tile under tag 0"
            for t in (m // 2, m - 1):
                tt, ft = lb.tiled_expectation(oracle, case, L, e[L][j], t)
                assert np.array_equal(tt, t0 + inside.astype(case.dtype) *
                                      np.asarray(t, case.dtype))
                assert np.array_equal(ft, f1)


def test_crc_of_parts_is_the_oracles(oracle):
    """tests/test_gpu_large_codecs.py checksums a GiB through the oracle in
    16 parts; the combination equals the oracle's checksum of the whole."""
    rng = np.random.default_rng(32)
    for n in (0, 1, 15, 16, 17, 1000, 65535 * 3 + 1, 1 << 20):
        buf = rng.integers(0, 256, n, dtype=np.uint8)
        assert lb.oracle_crc32c_parts(oracle, buf) == oracle.crc32c(buf), n
        for cut in (0, n // 3, n):
            assert lb.crc32c_combine(oracle.crc32c(buf[:cut]), oracle.crc32c(buf[cut:]),
                                     n - cut) == oracle.crc32c(buf), (n, cut)
