"""Shared pieces of the volume tiled tests (not a test module, not a conftest):
the cases, the volume geometry, and the expected bytes — always the oracle
pyramid (oracle.OracleDownsampler), tiled by oracle.tile_frame and placed by
oracle.chunk_frame_offsets, never the product's."""
import zlib

import numpy as np

from gpu_util import (assert_parity, empty_device, from_device, launch_stream, random_frames,
                      to_device)

SPACE, CHANNEL, TIME = 0, 1, 2
POISON = 0xA5

# A volume unit is 64 lanes x (16 / bytes per pixel) columns x 2^k rows x 2^k
# planes for a run of k <= 2 levels; these are the smallest shapes that reach
# each path.
# (w, h, planes, levels, dtype, tile_rows, tile_cols, volumes)
CASES = [
    (512, 8, 4, 3, np.uint16, 2, 128, 1),    # one interior unit, no edge, no overhang
    (64, 48, 4, 3, np.uint16, 16, 16, 2),    # a lone edge unit; two plane groups
    (1030, 37, 4, 3, np.uint8, 8, 64, 1),    # interior + 6-column edge unit; odd W, H twice
    (520, 22, 8, 3, np.float32, 5, 25, 1),   # 2 interior units + 8-column edge; lanes cross tiles
    (130, 10, 2, 2, np.int64, 4, 16, 3),     # a run of one level; 8-byte type
    (264, 24, 8, 4, np.uint8, 4, 16, 1),     # chained runs 2 + 1; second source 66 px from scratch
    (600, 40, 16, 5, np.uint16, 8, 32, 1),   # two chained runs of two levels
]


def case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}_L{c[3]}_{np.dtype(c[4]).name}_{c[5]}x{c[6]}"


def volume_geo(w, h, planes, levels):
    """(width, height, planes) per level of a pyramid halving X, Y and Z."""
    geo = [(w, h, planes)]
    for _ in range(1, levels):
        w, h, planes = (w + 1) // 2, (h + 1) // 2, planes // 2
        geo.append((w, h, planes))
    return geo


def zero_strip(w, levels, tile_cols):
    """Columns of the left-hand strip that, zeroed over the full height of a
    plane group, leaves whole zero tiles at every level that has more than one
    tile column: one tile wide at the deepest such level."""
    for l in range(levels - 1, 0, -1):
        if (tile_cols << l) < w:
            return tile_cols << l
    return max(w // 2, 1)


def case_frames(case, seed=None, specials=False):
    """The case's planes: random, the top left corner (zero_strip wide, the
    full height) zero through all planes of the first plane group, so that
    zero tiles exist at every level with more than one tile column."""
    w, h, planes, levels, dtype, _, tc, volumes = case
    rng = np.random.default_rng(w * 7919 + h if seed is None else seed)
    frames = random_frames(rng, dtype, (planes * volumes, h, w), specials=specials)
    frames[frames == 0] = 1  # no other zero tile by chance
    frames[: 1 << (levels - 1), :, : zero_strip(w, levels, tc)] = 0
    return frames


def oracle_planes(oracle, geo, dtype, method, frames):
    """planes[L] = every plane level L emits for `frames`, in order."""
    ref = oracle.OracleDownsampler(geo, dtype, method)
    out = [[] for _ in geo]
    for fr in frames:
        ref.add_frame(fr)
        for L in range(1, len(geo)):
            p = ref.take_frame(L)
            if p is not None:
                out[L].append(p)
    for L in range(1, len(geo)):
        assert len(out[L]) == len(frames) >> L, (L, len(out[L]))
    return out


def expected_tiled(oracle, planes, tiles):
    """Per level (tiles[n, n_tiles, tr, tc], nonzero[n, n_tiles] bool)."""
    want = [None]
    for L in range(1, len(planes)):
        tr, tc = tiles[L]
        t = [oracle.tile_frame(p, tr, tc) for p in planes[L]]
        want.append((np.stack([a for a, _ in t]), np.stack([b for _, b in t])))
    return want


def n_tiles(geo, L, tile):
    w, h, _ = geo[L]
    return (-(-h // tile[0])) * (-(-w // tile[1]))


# ---- chunk lattice -----------------------------------------------------------

# Level 1 is Z/Y/X = 4 x 24 x 32 u16 in chunks of 2 x 16 x 16 (ragged in Y, two
# layers); level 2 is 2 x 12 x 16 in chunks of 2 x 8 x 16.
CHUNK_GEO = volume_geo(64, 48, 8, 3)
CHUNK_SHAPES = [None, (2, 16, 16), (2, 8, 16)]  # (z, y, x) chunk per level


def chunk_dims(L, geo=CHUNK_GEO, shapes=CHUNK_SHAPES):
    """Level L as an array appended along Z."""
    w, h, _ = geo[L]
    cz, cy, cx = shapes[L]
    return [(SPACE, 0, cz, 1), (SPACE, h, cy, 1), (SPACE, w, cx, 1)]


def expected_chunked(oracle, planes, first, dtype, geo=CHUNK_GEO, shapes=CHUNK_SHAPES):
    """Per level (buffer bytes with poison where no plane writes, offsets,
    chunk_bytes, layer_bytes, capacity) for a batch whose level-0 planes start
    at plane `first` of the stack."""
    bpp = np.dtype(dtype).itemsize
    out = [None]
    for L in range(1, len(geo)):
        _, cy, cx = shapes[L]
        n = len(planes[L])
        offs, cb, lb = oracle.chunk_frame_offsets(chunk_dims(L, geo, shapes), bpp, first >> L, n)
        cap = (max(offs) // lb + 1) * lb
        buf = np.full(cap, POISON, np.uint8)
        tb = cy * cx * bpp
        for k, p in enumerate(planes[L]):
            tiles, _ = oracle.tile_frame(p, cy, cx)
            at = offs[k] + np.arange(tiles.shape[0], dtype=np.int64)[:, None] * cb
            buf[at + np.arange(tb, dtype=np.int64)[None, :]] = \
                tiles.view(np.uint8).reshape(tiles.shape[0], tb)
        out.append((buf, offs, cb, lb, cap))
    return out


# ---- the branches of the tiled volume kernel -----------------------------------

DECIMATE, MEAN = 0, 1

# Shapes for branches CASES does not reach, with the methods each runs under
# and the property (properties_of) that test_volume_tiled_fuzz_cases.py holds
# it to, so that an edit cannot turn one into a duplicate of another.
BRANCH_CASES = [
    # cov_w < pw at both levels (256 < 384, 128 < 384), interior units only,
    # two plane groups: the zero-fill's plane / row split with zrows == ph
    ((512, 8, 4, 3, np.uint16, 2, 384, 2), (MEAN,), "column_fill_both_levels"),
    # level 1 is covered (256 >= 200), level 2 is not (128 < 200)
    ((260, 12, 4, 3, np.float32, 3, 200, 1), (MEAN,), "column_fill_second_level_only"),
    # a lane's 8 / 4 columns cross tile edges, on edge units, ragged rows
    ((1030, 37, 4, 3, np.uint8, 8, 7, 1), (MEAN, DECIMATE), "crossing_co_8_4"),
    ((1030, 37, 4, 3, np.uint8, 5, 13, 1), (MEAN, DECIMATE), "crossing_co_8_4"),
    ((520, 22, 8, 3, np.uint16, 5, 25, 1), (MEAN,), "crossing_co_4_2"),
    # three chained runs of two levels: both halves of the chain scratch
    ((600, 40, 64, 7, np.uint16, 8, 32, 1), (MEAN,), "three_runs"),
    ((520, 22, 8, 3, np.float32, 64, 512, 1), (MEAN,), "one_tile_a_level"),
    ((64, 48, 4, 3, np.uint16, 1, 1, 1), (MEAN,), "one_pixel_tiles"),
]
# the cases of the element-offset test, by what they reach: column zero-fill
# at the second level, lane columns across tile edges for a 2-byte type, and
# the three chained runs (six tile outputs, each at an offset of its own)
OFFSET_CASES = [c for c, _, name in BRANCH_CASES
                if name in ("column_fill_second_level_only", "crossing_co_4_2", "three_runs")]


def level_geometry(w, h, levels, dtype, tiles):
    """What plan_volume_tiled derives for every level L >= 1, from the
    arithmetic alone: runs of up to two levels, a unit of 64 lanes x 16 / bpp
    columns x 2^k rows, `j` the level's place in its run (1 or 2)."""
    bpp = np.dtype(dtype).itemsize
    cols = 64 * (16 // bpp)
    out, L, run = [None], 1, 0
    while L < levels:
        k = min(levels - L, 2)
        ux, uy = -(-w // cols), -(-h // (1 << k))
        lw, lh = w, h
        for j in range(1, k + 1):
            lw, lh = (lw + 1) // 2, (lh + 1) // 2
            tr, tc = tiles[L + j - 1]
            out.append(dict(run=run, j=j, k=k, src_w=w, src_h=h, w=lw, h=lh, tr=tr, tc=tc,
                            units_x=ux, units_y=uy,
                            cov_w=ux * (cols >> j), cov_h=uy * ((1 << k) >> j),
                            pw=-(-lw // tc) * tc, ph=-(-lh // tr) * tr,
                            co=max((16 // bpp) >> j, 1),
                            interior=w >= cols and h >= (1 << k),
                            edge=w % cols != 0 or h % (1 << k) != 0))
        w, h = lw, lh
        L += k
        run += 1
    return out


def properties_of(w, h, levels, dtype, tiles):
    """The named branches a shape reaches, from level_geometry."""
    g = level_geometry(w, h, levels, dtype, tiles)[1:]
    props = set()
    for q in g:
        if q["cov_w"] < q["pw"]:
            props.add(f"column_fill_level_{q['j']}_of_run")
            if q["ph"] > 1:
                props.add("column_fill_many_rows")
        if q["cov_h"] < q["ph"]:
            props.add("row_fill")
        if q["tc"] % q["co"] != 0:
            props.add(f"crossing_co_{q['co']}")
        if q["tc"] > q["w"]:
            props.add("tile_wider_than_level")
        props.add("interior_and_edge_units" if q["interior"] and q["edge"] else
                  "edge_units_only" if not q["interior"] else "interior_units_only")
    props.add(f"runs_{g[-1]['run'] + 1}")
    return props


def case_tiles(case):
    return [None] + [(case[5], case[6])] * (case[3] - 1)


def case_properties(case):
    w, h, _, levels, dtype, _, _, _ = case
    return properties_of(w, h, levels, dtype, case_tiles(case))


# ---- seeded fuzz ----------------------------------------------------------------

DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16,
          np.int32, np.int64, np.float32, np.float64]
FUZZ_INPUT_BYTES = 16 << 20
# a padded level (tiles, or lattice capacity) is held to this as well: a
# 300-row tile over a one-row level would otherwise be 300 times its level
FUZZ_LEVEL_BYTES = 16 << 20
N_FUZZ_TILED, N_FUZZ_CHUNKED = 96, 32


def fuzz_wmin(bpp, levels):
    """The smallest width whose run sources (levels 0, 2, 4) hold one 16-byte
    load and whose every level is strictly narrower than the one before."""
    w = 1
    while True:
        ws = [w]
        for _ in range(1, levels):
            ws.append((ws[-1] + 1) // 2)
        if all(ws[L] >= 16 // bpp for L in (0, 2, 4) if L < levels - 1) and \
                all(ws[L] < ws[L - 1] for L in range(1, levels)):
            return w
        w += 1


def _fuzz_side(rng):
    if rng.random() < 0.4:
        return int(rng.choice([16, 32, 64, 128, 256]))
    return int(np.exp(rng.uniform(0, np.log(300))))


def _fuzz_pyramid(rng, level_weights):
    """dtype, method, levels, w, h, planes per stack, stacks: the input held
    to FUZZ_INPUT_BYTES by lowering the multipliers first, then the height."""
    weights = np.array([3, 6, 1, 1, 1, 1, 1, 1, 4, 1], dtype=float)
    dtype = DTYPES[int(rng.choice(len(DTYPES), p=weights / weights.sum()))]
    method = int(rng.integers(4))
    lv = np.array(level_weights, dtype=float)
    levels = 2 + int(rng.choice(len(lv), p=lv / lv.sum()))
    bpp = np.dtype(dtype).itemsize
    w = int(np.exp(rng.uniform(np.log(fuzz_wmin(bpp, levels)), np.log(2500))))
    h = int(rng.integers(1, 49))
    mult = int(rng.integers(1, 4))
    stacks = int(rng.integers(1, 3))
    unit = 1 << (levels - 1)
    while w * h * unit * mult * stacks * bpp > FUZZ_INPUT_BYTES and (mult > 1 or stacks > 1):
        if stacks > 1:
            stacks -= 1
        else:
            mult -= 1
    while w * h * unit * mult * stacks * bpp > FUZZ_INPUT_BYTES:
        h -= 1
    return dtype, method, levels, w, h, unit * mult, stacks


def fuzz_tiled_params(i):
    """Case i of test_fuzz_volume_tiled."""
    rng = np.random.default_rng(zlib.crc32(f"fuzz-volume-tiled{i}".encode()))
    dtype, method, levels, w, h, planes, stacks = _fuzz_pyramid(rng, [2, 5, 5, 4, 2, 2])
    bpp = np.dtype(dtype).itemsize
    geo = volume_geo(w, h, planes, levels)
    n = planes * stacks
    tiles = [None]
    for L in range(1, levels):
        lw, lh, _ = geo[L]
        tr, tc = _fuzz_side(rng), _fuzz_side(rng)
        if rng.random() < 0.15:
            tc = lw + int(rng.integers(1, 65))
        # hold the padded level to FUZZ_LEVEL_BYTES: halve the side that overhangs more
        while (n >> L) * (-(-lh // tr) * tr) * (-(-lw // tc) * tc) * bpp > FUZZ_LEVEL_BYTES:
            if -(-lh // tr) * tr * lw >= -(-lw // tc) * tc * lh and tr > 1:
                tr = (tr + 1) // 2
            else:
                tc = (tc + 1) // 2
        tiles.append((tr, tc))
    return dict(dtype=dtype, method=method, levels=levels, w=w, h=h, planes=planes,
                stacks=stacks, n=n, geo=geo, tiles=tiles,
                in_off=int(rng.integers(0, 8)),
                out_off=[0] + [int(rng.integers(0, 8)) for _ in range(1, levels)],
                flags=bool(rng.random() < 0.75), rng=rng)


def fuzz_chunked_params(i):
    """Case i of test_fuzz_volume_chunked: a Z/Y/X chunk shape per level and a
    batch that starts `first` planes into the stack."""
    rng = np.random.default_rng(zlib.crc32(f"fuzz-volume-chunked{i}".encode()))
    dtype, method, levels, w, h, planes, stacks = _fuzz_pyramid(rng, [1, 1, 1, 1])
    bpp = np.dtype(dtype).itemsize
    geo = volume_geo(w, h, planes, levels)
    n = planes * stacks
    first = (1 << (levels - 1)) * int(rng.integers(0, 4))
    shapes = [None]
    for L in range(1, levels):
        lw, lh, _ = geo[L]
        cz, cy, cx = int(rng.integers(1, 5)), _fuzz_side(rng), _fuzz_side(rng)
        # the lattice holds whole layers of cz planes: capacity within FUZZ_LEVEL_BYTES
        while ((n >> L) + 2 * cz) * (-(-lh // cy) * cy) * (-(-lw // cx) * cx) * bpp > \
                FUZZ_LEVEL_BYTES:
            if -(-lh // cy) * cy * lw >= -(-lw // cx) * cx * lh and cy > 1:
                cy = (cy + 1) // 2
            else:
                cx = (cx + 1) // 2
        shapes.append((cz, cy, cx))
    return dict(dtype=dtype, method=method, levels=levels, w=w, h=h, planes=planes,
                stacks=stacks, n=n, geo=geo, shapes=shapes, first=first,
                in_off=int(rng.integers(0, 8)), flags=bool(rng.random() < 0.75), rng=rng)


def fuzz_zero_strip(w, tile_cols):
    """zero_strip for a tile width per level (tile_cols[L], L >= 1)."""
    for l in range(len(tile_cols) - 1, 0, -1):
        if (tile_cols[l] << l) < w:
            return tile_cols[l] << l
    return max(w // 2, 1)


def fuzz_frames(c, tile_cols):
    """The case's planes: random with the float edge values, the left strip of
    the first plane group zero (case_frames' rule), so zero tiles exist."""
    frames = random_frames(c["rng"], c["dtype"], (c["n"], c["h"], c["w"]))
    frames[: 1 << (c["levels"] - 1), :, : fuzz_zero_strip(c["w"], tile_cols)] = 0
    return frames


def fuzz_tiled_classes(c):
    props = properties_of(c["w"], c["h"], c["levels"], c["dtype"], c["tiles"])
    if c["in_off"]:
        props.add("input_offset")
    if not c["flags"]:
        props.add("no_flags")
    return props


def fuzz_chunked_classes(c):
    props = set()
    if c["levels"] > 3:
        props.add("chained")
    if c["first"]:
        props.add("first_nonzero")
    for L in range(1, c["levels"]):
        lw, lh, _ = c["geo"][L]
        if lw % c["shapes"][L][2]:
            props.add("ragged_x")
        if lh % c["shapes"][L][1]:
            props.add("ragged_y")
    return props


# ---- device buffers of the GPU tests (torch is loaded at the first use) ------------

GUARD = 64  # poisoned bytes behind every buffer, checked after the run


def offset_input(frames, off=0):
    """The planes on the device `off` elements into a poisoned buffer, with
    guard bytes behind: (tensor, address of the first plane)."""
    bpp = frames.dtype.itemsize
    raw = np.full(off * bpp + frames.nbytes + GUARD, POISON, np.uint8)
    raw[off * bpp: off * bpp + frames.nbytes] = frames.view(np.uint8).reshape(-1)
    d = to_device(raw)
    return d, d.data_ptr() + off * bpp


class Outputs:
    """Poisoned tile and flag buffers of one batch of `n` level-0 planes.
    Level L's tiles start `offs[L]` elements into their buffer; every buffer
    ends in GUARD bytes, and check() wants the bytes in front and the guards
    still poisoned."""

    def __init__(self, geo, dtype, tiles, n, with_flags=True, offs=None):
        bpp = np.dtype(dtype).itemsize
        self.geo, self.dtype, self.tiles, self.n = geo, dtype, tiles, n
        self.offs = [0] * len(geo) if offs is None else offs
        self.nt = [None] + [n_tiles(geo, L, tiles[L]) for L in range(1, len(geo))]
        self.nbytes = [None] + [(n >> L) * self.nt[L] * tiles[L][0] * tiles[L][1] * bpp
                                for L in range(1, len(geo))]
        self.outs = [None] + [empty_device(self.offs[L] * bpp + self.nbytes[L] + GUARD)
                              for L in range(1, len(geo))]
        self.flags = [None] + [empty_device((n >> L) * self.nt[L] + GUARD) if with_flags else None
                               for L in range(1, len(geo))]
        self.poison()

    def poison(self):
        for b in self.outs[1:] + self.flags[1:]:
            if b is not None:
                b.fill_(POISON)

    def out_ptrs(self):
        bpp = np.dtype(self.dtype).itemsize
        return [0] + [o.data_ptr() + self.offs[L] * bpp for L, o in enumerate(self.outs) if L]

    def flag_ptrs(self):
        if self.flags[1] is None:
            return None
        return [0] + [f.data_ptr() for f in self.flags[1:]]

    def run(self, ds, d_in, stream=None):
        src = d_in if isinstance(d_in, int) else d_in.data_ptr()
        return ds.run_device_volume_tiled(
            src, self.n, self.tiles, self.out_ptrs(), self.flag_ptrs(),
            launch_stream() if stream is None else stream)

    def check(self, want, ctx):
        bpp = np.dtype(self.dtype).itemsize
        for L in range(1, len(self.geo)):
            tr, tc = self.tiles[L]
            want_t, want_nz = want[L]
            raw = from_device(self.outs[L], np.uint8, (-1,))
            at = self.offs[L] * bpp
            assert (raw[:at] == POISON).all(), f"{ctx} L{L}: bytes in front of the tiles written"
            assert (raw[at + self.nbytes[L]:] == POISON).all(), f"{ctx} L{L}: guard bytes written"
            got = raw[at: at + self.nbytes[L]].view(self.dtype).reshape(
                self.n >> L, self.nt[L], tr, tc)
            assert_parity(got, want_t, f"{ctx} L{L} tiles")
            if np.dtype(self.dtype).kind == "f":  # equal bits on every non-NaN value
                ib = np.dtype(f"u{bpp}")
                ok = ~np.isnan(want_t)
                assert np.array_equal(got.view(ib)[ok], want_t.view(ib)[ok]), f"{ctx} L{L} bits"
            if self.flags[L] is not None:
                raw = from_device(self.flags[L], np.uint8, (-1,))
                assert (raw[-GUARD:] == POISON).all(), f"{ctx} L{L}: flag guard bytes written"
                raw = raw[:-GUARD].reshape(self.n >> L, self.nt[L])
                assert np.isin(raw, (0, 1)).all(), f"{ctx} L{L}: a flag byte was left unwritten"
                assert np.array_equal(raw.astype(bool), want_nz), f"{ctx} L{L} zero scan"


class Lattice:
    """One chunked batch: the planes from `first` planes into the stack, a
    poisoned lattice buffer and flag buffer per level (GUARD bytes behind
    each), expected bytes from the oracle pyramid at the oracle's places.
    `room[L]`: allocate at least that many lattice bytes at level L, so that a
    batch run with another batch's offset table would still write inside its
    buffer, where the comparison finds it."""

    def __init__(self, oracle, geo, shapes, dtype, method, frames, first, with_flags=True,
                 in_off=0, room=None):
        self.geo, self.shapes, self.n = geo, shapes, len(frames)
        self.lv = oracle_planes(oracle, geo, dtype, method, frames)
        self.want = expected_chunked(oracle, self.lv, first, dtype, geo, shapes)
        self.d_in, self.src = offset_input(frames, in_off)
        levels = range(1, len(geo))
        self.bufs = [None] + [empty_device(max(self.want[L][4], room[L] if room else 0) + GUARD)
                              for L in levels]
        self.nt = [None] + [n_tiles(geo, L, shapes[L][1:]) for L in levels]
        self.flags = [None] + [empty_device((self.n >> L) * self.nt[L] + GUARD) if with_flags
                               else None for L in levels]
        for b in self.bufs[1:] + self.flags[1:]:
            if b is not None:
                b.fill_(POISON)

    def run(self, ds, stream):
        lats = [None]
        for L in range(1, len(self.geo)):
            _, offs, cb, _, cap = self.want[L]
            _, cy, cx = self.shapes[L]
            lats.append((self.bufs[L].data_ptr(), cap, cy, cx, cb, offs))
        flags = None
        if self.flags[1] is not None:
            flags = [0] + [f.data_ptr() for f in self.flags[1:]]
        return ds.run_device_volume_chunked(self.src, self.n, lats, flags, stream)

    def check(self, oracle, ctx):
        """Every lattice byte: tiles where a plane owns them, poison elsewhere
        and in the guards; flags exactly 0 or 1."""
        for L in range(1, len(self.geo)):
            got = from_device(self.bufs[L], np.uint8, (-1,))
            cap = self.want[L][4]
            assert (got[cap:] == POISON).all(), f"{ctx} L{L}: bytes past the lattice written"
            bad = np.flatnonzero(got[:cap] != self.want[L][0])
            assert bad.size == 0, f"{ctx} L{L}: {bad.size} bytes differ, first at {bad[0]}"
            if self.flags[L] is not None:
                nz = np.stack([oracle.tile_frame(p, *self.shapes[L][1:])[1] for p in self.lv[L]])
                raw = from_device(self.flags[L], np.uint8, (-1,))
                assert (raw[-GUARD:] == POISON).all(), f"{ctx} L{L}: flag guard bytes written"
                raw = raw[:-GUARD].reshape(nz.shape)
                assert np.isin(raw, (0, 1)).all(), f"{ctx} L{L}: a flag byte is neither 0 nor 1"
                assert np.array_equal(raw.astype(bool), nz), f"{ctx} L{L} flags"


# ---- $AQZ_TILED_ZROWS_PER_WAVE through the volume form ---------------------------

# The launch-rule child's cases: the first table's 1030 x 37 u8 shape (rows
# past cov_h to zero) and the column zero-fill shape, eight volumes each, so
# that one row per wave asks for more than the 64 waves every launch has.
ZROWS_CASES = [
    (1030, 37, 4, 3, np.uint8, 8, 64, 8),
    (512, 8, 4, 3, np.uint16, 2, 384, 8),
]
ZROWS_CASE_IDS = [case_id(c) + "/m1" for c in ZROWS_CASES]
# zwaves = max(overhang bytes >> 17 + 1, ceil(items / ZI) if ZI > 0), held to
# 64..4096, then rounded up to whole groups of 8 blocks of 4 waves.  Both
# cases have 8 plane groups and a few KiB of overhang (the byte rule gives 1).
#   u8 1030 x 37, tiles 8 x 64: 2 x 10 units a group; they reach 20 of level
#   1's 24 padded rows (twice per group) and 10 of level 2's 16: 4 * 2 + 6 =
#   14 items a group, 112 in all.  ZI = 1: 112 waves -> 28 blocks -> 32 -> 128
#   waves.  Unset, 1-byte types take ZI = 32: 4 waves, so 64.
#   u16 512 x 8, tiles 2 x 384: 1 x 2 units a group; columns 256.. and 128..
#   of every padded row, 4 rows * 2 + 2 = 10 items a group, 80 in all.
#   ZI = 1: 80 waves -> 20 blocks -> 24 -> 96 waves.  Unset: the byte rule.
# ZI = 0 leaves the byte rule: 64 on both.
# switch value (None: unset) -> launch-log fields of the u8 and the u16 case
ZROWS_PINS = {
    None: ({"family": "volume_tiled", "zwaves": 64, "zitems": 14, "units": 160, "units_x": 2},
           {"family": "volume_tiled", "zwaves": 64, "zitems": 10, "units": 16, "units_x": 1}),
    0: ({"family": "volume_tiled", "zwaves": 64, "zitems": 14},
        {"family": "volume_tiled", "zwaves": 64, "zitems": 10}),
    1: ({"family": "volume_tiled", "zwaves": 128, "zitems": 14},
        {"family": "volume_tiled", "zwaves": 96, "zitems": 10}),
}


# ---- plan_volume_tiled on the CPU --------------------------------------------------

_PROBE = {}


def parse_plan(line):
    """A launch-log line as a dict, or None for `invalid`."""
    if line == "invalid":
        return None
    rec = {}
    for kv in line.split():
        k, _, v = kv.partition("=")
        rec[k] = int(v) if v.lstrip("-").isdigit() else v
    return rec


def plan_probe():
    """ask(requests) -> plans: tests/cpp/volume_tiled_plan_probe.cpp with
    ds_plan.cpp alone, built once a process as a stand-alone program with the
    host compiler under ASan + UBSan."""
    import atexit
    import os
    import shutil
    import subprocess
    import tempfile

    if "exe" not in _PROBE:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        csrc = os.path.join(root, "acquire-zarr_amd", "csrc")
        out = tempfile.mkdtemp(prefix="volume_tiled_plan_probe")
        atexit.register(shutil.rmtree, out, ignore_errors=True)
        exe = os.path.join(out, "volume_tiled_plan_probe")
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + csrc,
                        os.path.join(root, "tests", "cpp", "volume_tiled_plan_probe.cpp"),
                        os.path.join(csrc, "ds_plan.cpp"), "-o", exe], check=True)
        _PROBE["exe"] = exe

    def ask(requests):
        env = {k: v for k, v in os.environ.items() if not k.startswith("AQZ_")}
        r = subprocess.run([_PROBE["exe"]], input="\n".join(requests) + "\n", env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(requests)
        return [parse_plan(l) for l in lines]
    return ask
