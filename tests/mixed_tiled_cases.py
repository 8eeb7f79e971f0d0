"""Shared pieces of the mixed tiled tests (not a test module, not a conftest):
the tile shapes of mixed_batch_cases.FIXED, the store branch of the tiled Z run
each shape reaches (from geometry alone), the run cut of
aqz_ds_mixed_flag_slots restated, the seeded fuzz cases, the expected bytes —
always oracle.tile_frame of mixed_batch_cases.oracle_levels at
oracle.chunk_frame_offsets' places, never the product's — and the device
buffers of the GPU tests."""
import zlib

import numpy as np

import mixed_batch_cases as mc
from gpu_util import assert_parity, empty_device, from_device, launch_stream, to_device

SPACE, TIME = 0, 2
POISON, GUARD = mc.POISON, mc.GUARD

# name -> tile shapes (rows, cols): one for every level, or one per level
# (index 0 unused)
FIXED_TILES = {
    "volume2_cascade2": [(32, 64), (48, 40)],
    "odd_widths_rows": [(16, 24)],
    "volume1_zrun3": [(16, 16), [None, (16, 16), (8, 32), (24, 20), (5, 7)], (64, 64)],
    "zrun3_zrun2_851": [(8, 5), (23, 37), (64, 64)],
    "z_then_xy": [(16, 12)],
    "xy_xyz_z": [(8, 8)],
    "one_element": [(1, 1), (4, 4)],
    "span_plus_1": [(1, 512)],
    "span_minus_1": [(1, 512)],
    "many_tiny_groups": [(1, 1), (4, 8)],
}


def tiles_for(geo, spec):
    return list(spec) if isinstance(spec, list) else [None] + [tuple(spec)] * (len(geo) - 1)


def tiles_id(spec):
    if isinstance(spec, list):
        return "-".join(f"{r}x{c}" for r, c in spec[1:])
    return f"{spec[0]}x{spec[1]}"


FIXED_CASES = [(name, spec) for name in mc.FIXED_NAMES for spec in FIXED_TILES[name]]
FIXED_IDS = [f"{name}-{tiles_id(spec)}" for name, spec in FIXED_CASES]

# ---- the store branches of the tiled Z run -------------------------------------

BRANCHES = ["vector_in_tile_row", "vector_across_tile_edge", "vector_across_row_end",
            "plane_tail", "column_fill", "row_fill", "tile_larger_than_frame"]


def z_level_branches(w, h, bpp, tile):
    """Branches one Z level of w x h reaches under `tile`: a lane's vector is
    16 bytes from element e = 16 / bpp * i of the plane, at (e // w, e % w)."""
    tr, tc = tile
    c = 16 // bpp
    x = (np.arange(w * h // c, dtype=np.int64) * c) % w
    one_row = x + c <= w
    one_tile = x % tc + c <= tc
    out = set()
    if (one_row & one_tile).any():
        out.add("vector_in_tile_row")
    if (one_row & ~one_tile).any():
        out.add("vector_across_tile_edge")
    if (~one_row).any():
        out.add("vector_across_row_end")
    if (w * h) % c:
        out.add("plane_tail")
    if w % tc:
        out.add("column_fill")
    if h % tr:
        out.add("row_fill")
    if tr > h and tc > w:
        out.add("tile_larger_than_frame")
    return out


def branches_of(geo, dtype, tiles):
    """Every branch the pyramid's Z levels reach."""
    bpp = np.dtype(dtype).itemsize
    out = set()
    for L, c in enumerate(mc.classes(geo)):
        if c == "Z":
            out |= z_level_branches(geo[L][0], geo[L][1], bpp, tiles[L])
    return out


# ---- aqz_ds_mixed_flag_slots' run cut ------------------------------------------

def run_of_level(geo, L):
    """(class, first level, levels) of the run that holds level L, restated:
    levels are classed one by one, a run ends where the class changes or the
    class's depth (2 / 4 / 3) is reached; None where a level has no class or
    pairs an odd plane count.  The cut does not depend on the batch."""
    cls = [None]
    for a, b in zip(geo, geo[1:]):
        xy, zh = b[0] < a[0] or b[1] < a[1], b[2] < a[2]
        if not (xy or zh) or (zh and a[2] % 2):
            return None
        cls.append("XYZ" if xy and zh else "XY" if xy else "Z")
    first = 1
    for l in range(2, L + 1):
        if cls[l] != cls[first] or l - first == {"XYZ": 2, "XY": 4, "Z": 3}[cls[first]]:
            first = l
    k = 1
    while (first + k < len(geo) and cls[first + k] == cls[first]
           and k < {"XYZ": 2, "XY": 4, "Z": 3}[cls[first]]):
        k += 1
    return cls[first], first, k


# ---- expectations ----------------------------------------------------------------

def expected_tiled(oracle, levels, tiles):
    """Per level (tiles[n, n_tiles, tr, tc], nonzero[n, n_tiles] bool)."""
    want = [None]
    for L in range(1, len(levels)):
        tr, tc = tiles[L]
        t = [oracle.tile_frame(p, tr, tc) for p in levels[L]]
        want.append((np.stack([a for a, _ in t]), np.stack([b for _, b in t])))
    return want


def n_tiles(geo, L, tile):
    w, h, _ = geo[L]
    return (-(-h // tile[0])) * (-(-w // tile[1]))


def chunk_dims(geo, L, shape, four_d=False):
    """Level L as an array appended along Z in chunks of shape (z, y, x); or
    (`four_d`) T/Z/Y/X: one stack of the level's planes a time point, appended
    along T, frame ids in storage order (time point x planes + plane)."""
    w, h, planes = geo[L]
    yx = [(SPACE, h, shape[1], 1), (SPACE, w, shape[2], 1)]
    if four_d:
        return [(TIME, 0, 1, 1), (SPACE, planes, shape[0], 1)] + yx
    return [(SPACE, 0, shape[0], 1)] + yx


def expected_chunked(oracle, geo, levels, shapes, firsts, dtype, four_d=False):
    """Per level (buffer bytes with poison where no frame writes, offsets,
    chunk_bytes, capacity) for a batch whose level-L frames start at frame
    firsts[L] of level L's own stack."""
    bpp = np.dtype(dtype).itemsize
    out = [None]
    for L in range(1, len(geo)):
        _, cy, cx = shapes[L]
        offs, cb, lb = oracle.chunk_frame_offsets(chunk_dims(geo, L, shapes[L], four_d), bpp, firsts[L],
                                                  len(levels[L]))
        cap = (max(offs) // lb + 1) * lb
        buf = np.full(cap, POISON, np.uint8)
        tb = cy * cx * bpp
        for k, p in enumerate(levels[L]):
            tiles, _ = oracle.tile_frame(p, cy, cx)
            at = offs[k] + np.arange(tiles.shape[0], dtype=np.int64)[:, None] * cb
            buf[at + np.arange(tb, dtype=np.int64)[None, :]] = \
                tiles.view(np.uint8).reshape(tiles.shape[0], tb)
        out.append((buf, offs, cb, cap))
    return out


# ---- seeded fuzz -----------------------------------------------------------------

N_FUZZ_TILED, N_FUZZ_CHUNKED = 48, 24


def _pyramid(rng, category):
    """mixed_batch_cases.fuzz_case's pyramid with what the tiled call adds: an
    XY level needs a source row of one 16-byte load as well (the row-major
    route has single-level kernels for narrower ones; the tiled one refuses),
    so such a level becomes a Z level.  Drawn again until it is of `category`
    (mixed_batch_cases.CATEGORIES), so that every category has its share."""
    while True:
        dtype = mc.DTYPES[int(rng.integers(len(mc.DTYPES)))]
        bpp = np.dtype(dtype).itemsize
        method = int(rng.integers(4))
        levels = int(rng.integers(2, 7))
        if rng.integers(2):
            head = int(rng.integers(0, levels - 1))
            tail = ["XY", "Z"][int(rng.integers(2))]
            cls = ["XYZ"] * head + [tail] * (levels - 1 - head)
        else:
            cls = [["XYZ", "XY", "Z"][int(rng.integers(3))] for _ in range(levels - 1)]
        w, h = int(rng.integers(1, 97)), int(rng.integers(1, 97))
        sizes = [(w, h)]
        for k, c in enumerate(cls):
            if c != "Z" and (max(w, h) == 1 or w * bpp < 16):
                c = cls[k] = "Z"
            if c != "Z":
                w, h = (w + 1) // 2, (h + 1) // 2
            sizes.append((w, h))
        if (len(set(cls)) == 1 and cls[0] != "Z") or \
                category not in mc.fuzz_categories(dict(cls=cls)):
            continue
        planes = [int(rng.integers(1, 4))]
        for c in reversed(cls):
            planes.insert(0, planes[0] * (1 if c == "XY" else 2))
        geo = [(sw, sh, p) for (sw, sh), p in zip(sizes, planes)]
        assert mc.classes(geo)[1:] == cls, (geo, cls)
        return geo, dtype, method, cls, planes[0] * int(rng.integers(1, 4))


def _tile(rng, w, h):
    """(rows, cols); one level in five under a tile larger than the frame."""
    if rng.random() < 0.2:
        return h + int(rng.integers(1, 9)), w + int(rng.integers(1, 9))
    return _side(rng, h), _side(rng, w)


def _side(rng, extent):
    r = rng.random()
    if r < 0.15:
        return extent + int(rng.integers(1, 9))      # larger than the frame
    if r < 0.45:
        return int(rng.choice([1, 2, 4, 8, 16, 32]))
    return int(rng.integers(1, extent + 1))


def fuzz_tiled_case(i):
    rng = np.random.default_rng(zlib.crc32(f"fuzz-mixed-tiled{i}".encode()))
    geo, dtype, method, cls, n = _pyramid(rng, mc.CATEGORIES[i % len(mc.CATEGORIES)])
    tiles = [None] + [_tile(rng, w, h) for w, h, _ in geo[1:]]
    offs = [int(x) for x in rng.integers(1, 8, len(geo))] if i % 2 else [0] * len(geo)
    return dict(geo=geo, n=n, dtype=dtype, method=method, cls=cls, tiles=tiles, offs=offs,
                flags=bool(i % 4 != 3), rng=rng)


def fuzz_chunked_case(i):
    rng = np.random.default_rng(zlib.crc32(f"fuzz-mixed-chunked{i}".encode()))
    geo, dtype, method, cls, n = _pyramid(rng, mc.CATEGORIES[i % len(mc.CATEGORIES)])
    shapes = [None] + [(int(rng.integers(1, 4)),) + _tile(rng, w, h) for w, h, _ in geo[1:]]
    em = mc.emitted(geo, n)
    # the batch starts this many of its own lengths into every level's stack
    lead = int(rng.integers(0, 3))
    return dict(geo=geo, n=n, dtype=dtype, method=method, cls=cls, shapes=shapes,
                tiles=[None] + [s[1:] for s in shapes[1:]],
                firsts=[lead * e for e in em], offs=[int(rng.integers(0, 8))] + [0] * (len(geo) - 1),
                flags=bool(i % 4 != 3), rng=rng)


# ---- device buffers of the GPU tests ---------------------------------------------

def device_input(frames, off=0):
    """The frames `off` elements into a poisoned buffer, GUARD bytes on both
    sides: (tensor, address of the first frame)."""
    bpp = frames.dtype.itemsize
    raw = np.full(2 * GUARD + off * bpp + frames.nbytes, POISON, np.uint8)
    at = GUARD + off * bpp
    raw[at: at + frames.nbytes] = np.ascontiguousarray(frames).view(np.uint8).reshape(-1)
    d = to_device(raw)
    return d, d.data_ptr() + at


class Outputs:
    """Poisoned tile and flag buffers of one batch of `n` frames: level L's
    tiles `offs[L]` elements into their buffer, GUARD poisoned bytes on both
    sides of tiles and flags.  `slots[L]`: flag bytes per tile."""

    def __init__(self, geo, dtype, tiles, n, slots, with_flags=True, offs=None):
        self.geo, self.dtype, self.tiles, self.n = geo, np.dtype(dtype), tiles, n
        self.bpp = self.dtype.itemsize
        self.offs = offs or [0] * len(geo)
        self.counts = mc.emitted(geo, n)
        self.slots = slots
        lv = range(1, len(geo))
        self.nt = [None] + [n_tiles(geo, L, tiles[L]) for L in lv]
        self.nbytes = [None] + [self.counts[L] * self.nt[L] * tiles[L][0] * tiles[L][1] * self.bpp
                                for L in lv]
        self.outs = [None] + [empty_device(2 * GUARD + self.offs[L] * self.bpp + self.nbytes[L])
                              for L in lv]
        self.fbytes = [None] + [self.counts[L] * self.nt[L] * slots[L] for L in lv]
        self.flags = [None] + [empty_device(2 * GUARD + self.fbytes[L]) if with_flags else None
                               for L in lv]
        self.poison()

    def poison(self):
        for b in self.outs[1:] + self.flags[1:]:
            if b is not None:
                b.fill_(POISON)

    def out_ptrs(self):
        return [0] + [self.outs[L].data_ptr() + GUARD + self.offs[L] * self.bpp
                      for L in range(1, len(self.geo))]

    def flag_ptrs(self):
        if self.flags[1] is None:
            return None
        return [0] + [f.data_ptr() + GUARD for f in self.flags[1:]]

    def run(self, ds, src, stream=None):
        return ds.run_device_mixed_tiled(src, self.n, self.tiles, self.out_ptrs(),
                                         self.flag_ptrs(),
                                         launch_stream() if stream is None else stream)

    def tile_bytes(self, L, ctx):
        raw = from_device(self.outs[L], np.uint8, (-1,))
        at = GUARD + self.offs[L] * self.bpp
        assert (raw[:at] == POISON).all(), f"{ctx} L{L}: bytes in front of the tiles written"
        assert (raw[at + self.nbytes[L]:] == POISON).all(), f"{ctx} L{L}: guard bytes written"
        return raw[at: at + self.nbytes[L]]

    def flag_bytes(self, L, ctx):
        raw = from_device(self.flags[L], np.uint8, (-1,))
        assert (raw[:GUARD] == POISON).all() and (raw[GUARD + self.fbytes[L]:] == POISON).all(), \
            f"{ctx} L{L}: flag guard bytes written"
        return raw[GUARD: GUARD + self.fbytes[L]]

    def untouched(self, ctx):
        for b in self.outs[1:] + self.flags[1:]:
            if b is not None:
                assert (from_device(b, np.uint8, (-1,)) == POISON).all(), f"{ctx}: bytes written"

    def check(self, want, ctx):
        got_all = [None]
        for L in range(1, len(self.geo)):
            tr, tc = self.tiles[L]
            want_t, want_nz = want[L]
            got = self.tile_bytes(L, ctx).view(self.dtype).reshape(self.counts[L], self.nt[L],
                                                                   tr, tc)
            assert_parity(got, want_t, f"{ctx} L{L} tiles")
            got_all.append(got)
            if self.flags[L] is not None:
                raw = self.flag_bytes(L, ctx).reshape(self.counts[L], self.nt[L], self.slots[L])
                assert np.isin(raw, (0, 1)).all(), f"{ctx} L{L}: a flag byte is neither 0 nor 1"
                assert np.array_equal(raw.any(axis=2), want_nz), f"{ctx} L{L} zero scan"
        return got_all


class Lattice:
    """One chunked batch: a poisoned lattice buffer and flag buffer per level,
    GUARD bytes on both sides of each."""

    def __init__(self, geo, dtype, shapes, n, want, slots, with_flags=True):
        self.geo, self.dtype, self.shapes, self.n = geo, np.dtype(dtype), shapes, n
        self.want, self.slots = want, slots
        self.counts = mc.emitted(geo, n)
        lv = range(1, len(geo))
        self.bufs = [None] + [empty_device(2 * GUARD + want[L][3]) for L in lv]
        self.nt = [None] + [n_tiles(geo, L, shapes[L][1:]) for L in lv]
        self.fbytes = [None] + [self.counts[L] * self.nt[L] * slots[L] for L in lv]
        self.flags = [None] + [empty_device(2 * GUARD + self.fbytes[L]) if with_flags else None
                               for L in lv]
        for b in self.bufs[1:] + self.flags[1:]:
            if b is not None:
                b.fill_(POISON)

    def lattices(self, offsets=None):
        lats = [None]
        for L in range(1, len(self.geo)):
            _, offs, cb, cap = self.want[L]
            _, cy, cx = self.shapes[L]
            lats.append((self.bufs[L].data_ptr() + GUARD, cap, cy, cx, cb,
                         offsets[L] if offsets else offs))
        return lats

    def flag_ptrs(self):
        if self.flags[1] is None:
            return None
        return [0] + [f.data_ptr() + GUARD for f in self.flags[1:]]

    def run(self, ds, src, stream=None):
        return ds.run_device_mixed_chunked(src, self.n, self.lattices(), self.flag_ptrs(),
                                           launch_stream() if stream is None else stream)

    def check(self, oracle, levels, ctx):
        """Every lattice byte: tiles where a frame owns them, poison elsewhere
        and in the guards; flags exactly 0 or 1."""
        for L in range(1, len(self.geo)):
            got = from_device(self.bufs[L], np.uint8, (-1,))
            cap = self.want[L][3]
            assert (got[:GUARD] == POISON).all() and (got[GUARD + cap:] == POISON).all(), \
                f"{ctx} L{L}: bytes around the lattice written"
            bad = np.flatnonzero(got[GUARD: GUARD + cap] != self.want[L][0])
            assert bad.size == 0, f"{ctx} L{L}: {bad.size} bytes differ, first at {bad[0]}"
            if self.flags[L] is not None:
                nz = np.stack([oracle.tile_frame(p, *self.shapes[L][1:])[1] for p in levels[L]])
                raw = from_device(self.flags[L], np.uint8, (-1,))
                assert (raw[:GUARD] == POISON).all() and \
                    (raw[GUARD + self.fbytes[L]:] == POISON).all(), f"{ctx} L{L}: flag guards"
                raw = raw[GUARD: GUARD + self.fbytes[L]].reshape(nz.shape + (self.slots[L],))
                assert np.isin(raw, (0, 1)).all(), f"{ctx} L{L}: a flag byte is neither 0 nor 1"
                assert np.array_equal(raw.any(axis=-1), nz), f"{ctx} L{L} flags"


# ---- plan_zrun_tiled on the CPU ----------------------------------------------------

_PROBE = {}


def plan_probe():
    """ask(requests) -> answer lines: tests/cpp/mixed_tiled_plan_probe.cpp with
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
        out = tempfile.mkdtemp(prefix="mixed_tiled_plan_probe")
        atexit.register(shutil.rmtree, out, ignore_errors=True)
        exe = os.path.join(out, "mixed_tiled_plan_probe")
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + csrc,
                        os.path.join(root, "tests", "cpp", "mixed_tiled_plan_probe.cpp"),
                        os.path.join(csrc, "ds_plan.cpp"), "-o", exe], check=True)
        _PROBE["exe"] = exe

    def ask(requests):
        env = {k: v for k, v in os.environ.items() if not k.startswith("AQZ_")}
        r = subprocess.run([_PROBE["exe"]], input="\n".join(requests) + "\n", env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(requests)
        return lines
    return ask
