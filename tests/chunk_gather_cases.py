"""Cases of the chunk -> frame gather (aqz_chunk_gather_frames_device), a numpy
model of it, and the CPU-built chunk buffers it reads (a plain helper, shared
by tests/test_chunk_gather_cases.py on the CPU and the tests/test_gpu_chunk_
gather*.py files on the GPU).

The source is never made by the code under test: a frame's tiles come from
oracle.tile_frame and go where oracle.chunk_lattice_index, tile_group_offset
and chunk_internal_offset say.  Every chunk byte no in-frame pixel owns — the
tiles' overhang, the places of frames outside the batch, slots no chunk maps
to — holds POISON, so a read outside the frame shows in the result.
"""
import numpy as np

POISON = 0xA5       # chunk bytes nobody owns
DST_POISON = 0x5A   # destination bytes before the call
GUARD = 64          # poisoned bytes on each side of a destination
ABSENT = 0xFFFFFFFF  # AQZ_CHUNK_SLOT_ABSENT
FRAMES_PER_LAUNCH = 64

SPACE, CHANNEL, TIME = 0, 1, 2

DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16,
          np.int32, np.int64, np.float32, np.float64]

FORMS = ("elem", "vec", "vec_straddle")


def form(width, tile_cols, bpp, dst_off_bytes=0):
    """The kernel form a geometry reaches, from the geometry alone:
    elem          no 16-byte vector fits a tile row;
    vec           the vector form and no vector is assembled: frame rows and
                  tile rows are 16-byte multiples and the frame starts on one;
    vec_straddle  the vector form with vectors that cross a tile edge or a
                  row end."""
    if tile_cols * bpp < 16 or width * bpp >= 1 << 31:
        return "elem"
    whole = width * bpp % 16 == 0 and dst_off_bytes % 16 == 0 and \
        (tile_cols * bpp % 16 == 0 or tile_cols >= width)
    return "vec" if whole else "vec_straddle"


def log_form(f):
    """What the launch log calls it (it cannot know of straddling)."""
    return f.split("_")[0]


def tyx(w, h, tile, t_chunk=1):
    return [(TIME, 0, t_chunk, 1), (SPACE, h, tile[0], 1), (SPACE, w, tile[1], 1)]


# (name, W, H, (tile_rows, tile_cols), dtype, form)
FIXED = [
    ("elem_ragged", 11, 7, (4, 3), np.uint8, "elem"),
    ("elem_one_px_tiles", 5, 3, (1, 1), np.uint32, "elem"),
    ("vec_two_per_tile_row", 64, 48, (16, 16), np.uint16, "vec"),
    ("vec_one_per_tile_row", 40, 9, (4, 8), np.uint16, "vec"),
    ("vec_f64_2x2", 4, 5, (2, 2), np.float64, "vec"),
    ("vec_tile_larger_than_frame", 10, 6, (8, 16), np.uint16, "vec_straddle"),
    ("vec_rows_2062", 1031, 517, (128, 256), np.uint16, "vec_straddle"),
    ("vec_tile_cols_250", 1031, 517, (128, 250), np.float32, "vec_straddle"),
]
FIXED_BY_NAME = {c[0]: c for c in FIXED}

# the level-0 geometries the tiling tests use (tests/test_gpu_tiled.py's
# TILED_CASES, which hold tests/test_gpu_parity.py's TILE_CASES):
# (W, H, dtype, tile_rows, tile_cols)
TILING_GEOMETRIES = [
    (64, 48, np.uint16, 16, 16), (1000, 600, np.float32, 64, 128), (300, 7, np.uint8, 4, 128),
    (4096, 4096, np.uint16, 256, 256), (257, 129, np.int64, 32, 32),
    (5472, 3648, np.uint16, 256, 256), (3000, 3000, np.uint16, 256, 256),
    (1031, 517, np.int16, 64, 64), (2100, 700, np.uint8, 8, 16), (4100, 600, np.uint8, 8, 8),
    (640, 480, np.uint16, 100, 60), (512, 512, np.float64, 3, 5),
]


def random_bytes_frames(rng, dtype, shape):
    """Random bytes viewed as `dtype`: every bit pattern, NaN payloads among
    them, none quieted on the way."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    return rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt).reshape(shape)


def float_patterns(dtype):
    """Every operand bit pattern of tests/float_cases.py's catalogue."""
    import float_cases as fc
    f = fc.Fmt(dtype)
    bits = sorted({int(b) for e in fc.catalogue(dtype) for b in e.ops})
    return np.array(bits, f.ut).view(f.dt)


def frame_places(oracle, dims, bpp, first, n):
    """(base[n], internal[n], chunk_bytes, n_chunks) from the oracle's three
    addressing functions; n_chunks covers the layers the batch touches."""
    counts = [-(-d[1] // d[2]) for d in dims]
    per_layer = 1
    for c in counts[1:]:
        per_layer *= c
    layer0 = oracle.chunk_lattice_index(dims, first, 0)
    base = [(oracle.chunk_lattice_index(dims, k, 0) - layer0) * per_layer +
            oracle.tile_group_offset(dims, k) for k in range(first, first + n)]
    internal = [oracle.chunk_internal_offset(dims, bpp, k) for k in range(first, first + n)]
    chunk_bytes = bpp
    for d in dims:
        chunk_bytes *= d[2]
    layers = oracle.chunk_lattice_index(dims, first + n - 1, 0) - layer0 + 1
    return (np.array(base, np.uint32), np.array(internal, np.uint64), chunk_bytes,
            layers * per_layer)


class Source:
    """Chunk buffers for frames first .. first + n - 1 of an array of `dims`.
    `table`: None (identity, n_slots == n_chunks) or a uint32 array over the
    chunks; chunk c is stored in slot table[c] unless that is ABSENT or not a
    slot.  `stride_extra` bytes of poison behind every chunk."""

    def __init__(self, oracle, dims, frames, first, table=None, n_slots=None, stride_extra=0):
        frames = np.ascontiguousarray(frames)
        n, h, w = frames.shape
        self.dims, self.frames, self.first = dims, frames, first
        self.dtype = frames.dtype
        bpp = self.bpp = frames.dtype.itemsize
        self.w, self.h = w, h
        self.tr, self.tc = dims[-2][2], dims[-1][2]
        assert (dims[-2][1], dims[-1][1]) == (h, w)
        self.base, self.internal, self.chunk_bytes, self.n_chunks = \
            frame_places(oracle, dims, bpp, first, n)
        self.stride = self.chunk_bytes + stride_extra
        self.table = None if table is None else np.asarray(table, np.uint32)
        self.n_slots = self.n_chunks if n_slots is None else n_slots
        assert self.table is not None or self.n_slots == self.n_chunks
        self.chunks = np.full((self.n_slots, self.stride), POISON, np.uint8)
        owned, _ = oracle.tile_frame(np.ones((h, w), np.uint8), self.tr, self.tc)
        owned = np.repeat(owned.reshape(owned.shape[0], -1).astype(bool), bpp, axis=1)
        tb = self.tr * self.tc * bpp
        for k in range(n):
            tiles, _ = oracle.tile_frame(frames[k], self.tr, self.tc)
            raw = tiles.view(np.uint8).reshape(tiles.shape[0], tb)
            raw = np.where(owned, raw, np.uint8(POISON))
            at = int(self.internal[k])
            for t in range(tiles.shape[0]):
                s = self.slot(int(self.base[k]) + t)
                if s is not None:
                    self.chunks[s, at:at + tb] = raw[t]

    def slot(self, c):
        s = c if self.table is None else int(self.table[c])
        return s if s < self.n_slots else None

    def expected(self):
        """The frames, with zeros where a chunk has no slot."""
        want = self.frames.copy()
        ntx = -(-self.w // self.tc)
        for k in range(len(want)):
            for t in range(-(-self.h // self.tr) * ntx):
                if self.slot(int(self.base[k]) + t) is None:
                    ty, tx = divmod(t, ntx)
                    want[k, ty * self.tr:(ty + 1) * self.tr, tx * self.tc:(tx + 1) * self.tc] = 0
        return want

    def bad(self):
        """1 when a chunk of the batch maps to a slot that is neither a slot
        nor ABSENT."""
        if self.table is None:
            return 0
        nt = -(-self.h // self.tr) * -(-self.w // self.tc)
        used = np.concatenate([self.table[int(b):int(b) + nt] for b in self.base])
        return int(((used >= self.n_slots) & (used != ABSENT)).any())


def gather_model(chunks, table, n_slots, base, internal, dtype, w, h, tr, tc):
    """aqz_chunk_gather_frames_device in numpy, pixel by pixel from the
    header's address formula: (frames[n, h, w], bad_slot)."""
    dt = np.dtype(dtype)
    bpp = dt.itemsize
    ntx = -(-w // tc)
    ys, xs = np.mgrid[0:h, 0:w]
    tile = (ys // tr) * ntx + xs // tc
    inside = ((ys % tr) * tc + xs % tc) * bpp
    flat = np.ascontiguousarray(chunks).reshape(-1)
    stride = chunks.shape[1]
    out = np.zeros((len(base), h, w), dt)
    bad = 0
    for k in range(len(base)):
        c = int(base[k]) + tile
        s = c if table is None else np.asarray(table, np.int64)[c]
        ok = s < n_slots
        bad |= int(((~ok) & (s != ABSENT)).any())
        at = np.where(ok, s, 0).astype(np.int64) * stride + int(internal[k]) + inside
        px = flat[at[..., None] + np.arange(bpp)]
        px = np.ascontiguousarray(px).view(dt)[..., 0]
        out[k] = np.where(ok, px, np.zeros((), dt))
    return out, bad


# ---- seeded fuzz ----------------------------------------------------------------------

N_FUZZ = 48


def fuzz_case(i):
    """3-5 dims, any dtype, frames up to 96 x 96, up to 12 frames, a random
    first frame, tiles from 1 x 1 to larger than the frame, a permuted slot
    table in every other case.  One case in three is drawn with 16-byte rows
    and tile rows, so that the form without straddling is reached as well."""
    rng = np.random.default_rng(0x6A7 + i)
    dtype = DTYPES[int(rng.integers(0, len(DTYPES)))]
    bpp = np.dtype(dtype).itemsize
    nd = int(rng.integers(3, 6))
    dims = [(TIME, 0, int(rng.integers(1, 4)), 1)]
    for _ in range(nd - 3):
        size = int(rng.integers(1, 4))
        dims.append((CHANNEL, size, int(rng.integers(1, size + 1)), 1))
    h = int(rng.integers(1, 97))
    tr = int(rng.integers(1, h + 9))
    if i % 3 == 0:
        q = 16 // bpp  # elements of one vector
        w = q * int(rng.integers(1, 96 // q + 1))
        tc = q * int(rng.integers(1, w // q + 2))
    else:
        w = int(rng.integers(1, 97))
        tc = int(rng.integers(1, min(w + 9, 24 if i % 3 == 1 else 200)))
    if i % 12 == 5:    # one tile, larger than the frame both ways
        tr, tc = h + int(rng.integers(1, 9)), w + int(rng.integers(1, 9))
    elif i % 12 == 10:  # one-pixel tiles
        tr = tc = 1
    dims += [(SPACE, h, tr, 1), (SPACE, w, tc, 1)]
    return dict(dims=dims, dtype=dtype, w=w, h=h, n=int(rng.integers(1, 13)),
                first=int(rng.integers(0, 40)), permute=i % 2 == 1, seed=0x51 + i,
                form=form(w, tc, bpp))


def fuzz_source(oracle, c):
    rng = np.random.default_rng(c["seed"])
    frames = random_bytes_frames(rng, c["dtype"], (c["n"], c["h"], c["w"]))
    bpp = np.dtype(c["dtype"]).itemsize
    table = n_slots = None
    if c["permute"]:
        n_chunks = frame_places(oracle, c["dims"], bpp, c["first"], c["n"])[3]
        n_slots = n_chunks + int(rng.integers(0, 4))
        table = rng.permutation(n_slots)[:n_chunks].astype(np.uint32)
    return Source(oracle, c["dims"], frames, c["first"], table, n_slots)
