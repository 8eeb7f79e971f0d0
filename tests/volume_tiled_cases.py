"""Shared pieces of the volume tiled tests (not a test module, not a conftest):
the cases, the volume geometry, and the expected bytes — always the oracle
pyramid (oracle.OracleDownsampler), tiled by oracle.tile_frame and placed by
oracle.chunk_frame_offsets, never the product's."""
import numpy as np

from gpu_util import random_frames

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
            for t in range(tiles.shape[0]):
                at = offs[k] + t * cb
                buf[at:at + tb] = tiles[t].view(np.uint8).reshape(-1)
        out.append((buf, offs, cb, lb, cap))
    return out
