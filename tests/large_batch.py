"""Batches past 4 GiB: the case table and the builders shared by
tests/test_large_batch_cases.py (CPU) and tests/test_gpu_large_batch.py (GPU).

The shift rule.  For Decimate, Mean, Min and Max, adding one constant t to a
whole frame adds t to every level of its pyramid, bit for bit, as long as no
value overflows and (floats) every intermediate is exact.  For a Z-halving
pyramid the constant goes to every plane of one plane group (the planes one
output frame of the last level is made from; for stacks that do not halve
evenly, one stack).  So a batch of any length needs one oracle run: a base
frame (or base plane group) gives E[L]; frame k of the batch is base + tag(k),
tag(k) = k mod M, and level L's frame k must be E[L] + tag(k).  Every frame is
distinct, so a frame read from or written to the wrong place, or never
processed, is a mismatch that names the level and the frame.

M is the largest prime not above dtype_max - base_max (float32: integer values,
base below 1024, M = 1021, so with at most 6 levels every sum stays below 2^24
and exact).  A truncated 32-bit offset lands 2^32 / frame_size or
2^31 / frame_size frames away; where that is integral it is a power of two,
never a multiple of the prime M, so the frame found there carries another tag.
"""
import math
from collections import namedtuple

import numpy as np

from test_gpu_parity import BATCH_GEOMETRIES, halving_geometry, seed_of

POISON, PAD = 0xA5, 64
SLAB_BYTES = 256 << 20   # device temporaries of the compare stay under 1 GiB

BASE_MAX = {"uint8": 4, "uint16": 4095, "float32": 1023}
DTYPE_MAX = {"uint8": 255, "uint16": 65535}


def largest_prime_at_most(n):
    def is_prime(x):
        return x >= 2 and all(x % d for d in range(2, math.isqrt(x) + 1))
    while not is_prime(n):
        n -= 1
    return n


def modulus(dtype):
    name = np.dtype(dtype).name
    if name == "float32":
        return 1021
    return largest_prime_at_most(DTYPE_MAX[name] - BASE_MAX[name])


# family: row (aqz_ds_run_device_batch, 2-D), volume (kind 2), zpath (kind 0),
#         tiled (aqz_ds_run_device_batch_tiled), lattice (..._chunked),
#         volume_tiled (aqz_ds_run_device_volume_tiled, kind 5),
#         volume_lattice (..._volume_chunked)
# depth:  shallow = the input passes 2^32 bytes; deep = level 1's output does
# tile:   (rows, columns) of every level, or a list with one per level
Case = namedtuple("Case", "id family name geo dtype method kind depth tile")
VOLUME_FAMILIES = ("volume", "volume_tiled", "volume_lattice")

BATCH_2D = ["2d", "2d_generic", "2d_narrow", "2d_oddw_deep", "2d_six", "2d_band_staged",
            "2d_wide_misaligned", "2d_band8_aligned", "2d_band6_edge_rows", "2d_band_segments",
            "2d_complete_8tile", "2d_complete_short_last", "2d_mis_segments"]
VOLUMES = ["3d_fused", "3d_fused_edge", "3d_fused_many_groups", "3d_fused_many_groups_edge"]
Z_PATH_GEO = [(2048, 1024, 6), (1024, 512, 3), (512, 256, 2)]
GENERIC_GEO = [(7, 8191, 1), (4, 4096, 1), (2, 2048, 1)]
TILED_SHAPES = [(1000, 600, 4, 64, 128), (512, 512, 4, 3, 5)]   # of TILED_CASES
# T / Y / X, 3 frames per chunk, ragged XY chunks (tests/test_gpu_lattice.py's
# test_time_chunks)
LATTICE_DIMS = [(2, 0, 3, 1), (0, 384, 128, 1), (0, 520, 96, 1)]
LATTICE_GEO = [(520, 384, 0), (260, 192, 0), (130, 96, 0)]   # the planner's, T unbounded
# tiled volumes: 72 x 40 x 8 under 8 x 16 tiles (level 1 is 36 x 20: four rows
# of overhang the units do not reach), under 64 x 64 tiles (deep: a 4096-byte
# padded u8 plane against 2 x 2880 bytes of input), and volume_tiled_cases'
# column zero-fill shape (512 x 8 x 4 under 2 x 384 tiles)
VOLUME_TILED_NAME = "3d_fused_many_groups_edge"
VOLUME_TILED_TILE, VOLUME_TILED_DEEP_TILE = (8, 16), (64, 64)
COLUMN_FILL_GEO = [(512, 8, 4), (256, 4, 2), (128, 2, 1)]
COLUMN_FILL_TILE = (2, 384)
# volume lattice: 200 x 61 x 8 u16; level 1 is 4 x 31 x 100 in chunks of
# 2 x 20 x 80 (ragged in Y and X, a padded plane of 12800 bytes), level 2 is
# 2 x 16 x 50 in chunks of 2 x 12 x 32
VOLUME_LATTICE_NAME = "3d_fused_edge"
VOLUME_LATTICE_SHAPES = [None, (2, 20, 80), (2, 12, 32)]   # (z, y, x) chunk per level


def _dn(d):
    return np.dtype(d).name


def _table():
    cases = []
    for name in BATCH_2D:
        geo, _, kind = BATCH_GEOMETRIES[name]
        for dt in (np.uint8, np.uint16, np.float32):
            for m in (0, 1):
                cases.append(Case(f"{name}-{_dn(dt)}-m{m}", "row", name, geo, dt, m, kind,
                                  "shallow", None))
    for name in VOLUMES:
        geo, _, kind = BATCH_GEOMETRIES[name]
        for dt in (np.uint8, np.uint16, np.float32):
            for m in (0, 1):
                cases.append(Case(f"{name}-{_dn(dt)}-m{m}", "volume", name, geo, dt, m, kind,
                                  "shallow", None))
    for name, dt in (("2d", np.uint8), ("2d_generic", np.uint8), ("3d_fused", np.uint8),
                     ("2d_band8_aligned", np.uint16)):
        geo, _, kind = BATCH_GEOMETRIES[name]
        fam = "volume" if kind == 2 else "row"
        cases.append(Case(f"deep-{name}-{_dn(dt)}-m1", fam, name, geo, dt, 1, kind, "deep", None))
    # a row the fused cascade refuses (7 bytes: under the narrowest tile's
    # 8-byte load), so every level is one batched xy_generic_kernel launch
    # (kind 3), its 64-bit thread index over more than 2^32 level-1 outputs
    cases.append(Case("deep-generic-7x8191-uint8-m1", "row", "generic_narrow", GENERIC_GEO,
                      np.uint8, 1, 3, "deep", None))
    cases.append(Case("zpath-2048x1024x6-uint8-m1", "zpath", "zpath", Z_PATH_GEO, np.uint8, 1, 0,
                      "shallow", None))
    for w, h, nl, tr, tc in TILED_SHAPES:
        for dt in (np.uint8, np.uint16):
            cases.append(Case(f"tiled-{w}x{h}-{tr}x{tc}-{_dn(dt)}-m1", "tiled", f"{w}x{h}",
                              halving_geometry(w, h, nl), dt, 1, 4, "deep", (tr, tc)))
    cases.append(Case("lattice-520x384-uint16-m1", "lattice", "lattice", LATTICE_GEO, np.uint16,
                      1, 4, "deep", (LATTICE_DIMS[1][2], LATTICE_DIMS[2][2])))
    geo = BATCH_GEOMETRIES[VOLUME_TILED_NAME][0]
    for name, g, tile in ((VOLUME_TILED_NAME, geo, VOLUME_TILED_TILE),
                          ("column_fill", COLUMN_FILL_GEO, COLUMN_FILL_TILE)):
        for dt, m in ((np.uint8, 1), (np.uint16, 1), (np.float32, 1), (np.uint16, 0)):
            cases.append(Case(f"vtiled-{name}-{tile[0]}x{tile[1]}-{_dn(dt)}-m{m}", "volume_tiled",
                              f"vtiled-{name}", g, dt, m, 5, "shallow", tile))
    tile = VOLUME_TILED_DEEP_TILE
    cases.append(Case(f"deep-vtiled-{VOLUME_TILED_NAME}-{tile[0]}x{tile[1]}-uint8-m1",
                      "volume_tiled", f"vtiled-{VOLUME_TILED_NAME}", geo, np.uint8, 1, 5, "deep",
                      tile))
    cases.append(Case(f"vlattice-{VOLUME_LATTICE_NAME}-uint16-m1", "volume_lattice",
                      f"vlattice-{VOLUME_LATTICE_NAME}", BATCH_GEOMETRIES[VOLUME_LATTICE_NAME][0],
                      np.uint16, 1, 5, "deep", [None] + [s[1:] for s in VOLUME_LATTICE_SHAPES[1:]]))
    return cases


CASES = _table()
BY_ID = {c.id: c for c in CASES}


def select(family=None, depth=None):
    return [c for c in CASES if (family is None or c.family == family)
            and (depth is None or c.depth == depth)]


# ---- geometry ---------------------------------------------------------------

def bpp(case):
    return np.dtype(case.dtype).itemsize


def group_planes(case):
    """Planes that share one tag: 1 for 2-D pyramids, 2^(levels - 1) for the
    fused volume, one stack for the per-frame Z path."""
    if case.family in VOLUME_FAMILIES:
        return 1 << (len(case.geo) - 1)
    if case.family == "zpath":
        return case.geo[0][2]
    return 1


def per_group(case, level):
    """Level-`level` frames one plane group emits."""
    if case.family in VOLUME_FAMILIES:
        return group_planes(case) >> level
    if case.family == "zpath":
        return case.geo[level][2]
    return 1


def tile_of(case, level):
    return case.tile[level] if isinstance(case.tile, list) else case.tile


def frame_elems(case, level):
    """Elements of one stored frame of the level: the padded tile area for
    chunk-tiled outputs."""
    w, h, _ = case.geo[level]
    if level and case.tile:
        tr, tc = tile_of(case, level)
        return (-(-h // tr) * tr) * (-(-w // tc) * tc)
    return w * h


def frame_bytes(case, level):
    return frame_elems(case, level) * bpp(case)


def frames_for(case):
    """ceil(2^32 / frame bytes) + 2 frames (shallow: of the input, deep: of
    level 1), rounded up to whole stacks (lattice: whole chunk layers)."""
    if case.depth == "shallow":
        n = -(-(1 << 32) // frame_bytes(case, 0)) + 2
    else:
        n1 = -(-(1 << 32) // frame_bytes(case, 1)) + 2
        n = -(-n1 * group_planes(case) // per_group(case, 1))
    unit = max(1, case.geo[0][2])
    if case.family == "lattice":
        unit = LATTICE_DIMS[0][2]
    if case.family == "volume_lattice":   # whole chunk layers at every level
        unit = math.lcm(unit, *[s[0] << L for L, s in enumerate(VOLUME_LATTICE_SHAPES) if L])
    return -(-n // unit) * unit


def level_frames(case, level, n=None):
    n = frames_for(case) if n is None else n
    if level == 0:
        return n
    return n // group_planes(case) * per_group(case, level)


def flag_bytes_bound(case, level):
    """Zero-scan flag bytes per frame, at most: a slot covers at least one
    element of its tile."""
    w, h, _ = case.geo[level]
    tr, tc = tile_of(case, level)
    return (-(-h // tr)) * (-(-w // tc)) * tr * tc


def need_bytes(case):
    """Device memory the case needs: input, every level with its poison, flag
    slots, and the compare's temporaries."""
    n = frames_for(case)
    total = n * frame_bytes(case, 0)
    for L in range(1, len(case.geo)):
        total += level_frames(case, L, n) * frame_bytes(case, L) + PAD
        if case.family in ("tiled", "volume_tiled"):
            total += level_frames(case, L, n) * flag_bytes_bound(case, L) + PAD
    return total + 4 * SLAB_BYTES + (64 << 20)


# ---- base and tags ----------------------------------------------------------

def base_group(case):
    """The base plane group (group_planes, h, w): random values up to
    BASE_MAX; chunk-tiled cases keep the top left quarter zero, so that whole
    tiles of every level are zero under tag 0."""
    w, h, _ = case.geo[0]
    rng = np.random.default_rng(seed_of("large-batch", case.name, _dn(case.dtype)))
    g = rng.integers(0, BASE_MAX[_dn(case.dtype)], (group_planes(case), h, w), endpoint=True)
    g = g.astype(case.dtype)
    if case.tile:
        g[:, : h // 2, : w // 2] = 0
    return g


def cpu_tags(case):
    m = modulus(case.dtype)
    return [0, 1, m // 2, m - 1]


def oracle_levels(oracle, case, groups):
    """The oracle stream over `groups` (a list of plane groups, in order):
    {L: (frames of the level, h, w)}."""
    ref = oracle.OracleDownsampler(case.geo, case.dtype, case.method)
    out = {L: [] for L in range(1, len(case.geo))}
    for g in groups:
        for plane in g:
            ref.add_frame(plane)
            for L in out:
                r = ref.take_frame(L)
                if r is not None:
                    out[L].append(r)
    return {L: np.stack(v) for L, v in out.items()}


_EXPECTED = {}


def expected_levels(oracle, case):
    """E[L] (per_group(L), h, w) of the base group: one oracle run per
    (geometry, dtype, method), shared and left unchanged."""
    key = (case.family, case.name, _dn(case.dtype), case.method)
    if key not in _EXPECTED:
        e = oracle_levels(oracle, case, [base_group(case)])
        for L, a in e.items():
            assert a.shape[0] == per_group(case, L)
            a.setflags(write=False)
        _EXPECTED[key] = e
    return _EXPECTED[key]


def tiled_expectation(oracle, case, level, e_level, tag):
    """oracle.tile_frame of E[level] + tag: (tiles, nonzero flags)."""
    if np.dtype(case.dtype).kind == "f":    # a Mean's level holds fractions: exact in float32
        shifted = e_level + np.asarray(tag, case.dtype)
    else:
        shifted = (e_level.astype(np.int64) + tag).astype(case.dtype)
    return oracle.tile_frame(shifted, *tile_of(case, level))


# ---- device side (torch is plumbing only) -----------------------------------

def torch_view_dtype(torch, dtype):
    """The torch dtype the bytes are added and compared in: uint16 as int16
    (two's-complement addition gives the same bits), float32 as itself."""
    return {"uint8": torch.uint8, "uint16": torch.int16, "float32": torch.float32}[_dn(dtype)]


def device_tags(torch, case, n_groups):
    """tag(group) as the view dtype, on the device."""
    t = torch.arange(n_groups, device="cuda", dtype=torch.int64) % modulus(case.dtype)
    if _dn(case.dtype) == "uint16":
        t = torch.where(t >= 32768, t - 65536, t)
    return t.to(torch_view_dtype(torch, case.dtype))


def to_view(torch, arr, dtype):
    """A host array on the device in the view dtype."""
    a = np.ascontiguousarray(arr)
    if _dn(dtype) == "uint16":
        a = a.view(np.int16)
    return torch.from_numpy(a.copy()).to("cuda")


def build_batch(torch, case, n):
    """The batch on the device: a uint8 tensor of n frames, plane k =
    base[k % group] + tag(k)."""
    gp = group_planes(case)
    w, h, _ = case.geo[0]
    raw = torch.empty(n * frame_bytes(case, 0), dtype=torch.uint8, device="cuda")
    vt = torch_view_dtype(torch, case.dtype)
    view = raw.view(vt).view(n // gp, gp, h, w)
    base = to_view(torch, base_group(case), case.dtype).view(1, gp, h, w)
    tags = device_tags(torch, case, n // gp).view(-1, 1, 1, 1)
    torch.add(base, tags, out=view)
    return raw


def poisoned(torch, nbytes):
    t = torch.empty(nbytes + PAD, dtype=torch.uint8, device="cuda")
    t.fill_(POISON)
    return t


def compare_frames(torch, got, want0, scale, tags, per, what):
    """got: (n, ...) frames in the view dtype, taken `per` at a time as
    groups (G, per, ...); group g must equal want0 + tags[g] * scale in bits
    (scale None: 1), where tags is (G,) or (G, ...) broadcastable against a
    group.  Compared in slabs; a mismatch names the frame and the element."""
    n = got.shape[0]
    item = tuple(got.shape[1:])
    G = n // per
    assert n % per == 0 and tags.shape[0] == G, what
    g = got.view(G, per, *item)
    if tags.dim() == 1:
        tags = tags.view(G, *((1,) * (g.dim() - 1)))
    assert tags.dim() == g.dim(), what
    bits = torch.int32 if got.dtype == torch.float32 else got.dtype
    step = max(1, SLAB_BYTES // (per * int(np.prod(item)) * got.element_size()))

    def expect(t):
        return want0 + t if scale is None else want0 + t * scale

    bad = []
    for a in range(0, G, step):
        b = min(G, a + step)
        ne = g[a:b].view(bits) != expect(tags[a:b]).view(bits)
        bad.append(ne.flatten(1).any(1))
        del ne
    bad = torch.cat(bad)
    n_bad = int(bad.sum())
    if n_bad == 0:
        return
    gi = int(torch.nonzero(bad)[0])
    exp = expect(tags[gi]).expand(per, *item)
    at = tuple(torch.nonzero(g[gi].view(bits) != exp.view(bits))[0].tolist())
    raise AssertionError(
        f"{what}: {n_bad} of {G} groups of {per} frame(s) differ; first at group {gi} "
        f"(level frame {gi * per + at[0]}, tag {int(tags[gi].flatten()[0])}) element {at[1:]}: "
        f"got {g[gi][at].item()!r}, expected {exp[at].item()!r}")


# ---- codec cases (tests/test_gpu_large_codecs.py) ------------------------------

FILTER_TS, FILTER_BS = 3, 3000
FILTER_CASES = {f"filter-s{s}-x{nbuf}": (s, nbuf) for s in (1, 2, 0) for nbuf in (1, 2)}


def filter_nbytes(nbuf):
    return ((1 << 31) if nbuf == 1 else (1 << 30)) + 3 * FILTER_BS + 1000


def filter_windows(nbuf):
    """(name, first global block, blocks) of the full-block run to compare,
    and the launch cap in blocks."""
    per = filter_nbytes(nbuf) // FILTER_BS
    total = per * nbuf
    cap = (1 << 31) // FILTER_BS
    assert total > cap
    win = [("first block", 0, 1), ("last full block", total - 1, 1)]
    for b in range(cap, total, cap):
        win.append((f"launch boundary at block {b}", b - 2, 4))
    if nbuf > 1:
        win.append(("buffer boundary", per - 1, 2))
    return win, cap, per, total


CRC_CASES = {
    "crc-all-levels": 65535 * 16384 - 7,             # every bit of the workgroup index set
    "crc-levels-15-9-0": ((1 << 15) + (1 << 9) + 1) * 16384,
}
CRC_LIMIT = "crc-limit"

LZ4_CHUNK = 131072
LZ4_PROTOS = 5
LZ4_CASES = {"lz4-batch": 0, "lz4-serial": 1}


def lz4_chunks():
    return -(-(1 << 32) // LZ4_CHUNK) + 5


# ---- the child process (tests/large_batch_child.py) --------------------------

_GROUPS = {}
CHILD_TIMEOUT_S = {"row": 900, "volume": 420, "deep": 420, "tiled": 420, "filter": 420,
                   "crc": 300, "lz4": 420,
                   # ten cases, 8 s in all when measured (profiles/volume_tiled_tests/)
                   "volume_tiled": 300}


def run_group(group):
    """{case id: record} of one child run per group and pytest process, the
    launch log on.  A child that ended by signal, abort, HIP error or timeout
    is not started again: its missing cases fail with that reason."""
    import json
    import os
    import subprocess
    import sys
    if group in _GROUPS:
        return _GROUPS[group]
    if any(r.get("_fatal") for r in _GROUPS.values()):
        _GROUPS[group] = {"_fatal": "not started: an earlier large-batch child ended badly"}
        return _GROUPS[group]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["AQZ_LAUNCH_LOG"] = "1"
    import tempfile
    fatal = None
    with tempfile.TemporaryFile("w+") as f:     # the child's lines, as they come
        try:
            r = subprocess.run([sys.executable, "-u",
                                os.path.join(root, "tests", "large_batch_child.py"),
                                "--group", group], cwd=root, env=env, stdout=f,
                               stderr=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT_S[group])
            if r.returncode != 0:
                fatal = f"child of group {group} ended with status {r.returncode}: " + \
                    r.stderr[-1500:]
        except subprocess.TimeoutExpired:
            fatal = f"child of group {group} timed out"
        f.seek(0)
        out = f.read()
    if not fatal and "DONE" not in out.splitlines():
        fatal = f"child of group {group} did not finish"
    recs = {}
    for line in out.splitlines():
        if line.startswith("{"):
            rec = json.loads(line)
            recs[rec["case"]] = rec
    if fatal:
        recs["_fatal"] = fatal
    _GROUPS[group] = recs
    return recs


def record_of(group, cid):
    """The child's record of one case; skips (memory, no liblz4) and failed
    comparisons are raised here, in the case's own test."""
    import pytest
    recs = run_group(group)
    rec = recs.get(cid)
    if rec is None:
        pytest.fail(f"{cid}: no record; {recs.get('_fatal', 'the child did not run it')}")
    print(f"{cid}: {rec['seconds']} s in the child")
    if rec["skip"]:
        pytest.skip(rec["skip"])
    assert rec["error"] is None, rec["error"]
    return rec


def shows(launches, fields):
    return any(all(rec.get(k) == v for k, v in fields.items()) for rec in launches)


# ---- CRC-32C of a large buffer, from the oracle's checksums of its parts ------

_CRC32C_POLY = 0x82F63B78


def _gf2_times(mat, vec):
    out, i = 0, 0
    while vec:
        if vec & 1:
            out ^= mat[i]
        vec >>= 1
        i += 1
    return out


def _gf2_square(mat):
    return [_gf2_times(mat, mat[n]) for n in range(32)]


def crc32c_combine(crc1, crc2, len2):
    """CRC-32C of A + B from crc(A), crc(B) and len(B): zlib's crc32_combine
    with the Castagnoli polynomial (tests/test_large_batch_cases.py holds it
    to oracle.crc32c of the whole)."""
    if len2 <= 0:
        return crc1
    odd = [_CRC32C_POLY] + [1 << n for n in range(31)]
    even = _gf2_square(odd)
    odd = _gf2_square(even)
    while True:
        even = _gf2_square(odd)
        if len2 & 1:
            crc1 = _gf2_times(even, crc1)
        len2 >>= 1
        if not len2:
            break
        odd = _gf2_square(even)
        if len2 & 1:
            crc1 = _gf2_times(odd, crc1)
        len2 >>= 1
        if not len2:
            break
    return crc1 ^ crc2


def oracle_crc32c_parts(oracle, buf, parts=16):
    """oracle.crc32c of `buf`, its parts checksummed side by side (the oracle
    goes byte by byte: a GiB takes it over ten seconds in one piece)."""
    from concurrent.futures import ThreadPoolExecutor
    n = buf.size
    cuts = [n * i // parts for i in range(parts + 1)]
    with ThreadPoolExecutor(parts) as pool:
        crcs = list(pool.map(lambda i: oracle.crc32c(buf[cuts[i]:cuts[i + 1]]), range(parts)))
    crc = crcs[0]
    for i in range(1, parts):
        crc = crc32c_combine(crc, crcs[i], cuts[i + 1] - cuts[i])
    return crc
