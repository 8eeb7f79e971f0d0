"""Shared pieces of the tiled-base tests (not a test module, not a conftest):
the cases tests/test_gpu_tiled_base.py runs on the GPU and
tests/test_tiled_base_plan.py plans on the CPU, the expected bytes — always the
oracle's (oracle.tile_frame of the frame itself for level 0, of
oracle.cascade_2d for the rest, placed by oracle.chunk_frame_offsets) — and the
poisoned device buffers."""
import zlib

import numpy as np

SPACE, CHANNEL, TIME = 0, 1, 2
POISON = 0xA5
GUARD = 64  # poisoned bytes behind every buffer, checked after the run
MAX_FUSED = 4

DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16,
          np.int32, np.int64, np.float32, np.float64]
DTYPE_CODE = {np.dtype(d).name: i for i, d in enumerate(DTYPES)}


def case(name, w, h, levels, dtype, tiles, frames=2):
    """tiles: (rows, cols) per level from 0; a list shorter than `levels`
    repeats its last entry."""
    tiles = list(tiles) + [tiles[-1]] * (levels - len(tiles))
    return dict(name=name, w=w, h=h, levels=levels, dtype=dtype, tiles=tiles, n=frames)


NEST = (8, 64)      # nests at every level >= 1 of 1024-wide u16, five levels
GENERAL = (100, 60)  # nests nowhere

# The named shapes, with the base path each has to reach (paths_of).
CASES = [
    # pw 1088 < cov_w 1536: columns 1031..1087 of every row come from lanes that
    # hold the next row's pixels, the last row of the last frame from a shifted load
    # (rows 528..575 of the padded base are the zero-fill waves', and so are their slots)
    (case("stale", 1031, 517, 5, np.uint16, [(64, 64)], 3), {"nested", "row_fill", "slot_fill"}),
    # base columns 512..599 belong to the zero-fill waves, 300..511 to the units
    (case("colfill_base", 300, 7, 2, np.uint8, [(4, 600), (4, 128)], 3),
     {"general", "column_fill"}),
    # ... and the reverse: only level 1 zero-fills
    (case("colfill_level1", 300, 7, 2, np.uint8, [(8, 512), (4, 300)], 3), {"nested"}),
    # rows 40..47 to the zero-fill waves; 60 is no multiple of a lane's 8 columns
    (case("rowfill", 640, 40, 3, np.uint16, [(48, 60), (24, 30)], 2), {"row_fill", "general"}),
    # flag slots: blocks (16 rows x 512 columns) spanning two tiles, inside a
    # tile, and not nesting; each with the other levels nested or one general
    (case("slots_span", 1024, 64, 5, np.uint16, [(32, 256), NEST], 3), {"nested"}),
    (case("slots_span_l2gen", 1024, 64, 5, np.uint16, [(32, 256), NEST, GENERAL, NEST], 3),
     {"nested"}),
    (case("slots_inside", 1024, 64, 5, np.uint16, [(16, 1024), NEST], 3), {"nested"}),
    (case("slots_inside_l2gen", 1024, 64, 5, np.uint16, [(16, 1024), NEST, GENERAL, NEST], 3),
     {"nested"}),
    (case("slots_none", 1024, 64, 5, np.uint16, [GENERAL, NEST], 3), {"general"}),
    (case("slots_none_l2gen", 1024, 64, 5, np.uint16, [GENERAL, NEST, GENERAL, NEST], 3),
     {"general"}),
    # the slot row over rows 48..63 belongs to no wave: zero-fill waves write it
    (case("slots_rowfill", 1024, 40, 5, np.uint16, [(32, 256), NEST], 3),
     {"nested", "row_fill", "slot_fill"}),
    (case("slots_f32", 1024, 64, 5, np.float32, [(32, 256), NEST], 3), {"nested"}),
    # chains: only the first run knows level 0
    (case("chain2_small", 2100, 700, 7, np.uint8, [(8, 16)], 2), set()),
    (case("chain2_big", 2100, 700, 7, np.uint8, [(64, 256), (8, 16)], 2), set()),
    (case("chain3_small", 4100, 600, 10, np.uint8, [(8, 16), (8, 8)], 2), set()),
    (case("chain3_big", 4100, 600, 10, np.uint8, [(64, 256), (8, 8)], 2), set()),
]
CASE = {c["name"]: c for c, _ in CASES}
SLOT_CASES = {"slots_span": 2, "slots_span_l2gen": 2, "slots_inside": 2, "slots_inside_l2gen": 2,
              "slots_none": 1, "slots_none_l2gen": 1, "slots_rowfill": 2}
SWEEP = dict(w=520, h=301, levels=4, tile=(64, 96))  # every dtype x every method
# f32 / f64 widths by the tile width the planner picks: rows of whole KiB take
# the half-width tile, others the full one (32 bytes a lane)
COLS_CASES = [(np.float32, 520, 8), (np.float32, 512, 4), (np.float64, 520, 4),
              (np.float64, 512, 2)]


def halving(w, h, n):
    geo = [(w, h, 1)]
    for _ in range(1, n):
        w, h = (w + 1) // 2, (h + 1) // 2
        geo.append((w, h, 1))
    return geo


def n_tiles(geo, L, tile):
    w, h, _ = geo[L]
    return (-(-h // tile[0])) * (-(-w // tile[1]))


def request(c, n=None, extra=""):
    """The probe request of the case's first fused run (the run with the base)."""
    k = min(c["levels"] - 1, MAX_FUSED)
    tiles = ",".join(f"{r}x{q}" for r, q in c["tiles"][: k + 1])
    return f"{DTYPE_CODE[np.dtype(c['dtype']).name]} {c.get('method', 1)} {c['w']} {c['h']} " \
           f"{k} {c['n'] if n is None else n} tiles={tiles} {extra}".strip()


def paths_of(rec, flags=True):
    """The base paths a plan (parse_plan of the probe's line) takes."""
    p = {"nested" if rec["slots0"] else "general"}
    if rec["cov_w0"] < rec["pw0"]:
        p.add("column_fill")
    elif rec["cov_h0"] < rec["ph0"]:
        p.add("row_fill")
    if flags and rec["slots0"] and (rec["cov_w0"] < rec["pw0"] or rec["cov_h0"] < rec["ph0"]):
        p.add("slot_fill")
    return p


PATHS = ("nested", "general", "column_fill", "row_fill", "slot_fill")


# ---- expected bytes ---------------------------------------------------------------

def case_frames(c, seed=None, specials=False):
    """Random frames; the first has its top left quarter zero (zero tiles at
    every level), the second is all zero but one pixel."""
    from gpu_util import random_frames
    rng = np.random.default_rng(c["w"] * 7919 + c["h"] if seed is None else seed)
    frames = random_frames(rng, c["dtype"], (c["n"], c["h"], c["w"]), specials=specials)
    frames[0][: c["h"] // 2, : c["w"] // 2] = 0
    if c["n"] > 1:
        frames[1][:] = 0
        frames[1][c["h"] - 1, c["w"] // 3] = 1
    return frames


def expected(oracle, frames, levels, method, tiles):
    """want[L] = (tiles[n, n_tiles, tr, tc], nonzero[n, n_tiles] bool), L from 0."""
    per = [[] for _ in range(levels)]
    for fr in frames:
        lv = [fr] + list(oracle.cascade_2d(fr, levels, method))
        for L in range(levels):
            per[L].append(oracle.tile_frame(lv[L], *tiles[L]))
    return [(np.stack([a for a, _ in p]), np.stack([b for _, b in p])) for p in per]


def offset_input(frames, off=0):
    """The frames on the device `off` elements into a poisoned buffer, with
    guard bytes behind: (tensor, address of the first frame)."""
    from gpu_util import to_device
    bpp = frames.dtype.itemsize
    raw = np.full(off * bpp + frames.nbytes + GUARD, POISON, np.uint8)
    raw[off * bpp: off * bpp + frames.nbytes] = frames.view(np.uint8).reshape(-1)
    d = to_device(raw)
    return d, d.data_ptr() + off * bpp


class Outputs:
    """Poisoned tile and flag buffers of one batch of `n` frames, level 0
    included (base=False: the existing call's, index 0 unused).  Level L's
    tiles start `offs[L]` elements into their buffer; every buffer ends in
    GUARD bytes, and check() wants the bytes in front and the guards still
    poisoned."""

    def __init__(self, ds, geo, dtype, tiles, n, with_flags=True, offs=None, base=True):
        from gpu_util import empty_device
        bpp = np.dtype(dtype).itemsize
        self.geo, self.dtype, self.tiles, self.n, self.base = geo, dtype, tiles, n, base
        self.levels = list(range(0 if base else 1, len(geo)))
        self.offs = [0] * len(geo) if offs is None else offs
        self.nt, self.slots, self.nbytes = {}, {}, {}
        self.outs, self.flags = {}, {}
        for L in self.levels:
            self.nt[L] = n_tiles(geo, L, tiles[L])
            self.slots[L] = ds.tiled_flag_slots(L, *tiles[L]) if L else \
                ds.tiled_base_flag_slots(*tiles[0])
            assert self.slots[L] >= 1, (L, tiles[L])
            self.nbytes[L] = n * self.nt[L] * tiles[L][0] * tiles[L][1] * bpp
            self.outs[L] = empty_device(self.offs[L] * bpp + self.nbytes[L] + GUARD)
            self.flags[L] = empty_device(n * self.nt[L] * self.slots[L] + GUARD) \
                if with_flags else None
        self.poison()

    def poison(self):
        for b in list(self.outs.values()) + list(self.flags.values()):
            if b is not None:
                b.fill_(POISON)

    def out_ptrs(self):
        bpp = np.dtype(self.dtype).itemsize
        return [self.outs[L].data_ptr() + self.offs[L] * bpp if L in self.outs else 0
                for L in range(len(self.geo))]

    def flag_ptrs(self):
        if self.flags[self.levels[0]] is None:
            return None
        return [self.flags[L].data_ptr() if L in self.flags else 0 for L in range(len(self.geo))]

    def run(self, ds, src, stream=None):
        from gpu_util import launch_stream
        fn = ds.run_device_batch_tiled_base if self.base else ds.run_device_batch_tiled
        tiles = [self.tiles[L] if L in self.outs else None for L in range(len(self.geo))]
        return fn(src, self.n, tiles, self.out_ptrs(), self.flag_ptrs(),
                  launch_stream() if stream is None else stream)

    def tile_bytes(self, L):
        from gpu_util import from_device
        raw = from_device(self.outs[L], np.uint8, (-1,))
        at = self.offs[L] * np.dtype(self.dtype).itemsize
        return raw[:at], raw[at: at + self.nbytes[L]], raw[at + self.nbytes[L]:]

    def flag_bytes(self, L):
        from gpu_util import from_device
        raw = from_device(self.flags[L], np.uint8, (-1,))
        return raw[:-GUARD].reshape(self.n, self.nt[L], self.slots[L]), raw[-GUARD:]

    def still_poison(self):
        from gpu_util import from_device
        return all((from_device(b, np.uint8, (-1,)) == POISON).all()
                   for b in list(self.outs.values()) + list(self.flags.values()) if b is not None)

    def check(self, want, ctx, levels=None):
        from gpu_util import assert_parity
        for L in (self.levels if levels is None else levels):
            tr, tc = self.tiles[L]
            want_t, want_nz = want[L]
            front, body, guard = self.tile_bytes(L)
            assert (front == POISON).all(), f"{ctx} L{L}: bytes in front of the tiles written"
            assert (guard == POISON).all(), f"{ctx} L{L}: guard bytes written"
            got = body.view(self.dtype).reshape(self.n, self.nt[L], tr, tc)
            assert_parity(got, want_t, f"{ctx} L{L} tiles")
            if self.flags[L] is not None:
                raw, guard = self.flag_bytes(L)
                assert (guard == POISON).all(), f"{ctx} L{L}: flag guard bytes written"
                assert np.isin(raw, (0, 1)).all(), f"{ctx} L{L}: a flag byte is neither 0 nor 1"
                assert np.array_equal(raw.any(axis=-1), want_nz), f"{ctx} L{L} zero scan"


# ---- chunk lattice ------------------------------------------------------------------

def chunk_dims(geo, L, shape):
    """Level L as a T/Y/X array appended along T, chunks of shape (t, y, x)."""
    w, h, _ = geo[L]
    return [(TIME, 0, shape[0], 1), (SPACE, h, shape[1], 1), (SPACE, w, shape[2], 1)]


class Lattice:
    """One chunked batch with the base: frames first .. first + n - 1 of the
    stream, a poisoned lattice and flag buffer per level from 0 (GUARD bytes
    behind each), expected bytes from the oracle at the oracle's places.
    `room`: lattice bytes to allocate at the least per level."""

    def __init__(self, oracle, ds, geo, shapes, dtype, method, frames, first, with_flags=True,
                 in_off=0, room=0):
        from gpu_util import empty_device
        self.geo, self.shapes, self.n, self.dtype = geo, shapes, len(frames), dtype
        bpp = np.dtype(dtype).itemsize
        tiles = [s[1:] for s in shapes]
        self.tiles = tiles
        self.want_tiles = expected(oracle, frames, len(geo), method, tiles)
        self.d_in, self.src = offset_input(frames, in_off)
        self.want, self.bufs, self.flags, self.nt, self.slots = [], [], [], [], []
        for L in range(len(geo)):
            offs, cb, lb = oracle.chunk_frame_offsets(chunk_dims(geo, L, shapes[L]), bpp, first,
                                                      self.n)
            cap = (max(offs) // lb + 1) * lb
            buf = np.full(cap, POISON, np.uint8)
            tb = tiles[L][0] * tiles[L][1] * bpp
            for k in range(self.n):
                t = self.want_tiles[L][0][k]
                at = offs[k] + np.arange(t.shape[0], dtype=np.int64)[:, None] * cb
                buf[at + np.arange(tb, dtype=np.int64)[None, :]] = \
                    t.view(np.uint8).reshape(t.shape[0], tb)
            self.want.append((buf, offs, cb, lb, cap))
            self.bufs.append(empty_device(max(cap, room) + GUARD))
            self.nt.append(n_tiles(geo, L, tiles[L]))
            self.slots.append(ds.tiled_flag_slots(L, *tiles[L]) if L else
                              ds.tiled_base_flag_slots(*tiles[0]))
            self.flags.append(empty_device(self.n * self.nt[L] * self.slots[L] + GUARD)
                              if with_flags else None)
        self.poison()

    def poison(self):
        for b in self.bufs + self.flags:
            if b is not None:
                b.fill_(POISON)

    def lattices(self, **change):
        """The call's lattice tuples; change = {L: {field: value}} overrides."""
        lats = []
        for L in range(len(self.geo)):
            _, offs, cb, _, cap = self.want[L]
            d = dict(base=self.bufs[L].data_ptr(), cap=cap, tr=self.tiles[L][0],
                     tc=self.tiles[L][1], stride=cb, offs=list(offs))
            d.update(change.get(f"L{L}", {}))
            lats.append((d["base"], d["cap"], d["tr"], d["tc"], d["stride"], d["offs"]))
        return lats

    def run(self, ds, stream, **change):
        flags = None
        if self.flags[0] is not None:
            flags = [f.data_ptr() for f in self.flags]
        return ds.run_device_batch_chunked_base(self.src, self.n, self.lattices(**change), flags,
                                                stream)

    def still_poison(self):
        from gpu_util import from_device
        return all((from_device(b, np.uint8, (-1,)) == POISON).all()
                   for b in self.bufs + self.flags if b is not None)

    def check(self, ctx):
        """Every lattice byte: tiles where a frame owns them, poison elsewhere
        and in the guards; flags exactly 0 or 1."""
        from gpu_util import from_device
        for L in range(len(self.geo)):
            got = from_device(self.bufs[L], np.uint8, (-1,))
            cap = self.want[L][4]
            assert (got[cap:] == POISON).all(), f"{ctx} L{L}: bytes past the lattice written"
            bad = np.flatnonzero(got[:cap] != self.want[L][0])
            assert bad.size == 0, f"{ctx} L{L}: {bad.size} bytes differ, first at {bad[0]}"
            if self.flags[L] is not None:
                raw = from_device(self.flags[L], np.uint8, (-1,))
                assert (raw[-GUARD:] == POISON).all(), f"{ctx} L{L}: flag guard bytes written"
                raw = raw[:-GUARD].reshape(self.n, self.nt[L], self.slots[L])
                assert np.isin(raw, (0, 1)).all(), f"{ctx} L{L}: a flag byte is neither 0 nor 1"
                assert np.array_equal(raw.any(axis=-1), self.want_tiles[L][1]), f"{ctx} L{L} flags"


# ---- seeded fuzz ----------------------------------------------------------------------

FUZZ_INPUT_BYTES = 8 << 20
FUZZ_LEVEL_BYTES = 16 << 20  # every padded level (tiles, or lattice capacity)
N_FUZZ_TILED, N_FUZZ_CHUNKED = 64, 24


def fuzz_wmin(bpp, levels):
    """The smallest width whose run sources (levels 0, 4) hold one 16-byte
    load and whose every level is strictly narrower than the one before."""
    w = 1
    while True:
        ws = [w]
        for _ in range(1, levels):
            ws.append((ws[-1] + 1) // 2)
        if all(ws[L] >= 16 // bpp for L in (0, 4) if L < levels - 1) and \
                all(ws[L] < ws[L - 1] for L in range(1, levels)):
            return w
        w += 1


def _fuzz_side(rng):
    if rng.random() < 0.5:
        return int(rng.choice([16, 32, 64, 128, 256, 512, 1024]))
    return int(np.exp(rng.uniform(0, np.log(300))))


def _fuzz_pyramid(rng):
    weights = np.array([3, 6, 1, 1, 1, 1, 1, 1, 4, 1], dtype=float)
    dtype = DTYPES[int(rng.choice(len(DTYPES), p=weights / weights.sum()))]
    method = int(rng.integers(4))
    levels = int(rng.integers(2, 8))
    bpp = np.dtype(dtype).itemsize
    w = int(np.exp(rng.uniform(np.log(fuzz_wmin(bpp, levels)), np.log(2500))))
    h = int(np.exp(rng.uniform(0, np.log(200))))
    n = int(rng.integers(1, 5))
    while w * h * n * bpp > FUZZ_INPUT_BYTES and n > 1:
        n -= 1
    while w * h * n * bpp > FUZZ_INPUT_BYTES:
        h -= 1
    return dtype, method, levels, w, h, n


def _fit(lw, lh, tr, tc, planes, bpp):
    """Hold planes x the padded level to FUZZ_LEVEL_BYTES: halve the side that
    overhangs more."""
    while planes * (-(-lh // tr) * tr) * (-(-lw // tc) * tc) * bpp > FUZZ_LEVEL_BYTES:
        if -(-lh // tr) * tr * lw >= -(-lw // tc) * tc * lh and tr > 1:
            tr = (tr + 1) // 2
        else:
            tc = (tc + 1) // 2
    return tr, tc


def fuzz_tiled_params(i):
    """Case i of the tiled fuzz: a tile shape per level, base included."""
    rng = np.random.default_rng(zlib.crc32(f"fuzz-tiled-base{i}".encode()))
    dtype, method, levels, w, h, n = _fuzz_pyramid(rng)
    bpp = np.dtype(dtype).itemsize
    geo = halving(w, h, levels)
    tiles = []
    # one case in five: power-of-two tiles of whole blocks at every level, which
    # nest with the wave blocks, so that the all-nested kernel runs too
    nesting = rng.random() < 0.2
    for L in range(levels):
        lw, lh, _ = geo[L]
        tr, tc = _fuzz_side(rng), _fuzz_side(rng)
        if nesting:
            tr, tc = 16 << int(rng.integers(0, 3)), 64 << int(rng.integers(0, 5))
        elif L == 0 and rng.random() < 0.3:
            # past what the units reach (64 lanes of up to 32 bytes): the base's column fill
            tc = -(-lw // (2048 // bpp)) * (2048 // bpp) + int(rng.integers(1, 65))
        elif rng.random() < 0.15:
            tc = lw + int(rng.integers(1, 65))
        if L == 0 and rng.random() < 0.4:
            tr = 16 * int(rng.integers(1, 9))  # whole blocks of a four-level run
        tiles.append(_fit(lw, lh, tr, tc, n, bpp))
    return dict(name=f"fuzz{i}", dtype=dtype, method=method, levels=levels, w=w, h=h, n=n,
                geo=geo, tiles=tiles, in_off=int(rng.integers(0, 8)),
                out_off=[int(rng.integers(0, 8)) for _ in range(levels)],
                flags=bool(rng.random() < 0.75), rng=rng)


def fuzz_chunked_params(i):
    """Case i of the chunked fuzz: a T/Y/X chunk shape per level, base included,
    and a batch that starts `first` frames into the stream."""
    rng = np.random.default_rng(zlib.crc32(f"fuzz-chunked-base{i}".encode()))
    dtype, method, levels, w, h, n = _fuzz_pyramid(rng)
    bpp = np.dtype(dtype).itemsize
    geo = halving(w, h, levels)
    first = int(rng.integers(0, 7))
    shapes = []
    for L in range(levels):
        lw, lh, _ = geo[L]
        ct, cy, cx = int(rng.integers(1, 5)), _fuzz_side(rng), _fuzz_side(rng)
        cy, cx = _fit(lw, lh, cy, cx, n + 2 * ct, bpp)  # whole layers of ct frames
        shapes.append((ct, cy, cx))
    return dict(name=f"fuzzc{i}", dtype=dtype, method=method, levels=levels, w=w, h=h, n=n,
                geo=geo, shapes=shapes, tiles=[s[1:] for s in shapes], first=first,
                in_off=int(rng.integers(0, 8)), flags=bool(rng.random() < 0.75), rng=rng)


def fuzz_frames(c):
    """Random frames with the float edge values; the first frame's top left
    quarter and the whole second frame zero, so zero tiles exist."""
    from gpu_util import random_frames
    frames = random_frames(c["rng"], c["dtype"], (c["n"], c["h"], c["w"]))
    frames[0][: max(c["h"] // 2, 1), : max(c["w"] // 2, 1)] = 0
    if c["n"] > 1:
        frames[1][:] = 0
    return frames


# ---- plan_cascade_tiled with a base, on the CPU -----------------------------------------

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
    """ask(requests) -> output lines: tests/cpp/tiled_base_plan_probe.cpp with
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
        out = tempfile.mkdtemp(prefix="tiled_base_plan_probe")
        atexit.register(shutil.rmtree, out, ignore_errors=True)
        exe = os.path.join(out, "tiled_base_plan_probe")
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + csrc,
                        os.path.join(root, "tests", "cpp", "tiled_base_plan_probe.cpp"),
                        os.path.join(csrc, "ds_plan.cpp"), "-o", exe], check=True)
        _PROBE["exe"] = exe

    def ask(requests):
        env = {k: v for k, v in os.environ.items() if not k.startswith("AQZ_")}
        r = subprocess.run([_PROBE["exe"]], input="\n".join(requests) + "\n", env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(requests)
        return lines
    return ask
