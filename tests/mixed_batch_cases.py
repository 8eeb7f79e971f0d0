"""Shared pieces of the mixed-pyramid batch tests (not a test module, not a
conftest): the fixed shapes, the class arithmetic restated from the issue of
the route (level classes, runs, frames a level emits), the level-by-level
numpy model, the seeded fuzz generator, the device buffers of the GPU tests and
the CPU plan probe.  Expected bytes always come from oracle.OracleDownsampler
streaming the same frames, never from the product."""
import zlib

import numpy as np

from gpu_util import (assert_parity, empty_device, from_device, launch_stream, random_frames,
                      to_device)

DECIMATE, MEAN, MIN, MAX = 0, 1, 2, 3
METHODS = [DECIMATE, MEAN, MIN, MAX]
DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16,
          np.int32, np.int64, np.float32, np.float64]
POISON, GUARD = 0xA5, 64

# launch depths: fused volume, fused cascade, Z run
DEPTH = {"XYZ": 2, "XY": 4, "Z": 3}
SPAN_BYTES = 64 * 2 * 16   # a Z-run unit: 64 lanes x 2 vectors of 16 bytes

# name: ((w, h, planes) per level, frames in the batch, dtype, runs as
#        (class, first level, levels, frames in))
FIXED = {
    "volume2_cascade2": ([(256, 128, 8), (128, 64, 4), (64, 32, 2), (32, 16, 2), (16, 8, 2)], 16,
                         np.uint16, [("XYZ", 1, 2, 16), ("XY", 3, 2, 4)]),
    "odd_widths_rows": ([(201, 61, 4), (101, 31, 2), (51, 16, 2), (26, 8, 2)], 8, np.uint8,
                        [("XYZ", 1, 1, 8), ("XY", 2, 2, 4)]),
    "volume1_zrun3": ([(64, 48, 16), (32, 24, 8), (32, 24, 4), (32, 24, 2), (32, 24, 1)], 32,
                      np.float32, [("XYZ", 1, 1, 32), ("Z", 2, 3, 16)]),
    # 851 elements a plane: every u8 plane starts off the 16-byte grid, 3-byte tail
    "zrun3_zrun2_851": ([(37, 23, 32), (37, 23, 16), (37, 23, 8), (37, 23, 4), (37, 23, 2),
                         (37, 23, 1)], 64, np.uint8, [("Z", 1, 3, 64), ("Z", 4, 2, 8)]),
    "z_then_xy": ([(64, 32, 4), (64, 32, 2), (32, 16, 2)], 8, np.uint16,
                  [("Z", 1, 1, 8), ("XY", 2, 1, 4)]),
    "xy_xyz_z": ([(100, 50, 8), (50, 25, 8), (25, 13, 4), (25, 13, 2)], 16, np.int16,
                 [("XY", 1, 1, 16), ("XYZ", 2, 1, 16), ("Z", 3, 1, 8)]),
    "one_element": ([(1, 1, 2), (1, 1, 1)], 6, np.uint16, [("Z", 1, 1, 6)]),
    # one byte past, and one byte short of, one span of 2048 bytes
    "span_plus_1": ([(2049, 1, 8), (2049, 1, 4), (2049, 1, 2), (2049, 1, 1)], 8, np.uint8,
                    [("Z", 1, 3, 8)]),
    "span_minus_1": ([(2047, 1, 8), (2047, 1, 4), (2047, 1, 2), (2047, 1, 1)], 8, np.uint8,
                     [("Z", 1, 3, 8)]),
    "many_tiny_groups": ([(8, 4, 4), (8, 4, 2)], 2048, np.uint16, [("Z", 1, 1, 2048)]),
}
FIXED_NAMES = list(FIXED)
SWEEP_SHAPES = ["zrun3_zrun2_851", "xy_xyz_z"]       # the fourth and the sixth
OFFSET_SHAPES = ["volume2_cascade2", "zrun3_zrun2_851"]   # the first and the fourth
FLOAT_SHAPES = ["volume1_zrun3", "zrun3_zrun2_851"]  # the third and the fourth


# ---- class arithmetic ------------------------------------------------------------

def level_class(a, b):
    """Class of level `b` = (w, h, planes) behind level `a`, or None."""
    xy = b[0] < a[0] or b[1] < a[1]
    zh = b[2] < a[2]
    return "XYZ" if xy and zh else "XY" if xy else "Z" if zh else None


def classes(geo):
    return [None] + [level_class(geo[l - 1], geo[l]) for l in range(1, len(geo))]


def zcount(geo, L):
    return sum(1 for c in classes(geo)[1:L + 1] if c in ("XYZ", "Z"))


def emitted(geo, n):
    """Frames every level emits for a batch of n frames."""
    return [n >> zcount(geo, L) for L in range(len(geo))]


def runs_of(geo, n):
    """The run list by the rule alone: maximal stretches of one class in
    pieces of the class's launch depth; or None where the route refuses
    (a classless level, an odd plane count in front of a Z-halving level,
    n off the multiple).  Stored planes are the caller's to add."""
    cls = classes(geo)
    for l in range(1, len(geo)):
        if cls[l] is None or (cls[l] != "XY" and geo[l - 1][2] % 2):
            return None
    if n == 0 or n % (1 << zcount(geo, len(geo) - 1)):
        return None
    out, l = [], 1
    while l < len(geo):
        end = l
        while end < len(geo) and cls[end] == cls[l]:
            end += 1
        while l < end:
            k = min(DEPTH[cls[l]], end - l)
            out.append((cls[l], l, k, n >> zcount(geo, l - 1)))
            l += k
    return out


def zrun_shape(elems, bpp, n_out, planes):
    """(groups, spans, grid) of a Z run, from the unit shape: one wave a plane
    group by span, spans fastest, four waves a workgroup."""
    groups = planes >> n_out
    spans = -(-(elems * bpp) // SPAN_BYTES)
    return groups, spans, -(-(groups * spans) // 4)


# ---- expectations ----------------------------------------------------------------

def oracle_levels(oracle, geo, dtype, method, frames, ref=None):
    """levels[L] = the frames level L emits for `frames`, stacked (an empty
    list where it emits none)."""
    ref = ref or oracle.OracleDownsampler(geo, dtype, method)
    out = [[] for _ in geo]
    for fr in frames:
        ref.add_frame(fr)
        for L in range(1, len(geo)):
            p = ref.take_frame(L)
            if p is not None:
                out[L].append(p)
    return [None] + [np.stack(v) if v else np.empty((0, geo[L][1], geo[L][0]), dtype)
                     for L, v in enumerate(out) if L]


def _reduce(method, ops, dtype):
    """The reference's reducers on stacked operands (u8 and f32 as the issue's
    CPU run; narrow integers promote to int, floats sum left to right)."""
    if method == DECIMATE:
        return ops[0].copy()
    if method == MEAN:
        if np.dtype(dtype).kind == "f":
            s = ops[0]
            for o in ops[1:]:
                s = (s + o).astype(dtype)
            return (s / dtype(len(ops))).astype(dtype)
        s = sum(o.astype(np.int64) for o in ops)
        return (s // len(ops)).astype(dtype)
    v = ops[0].copy()
    for o in ops[1:]:
        v = np.where(o < v, o, v) if method == MIN else np.where(o > v, o, v)
    return v


def model_levels(geo, dtype, method, frames):
    """Level by level: XY-reduce every plane (odd edges replicated), then pair
    consecutive planes.  Finite inputs, u8 and f32."""
    dtype = np.dtype(dtype).type
    cur = np.asarray(frames)
    out = [None]
    for L in range(1, len(geo)):
        c = level_class(geo[L - 1], geo[L])
        if c in ("XYZ", "XY"):
            n, h, w = cur.shape
            pad = np.pad(cur, ((0, 0), (0, h % 2), (0, w % 2)), mode="edge")
            ops = [pad[:, 0::2, 0::2], pad[:, 0::2, 1::2], pad[:, 1::2, 0::2], pad[:, 1::2, 1::2]]
            cur = _reduce(method, ops, dtype)
        if c in ("XYZ", "Z"):
            cur = _reduce(method, [cur[0::2], cur[1::2]], dtype)
        assert cur.shape[1:] == (geo[L][1], geo[L][0]), (L, cur.shape, geo[L])
        out.append(cur)
    return out


def fixed_frames(name, dtype=None, seed=0):
    geo, n, dt, _ = FIXED[name]
    dtype = dt if dtype is None else dtype
    rng = np.random.default_rng(zlib.crc32(f"mixed-{name}-{np.dtype(dtype).name}-{seed}".encode()))
    return random_frames(rng, dtype, (n, geo[0][1], geo[0][0]))


# ---- seeded fuzz -----------------------------------------------------------------

N_FUZZ = 48
CATEGORIES = ["xyz_then_xy", "xyz_then_z", "z_first", "z_then_xy", "all_three"]


def fuzz_case(i):
    """Case i: 2-6 levels, a random class per level (every other case in the
    level planner's own form: XYZ levels, then a tail of one class), w, h <=
    96, plane counts built backwards from 1-3 at the last level, 1-3 stacks,
    any dtype and method, element offsets in every other case.  Only pyramids
    the route accepts: an XY-halving level needs something left to halve, a
    fused-volume level a source row of one 16-byte load; never pure XY or
    pure XYZ (those are kinds 1 and 2)."""
    rng = np.random.default_rng(zlib.crc32(f"fuzz-mixed-batch{i}".encode()))
    while True:
        dtype = DTYPES[int(rng.integers(len(DTYPES)))]
        bpp = np.dtype(dtype).itemsize
        method = int(rng.integers(4))
        levels = int(rng.integers(2, 7))
        if i % 2:
            head = int(rng.integers(0, levels - 1))
            tail = ["XY", "Z"][int(rng.integers(2))]
            cls = ["XYZ"] * head + [tail] * (levels - 1 - head)
        else:
            cls = [["XYZ", "XY", "Z"][int(rng.integers(3))] for _ in range(levels - 1)]
        w, h = int(rng.integers(1, 97)), int(rng.integers(1, 97))
        sizes = [(w, h)]
        for k, c in enumerate(cls):
            if c != "Z" and (max(w, h) == 1 or (c == "XYZ" and w * bpp < 16)):
                c = cls[k] = "Z"
            if c != "Z":
                w, h = (w + 1) // 2, (h + 1) // 2
            sizes.append((w, h))
        if len(set(cls)) == 1 and cls[0] != "Z":
            continue
        planes = [int(rng.integers(1, 4))]
        for c in reversed(cls):
            planes.insert(0, planes[0] * (1 if c == "XY" else 2))
        geo = [(sw, sh, p) for (sw, sh), p in zip(sizes, planes)]
        stacks = int(rng.integers(1, 4))
        offs = [int(x) for x in rng.integers(1, 8, levels)] if i % 4 >= 2 else [0] * levels
        assert classes(geo)[1:] == cls, (geo, cls)
        return dict(geo=geo, n=planes[0] * stacks, dtype=dtype, method=method, offs=offs,
                    cls=cls, rng=rng)


def fuzz_categories(c):
    cls = c["cls"]
    pairs = set(zip(cls, cls[1:]))
    out = set()
    if ("XYZ", "XY") in pairs:
        out.add("xyz_then_xy")
    if ("XYZ", "Z") in pairs:
        out.add("xyz_then_z")
    if cls[0] == "Z":
        out.add("z_first")
    if ("Z", "XY") in pairs:
        out.add("z_then_xy")
    if set(cls) == {"XYZ", "XY", "Z"}:
        out.add("all_three")
    return out


# ---- device buffers of the GPU tests (torch is loaded at the first use) ------------

class Batch:
    """One batch on the device: the frames `offs[0]` elements into a poisoned
    buffer, every level's output `offs[L]` elements into one, GUARD poisoned
    bytes on both sides of each.  check() wants the levels equal to the
    expectation bit for bit and every byte around them still poisoned."""

    def __init__(self, geo, dtype, frames, counts, offs=None):
        self.geo, self.dtype, self.n = geo, np.dtype(dtype), len(frames)
        self.bpp = self.dtype.itemsize
        self.offs = offs or [0] * len(geo)
        self.counts = counts
        raw = np.full(2 * GUARD + self.offs[0] * self.bpp + frames.nbytes, POISON, np.uint8)
        at = GUARD + self.offs[0] * self.bpp
        raw[at: at + frames.nbytes] = np.ascontiguousarray(frames).view(np.uint8).reshape(-1)
        self.d_in = to_device(raw)
        self.src = self.d_in.data_ptr() + at
        self.nbytes = [0] + [counts[L] * geo[L][0] * geo[L][1] * self.bpp
                             for L in range(1, len(geo))]
        self.outs = [None] + [empty_device(2 * GUARD + self.offs[L] * self.bpp + self.nbytes[L])
                              for L in range(1, len(geo))]
        for o in self.outs[1:]:
            o.fill_(POISON)

    def ptrs(self):
        return [0] + [self.outs[L].data_ptr() + GUARD + self.offs[L] * self.bpp
                      for L in range(1, len(self.geo))]

    def run(self, ds, stream=None):
        return ds.run_device_batch(self.src, self.n, self.ptrs(),
                                   launch_stream() if stream is None else stream)

    def levels(self, ctx):
        """The levels read back; the bytes around them must be poison."""
        got = [None]
        for L in range(1, len(self.geo)):
            raw = from_device(self.outs[L], np.uint8, (-1,))
            at = GUARD + self.offs[L] * self.bpp
            assert (raw[:at] == POISON).all(), f"{ctx} L{L}: bytes in front of the level written"
            assert (raw[at + self.nbytes[L]:] == POISON).all(), f"{ctx} L{L}: guard bytes written"
            w, h, _ = self.geo[L]
            got.append(raw[at: at + self.nbytes[L]].view(self.dtype).reshape(self.counts[L], h, w))
        return got

    def check(self, want, ctx):
        got = self.levels(ctx)
        for L in range(1, len(self.geo)):
            assert_parity(got[L], want[L], f"{ctx} L{L}")
        return got


# ---- the planner on the CPU --------------------------------------------------------

_PROBE = {}


def parse_line(line):
    """A launch-log line as a dict."""
    rec = {}
    for kv in line.split():
        k, _, v = kv.partition("=")
        rec[k] = int(v) if v.lstrip("-").isdigit() else v
    return rec


def runs_request(geo, n, holds=()):
    return f"runs {n} " + " ".join(f"{w}x{h}x{p}" + ("*" if L in holds else "")
                                   for L, (w, h, p) in enumerate(geo))


def parse_runs(line):
    """[(class, first, levels, frames in)] of an `ok` answer, None of a refusal."""
    head, *rest = line.split()
    if head != "ok":
        assert head == "refused" and rest, line
        return None
    return [(c, int(a), int(b), int(d)) for c, a, b, d in (t.split(":") for t in rest)]


def plan_probe():
    """ask(requests) -> answer lines: tests/cpp/mixed_plan_probe.cpp with
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
        out = tempfile.mkdtemp(prefix="mixed_plan_probe")
        atexit.register(shutil.rmtree, out, ignore_errors=True)
        exe = os.path.join(out, "mixed_plan_probe")
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + csrc, os.path.join(root, "tests", "cpp", "mixed_plan_probe.cpp"),
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
