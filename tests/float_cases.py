"""Float frames built to reach named result classes (a plain helper, shared by
tests/test_float_cases.py on the CPU, tests/test_gpu_float_classes.py and
tests/launch_rule_child.py on the GPU, and tests/golden/
make_reference_vectors.py --float-classes).

gpu_util.random_frames never yields a Mean output that is -0.0, subnormal or
an overflow from finite operands (test_float_cases.py counts them), so the
sign of a zero, rounding in the subnormal range, intermediate overflow, zero
ties of Min / Max and signalling NaNs never reached a multi-tile launch.  The
frames here are deterministic catalogues of 2x2 windows (and Z pairs), written
as bit patterns so that nothing quiets a NaN on the way.

A class is named by the operands of ONE output and the result the reference
gives.  Operands are a, b, c, d in the order reduce4 takes them (here, right,
down, diag), or a, b for a Z pair (earlier plane, later plane).

Mean:
  neg_zero    every operand -0.0                              -> -0.0
  mixed_zero  +-0.0 mixed, x and -x cancelling                -> +0.0
  sub_exact   a subnormal result that is exact
  sub_round   sum = k x smallest subnormal, k = +-1..7 (pairs: +-1..3):
              sum/4 rounds down, up and to even both ways; k = +-1 -> +-0.0
  overflow    finite operands -> +-inf: four times max, and
              (max, max, -max, -max), whose true mean is 0
  absorb      (1e8, 1, -1e8, 1) and its orders (1e17 for float64): the
              left-to-right sum and a pairwise one differ
  nan_first   the first NaN operand at each position, quiet and signalling,
              either sign, a second NaN of another payload behind it
                                                   -> the first one, quieted
  nan_default inf + -inf at each add of the chain, also with a NaN operand
              behind it                       -> the negative default NaN
Min, Max:
  zero_tie    +0.0 against -0.0 in every order: the first operand that is
              not strictly beaten wins            -> a's bits
  sub_cmp     0 against +-smallest, +-smallest against +-3 x smallest
  nan_a       a signalling NaN with a payload at a       -> a's bits, unchanged
  nan_later   a NaN at b, c or d only                    -> ignored
  inf_max     +-inf against +-max
Decimate:
  pass_bits   a signalling NaN, -0.0 and a subnormal at a -> a's bits

Z pairs carry the same class names with two operands.  The reference's
min2 / max2 are `a < b ? a : b` and `a > b ? a : b` (downsampler.cpp:125-137):
a tie or an unordered compare gives b, not a as in the 2x2 chain.  For a pair,
zero_tie therefore comes out as b's bits, nan_a (NaN at a) is the ignored one
and nan_later (NaN at b) comes out unchanged.

Placement.  A window planted for level k holds each operand constant over a
2^(k-1) x 2^(k-1) block of level 0 (and over the planes that feed one plane of
the pair).  A constant c survives Min, Max and Decimate always, and Mean
whenever 4c is finite, since 4c / 4 is exact, subnormals included; a NaN
survives Mean quieted.  Two kinds of entries therefore exist at level 1 only,
by arithmetic (Entry.raw_only):
  * overflow under Mean: every finite level-1 value is at most max / 4 in
    magnitude, so four of them cannot overflow;
  * whatever needs a signalling NaN under Mean (half of nan_first): level 1
    quiets it.
A Z pair at a level that also halves XY sees its operands behind that level's
own 2x2 step, so there these entries do not exist at all.  Every other entry
is planted at every level of the requested geometry.

The frame is cut into S x S cells, S = 2^(XY halvings); cell (cy, cx) belongs
to level 1 + (cy + cx) % (levels - 1) and is filled with that level's windows.
Windows take the level's entries in turn, one class after the other
(round robin), so any run of len(classes) neighbouring windows holds every
class: on frames of 1024 px and more every class falls in the first 512 px,
in the last 256 px of a row band and in the last band of rows, at every
level (asserted by test_float_cases.py).  Each stack starts the turn at
another entry.

Odd edges.  Where a level's parent is odd, the last output column and row
replicate operands (right = here, down = here).  Windows there take entries
of the classes that still make sense (EDGE_CLASSES; of nan_first those whose
first NaN is at a, the operand replication keeps) in a turn of their own.

`planted()` gives, per output element, the class and the operands as that
output's reduce step sees them; test_float_cases.py holds the oracle to them.
"""
import functools
from collections import namedtuple

import numpy as np

DECIMATE, MEAN, MIN, MAX = 0, 1, 2, 3

CLASSES = {
    MEAN: ["neg_zero", "mixed_zero", "sub_exact", "sub_round", "overflow", "absorb",
           "nan_first", "nan_default"],
    MIN: ["zero_tie", "sub_cmp", "nan_a", "nan_later", "inf_max"],
    MAX: ["zero_tie", "sub_cmp", "nan_a", "nan_later", "inf_max"],
    DECIMATE: ["pass_bits"],
}
# classes that keep their meaning when operands are replicated at an odd edge
EDGE_CLASSES = ["neg_zero", "nan_a", "pass_bits", "sub_round", "zero_tie", "nan_first"]

# kind: 4 = a 2x2 window (a, b, c, d), 2 = a Z pair (a, b)
Entry = namedtuple("Entry", "name kind ops methods raw_only")
# one planted output: `frame` counts the level's emitted frames, `ops` are the
# operand bits as the output's reduce step sees them (replicated at odd edges,
# quieted behind an earlier Mean step; one operand where the last plane of an
# odd stack passes through)
Plant = namedtuple("Plant", "frame y x name ops")


class Fmt:
    """Bit patterns of one float type, as Python ints."""

    def __init__(self, dtype):
        self.dt = np.dtype(dtype)
        assert self.dt.kind == "f" and self.dt.itemsize in (4, 8), dtype
        self.ut = np.dtype(f"u{self.dt.itemsize}")
        self.nbits = 8 * self.dt.itemsize
        self.mant = 23 if self.dt.itemsize == 4 else 52
        self.sign = 1 << (self.nbits - 1)
        self.inf = ((1 << (self.nbits - 1 - self.mant)) - 1) << self.mant
        self.ninf = self.sign | self.inf
        self.quiet = 1 << (self.mant - 1)
        self.max = self.inf - 1          # largest finite value
        self.tiny = 1 << self.mant       # smallest normal value
        self.pz, self.nz = 0, self.sign
        self.default_nan = self.sign | self.inf | self.quiet  # x86's for inf - inf

    def val(self, x):
        return int(np.array(x, self.dt).view(self.ut))

    def neg(self, b):
        return b ^ self.sign

    def sub(self, k):
        """k x the smallest subnormal (its bit pattern is |k|)."""
        return k if k >= 0 else self.sign | -k

    def qnan(self, payload, neg=False):
        return (self.sign if neg else 0) | self.inf | self.quiet | payload

    def snan(self, payload, neg=False):
        assert 0 < payload < self.quiet
        return (self.sign if neg else 0) | self.inf | payload

    def is_nan(self, b):
        return (b & ~self.sign) > self.inf

    def settle(self, b):
        """What a block of constant b is behind a Mean step."""
        return b | self.quiet if self.is_nan(b) else b


def catalogue(dtype):
    f = Fmt(dtype)
    pz, nz, inf, ninf, M = f.pz, f.nz, f.inf, f.ninf, f.max
    nM = f.neg(M)
    one, two, three = f.val(1.0), f.val(2.0), f.val(3.0)
    x, nx = f.val(1.5), f.val(-1.5)
    s = f.sub
    big = f.val(1e8 if f.dt.itemsize == 4 else 1e17)   # exact; big + 1 == big
    nbig = f.neg(big)
    out = []

    def add(name, methods, ops, raw_only=False):
        out.append(Entry(name, len(ops), tuple(ops), frozenset(methods), raw_only))

    mean = (MEAN,)
    # ---- Mean, 2x2
    add("neg_zero", mean, (nz, nz, nz, nz))
    for ops in ((pz, nz, pz, nz), (nz, pz, pz, pz), (nz, nz, nz, pz), (x, nx, pz, nz),
                (nz, nz, x, nx), (s(5), s(-5), nz, nz)):
        add("mixed_zero", mean, ops)
    for ops in ((s(4),) * 4, (s(1),) * 4, (s(-2),) * 4, (f.tiny, pz, pz, pz),
                (s(3), s(5), s(7), s(1)), (f.tiny, s(-4), pz, pz)):
        add("sub_exact", mean, ops)
    for k in range(1, 8):
        parts = (k - 3 * (k // 4), k // 4, k // 4, k // 4)
        add("sub_round", mean, [s(p) for p in parts])
        add("sub_round", mean, [s(-p) if p else pz for p in parts])
    for ops in ((M, M, M, M), (nM, nM, nM, nM), (M, M, nM, nM), (nM, nM, M, M)):
        add("overflow", mean, ops, raw_only=True)
    for ops in ((big, one, nbig, one), (one, big, nbig, one), (one, one, big, nbig),
                (big, nbig, one, one), (nbig, one, big, one), (big, one, one, nbig)):
        add("absorb", mean, ops)
    for p in range(4):
        for signalling in (False, True):
            for neg in (False, True):
                nan = f.snan if signalling else f.qnan
                ops = [one, two, three, x]
                ops[p] = nan(0x1230 + p, neg)
                if p < 3:
                    ops[3 if p == 0 else p + 1] = nan(0x0ABC + p, not neg)
                add("nan_first", mean, ops, raw_only=signalling)
    q = f.qnan(0x0777)
    for ops in ((inf, ninf, one, one), (ninf, inf, one, two), (one, inf, ninf, one),
                (one, one, inf, ninf), (inf, ninf, q, one), (one, ninf, inf, q)):
        add("nan_default", mean, ops)
    # ---- Mean, Z pairs
    add("neg_zero", mean, (nz, nz))
    for ops in ((pz, nz), (nz, pz), (x, nx), (s(-3), s(3))):
        add("mixed_zero", mean, ops)
    for ops in ((s(2), s(4)), (s(1), s(1)), (f.tiny, pz), (s(-5), s(-1))):
        add("sub_exact", mean, ops)
    for k in (1, 2, 3):
        add("sub_round", mean, (s(k), pz))
        add("sub_round", mean, (pz, s(-k)))
    add("sub_round", mean, (s(2), s(1)))
    for ops in ((M, M), (nM, nM)):
        add("overflow", mean, ops, raw_only=True)
    for signalling in (False, True):
        for neg in (False, True):
            nan = f.snan if signalling else f.qnan
            add("nan_first", mean, (nan(0x1240, neg), nan(0x0AC0, not neg)), signalling)
            add("nan_first", mean, (one, nan(0x1241, neg)), signalling)
    for ops in ((inf, ninf), (ninf, inf)):
        add("nan_default", mean, ops)
    # ---- Min / Max, 2x2
    mm = (MIN, MAX)
    for m in range(1, 15):  # every mix of +0.0 and -0.0 over the four positions
        add("zero_tie", mm, [nz if (m >> i) & 1 else pz for i in range(4)])
    for ops in ((pz, s(1), s(-1), pz), (s(1), pz, nz, s(-1)), (s(-1), nz, s(1), pz),
                (nz, s(-1), pz, s(1)), (s(1), s(3), s(-1), s(-3)), (s(3), s(1), s(-3), s(-1)),
                (s(-3), s(-1), s(1), s(3)), (s(-1), s(-3), s(3), s(1))):
        add("sub_cmp", mm, ops)
    sa, sb = f.snan(0x1357), f.snan(0x0246, neg=True)
    for ops in ((sa, one, two, three), (sb, inf, ninf, pz), (sa, q, one, one),
                (sb, three, sa, one)):
        add("nan_a", mm, ops)
    for ops in ((two, sa, one, three), (two, one, sb, three), (two, three, one, q),
                (two, sa, sb, q), (one, q, three, two)):
        add("nan_later", mm, ops)
    for ops in ((inf, M, nM, ninf), (M, inf, ninf, nM), (nM, ninf, M, inf),
                (ninf, nM, inf, M), (M, M, inf, inf), (nM, ninf, ninf, nM)):
        add("inf_max", mm, ops)
    # ---- Min / Max, Z pairs
    for ops in ((pz, nz), (nz, pz)):
        add("zero_tie", mm, ops)
    for ops in ((pz, s(1)), (s(1), pz), (s(-1), pz), (nz, s(-1)), (s(1), s(3)), (s(-3), s(-1))):
        add("sub_cmp", mm, ops)
    for ops in ((sa, one), (sb, q)):
        add("nan_a", mm, ops)
    for ops in ((one, sa), (two, q)):
        add("nan_later", mm, ops)
    for ops in ((inf, M), (M, inf), (ninf, nM), (nM, ninf)):
        add("inf_max", mm, ops)
    # ---- Decimate
    dec = (DECIMATE,)
    for ops in ((sa, one, two, three), (nz, one, one, one), (s(1), two, two, two),
                (s(-3), one, q, one), (sb, one), (nz, two), (s(1), one)):
        add("pass_bits", dec, ops)
    return out


def pyramid(h, w, n_levels, planes=1):
    """(w, h, planes) per level: XY halves at every level, and so does Z
    while there is more than one plane."""
    geo = [(w, h, planes)]
    for _ in range(1, n_levels):
        w, h, planes = (w + 1) // 2, (h + 1) // 2, (planes + 1) // 2
        geo.append((w, h, planes))
    return geo


def _halves(geo, L):
    """(XY halves, Z halves) at level L."""
    return geo[L][:2] != geo[L - 1][:2], geo[L][2] < geo[L - 1][2]


def _applies(entry, geo, L):
    xy, z = _halves(geo, L)
    if not (xy if entry.kind == 4 else z):
        return False
    raw = L == 1 and (entry.kind == 4 or not xy)
    return raw or not entry.raw_only


def _turn(f, cat, geo, L, edge):
    """Catalogue indices in planting order: one class after the other.  An
    odd edge takes 2x2 entries of EDGE_CLASSES only, and of nan_first those
    whose first NaN is at a (replication drops b, c or d)."""
    by_class = {}
    for i, e in enumerate(cat):
        if edge and (e.kind != 4 or e.name not in EDGE_CLASSES or
                     (e.name == "nan_first" and not f.is_nan(e.ops[0]))):
            continue
        if _applies(e, geo, L):
            by_class.setdefault(e.name, []).append(i)
    order = [n for n in (EDGE_CLASSES if edge else sum(CLASSES.values(), [])) if n in by_class]
    order = list(dict.fromkeys(order))
    if not order:
        return []
    rounds = max(len(v) for v in by_class.values())
    return [by_class[n][r % len(by_class[n])] for r in range(rounds) for n in order]


def claimed(dtype, geometry, method, level):
    """The class names this module plants for (method, level)."""
    cat = catalogue(dtype)
    return {e.name for e in cat if method in e.methods and _applies(e, geometry, level)}


def _feeding_planes(geo, L, j):
    """Level-0 planes (within a stack) that feed plane j of level L."""
    if L == 0:
        return [j]
    if geo[L][2] < geo[L - 1][2]:
        prev = [p for p in (2 * j, 2 * j + 1) if p < geo[L - 1][2]]
    else:
        prev = [j]
    return [q for p in prev for q in _feeding_planes(geo, L - 1, p)]


def _pair_planes(geo, L, j):
    """(planes feeding the earlier operand, planes feeding the later one)."""
    if geo[L][2] < geo[L - 1][2]:
        later = _feeding_planes(geo, L - 1, 2 * j + 1) if 2 * j + 1 < geo[L - 1][2] else []
        return _feeding_planes(geo, L - 1, 2 * j), later
    return _feeding_planes(geo, L - 1, j), None


@functools.lru_cache(maxsize=8)
def _layout(dtype_name, n, geo):
    f = Fmt(dtype_name)
    cat = catalogue(dtype_name)
    w, h, planes = geo[0]
    assert n % planes == 0, "whole stacks only"
    n_levels = len(geo)
    ops = np.zeros((len(cat), 4), f.ut)
    for i, e in enumerate(cat):
        ops[i, :e.kind] = [f.ut.type(b) for b in e.ops]
    kind4 = np.array([e.kind == 4 for e in cat])
    # background: small positive integers, different in every pixel of a window
    yy, xx = np.mgrid[0:h, 0:w]
    bits = np.empty((n, h, w), f.ut)
    for k in range(n):
        bits[k] = (((xx * 3 + yy * 5 + k * 7) % 97 + 1).astype(f.dt)).view(f.ut)
    kxy = [0]
    for L in range(1, n_levels):
        kxy.append(kxy[-1] + int(_halves(geo, L)[0]))
    S = 1 << kxy[-1]
    ncy, ncx = -(-h // S), -(-w // S)
    records = {L: [] for L in range(1, n_levels)}
    for t in range(n // planes):
        for L in range(1, n_levels):
            xy, _ = _halves(geo, L)
            side = 1 << (kxy[L] - 1 if xy else kxy[L])   # one operand's block
            win = 2 * side if xy else side
            m = S // win
            cy, cx, wy, wx = np.meshgrid(np.arange(ncy), np.arange(ncx), np.arange(m),
                                         np.arange(m), indexing="ij")
            keep = (cy + cx) % (n_levels - 1) == L - 1
            y0, x0 = (cy * S + wy * win)[keep], (cx * S + wx * win)[keep]
            inside = (y0 < h) & (x0 < w)
            y0, x0 = y0[inside], x0[inside]
            padw = (x0 + side >= w) if xy else np.zeros(y0.size, bool)
            padh = (y0 + side >= h) if xy else np.zeros(y0.size, bool)
            edge = padw | padh
            turns = [np.array(_turn(f, cat, geo, L, edge)) for edge in (False, True)]
            for j in range(geo[L][2]):
                start = 37 * t + 11 * j
                entry = np.empty(y0.size, np.int64)
                for is_edge, turn in enumerate(turns):
                    sel = edge == bool(is_edge)
                    if not sel.any():
                        continue
                    entry[sel] = turn[(start + np.arange(int(sel.sum()))) % len(turn)]
                earlier, later = _pair_planes(geo, L, j)
                for pl, pair_col in ((earlier, 0), (later or [], 1)):
                    for pos in range(4 if xy else 1):
                        v = np.where(kind4[entry], ops[entry, pos], ops[entry, pair_col])
                        oy, ox = (pos // 2) * side, (pos % 2) * side
                        for dy in range(side):
                            for dx in range(side):
                                py, px = y0 + oy + dy, x0 + ox + dx
                                ok = (py < h) & (px < w)
                                for p in pl:
                                    bits[t * planes + p, py[ok], px[ok]] = v[ok]
                records[L].append((t * geo[L][2] + j, y0 >> kxy[L], x0 >> kxy[L], entry, padw,
                                   padh, later is not None and not later))
    bits.setflags(write=False)
    return bits.view(f.dt), records


def _geometry(h, w, n_levels, planes, geometry):
    geo = tuple(tuple(g) for g in (geometry or pyramid(h, w, n_levels, planes)))
    assert geo[0] == (w, h, planes) and len(geo) == n_levels, (geo, h, w, n_levels, planes)
    return geo


def edge_frames(dtype, n, h, w, n_levels, planes=1, geometry=None):
    """`n` frames (n, h, w) of `dtype` for the pyramid of `n_levels` levels
    over w x h x planes: `geometry` when given ((w, h, planes) per level, as
    the Downsampler takes it), else pyramid().  Whole stacks only.  The array
    is shared between callers and read-only."""
    geo = _geometry(h, w, n_levels, planes, geometry)
    return _layout(np.dtype(dtype).name, n, geo)[0]


def planted(dtype, n, h, w, n_levels, method, level, planes=1, geometry=None):
    """Every output of `level` planted for `method`, as Plant tuples."""
    geo = _geometry(h, w, n_levels, planes, geometry)
    f = Fmt(dtype)
    cat = catalogue(dtype)
    xy, _ = _halves(geo, level)
    res = []
    for_method = np.array([method in e.methods for e in cat])
    for frame, oy, ox, entry, padw, padh, single in _layout(f.dt.name, n, geo)[1][level]:
        for i in np.flatnonzero(for_method[entry]):
            e = cat[entry[i]]
            ops = list(e.ops)
            if e.kind == 4:
                a, b, c, d = ops
                pw, ph = bool(padw[i]), bool(padh[i])
                ops = [a, a if pw else b, a if ph else c,
                       a if pw and ph else c if pw else b if ph else d]
                behind = level > 1
            else:
                if single:
                    ops = ops[:1]
                behind = level > 1 or xy
            if method == MEAN and behind:
                ops = [f.settle(b) for b in ops]
            res.append(Plant(int(frame), int(oy[i]), int(ox[i]), e.name, tuple(ops)))
    return res


def class_map(dtype, n, h, w, n_levels, method, level, planes=1, geometry=None):
    """Object array (frames of the level, rows, columns): the name of the class
    each output was planted for under `method`, or None."""
    geo = _geometry(h, w, n_levels, planes, geometry)
    gw, gh, gp = geo[level]
    out = np.full((n // planes * gp, gh, gw), None, dtype=object)
    for p in planted(dtype, n, h, w, n_levels, method, level, planes, geometry):
        out[p.frame, p.y, p.x] = p.name
    return out


# ---- zero tiles of a volume ------------------------------------------------------

ZERO_TILE = (8, 16)  # tile rows x columns of the zero-region checks


def zero_region_stack(stack):
    """A copy of a stack of 8 planes (two groups of 4: one level-2 plane each)
    whose top half is +0.0 and whose bottom left quarter is -0.0, through all
    planes.  Planes 0-1 carry one 2 x 2 window of -0.0 at (2, 2): level 1's
    plane 0 gets one -0.0 at (1, 1) among +0.0.  Planes 4-7 carry one 4 x 4
    window at (4, 4): level 2's plane 1 gets one -0.0 at (1, 1).  The classes
    stay in the bottom right quarter."""
    f = np.array(stack)
    n, h, w = f.shape
    assert n == 8 and h >= 64 and w >= 128
    f[:, : h // 2] = 0.0
    f[:, h // 2:, : w // 2] = -0.0
    f[0:2, 2:4, 2:4] = -0.0
    f[4:8, 4:8, 4:8] = -0.0
    return f


def check_zero_region_tiles(dtype, level, tiles, nonzero, level_h, level_w):
    """`tiles` (planes, n_tiles, tr, tc) and `nonzero` (planes, n_tiles) of
    `level` (1 or 2) of a zero_region_stack under ZERO_TILE hold what the stack
    was built for: whole tiles of +0.0 with flag 0, whole tiles of -0.0 with
    flag 1 (the scan is byte-wise), and on plane level - 1 a tile 0 whose only
    nonzero bytes are one -0.0 at (1, 1)."""
    tr, tc = ZERO_TILE
    ut = np.dtype(f"u{np.dtype(dtype).itemsize}")
    sign = ut.type(1 << (8 * ut.itemsize - 1))
    ntx = -(-level_w // tc)
    k = level - 1
    bits = np.ascontiguousarray(tiles).view(ut)
    b0 = bits[k, 0].reshape(-1)
    assert nonzero[k, 0] and (b0 != 0).sum() == 1 and b0[tc + 1] == sign, \
        f"level {level}: tile 0 of plane {k} is not one -0.0 among +0.0"
    # the tile right of it, and tile 0 of a plane without a window: +0.0, flag 0
    assert not nonzero[k, 1] and not bits[k, 1].any()
    p = 1 - k  # level 1's plane 1 (planes 2-3), level 2's plane 0 (one -0.0 in eight)
    assert not nonzero[p, 0] and not bits[p, 0].any()
    # the first tile of the last full tile row, in the bottom left quarter: -0.0 alone
    ty = level_h // tr - 1
    assert ty * tr >= (level_h + 1) // 2 and tc <= level_w // 2
    t = ty * ntx
    assert all(nonzero[p, t] and (bits[p, t] == sign).all() for p in range(bits.shape[0])), \
        f"level {level}: tile {t} is not -0.0 alone"
