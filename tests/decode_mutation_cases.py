"""Mutated LZ4 blocks and blosc frames for the two decoders (a plain helper,
shared by tests/test_decode_mutation_cases.py on the CPU and
tests/test_gpu_decode_mutations.py on the GPU).

csrc/blosc_decode.hh states the decoder serially; tests/cpp/blosc_decode_sweep.cpp
runs that statement under the host sanitizers over seeded mutations.  The wave
decoder of csrc/codec_kernels.hip is separate code, and this module gives it
the same kinds of input: about 3,000 mutated bare blocks and about 24 mutants
of every frame seed, each with the serial decoder's answer as the expectation.

Seeds and mutations are fixed: every generator is seeded with zlib.crc32 of a
name, so the corpus is the same on every build of it.

The margin.  A mutant is decoded inside memory the test owns and poisons:
[M poison | inputs | M poison | outputs | M poison].  M is the farthest one
missing bound check of wave_decode_block, locate_split or the copies could
reach from the ranges it was given:

    M = 65,536 + 19 + 255 * B

  * 65,536: an offset is 16 bits, so a match source lies less than 64 KiB
    before the output position, which itself lies inside the slot;
  * 255 * B: a length is the sum of its run bytes, each at most 255, and an
    input of B bytes has fewer than B of them, so no literal run, match or
    input position goes further than 255 * B past where it starts;
  * 19: the 15 of the nibble and the 4 of the least match.
B is the largest block mutant (blocks) or the frame stride (frames, where a
32-bit field could point further: those mutations touch the low two bytes of
cbytes, block starts and split sizes only, so a pointer moves by less than
64 KiB).  Both M stay under 32 MiB; a seed that would break that is left
out, the margin is not shrunk.
"""
import struct
import zlib
from collections import namedtuple

import numpy as np

import blosc_decode_cases as bd
import lz4_cases as lc

POISON = 0xA5
MARGIN_LIMIT = 32 << 20
MAX_CHUNK = 64 << 10

KINDS = ["random", "sparse", "period37", "ramp", "echo"]
PLAIN_SIZES = [1, 5, 12, 13, 14, 64, 160, 300, 4097, 20000]
SET_VALUES = [0x00, 0xFF, 0x0F, 0xF0]

OK, ABSENT, BAD_HEADER, UNSUPPORTED, CORRUPT = range(5)

BlockSeed = namedtuple("BlockSeed", "name block plain")
BlockMutant = namedtuple("BlockMutant", "name seed kind block cap")
FrameSeed = namedtuple("FrameSeed", "name frame src ts filt written")
FrameMutant = namedtuple("FrameMutant", "name seed kind frame place")


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def margin(b):
    return 65536 + 19 + 255 * b


def waves_of(nbytes):
    """launch_blosc_decode's rule: a wave for every 8 KiB, 1 to 32."""
    return min(max(nbytes // 8192, 1), 32)


def make_data(rng, kind, n):
    """The five kinds of tests/cpp/blosc_decode_sweep.cpp's make_data."""
    i = np.arange(n)
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "sparse":
        v = rng.integers(0, 256, n, dtype=np.uint8)
        v[rng.integers(0, 16, n) != 0] = 0
        return v
    if kind == "period37":
        return ((i % 37) * 7).astype(np.uint8)
    if kind == "ramp":
        return (i // 300).astype(np.uint8)
    assert kind == "echo"
    v = rng.integers(0, 256, n, dtype=np.uint8)
    echo = (i >= 64) & ((i // 64) % 2 == 1)
    v[echo] = v[i[echo] - 64]  # the block before an odd block is fresh
    return v


# ---- blocks ---------------------------------------------------------------------

def walk_block(block):
    """Where a valid block's fields lie, from the Python decoder's sequence
    list: per sequence dict(token, lit_run, offset, ml_run) of input
    positions (offset None in the closing sequence)."""
    _, seqs = lc.decode(block)
    out, i = [], 0
    for lit, off, ml in seqs:
        tok = i
        i += 1
        lit_run = []
        if lit >= 15:
            k = (lit - 15) // 255 + 1
            lit_run = list(range(i, i + k))
            i += k
        i += lit
        if off == 0:
            out.append(dict(token=tok, lit_run=lit_run, offset=None, ml_run=[]))
            break
        offset = i
        i += 2
        ml_run = []
        if ml - 4 >= 15:
            k = (ml - 19) // 255 + 1
            ml_run = list(range(i, i + k))
            i += k
        out.append(dict(token=tok, lit_run=lit_run, offset=offset, ml_run=ml_run))
    assert i == len(block)
    return out


def _sequence_block(rng, size):
    """A block of about `size` bytes with many short sequences, written from
    the format: every prefix of it ends in another field."""
    seqs, op = [], 0
    n = 0
    while n < size:
        lit = int(rng.integers(0 if op else 1, 41))
        if rng.integers(0, 8) == 0:
            lit += 15
        data = rng.integers(0, 256, lit, dtype=np.uint8).tobytes()
        op += lit
        off = int(rng.integers(1, op + 1))
        ml = int(rng.integers(4, 41)) if rng.integers(0, 6) else int(rng.integers(19, 19 + 300))
        seqs.append((data, off, ml))
        op += ml
        n += 3 + lit + (1 if lit >= 15 else 0) + (ml >= 19) + (ml >= 19 + 255)
    return bd.block(seqs, last=b"twelve bytes")


def refill_blocks():
    """(name, block): the input window of wave_decode_block refills at input
    byte 256.  Blocks whose second offset pair lies at bytes 255|256, whose
    literal length run crosses them, and whose match length run crosses them."""
    pool = rng_of("refill-pool").integers(0, 256, 2000, dtype=np.uint8).tobytes()
    head = (pool[:40], 40, 300)
    out = []

    def find(name, build, hit):
        for L in range(0, 300):
            b = build(L)
            if hit(walk_block(b)):
                out.append((name, b))
                return
        raise AssertionError(name)

    find("refill-offset", lambda L: bd.block([head, (pool[40:40 + L], 0x0123, 20)],
                                             last=b"twelve bytes"),
         lambda w: w[1]["offset"] == 255)
    find("refill-literal-run",
         lambda L: bd.block([head, (pool[40:40 + L], 7, 8), (pool[400:400 + 15 + 510 + 9], 300, 8)],
                            last=b"twelve bytes"),
         lambda w: {255, 256} <= set(w[2]["lit_run"]))
    find("refill-match-run", lambda L: bd.block([head, (pool[40:40 + L], 7, 19 + 510 + 9)],
                                                last=b"twelve bytes"),
         lambda w: {255, 256} <= set(w[1]["ml_run"]))
    return out


def block_seeds(aqz):
    seeds = []
    for si, n in enumerate(PLAIN_SIZES):
        for ki, kind in enumerate(KINDS):
            accel = 1 + (2 * ki + si) % 9
            name = f"{kind}-n{n}-a{accel}"
            data = make_data(rng_of("block-seed/" + name), kind, n)
            csize, block, _ = aqz.debug_lz4_block_host(data, lc.bound(n), accel)
            assert csize > 0
            seeds.append(BlockSeed(name, block, data.tobytes()))
    for name, b, want in bd.length_blocks():
        seeds.append(BlockSeed(name, b, want))
    near = [c for c in bd.overlap_blocks() if int(c[0].split("-")[1][1:]) <= 300][::3]
    far = [c for c in bd.overlap_blocks() if c[0].startswith("overlap-o65535-")]
    for name, b, want in near + [far[0], far[-1]]:
        seeds.append(BlockSeed(name, b, want))
    return seeds


def prefix_seeds(aqz):
    """The two blocks of about 600 bytes of which every prefix is a mutant."""
    data = make_data(rng_of("block-seed/prefix-echo"), "echo", 1100)
    csize, block, _ = aqz.debug_lz4_block_host(data, lc.bound(1100), 1)
    assert csize > 0
    b = _sequence_block(rng_of("block-seed/prefix-sequences"), 600)
    return [BlockSeed("prefix-echo", block, data.tobytes()),
            BlockSeed("prefix-sequences", b, lc.decode(b)[0])]


def draw_cap(rng, n):
    pick = int(rng.integers(0, 4))
    if pick == 0:
        return n
    if pick == 1:
        return max(n - 1, 0)
    if pick == 2:
        return n + 9
    return int(rng.integers(0, n + 1))


def _other(rng, old):
    """A byte value that is not `old`."""
    return (old + int(rng.integers(1, 256))) & 0xFF


def _with(b, at, value):
    out = bytearray(b)
    out[at] = value
    return bytes(out)


def block_mutants(aqz):
    """(seeds, mutants) of the block corpus."""
    seeds = block_seeds(aqz)
    pre = prefix_seeds(aqz)
    refill = refill_blocks()
    muts = []

    def add(si, seed, kind, block, rng, cap=None):
        cap = draw_cap(rng, len(seed.plain)) if cap is None else cap
        muts.append(BlockMutant(f"{seed.name}/{kind}/cap{cap}", si, kind, bytes(block), cap))

    for si, seed in enumerate(seeds):
        r = rng_of("block-mut/" + seed.name)
        b, n = seed.block, len(seed.block)
        for _ in range(5):
            at, bit = int(r.integers(0, n)), int(r.integers(0, 8))
            add(si, seed, f"bit@{at}.{bit}", _with(b, at, b[at] ^ (1 << bit)), r)
        for v in SET_VALUES:
            at = int(r.integers(0, n))
            add(si, seed, f"set@{at}={v:02x}", _with(b, at, v), r)
        for _ in range(2):
            cut = int(r.integers(0, n))
            add(si, seed, f"cut{cut}", b[:cut], r)
        for _ in range(2):
            extra = r.integers(0, 256, int(r.integers(1, 4)), dtype=np.uint8).tobytes()
            add(si, seed, f"append:{extra.hex()}", b + extra, r)
        w = walk_block(b)
        matches = [s for s in w if s["offset"] is not None]
        if matches:
            s = matches[int(r.integers(0, len(matches)))]
            add(si, seed, f"token@{s['token']}", _with(b, s["token"], _other(r, b[s["token"]])), r)
            for k in (0, 1):
                at = s["offset"] + k
                add(si, seed, f"offset@{at}", _with(b, at, _other(r, b[at])), r)
        runs = [p for s in w for p in s["lit_run"] + s["ml_run"]]
        if runs:
            at = runs[int(r.integers(0, len(runs)))]
            v = [0, 255, _other(r, b[at])][int(r.integers(0, 3))]
            add(si, seed, f"run@{at}={v:02x}", _with(b, at, v if v != b[at] else v ^ 1), r)
        at = w[-1]["token"]
        add(si, seed, f"last-token@{at}", _with(b, at, _other(r, b[at])), r)

    base = len(seeds)
    for k, seed in enumerate(pre):
        r = rng_of("block-mut/" + seed.name)
        for cut in range(len(seed.block)):
            add(base + k, seed, f"prefix{cut}", seed.block[:cut], r)
    seeds = seeds + pre

    for name, b in refill:
        si = len(seeds)
        seed = BlockSeed(name, b, lc.decode(b)[0])
        seeds.append(seed)
        r = rng_of("block-mut/" + name)
        n = len(seed.plain)
        add(si, seed, "valid", b, r, cap=n)
        add(si, seed, "valid-roomy", b, r, cap=n + 9)
        for at in (255, 256):
            bit = int(r.integers(0, 8))
            add(si, seed, f"bit@{at}.{bit}", _with(b, at, b[at] ^ (1 << bit)), r)
        for cut in (255, 256, 257):
            add(si, seed, f"cut{cut}", b[:cut], r)

    # a size of 0 and a capacity of 0, whatever the draws gave
    r = rng_of("block-mut/zero")
    add(0, seeds[0], "zero-size", b"", r, cap=13)
    add(base, seeds[base], "zero-capacity", seeds[base].block, r, cap=0)
    add(0, seeds[0], "empty-block-zero-capacity", b"\x00", r, cap=0)
    return seeds, muts


# ---- frames ---------------------------------------------------------------------

def block_filter(filt, ts, bsize):
    """blosc::block_filter: what a block of bsize bytes goes through."""
    if filt == 1:
        return 1 if ts > 1 else 0
    if filt == 2:
        return 2 if bsize >= ts and (bsize // ts) % 8 == 0 else 0
    return 0


def filter_block(filt, ts, blk):
    """The forward filter of one block in numpy: element i byte j -> plane j;
    bit b of byte j of element i -> bit i % 8 of byte i / 8 of row j * 8 + b;
    the blocksize % typesize tail copied."""
    kind = block_filter(filt, ts, blk.size)
    out = blk.copy()
    if kind == 0:
        return out
    ne = blk.size // ts
    e = blk[:ne * ts].reshape(ne, ts)
    if kind == 1:
        out[:ne * ts] = e.T.reshape(-1)
    else:
        bits = np.unpackbits(e[:, :, None], axis=2, bitorder="little")  # [i, j, b]
        rows = bits.transpose(1, 2, 0).reshape(ts * 8, ne)
        out[:ne * ts] = np.packbits(rows, axis=1, bitorder="little").reshape(-1)
    return out


def make_frame(aqz, src, ts, bs, filt, accel):
    """make_frame of tests/cpp/blosc_decode_sweep.cpp: a c-blosc style LZ4
    frame of `src` in blocks of `bs`, split into typesize streams under
    blosc's rule (0x10 set where it does not hold), splits the encoder cannot
    shrink stored raw."""
    src = np.frombuffer(bytes(src), np.uint8)
    n = src.size
    split = ts <= 16 and bs // ts >= 128 and bs % ts == 0
    nblocks = -(-n // bs)
    flags = 0x20 | {0: 0, 1: 0x1, 2: 0x4}[filt] | (0 if split else 0x10)
    starts, body = [], bytearray()
    for b in range(nblocks):
        blk = filter_block(filt, ts, src[b * bs:min((b + 1) * bs, n)])
        starts.append(16 + 4 * nblocks + len(body))
        nsp = ts if split and blk.size == bs else 1
        neb = blk.size // nsp
        for j in range(nsp):
            piece = blk[j * neb:(j + 1) * neb]
            csize, c, _ = aqz.debug_lz4_block_host(piece, lc.bound(neb), accel)
            if csize <= 0 or csize >= neb:
                c = piece.tobytes()
            body += struct.pack("<I", len(c)) + c
    total = 16 + 4 * nblocks + len(body)
    return bd.header(flags, ts, n, bs, total) + struct.pack(f"<{nblocks}I", *starts) + bytes(body)


# headers c-blosc would not write: (name, typesize, nbytes, blocksize)
WRITTEN_SHAPES = [
    ("ts3-bs1200", 3, 3001, 1200),
    ("ts16-bs2064", 16, 5000, 2064),
    ("ts2-bs100-unsplit", 2, 300, 100),
    ("ts4-bs4098", 4, 8206, 4098),
    ("ts2-bs-is-nbytes", 2, 4096, 4096),
    ("ts1-bs1", 1, 64, 1),
    ("ts2-leftover-405-elements", 2, 9003, 4096),
    ("ts8-leftover-13", 8, 8205, 4096),
]
# several waves a frame: 16 KiB and up
WAVE_SHAPES = [
    ("ts2-waves", 2, 16384 + 4096 + 38, 4096, (0, 1, 2)),
    ("ts4-waves", 4, 3 * 8192 + 12, 8192, (1, 2)),
    ("ts8-waves", 8, 4 * 8192 + 24, 8192, (0, 2)),
]
FILTER_NAMES = ["nofilter", "shuffle", "bitshuffle"]
# the three frames of the shard sweep: unsplit; split and byte-shuffled;
# multi-block and bit-shuffled with a leftover
SHARD_SEEDS = ["ts2-bs100-unsplit/nofilter", "ts2-leftover-405-elements/shuffle",
               "ts8-leftover-13/bitshuffle"]
LAUNCH_LOG_SEEDS = ["ts4-bs4098/shuffle", "ts3-bs1200/bitshuffle"]  # form=vec, form=generic


def frame_seeds(aqz):
    seeds = []
    for key, fr, src, ts in bd.golden():
        if "__lz4__" in key and len(src) <= MAX_CHUNK:
            filt = 1 if fr[2] & 0x1 and ts > 1 else 2 if fr[2] & 0x4 else 0
            seeds.append(FrameSeed("golden/" + key, fr, src, ts, filt, False))
    shapes = [s + ((0, 1, 2),) for s in WRITTEN_SHAPES] + WAVE_SHAPES
    for k, (name, ts, n, bs, filts) in enumerate(shapes):
        for filt in filts:
            full = f"{name}/{FILTER_NAMES[filt]}"
            kind = KINDS[1 + (k + filt) % 4]  # the four kinds an encoder shrinks
            data = make_data(rng_of("frame-seed/" + full), kind, n)
            if kind in ("period37", "ramp"):  # a little noise: literals between the matches
                noise = rng_of("frame-noise/" + full)
                at = noise.integers(0, n, max(n // 50, 1))
                data[at] = noise.integers(0, 256, at.size, dtype=np.uint8)
            fr = make_frame(aqz, data, ts, bs, filt, 1 + k % 9)
            seeds.append(FrameSeed(full, fr, data.tobytes(), ts, filt, True))
    return seeds


Field = namedtuple("Field", "lo hi place block split raw")


def layout(frame):
    """The fields of a valid frame: header, block starts, and per split its
    size field and payload with the place a change there is recorded under."""
    flags, ts = frame[2], frame[3]
    nbytes, bs, cbytes = struct.unpack_from("<III", frame, 4)
    out = [Field(0, 16, "header", -1, -1, False)]
    if flags & 0x2:
        out.append(Field(16, len(frame), "memcpy", 0, 0, True))
        return out
    split = not flags & 0x10 and ts <= 16 and bs // ts >= 128
    nb = -(-nbytes // bs)
    out.append(Field(16, 16 + 4 * nb, "block-starts", -1, -1, False))
    starts = struct.unpack_from(f"<{nb}I", frame, 16)
    for b, p in enumerate(starts):
        bsize = min(bs, nbytes - b * bs)
        leftover = bsize != bs
        nsp = ts if split and not leftover else 1
        for j in range(nsp):
            (c,) = struct.unpack_from("<I", frame, p)
            out.append(Field(p, p + 4, "split-size", b, j, False))
            place = ("leftover" if leftover else "later-block" if b else
                     "later-split" if j else "split0")
            out.append(Field(p + 4, p + 4 + c, place, b, j, c == bsize // nsp))
            p += 4 + c
    assert p == len(frame) == cbytes
    return out


def place_of(fields, pos):
    for f in fields:
        if f.lo <= pos < f.hi:
            return f.place
    return "outside"


def pointer_fields(fields):
    """(lo, hi) of the 32-bit fields a walk follows: cbytes, block starts,
    split sizes."""
    out = [(12, 16)]
    for f in fields:
        if f.place == "block-starts":
            out += [(p, p + 4) for p in range(f.lo, f.hi, 4)]
        elif f.place == "split-size":
            out.append((f.lo, f.hi))
    return out


def _low_bytes(ptr, pos):
    """`pos`, moved to the same field's low two bytes where it lies in bytes
    2 to 3 of a pointer field."""
    for lo, hi in ptr:
        if lo + 2 <= pos < hi:
            return pos - 2
    return pos


def frame_mutants(aqz, seed, si, per_seed=1.0):
    """About 24 mutants of one seed, each with the place of its change."""
    fr, n = seed.frame, len(seed.frame)
    fields = layout(fr)
    ptr = pointer_fields(fields)
    r = rng_of("frame-mut/" + seed.name)
    muts = []

    def add(kind, frame, place):
        muts.append(FrameMutant(f"{seed.name}/{kind}", si, kind, bytes(frame), place))

    def flip(limit, tag):
        at = _low_bytes(ptr, int(r.integers(0, min(n, limit))))
        bit = int(r.integers(0, 8))
        add(f"{tag}bit@{at}.{bit}", _with(fr, at, fr[at] ^ (1 << bit)), place_of(fields, at))

    def byte_set(limit, tag):
        at = _low_bytes(ptr, int(r.integers(0, min(n, limit))))
        v = SET_VALUES[int(r.integers(0, 4))]
        add(f"{tag}set@{at}={v:02x}", _with(fr, at, v), place_of(fields, at))

    def times(k):
        return max(1, int(round(k * per_seed)))

    for _ in range(times(3)):
        flip(n, "")
    for _ in range(times(2)):
        byte_set(n, "")
    for _ in range(times(3)):
        flip(48, "head-")
    for _ in range(times(2)):
        byte_set(48, "head-")
    for _ in range(times(2)):
        cut = int(r.integers(0, n))
        add(f"cut{cut}", fr[:cut], place_of(fields, cut))
    for _ in range(times(2)):
        extra = r.integers(0, 256, int(r.integers(1, 4)), dtype=np.uint8).tobytes()
        add(f"append:{extra.hex()}", fr + extra, "outside")
    # directed: the header ...
    add("flags", _with(fr, 2, fr[2] ^ (1 << int(r.integers(0, 8)))), "header")
    at = 8 + int(r.integers(0, 2))
    add(f"blocksize@{at}", _with(fr, at, _other(r, fr[at])), "header")
    at = 12 + int(r.integers(0, 2))
    add(f"cbytes@{at}", _with(fr, at, _other(r, fr[at])), "header")
    if seed.name.startswith("ts4-bs4098/"):
        add("clear-0x10", _with(fr, 2, fr[2] & ~0x10), "header")  # a split of 4098 / 4: refused
    # ... the block starts, the size fields, and a token and a byte of a
    # payload in every place the seed has
    starts = [f for f in fields if f.place == "block-starts"]
    if starts:
        nb = (starts[0].hi - starts[0].lo) // 4
        for b in sorted({0, nb - 1}):
            at = 16 + 4 * b + int(r.integers(0, 2))
            add(f"start{b}@{at}", _with(fr, at, _other(r, fr[at])), "block-starts")
    sizes = [f for f in fields if f.place == "split-size"]
    for f in ([sizes[0], sizes[-1]] if len(sizes) > 1 else sizes):
        at = f.lo + int(r.integers(0, 2))
        add(f"size-b{f.block}s{f.split}@{at}", _with(fr, at, _other(r, fr[at])), "split-size")
    for place in ("split0", "later-split", "later-block", "leftover"):
        here = [f for f in fields if f.place == place and f.hi > f.lo]
        if not here:
            continue
        streams = [f for f in here if not f.raw] or here
        f = streams[int(r.integers(0, len(streams)))]
        add(f"{place}-token@{f.lo}", _with(fr, f.lo, _other(r, fr[f.lo])), place)
        at = int(r.integers(f.lo, f.hi))
        add(f"{place}-byte@{at}", _with(fr, at, _other(r, fr[at])), place)
    return muts


_CORPUS = {}


def build(aqz, per_seed=1.0):
    """The whole corpus, built afresh: dict(block_seeds, block_mutants,
    frame_seeds, frame_mutants (a list per seed), B and M of both)."""
    bseeds, bmuts = block_mutants(aqz)
    fseeds = frame_seeds(aqz)
    fmuts = [frame_mutants(aqz, s, si, per_seed) for si, s in enumerate(fseeds)]
    b_blocks = max(len(m.block) for m in bmuts)
    # a seed whose margin would pass the limit is dropped, the margin stays
    keep = [si for si in range(len(fseeds)) if margin(frame_stride(fseeds[si], fmuts[si])) <= MARGIN_LIMIT]
    fseeds = [fseeds[si] for si in keep]
    fmuts = [[m._replace(seed=k) for m in fmuts[si]] for k, si in enumerate(keep)]
    b_frames = max(frame_stride(s, m) for s, m in zip(fseeds, fmuts))
    return dict(block_seeds=bseeds, block_mutants=bmuts, frame_seeds=fseeds, frame_mutants=fmuts,
                B_blocks=b_blocks, M_blocks=margin(b_blocks), B_frames=b_frames,
                M_frames=margin(b_frames))


def corpus(aqz):
    """build(aqz), once a process."""
    if "corpus" not in _CORPUS:
        _CORPUS["corpus"] = build(aqz)
    return _CORPUS["corpus"]


def frame_stride(seed, muts):
    """A byte-odd stride every mutant of the seed fits into."""
    return (max([len(seed.frame)] + [len(m.frame) for m in muts]) + 5) | 1


# ---- what the serial decoder says -------------------------------------------------

def block_expectations(aqz):
    """Per block mutant (result, the cap output bytes) of the serial decoder."""
    if "blocks" not in _CORPUS:
        _CORPUS["blocks"] = [aqz.debug_lz4_decode_host(m.block, m.cap)
                             for m in corpus(aqz)["block_mutants"]]
    return _CORPUS["blocks"]


def decode_sized(aqz, frame, ts, nbytes):
    """The host path on a frame whose extent is its length: (status, bytes)."""
    return aqz.debug_blosc_decode_host(frame, ts, nbytes)


def decode_from_header(aqz, slot, ts, nbytes):
    """The host path on a slot of `stride` bytes without a size table:
    span_strided takes the extent from the header's cbytes, bounded by the
    stride."""
    stride = len(slot)
    if stride < 16:
        return BAD_HEADER, np.full(nbytes, POISON, np.uint8)
    (cbytes,) = struct.unpack_from("<I", slot, 12)
    if cbytes < 16 or cbytes > stride:
        return BAD_HEADER, np.full(nbytes, POISON, np.uint8)
    return aqz.debug_blosc_decode_host(slot[:cbytes], ts, nbytes)


def slot_of(frame, stride):
    return bytes(frame) + bytes([POISON]) * (stride - len(frame))


def frame_expectations(aqz, form):
    """Per seed, per mutant (status, bytes) of the host path; form "sizes":
    the extent is the mutant's length; form "header": it comes out of the
    slot's header."""
    key = "frames-" + form
    if key not in _CORPUS:
        c = corpus(aqz)
        out = []
        for seed, muts in zip(c["frame_seeds"], c["frame_mutants"]):
            stride = frame_stride(seed, muts)
            n = len(seed.src)
            if form == "sizes":
                out.append([decode_sized(aqz, m.frame, seed.ts, n) for m in muts])
            else:
                out.append([decode_from_header(aqz, slot_of(m.frame, stride), seed.ts, n)
                            for m in muts])
        _CORPUS[key] = out
    return _CORPUS[key]


def seed_named(aqz, name):
    c = corpus(aqz)
    (si,) = [k for k, s in enumerate(c["frame_seeds"]) if s.name == name]
    return si, c["frame_seeds"][si], c["frame_mutants"][si]
