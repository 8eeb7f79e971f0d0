"""Hand-made LZ4 blocks and blosc frames for the decoders (a plain helper,
shared by tests/test_lz4_decode.py and tests/test_blosc_decode.py on the CPU and
tests/test_gpu_blosc_decode.py on the GPU).

The device decoder (wave_decode_block, csrc/codec_kernels.hip) restates
lz4::decode_block of csrc/blosc_decode.hh for a wave.  What it has and the
serial statement lacks: a 256-byte input window read through lanes, 16-byte
literal copies, and a match copy that is periodic where the match overlaps
itself (offset < length).  overlap_blocks() crosses the offsets and lengths
at which that copy changes its path; defects() holds one frame per way a
stream can point outside its ranges, each by less than 64 KiB.

Blocks are written from the format alone; what they stand for comes from
tests/lz4_cases.decode, the Python decoder.
"""
import os
import struct

import numpy as np

import lz4_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))

OK, ABSENT, BAD_HEADER, UNSUPPORTED, CORRUPT = range(5)

OVERLAP_OFFSETS = [1, 2, 3, 4, 7, 15, 16, 17, 63, 64, 65, 300, 65535]
MATCH_LENGTHS = [4 + c for c in lc.COUNT_EDGES]


def _run(n):
    """The bytes after a nibble of 15 for a run of n >= 15."""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def block(seqs, last=b""):
    """An LZ4 block from sequences (literal bytes, offset, match length >= 4)
    and the closing literals."""
    out = bytearray()
    for lit, off, ml in seqs:
        m = ml - 4
        out.append((min(len(lit), 15) << 4) | min(m, 15))
        if len(lit) >= 15:
            out += _run(len(lit))
        out += lit
        out += struct.pack("<H", off)
        if m >= 15:
            out += _run(m)
    out.append(min(len(last), 15) << 4)
    if len(last) >= 15:
        out += _run(len(last))
    out += last
    return bytes(out)


_OVERLAP = {}


def overlap_blocks():
    """(name, block, decoded bytes): `off` fresh bytes, then a match of every
    length of MATCH_LENGTHS at offset `off`, and again after 5 more literals
    (so the second match starts at an odd distance from the first), for every
    offset of OVERLAP_OFFSETS."""
    if _OVERLAP:
        return _OVERLAP["cases"]
    cases = []
    for off in OVERLAP_OFFSETS:
        rng = np.random.default_rng(900 + off)
        head = rng.integers(0, 256, off, dtype=np.uint8).tobytes()
        for ml in MATCH_LENGTHS:
            mid = rng.integers(0, 256, 5, dtype=np.uint8).tobytes()
            # the second match reaches back over the 5 literals into the first
            b = block([(head, off, ml), (mid, min(off, 7) if off < 65535 else off, ml + 1)],
                      last=b"twelve bytes")  # liblz4 wants 12 at an exact capacity
            want, _ = lc.decode(b)
            cases.append((f"overlap-o{off}-m{ml}", b, want))
    _OVERLAP["cases"] = cases
    return cases


def length_blocks():
    """Literal runs, match lengths and last runs at lz4_cases.LENGTH_EDGES
    (one and 64 length bytes), written from the format."""
    cases = []
    rng = np.random.default_rng(77)
    for e in lc.LENGTH_EDGES:
        lit = rng.integers(0, 256, e, dtype=np.uint8).tobytes()
        last = rng.integers(0, 256, e, dtype=np.uint8).tobytes()
        b = block([(lit, e, e)], last=last)
        cases.append((f"length-{e}", b, lc.decode(b)[0]))
    return cases


# ---- frames -------------------------------------------------------------------

def header(flags, ts, nbytes, bs, cbytes, version=2, versionlz=1):
    return struct.pack("<BBBBIII", version, versionlz, flags, ts, nbytes, bs, cbytes)


def frame_of_blocks(payloads, nbytes, ts=1, flags=0x30, bs=None, cbytes=None, sizes=None):
    """A frame of one block whose splits hold `payloads` (flags 0x30: LZ4,
    not split, no filter, so one payload), or of len(payloads) blocks when
    `bs` is given; `sizes` overrides the int32 written before each payload."""
    bs = nbytes if bs is None else bs
    nb = -(-nbytes // bs)
    body = bytearray()
    starts = []
    per = len(payloads) // nb
    for b in range(nb):
        starts.append(16 + 4 * nb + len(body))
        for j in range(per):
            p = payloads[b * per + j]
            s = len(p) if sizes is None else sizes[b * per + j]
            body += struct.pack("<i", s) + p
    total = 16 + 4 * nb + len(body)
    return (header(flags, ts, nbytes, bs, total if cbytes is None else cbytes) +
            struct.pack(f"<{nb}i", *starts) + bytes(body))


def defects():
    """(name, frame bytes, typesize, nbytes, status) — every frame is wrong in
    one named way; the bytes a missing check would touch lie less than 64 KiB
    outside the frame or the chunk."""
    rng = np.random.default_rng(5)
    n = 4096
    data = rng.integers(0, 256, 600, dtype=np.uint8).tobytes()
    good = block([(data, 600, n - 600 - 5)], last=b"12345")
    assert len(lc.decode(good)[0]) == n
    out = []
    fr = frame_of_blocks([good], n)
    out.append(("good", fr, 1, n, OK))
    out.append(("truncated-header", fr[:10], 1, n, BAD_HEADER))
    out.append(("cbytes-above-extent", frame_of_blocks([good], n, cbytes=len(fr) + 40000), 1, n,
                BAD_HEADER))
    out.append(("cbytes-below-extent", frame_of_blocks([good], n, cbytes=len(fr) - 1), 1, n,
                BAD_HEADER))
    out.append(("wrong-typesize", fr, 2, n, BAD_HEADER))
    out.append(("wrong-nbytes", fr, 1, n + 1, BAD_HEADER))
    out.append(("blocksize-0", frame_of_blocks([good], n)[:8] + b"\0\0\0\0" + fr[12:], 1, n,
                BAD_HEADER))
    out.append(("zstd-codec", fr[:2] + bytes([0x90]) + fr[3:], 1, n, UNSUPPORTED))
    bad_start = bytearray(fr)
    bad_start[16:20] = struct.pack("<i", len(fr) + 30000)
    out.append(("block-start-outside", bytes(bad_start), 1, n, CORRUPT))
    bad_start[16:20] = struct.pack("<i", -8)
    out.append(("block-start-negative", bytes(bad_start), 1, n, CORRUPT))
    # 64 blocks of 64 bytes need 256 bytes of starts; the frame ends inside them
    short = header(0x30, 1, n, 64, 100) + bytes(84)
    out.append(("block-starts-past-frame", short, 1, n, CORRUPT))
    out.append(("split-size-negative", frame_of_blocks([good], n, sizes=[-5]), 1, n, CORRUPT))
    out.append(("split-size-past-block", frame_of_blocks([good], n, sizes=[n + 1000]), 1, n,
                CORRUPT))
    out.append(("split-size-past-frame", frame_of_blocks([good], n, sizes=[len(good) + 9]), 1, n,
                CORRUPT))

    def lz(name, payload):
        out.append((name, frame_of_blocks([payload], n), 1, n, CORRUPT))

    lz("offset-0", block([(data, 0, n - 600 - 5)], last=b"12345"))
    lz("offset-before-output", block([(data, 601, n - 600 - 5)], last=b"12345"))
    lz("offset-far-before-output", block([(data, 65535, n - 600 - 5)], last=b"12345"))
    # the first token promises 15 + 255 * 100 + 7 literals; 40 follow
    lz("literals-past-input", bytes([0xF0]) + b"\xff" * 100 + b"\x07" + data[:40])
    # literals that the input has but the split has no room for: 600 + 3000
    # bytes are out when 600 more come
    lz("literals-past-output", block([(data, 600, 3000)], last=data))
    lz("match-past-split", block([(data, 600, n - 600 - 5 + 30000)], last=b"12345"))
    lz("match-one-past-split", block([(data, 600, n - 600 - 5 + 1)], last=b"12345"))
    lz("short-of-nbytes", block([(data, 600, n - 600 - 5 - 1)], last=b"12345"))
    lz("ends-in-match", block([(data, 600, n - 600)])[:-1])
    lz("trailing-bytes", good + b"\x00")
    lz("trailing-token", good + b"\x10A")
    lz("length-bytes-run-out", bytes([0xF0]) + b"\xff" * 20)
    return out


def golden():
    """tests/golden/blosc_frames.npz and blosc_decode_frames.npz: [(key,
    frame bytes, input bytes, typesize)], c-blosc 1.21.0's own frames."""
    out = []
    for fn in ("blosc_frames.npz", "blosc_decode_frames.npz"):
        path = os.path.join(HERE, "golden", fn)
        if not os.path.exists(path):
            continue
        z = np.load(path)
        for k in z.files:
            if not k.startswith("frame__"):
                continue
            key = k[len("frame__"):]
            name, cname, clevel, shuffle, ts = key.split("__")
            out.append((key, z[k].tobytes(), z[f"in__{name}"].view(np.uint8).reshape(-1).tobytes(),
                        int(ts)))
    return out


def frame_class(fr):
    """memcpy / split / unsplit, and whether any split is stored raw."""
    flags, ts = fr[2], fr[3]
    nbytes, bs, _ = struct.unpack_from("<III", fr, 4)
    if flags & 0x2:
        return "memcpy", False
    split = not flags & 0x10 and ts <= 16 and bs // ts >= 128
    nb = -(-nbytes // bs)
    starts = struct.unpack_from(f"<{nb}i", fr, 16)
    raw = False
    for b, p in enumerate(starts):
        bsize = min(bs, nbytes - b * bs)
        nsp = ts if split and bsize == bs else 1
        for _ in range(nsp):
            (c,) = struct.unpack_from("<i", fr, p)
            raw |= c == bsize // nsp
            p += 4 + c
    return ("split" if split else "unsplit"), raw
