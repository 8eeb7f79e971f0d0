"""Generate tests/golden/blosc_decode_frames.npz: more c-blosc LZ4 frames for
the decoders, in the classes tests/golden/blosc_frames.npz lacks.

That file's LZ4 frames are split frames, single-stream frames of 1-byte types
and memcpy frames.  A frame reader also has to meet:
  * frames with 0x10 set that are not memcpy frames (fewer than 128 elements a
    block: one stream per block whatever the typesize);
  * split frames in which some streams are stored raw and others compressed;
  * several blocks with a leftover block, bit-shuffled, whose leftover holds a
    number of elements that is no multiple of 8 (copied, not bit-shuffled).
Same layout and the same call as make_blosc_frames.py:
blosc_compress_ctx(clevel, shuffle, typesize, nbytes, src, dest, nbytes + 16,
"lz4", 0, 1) of the image's c-blosc 1.21.0.

Run: python tests/golden/make_blosc_decode_frames.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import blosc_ref  # noqa: E402


def inputs():
    rng = np.random.default_rng(20261021)
    # 100 elements of 16 bytes: below the split threshold, compressible
    rec = np.zeros((100, 16), np.uint8)
    rec[:, 0] = np.arange(100)
    rec[:, 5] = 7
    yield "unsplit_ts16_100", rec, 16
    # u16 below 256: the low-byte plane is random (stored raw), the high one zeros
    yield "rawsplit_u16_20000", rng.integers(0, 256, 20000).astype(np.uint16), 2
    # three 64 KiB blocks at clevel 1 and a leftover of 3402 bytes = 1701 elements
    walk = (np.cumsum(rng.integers(-2, 3, 100005)) + 30000).astype(np.uint16)
    yield "blocks_u16_100005", walk, 2
    # f64 with a leftover block shorter than one element at clevel 1
    yield "tail_f64_16385", np.frombuffer(
        (np.arange(16384, dtype=np.float64) / 3).tobytes() + b"\x01\x02\x03", np.uint8), 8


CASES = [(1, 0), (1, 1), (1, 2), (5, 1), (5, 2)]


def main():
    out = {}
    names = []
    for name, arr, ts in inputs():
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        out[f"in__{name}"] = raw
        for clevel, shuffle in CASES:
            fr = blosc_ref.compress(raw, clevel, shuffle, ts, "lz4")
            assert not isinstance(fr, int), (name, clevel, shuffle, fr)
            key = f"{name}__lz4__{clevel}__{shuffle}__{ts}"
            out[f"frame__{key}"] = np.frombuffer(fr, np.uint8)
            names.append(key)
    out["version"] = np.frombuffer(blosc_ref.version().encode(), np.uint8)
    path = os.path.join(HERE, "blosc_decode_frames.npz")
    np.savez_compressed(path, **out)
    print(path, len(names), "frames", os.path.getsize(path), "bytes, c-blosc",
          blosc_ref.version())


if __name__ == "__main__":
    main()
