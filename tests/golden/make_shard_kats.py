"""Generate tests/golden/reference_shard_kats.json.

The fixture is the reference's own shard-addressing assertions
(acquire-zarr v0.8.1), written down as data.  Sources:

  S1 tests/unit-tests/array-dimensions-shard-index-for-chunk.cpp
  S2 tests/unit-tests/array-dimensions-shard-internal-index.cpp
  S3 tests/unit-tests/shard-finalize.cpp

S1 and S2: every EXPECT_EQ line is read straight out of the test file when
this script runs, one entry per line with its line number, together with the
dimensions the file declares; nothing is computed.  S3: the file's constants
(chunks per shard, bytes per chunk, the fill byte of its first test) are read
out of it, and `expected_shard_size` (:14-20) is evaluated with the file's
own formula for the two chunk counts its tests use (:55, :77).

The script needs the reference checkout only when it is re-run; the tests
read the committed JSON alone.  Data only: no reference code is run.

Run: python tests/golden/make_shard_kats.py [reference root]
"""
from __future__ import annotations

import json
import os
import re
import sys

DIM_TYPES = {"Space": 0, "Channel": 1, "Time": 2, "Other": 3}
DTYPE_CODES = {"uint8": 0, "uint16": 1, "uint32": 2, "uint64": 3, "int8": 4,
               "int16": 5, "int32": 6, "int64": 7, "float32": 8, "float64": 9}


def addressing_case(ref, tag, fname):
    path = os.path.join(ref, "tests", "unit-tests", fname)
    with open(path) as f:
        text = f.read()
    flat = re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", text))
    dims = [[DIM_TYPES[t], int(a), int(c), int(s)] for _, t, a, c, s in re.findall(
        r'emplace_back\(\s*"(\w+)",\s*ZarrDimensionType_(\w+),\s*(\d+),\s*(\d+),\s*(\d+)\s*\)',
        flat)]
    dtype = DTYPE_CODES[re.search(
        r"ArrayDimensions dimensions\(std::move\(dims\), ZarrDataType_(\w+)\)", text).group(1)]
    kat = re.compile(r"EXPECT_EQ\(int, dimensions\.(\w+)\((\d+)\), (\d+)\);")
    asserts = []
    for no, line in enumerate(text.splitlines(), 1):
        m = kat.search(line)
        if m:
            asserts.append({"line": no, "function": m.group(1), "chunk": int(m.group(2)),
                            "expect": int(m.group(3))})
    assert len(asserts) == text.count("EXPECT_EQ(")
    return {"name": fname[:-4], "src": f"{tag}:{asserts[0]['line']}-{asserts[-1]['line']}",
            "dims": dims, "dtype": dtype, "asserts": asserts}


def finalize_case(ref):
    path = os.path.join(ref, "tests", "unit-tests", "shard-finalize.cpp")
    with open(path) as f:
        text = f.read()
    cps = int(re.search(r"constexpr size_t chunks_per_shard = (\d+);", text).group(1))
    bpc = int(re.search(r"constexpr size_t bytes_per_chunk = (\d+);", text).group(1))
    fill = int(re.search(r"buffer\(bytes_per_chunk, (0x[0-9A-Fa-f]+)\)", text).group(1), 16)
    written = sorted({int(n) for n in re.findall(r"expected_shard_size\((\d+)\)\);", text)})
    # :18-19  n_written_chunks * bytes_per_chunk +
    #         2 * chunks_per_shard * sizeof(uint64_t) + sizeof(uint32_t)
    sizes = {str(n): n * bpc + 2 * cps * 8 + 4 for n in written}
    return {"name": "shard-finalize", "src": "S3:11-20,40,55,77", "chunks_per_shard": cps,
            "bytes_per_chunk": bpc, "fill_byte": fill, "expected_shard_size": sizes}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    out = {"reference": "acquire-project/acquire-zarr v0.8.1",
           "generator": "tests/golden/make_shard_kats.py",
           "addressing": [
               addressing_case(ref, "S1", "array-dimensions-shard-index-for-chunk.cpp"),
               addressing_case(ref, "S2", "array-dimensions-shard-internal-index.cpp")],
           "finalize": finalize_case(ref)}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_shard_kats.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
