"""GPU: the codec stages at sizes that reach code no smaller test runs.

* Filter split launches (split_launch, BlockRun::g0 in codec_kernels.hip): a
  run of 2^31 + 3 * blocksize + 1000 bytes, typesize 3, blocksize 3000, so the
  generic kernels (one thread per byte) need a second launch:
  shuffle_generic_kernel, bitshuffle_generic_kernel and copy_kernel; and the
  same with two buffers of just over 2^30 bytes, where the buffer index
  changes inside a launch.  Random bytes made on the device; compared with
  oracle.blosc_filter on the first block, the two blocks on either side of
  the launch boundary (2^31 / blocksize blocks), the last full block and the
  leftover (the copy also whole, on the device).  The launch log must show
  more than one launch of the run.  The vector kernels take 8 elements or
  more per thread and would need 32 GiB and more for a second launch: they
  stay out.
* CRC-32C power levels: 2 buffers of 65,535 x 16,384 - 7 bytes (every bit of
  the workgroup index set, a short first segment) at a stride of nbytes + 13,
  and of (2^15 + 2^9 + 1) x 16,384 bytes, against oracle.crc32c;
  65,536 x 16,384 bytes is refused.
* Device LZ4 frames: ceil(2^32 / 128 KiB) + 5 chunks cycling 5 prototypes,
  shuffle 1, clevel 5, both probe forms; every chunk's size, bytes and the
  poison behind it against the host path's frames of the prototypes.

The cases run in tests/large_batch_child.py, one child per group, the launch
log on.
"""
import pytest

import large_batch as lb

pytestmark = pytest.mark.gpu

FAMILY = {1: "shuffle", 2: "bitshuffle", 0: "copy"}


@pytest.mark.parametrize("name", list(lb.FILTER_CASES))
def test_filter_split_launches(name):
    shuffle, nbuf = lb.FILTER_CASES[name]
    rec = lb.record_of("filter", name)
    _, cap, per, total = lb.filter_windows(nbuf)
    runs = [r for r in rec["launches"] if r.get("bs") == lb.FILTER_BS]
    assert all(r["family"] == FAMILY[shuffle] and r["form"] == "generic" for r in runs), runs
    # more than one launch of the full-block run: the first at the cap
    assert len(runs) >= 2 and runs[0]["blocks"] == cap, runs
    assert sum(r["blocks"] for r in runs) == total
    rest = lb.filter_nbytes(nbuf) - per * lb.FILTER_BS
    left = [r for r in rec["launches"] if r.get("bs") == rest]
    assert len(left) == 1 and left[0]["blocks"] == nbuf


@pytest.mark.parametrize("name", list(lb.CRC_CASES) + [lb.CRC_LIMIT])
def test_crc32c_power_levels(name):
    lb.record_of("crc", name)


def test_crc_sizes_set_the_bits_they_claim():
    wgs = [-(-n // 16384) for n in lb.CRC_CASES.values()]
    assert wgs[0] == 65535 and (wgs[0] - 1) == 0xFFFE and lb.CRC_CASES["crc-all-levels"] % 64
    assert wgs[1] - 1 == (1 << 15) + (1 << 9)


@pytest.mark.parametrize("name", list(lb.LZ4_CASES))
def test_lz4_frames_past_4gib(name):
    rec = lb.record_of("lz4", name)
    n = lb.lz4_chunks()
    assert n * lb.LZ4_CHUNK > 1 << 32 and n % lb.LZ4_PROTOS
    lz4 = [r for r in rec["launches"] if r.get("family") == "lz4"]
    assert lz4 and lz4[0]["probe"] == ("serial" if lb.LZ4_CASES[name] else "batch")
