"""CPU: the serial LZ4 block decoder lz4::decode_block (csrc/blosc_decode.hh,
through aqz_debug_lz4_decode_host), what the device decoder must reproduce.

Against tests/lz4_cases.decode (the Python decoder) on every case of
tests/lz4_cases.py encoded by the serial encoder, on blocks written by hand
from the format (tests/blosc_decode_cases.py: overlapping matches at every
offset and length the device copy changes its path at), and against
LZ4_decompress_safe of the liblz4 the frame writer loads, where it loads.
Every output buffer is exactly `cap` long.
"""
import ctypes
import re

import numpy as np
import pytest

import blosc_decode_cases as bd
import lz4_cases as lc

ERR_TRUNCATED, ERR_LIT_IN, ERR_LIT_OUT, ERR_OFF0, ERR_OFF_BEFORE, ERR_MATCH_OUT, ERR_ENDS_MATCH = \
    -2, -3, -4, -5, -6, -7, -8


@pytest.fixture(scope="module")
def lz4_safe(aqz):
    m = re.match(r"lz4 \S+ \(([^)]+)\)", aqz.blosc_codec_info())
    if not m:
        return None
    fn = ctypes.CDLL(m.group(1)).LZ4_decompress_safe
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]

    def decompress(block, cap):
        src = np.frombuffer(bytes(block), np.uint8)
        dst = np.zeros(cap + 1, np.uint8)
        n = fn(src.ctypes.data, dst.ctypes.data, src.size, cap)
        return n, dst[:max(n, 0)].tobytes()

    return decompress


def check_block(aqz, lz4_safe, block, want, ctx):
    n = len(want)
    got_n, out = aqz.debug_lz4_decode_host(block, n)
    assert got_n == n, (ctx, got_n, n)
    assert out.tobytes() == want, ctx
    # a roomier destination: the same bytes, the rest untouched
    got_n, out = aqz.debug_lz4_decode_host(block, n + 9)
    assert got_n == n and out[:n].tobytes() == want and (out[n:] == 0xA5).all(), ctx
    # one byte short: refused, nothing past the end (the array ends there)
    if n:
        got_n, _ = aqz.debug_lz4_decode_host(block, n - 1)
        assert got_n in (ERR_LIT_OUT, ERR_MATCH_OUT), (ctx, got_n)
    if lz4_safe is not None and n:
        lib_n, lib_out = lz4_safe(block, n)
        assert (lib_n, lib_out) == (n, want), (ctx, lib_n)


@pytest.mark.parametrize("group", sorted(lc.GROUPS))
def test_every_encoder_case_round_trips(aqz, lz4_safe, group):
    """decode_block(encode_block(x)) == x == lz4_cases.decode, on every case;
    "small" holds the lengths 1..160, "length" LENGTH_EDGES, "counter" the
    match lengths 4 + COUNT_EDGES at offsets 1, 2, 3, 4, 7 and 300."""
    n_blocks = 0
    for name, n, accel, bufs in lc.cases(group, aqz):
        for k, buf in enumerate(bufs):
            csize, block, need = aqz.debug_lz4_block_host(buf, lc.bound(n), accel)
            assert csize > 0
            want, _ = lc.decode(block)
            assert want == buf.tobytes()
            check_block(aqz, lz4_safe, block, want, (name, k))
            n_blocks += 1
    assert n_blocks >= 3


def test_overlapping_matches_at_every_offset_and_length(aqz, lz4_safe):
    """offset x length over 1, 2, 3, 4, 7, 15, 16, 17, 63, 64, 65, 300, 65535
    and 4 + COUNT_EDGES: blocks written from the format."""
    cases = bd.overlap_blocks()
    assert len(cases) == len(bd.OVERLAP_OFFSETS) * len(bd.MATCH_LENGTHS)
    offs = set()
    for name, block, want in cases:
        check_block(aqz, lz4_safe, block, want, name)
        offs |= {off for _, off, _ in lc.decode(block)[1]}
    assert set(bd.OVERLAP_OFFSETS) <= offs


def test_run_lengths_at_the_length_byte_edges(aqz, lz4_safe):
    for name, block, want in bd.length_blocks():
        check_block(aqz, lz4_safe, block, want, name)


def test_named_defects_give_named_errors(aqz):
    data = bytes(range(200))
    cap = 4096

    def run(block, cap=cap):
        n, out = aqz.debug_lz4_decode_host(block, cap)
        return n

    assert run(b"") == -1
    assert run(bd.block([(data, 0, 8)], last=b"12345")) == ERR_OFF0
    assert run(bd.block([(data, 201, 8)], last=b"12345")) == ERR_OFF_BEFORE
    assert run(bd.block([(data, 65535, 8)], last=b"12345")) == ERR_OFF_BEFORE
    assert run(bytes([0xF0, 0xFF, 0x10]) + data) == ERR_LIT_IN
    assert run(bd.block([], last=data), cap=199) == ERR_LIT_OUT
    assert run(bd.block([(data, 200, 5000)], last=b"12345")) == ERR_MATCH_OUT
    assert run(bd.block([(data, 200, 8)])[:-1]) == ERR_ENDS_MATCH
    assert run(bytes([0xF0]) + b"\xff" * 9) == ERR_TRUNCATED
    good = bd.block([(data, 200, 8)], last=b"12345")
    assert run(good) == 213
    assert run(good + b"\x00") == ERR_TRUNCATED       # one trailing byte: no room for an offset
    assert run(good[:-1]) == ERR_LIT_IN               # the last literals cut short
    assert run(good[:203]) == ERR_TRUNCATED           # cut inside the offset
    # the one-byte block that stands for nothing
    assert run(b"\x00", cap=0) == 0


def test_flips_and_truncations_stay_inside_the_buffers(aqz):
    """Seeded single-byte flips and truncations of valid blocks: the result
    is a size within cap or a named error, and the bytes past a returned
    size still hold the fill.  (The accesses themselves are checked under
    the sanitizers by tests/cpp/blosc_decode_sweep.cpp.)"""
    rng = np.random.default_rng(11)
    blocks = [b for _, b, _ in bd.overlap_blocks()[:40]] + [b for _, b, _ in bd.length_blocks()[:3]]
    refused = 0
    for block in blocks:
        want_n = len(lc.decode(block)[0])
        for _ in range(25):
            b = bytearray(block)
            if rng.integers(0, 4) == 0:
                b = b[:int(rng.integers(0, len(b)))]
            else:
                b[int(rng.integers(0, min(len(b), 64)))] ^= 1 << int(rng.integers(0, 8))
            n, out = aqz.debug_lz4_decode_host(bytes(b), want_n)
            assert -8 <= n <= want_n
            if n >= 0:
                assert (out[n:] == 0xA5).all()
            refused += n < 0
    assert refused > 100


def test_bad_arguments(aqz):
    lib = aqz.lib()
    buf = np.zeros(16, np.uint8)
    assert lib.aqz_debug_lz4_decode_host(None, 16, buf.ctypes.data, 16) == -100
    assert lib.aqz_debug_lz4_decode_host(buf.ctypes.data, 16, None, 16) == -100
