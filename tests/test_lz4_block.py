"""CPU: the serial LZ4 block encoder of csrc/lz4_block.hh (what the device
kernel must produce) against LZ4_compress_fast of the liblz4 the frame writer
itself loads (aqz_blosc_codec_info), return value and bytes.

c-blosc compresses every split with LZ4_compress_fast(split, out, n, cap,
10 - clevel) (blosc_compress_ctx, reached from zarr.common.cpp:106-137); cap
is at most the split size, so the zero results matter as much as the bytes.
The encoder also reports `need`, the capacity its parse asked for: it must
predict the library's zero / non-zero result at every cap.
"""
import ctypes
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lz4(aqz):
    m = re.match(r"lz4 \S+ \(([^)]+)\)", aqz.blosc_codec_info())
    if not m:
        pytest.skip("no liblz4 loaded: " + aqz.blosc_codec_info())
    lib = ctypes.CDLL(m.group(1))
    fn = lib.LZ4_compress_fast
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]

    def compress(data, cap, accel):
        dst = np.zeros(cap + 1, np.uint8)
        n = fn(data.ctypes.data, dst.ctypes.data, data.size, cap, accel)
        return n, dst[:n].tobytes()

    return compress


KINDS = ["random", "sparse", "periodic", "far_repeat", "runs"]


def make_data(rng, kind, n):
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "sparse":
        v = rng.integers(0, 256, n, dtype=np.uint8)
        v[rng.integers(0, 16, n) != 0] = 0
        return v
    if kind == "periodic":
        period = int(rng.integers(1, 300))
        v = ((np.arange(n) % period) * 7).astype(np.uint8)
        noise = rng.integers(0, 64, n) == 0
        v[noise] = rng.integers(0, 256, int(noise.sum()), dtype=np.uint8)
        return v
    if kind == "far_repeat":
        v = rng.integers(0, 256, n, dtype=np.uint8)
        i = 16
        while i < n:
            ln = int(rng.integers(1, 200))
            if rng.integers(0, 2):
                back = int(rng.integers(1, min(i, 200000) + 1))
                ln = min(ln, n - i, back)
                v[i:i + ln] = v[i - back:i - back + ln]
            i += ln
        return v
    v = np.empty(n, np.uint8)
    i = 0
    while i < n:
        ln = int(rng.integers(1, 5000))
        v[i:i + ln] = rng.integers(0, 256)
        i += ln
    return v


def check(aqz, lz4, data, cap, accel, ctx):
    want_n, want = lz4(data, cap, accel)
    got_n, got, need = aqz.debug_lz4_block_host(data, cap, accel)
    assert got_n == want_n, (ctx, cap, accel, got_n, want_n, need)
    assert got == want, (ctx, cap, accel)
    assert (need <= cap) == (want_n != 0), (ctx, cap, accel, need, want_n)
    return need


def sweep(aqz, lz4, sizes, seed, accels=None):
    rng = np.random.default_rng(seed)
    zeros = cases = 0
    for n in sizes:
        for kind in KINDS:
            data = make_data(rng, kind, n)
            for accel in (accels or [int(rng.integers(1, 11))]):
                ctx = (n, kind)
                # above: the parse's whole need; then at, just below and well below it
                need = check(aqz, lz4, data, n + n // 255 + 16, accel, ctx)
                caps = {n, need, need - 1, need + 1, n - 1, n // 2, 1, 0}
                if n > 20:
                    caps.add(int(rng.integers(0, n)))
                for cap in sorted(c for c in caps if c >= 0):
                    check(aqz, lz4, data, cap, accel, ctx)
                    cases += 1
                    zeros += lz4(data, cap, accel)[0] == 0
    return cases, zeros


def test_small_sizes_every_acceleration(aqz, lz4):
    """0..64 bytes (12 / 13 is where matching starts), accelerations 1-10."""
    cases, zeros = sweep(aqz, lz4, list(range(0, 65)), 1, accels=list(range(1, 11)))
    assert cases > 10000 and zeros > 1000


def test_table_switch(aqz, lz4):
    """65,546 bytes still take the u16 table, 65,547 the u32 one with the
    distance rule."""
    cases, zeros = sweep(aqz, lz4, [65535, 65545, 65546, 65547, 65548, 65600], 2,
                         accels=[1, 5, 9])
    assert zeros > 50


def test_sizes_up_to_1mib(aqz, lz4):
    rng = np.random.default_rng(3)
    sizes = [int(x) for x in rng.integers(65, 40000, 24)] + [100000, 131072, 262144, 1 << 20]
    cases, zeros = sweep(aqz, lz4, sizes, 4)
    assert cases > 1000 and zeros > 200


def test_accelerations_on_compressible_data(aqz, lz4):
    sweep(aqz, lz4, [4096, 32768, 70000], 5, accels=list(range(1, 11)))


def test_bad_arguments(aqz):
    lib = aqz.lib()
    need = ctypes.c_uint32()
    buf = np.zeros(16, np.uint8)
    assert lib.aqz_debug_lz4_block_host(None, 16, buf.ctypes.data, 16, 1, ctypes.byref(need)) == -1
    assert lib.aqz_debug_lz4_block_host(buf.ctypes.data, 16, None, 16, 1, ctypes.byref(need)) == -1
    # need may be NULL
    out = np.zeros(32, np.uint8)
    assert lib.aqz_debug_lz4_block_host(buf.ctypes.data, 16, out.ctypes.data, 0, 1, None) == 0
    assert lib.aqz_debug_lz4_block_host(buf.ctypes.data, 16, out.ctypes.data, 32, 1, None) > 0
