"""CPU: whole blosc frames through the frame walker, the serial LZ4 decoder
and the host unfilter of csrc/blosc_decode.hh (aqz_debug_blosc_decode_host,
aqz_blosc_frame_info) — the statement the device decode must reproduce.

c-blosc's own frames (tests/golden/blosc_frames.npz and
blosc_decode_frames.npz, made by libblosc 1.21.0 with their inputs beside
them) must decode to their inputs byte for byte; fresh frames are compared
with blosc_decompress_ctx where libblosc is present; each named defect of
tests/blosc_decode_cases.defects gives its named status.
"""
import numpy as np
import pytest

import blosc_decode_cases as bd
import blosc_ref

needs_blosc = pytest.mark.skipif(not blosc_ref.available(), reason="no libblosc in this image")


def test_golden_lz4_frames_decode_to_their_inputs(aqz):
    classes = {"memcpy": 0, "raw": 0, "split": 0, "unsplit": 0}
    first_file = 0
    for key, fr, src, ts in bd.golden():
        if "__lz4__" not in key:
            continue
        first_file += not key.startswith(("unsplit_", "rawsplit_", "blocks_", "tail_"))
        st, out = aqz.debug_blosc_decode_host(fr, ts, len(src))
        assert st == aqz.FRAME_OK, key
        assert out.tobytes() == src, key
        kind, raw = bd.frame_class(fr)
        classes[kind] += 1
        classes["raw"] += raw
        info = aqz.blosc_frame_info(fr)
        assert info["status"] == aqz.FRAME_OK and info["nbytes"] == len(src), key
        assert info["memcpyed"] == (kind == "memcpy")
        assert info["nsplits"] == (ts if kind == "split" else 1) or kind == "memcpy"
    assert first_file == 28
    assert all(classes.values()), classes


def test_golden_zstd_frames_are_unsupported_unless_memcpy(aqz):
    seen = {aqz.FRAME_OK: 0, aqz.FRAME_UNSUPPORTED: 0}
    for key, fr, src, ts in bd.golden():
        if "__zstd__" not in key:
            continue
        st, out = aqz.debug_blosc_decode_host(fr, ts, len(src))
        if fr[2] & 0x2:
            assert st == aqz.FRAME_OK and out.tobytes() == src, key
        else:
            assert st == aqz.FRAME_UNSUPPORTED, key
        seen[st] += 1
    assert seen[aqz.FRAME_OK] and seen[aqz.FRAME_UNSUPPORTED] >= 10


def fresh_inputs(rng, ts, n):
    yield "random", rng.integers(0, 256, n, dtype=np.uint8)
    x = np.arange(n)
    yield "smooth", ((x // ts % 251) + rng.integers(0, 3, n)).astype(np.uint8)
    yield "zeros", np.zeros(n, np.uint8)
    m = np.zeros(n, np.uint8)
    m[n // 3:n // 2] = rng.integers(0, 256, n // 2 - n // 3, dtype=np.uint8)
    yield "mixed", m


@needs_blosc
@pytest.mark.parametrize("shuffle", [0, 1, 2])
@pytest.mark.parametrize("ts", [1, 2, 3, 4, 8, 16])
def test_fresh_frames_against_cblosc(aqz, ts, shuffle):
    """Leftover blocks of 1, 3, 12, 13 and 17 bytes behind one and two 64 KiB
    blocks (clevel 1), element counts that are no multiple of 8, sizes below
    the split threshold, and the destination sizes that make c-blosc store
    splits raw or fall back to memcpy."""
    rng = np.random.default_rng(100 * ts + shuffle)
    bs1 = aqz.blosc_blocksize(1, ts, 1 << 20, "lz4")
    sizes = [bs1 + left for left in (1, 3, 12, 13, 17)] + [2 * bs1 + 13]
    sizes += [128 * ts, 128 * ts - 1, 131 * ts + 1, 1000 * ts + 5 * ts, 50, 4096 + 24]
    n_frames = 0
    for n in sizes:
        for kind, src in fresh_inputs(rng, ts, n):
            for clevel in (1, 5):
                fr = blosc_ref.compress(src, clevel, shuffle, ts, "lz4")
                want = blosc_ref.decompress(fr, n)
                assert want.tobytes() == src.tobytes()
                st, out = aqz.debug_blosc_decode_host(fr, ts, n)
                assert st == aqz.FRAME_OK, (n, kind, clevel, blosc_ref.header(fr))
                assert out.tobytes() == src.tobytes(), (n, kind, clevel, blosc_ref.header(fr))
                n_frames += 1
    assert n_frames == len(sizes) * 8


@pytest.mark.parametrize("case", bd.defects(), ids=lambda c: c[0])
def test_named_defects(aqz, case):
    name, fr, ts, n, status = case
    st, out = aqz.debug_blosc_decode_host(fr, ts, n)
    assert st == status, name
    info = aqz.blosc_frame_info(fr, ts, n)
    if status in (aqz.FRAME_BAD_HEADER, aqz.FRAME_UNSUPPORTED) or name.startswith("block-starts"):
        assert info["status"] == status
    else:
        assert info["status"] == aqz.FRAME_OK  # the header is fine; the bytes are not


def test_memcpy_bit_wins_over_the_codec_bits(aqz):
    src = (np.arange(300) % 256).astype(np.uint8)
    for codec in (0, 1, 4, 7):
        fr = bd.header(0x2 | (codec << 5), 1, 300, 300, 316) + src.tobytes()
        st, out = aqz.debug_blosc_decode_host(fr, 1, 300)
        assert st == aqz.FRAME_OK and out.tobytes() == src.tobytes()
    # ... but not over its own size
    fr = bd.header(0x22, 1, 300, 300, 315) + src.tobytes()[:-1]
    assert aqz.debug_blosc_decode_host(fr, 1, 300)[0] == aqz.FRAME_BAD_HEADER


def test_invalid_arguments(aqz):
    with pytest.raises(aqz.AqzError):
        aqz.debug_blosc_decode_host(b"x" * 32, 0, 100)
    lib = aqz.lib()
    assert lib.aqz_blosc_frame_info(None, 0, 1, 1, None) != 0
