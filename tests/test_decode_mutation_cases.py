"""CPU: the mutation corpus of tests/decode_mutation_cases.py on the serial
decoder alone (aqz_debug_lz4_decode_host, aqz_debug_blosc_decode_host) — what
tests/test_gpu_decode_mutations.py holds the wave decoder to.

The corpus is only worth something if it reaches every outcome in every place
the wave decoder has code of its own for; the counts below say so.  Nothing
here comes from a device.
"""
import ctypes
import re
import struct
from collections import Counter

import numpy as np
import pytest

import blosc_ref
import decode_mutation_cases as dm


@pytest.fixture(scope="module")
def corpus(aqz):
    return dm.corpus(aqz)


@pytest.fixture(scope="module")
def lz4_safe(aqz):
    m = re.match(r"lz4 \S+ \(([^)]+)\)", aqz.blosc_codec_info())
    if not m:
        return None
    fn = ctypes.CDLL(m.group(1)).LZ4_decompress_safe
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]

    def decompress(block, cap):
        src = np.frombuffer(bytes(block) + b"\0", np.uint8)  # a pointer even for no bytes
        dst = np.zeros(cap + 1, np.uint8)
        n = fn(src.ctypes.data, dst.ctypes.data, src.size - 1, cap)
        return n, dst[:max(n, 0)].tobytes()

    return decompress


def test_the_corpus_is_the_same_on_two_builds(aqz, corpus):
    again = dm.build(aqz)
    assert again["block_seeds"] == corpus["block_seeds"]
    assert again["block_mutants"] == corpus["block_mutants"]
    assert again["frame_seeds"] == corpus["frame_seeds"]
    assert again["frame_mutants"] == corpus["frame_mutants"]
    assert (again["M_blocks"], again["M_frames"]) == (corpus["M_blocks"], corpus["M_frames"])


def test_block_seeds_decode_to_their_bytes(aqz, corpus):
    seeds = corpus["block_seeds"]
    assert len(seeds) >= 50 + 9 + 40 + 2 + 2 + 3
    for s in seeds:
        n, out = aqz.debug_lz4_decode_host(s.block, len(s.plain))
        assert n == len(s.plain) and out.tobytes() == s.plain, s.name
    pre = [s for s in seeds if s.name.startswith("prefix-")]
    assert len(pre) == 2 and all(500 <= len(s.block) <= 700 for s in pre), [len(s.block) for s in pre]
    # the three blocks that straddle the first window refill do
    by = {s.name: dm.walk_block(s.block) for s in seeds if s.name.startswith("refill-")}
    assert by["refill-offset"][1]["offset"] == 255
    assert {255, 256} <= set(by["refill-literal-run"][2]["lit_run"])
    assert {255, 256} <= set(by["refill-match-run"][1]["ml_run"])


def test_every_block_outcome_is_present(aqz, corpus):
    seeds, muts = corpus["block_seeds"], corpus["block_mutants"]
    want = dm.block_expectations(aqz)
    assert 2800 <= len(muts) <= 3600, len(muts)
    codes = Counter(n for n, _ in want if n < 0)
    print("block mutants:", len(muts), "codes:", dict(sorted(codes.items())))
    for code in range(-8, 0):
        assert codes[code] >= 8, (code, codes)
    other = sum(1 for m, (n, out) in zip(muts, want)
                if n >= 0 and out[:n].tobytes() != seeds[m.seed].plain)
    assert other >= 100, other
    # refused at the drawn capacity, accepted with all the room a block of
    # its size can ask for (255 bytes out of every byte in)
    by_cap = 0
    for m, (n, _) in zip(muts, want):
        if n in (-4, -7) and len(m.block) <= 8192 and by_cap < 60:
            by_cap += aqz.debug_lz4_decode_host(m.block, 255 * len(m.block) + 64)[0] >= 0
    print("accepted with other bytes:", other, "refused by the capacity alone:", by_cap)
    assert by_cap >= 20, by_cap
    assert any(len(m.block) == 0 for m in muts) and any(m.cap == 0 for m in muts)
    kinds = Counter(re.split(r"[@:0-9]", m.kind)[0] for m in muts)
    for kind in ("bit", "set", "cut", "append", "prefix", "token", "offset", "run", "last-token"):
        assert kinds[kind] >= 6, (kind, kinds)
    assert kinds["prefix"] == sum(len(s.block) for s in seeds if s.name.startswith("prefix-"))
    for name in ("refill-offset", "refill-literal-run", "refill-match-run"):
        mine = [m.kind for m in muts if seeds[m.seed].name == name]
        assert len(mine) == 7 and {"valid", "cut255", "cut256", "cut257"} <= set(mine), mine


def test_liblz4_accepts_no_block_the_serial_decoder_refuses(aqz, corpus, lz4_safe):
    """Every mutant LZ4_decompress_safe accepts at its capacity the serial
    decoder accepts with the same bytes.  Not the reverse: the library's
    end-of-block rules are stricter.  One exception, which decode_block's
    comment in csrc/blosc_decode.hh states: liblz4 1.9.3 does not look at an
    offset of 0 and copies output bytes nobody has written; the serial decoder
    answers kDecOffsetZero (-5), and that is the only answer it may give to a
    block the library takes."""
    if lz4_safe is None:
        pytest.skip("no liblz4 loaded: " + aqz.blosc_codec_info())
    agreed = offset_zero = 0
    for m, (n, out) in zip(corpus["block_mutants"], dm.block_expectations(aqz)):
        lib_n, lib_out = lz4_safe(m.block, m.cap)
        if lib_n < 0:
            continue
        if n == -5:
            offset_zero += 1
            continue
        assert n == lib_n and out[:n].tobytes() == lib_out, (m.name, n, lib_n)
        agreed += 1
    print("liblz4 accepts", agreed + offset_zero, "mutants;", offset_zero, "of them with an offset of 0")
    assert agreed >= 300, agreed


def test_frame_seeds_decode_to_their_sources(aqz, corpus):
    seeds = corpus["frame_seeds"]
    written = [s for s in seeds if s.written]
    assert len(written) == 3 * len(dm.WRITTEN_SHAPES) + sum(len(w[4]) for w in dm.WAVE_SHAPES)
    assert sum(not s.written for s in seeds) >= 30
    n_cblosc = 0
    for s in seeds:
        assert len(s.src) <= dm.MAX_CHUNK
        st, out = aqz.debug_blosc_decode_host(s.frame, s.ts, len(s.src))
        assert st == dm.OK and out.tobytes() == s.src, s.name
        # c-blosc reads a header whose blocksize is a multiple of the typesize
        # or which is not split; it computes the split rule itself
        bs = struct.unpack_from("<I", s.frame, 8)[0]
        if s.written and blosc_ref.available() and bs % s.ts == 0:
            assert blosc_ref.decompress(s.frame, len(s.src)).tobytes() == s.src, s.name
            n_cblosc += 1
    if blosc_ref.available():
        assert n_cblosc >= 20, n_cblosc
    # the shapes asked for by name
    by = {s.name: s for s in seeds}
    for name in dm.SHARD_SEEDS + dm.LAUNCH_LOG_SEEDS:
        assert name in by
    # a bit-shuffled leftover whose element count is no multiple of 8
    s = by["ts2-leftover-405-elements/bitshuffle"]
    assert (len(s.src) % 4096) // 2 % 8 != 0
    # several waves on a frame, for every one of typesize 2, 4 and 8
    for ts in (2, 4, 8):
        assert any(s.ts == ts and dm.waves_of(len(s.src)) >= 2 and not s.frame[2] & 0x2
                   for s in seeds), ts
    # the split of 4098 / 4 is refused, the same frame with 0x10 is a seed
    for filt in dm.FILTER_NAMES:
        si, seed, muts = dm.seed_named(aqz, "ts4-bs4098/" + filt)
        (m,) = [m for m in muts if m.kind == "clear-0x10"]
        assert seed.frame[2] & 0x10
        assert aqz.debug_blosc_decode_host(m.frame, 4, len(seed.src))[0] == dm.BAD_HEADER


def test_every_frame_outcome_is_present(aqz, corpus):
    seeds, per_seed = corpus["frame_seeds"], corpus["frame_mutants"]
    want = dm.frame_expectations(aqz, "sizes")
    status, place, filt, waves = Counter(), Counter(), Counter(), 0
    n = 0
    for seed, muts, exp in zip(seeds, per_seed, want):
        assert 15 <= len(muts) <= 34, (seed.name, len(muts))
        for m, (st, _) in zip(muts, exp):
            n += 1
            status[st] += 1
            if st == dm.CORRUPT:
                place[m.place] += 1
                filt[seed.filt] += 1
                waves += dm.waves_of(len(seed.src)) >= 2
    print("frame mutants:", n, "of", len(seeds), "seeds; statuses:", dict(sorted(status.items())))
    print("CORRUPT by place:", dict(place), "by filter:", dict(filt), "in frames of 2+ waves:", waves)
    assert status[dm.OK] >= 50 and status[dm.BAD_HEADER] >= 50
    assert status[dm.UNSUPPORTED] >= 5 and status[dm.CORRUPT] >= 100
    assert status[dm.ABSENT] == 0
    for p in ("split-size", "later-split", "later-block", "leftover"):
        assert place[p] >= 10, (p, place)
    for f in (0, 1, 2):
        assert filt[f] >= 10, (f, filt)
    assert waves >= 10, waves
    # the header form gives every outcome too
    hdr = Counter(st for exp in dm.frame_expectations(aqz, "header") for st, _ in exp)
    print("header form:", dict(sorted(hdr.items())))
    assert hdr[dm.OK] >= 50 and hdr[dm.BAD_HEADER] >= 50 and hdr[dm.CORRUPT] >= 100


def test_the_margin_arithmetic(aqz, corpus):
    b = max(len(m.block) for m in corpus["block_mutants"])
    assert corpus["B_blocks"] == b and corpus["M_blocks"] == 65536 + 19 + 255 * b
    strides = [dm.frame_stride(s, m) for s, m in zip(corpus["frame_seeds"], corpus["frame_mutants"])]
    assert all(s % 2 == 1 for s in strides)
    assert corpus["B_frames"] == max(strides)
    assert corpus["M_frames"] == 65536 + 19 + 255 * max(strides)
    print("M blocks", corpus["M_blocks"], "B", b, "M frames", corpus["M_frames"], "B", max(strides))
    assert corpus["M_blocks"] <= 32 << 20 and corpus["M_frames"] <= 32 << 20
    # a pointer field moves in its low two bytes only
    for seed, muts in zip(corpus["frame_seeds"], corpus["frame_mutants"]):
        ptr = dm.pointer_fields(dm.layout(seed.frame))
        for m in muts:
            for lo, hi in ptr:
                if hi <= len(m.frame):
                    assert m.frame[lo + 2:hi] == seed.frame[lo + 2:hi], (m.name, lo)
    assert dm.waves_of(8191) == 1 and dm.waves_of(16384) == 2 and dm.waves_of(1 << 20) == 32


def test_the_numpy_filter_is_the_oracle_s(oracle):
    """filter_block against the unfilter of the C oracle: unfilter(filter(x)) == x."""
    rng = np.random.default_rng(3)
    for ts, bs, n in ((2, 4096, 9003), (3, 1200, 3001), (16, 2064, 5000), (4, 4098, 8206), (8, 4096, 8205)):
        x = rng.integers(0, 256, n, dtype=np.uint8)
        for filt in (1, 2):
            y = np.concatenate([dm.filter_block(filt, ts, x[o:o + bs]) for o in range(0, n, bs)])
            assert np.array_equal(oracle.blosc_unfilter(y, filt, ts, bs), x), (ts, bs, filt)
