"""GPU: reading blosc LZ4 frames back on the device — the wave-cooperative
split decoder, the unfilter kernels, aqz_blosc_lz4_decompress_device and
aqz_zarr_shard_decompress_device (csrc/codec_kernels.hip) — against the serial
statement in csrc/blosc_decode.hh, which tests/test_lz4_decode.py and
tests/test_blosc_decode.py pin to liblz4, c-blosc and c-blosc's own frames.

What the kernels have and the serial code lacks: a match copy that is
periodic where the match overlaps itself, stores of one lane read by another
a sequence later (ordered by a workgroup fence), 16-byte copies with byte
ends, a lane-read input window, several waves sharing one frame's status.
Outputs are poisoned with 0xA5; whatever a call must not touch has to hold it
afterwards.
"""
import numpy as np
import pytest

import blosc_decode_cases as bd
import lz4_cases as lc
import tiled_base_cases as tb
from gpu_util import empty_device, from_device, launch_stream, to_device, torch_cuda

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 256


@pytest.fixture(scope="module")
def ctx(aqz):
    c = aqz.BloscContext(0, 0)
    yield c
    c.close()


# ---- 1. the split decoder, one block per wave ---------------------------------

def decode_blocks(aqz, ctx, blocks, caps, gap=37):
    """One launch: block k packed behind block k - 1 (byte-granular), output
    slot k of caps[k] + gap bytes (gap odd: slots start at odd and even
    addresses).  Returns per block (result, slot bytes) and the guard."""
    nb = len(blocks)
    comp = np.frombuffer(b"".join(blocks), np.uint8)
    csize = np.array([len(b) for b in blocks], np.uint32)
    coff = np.concatenate([[0], np.cumsum(csize[:-1], dtype=np.uint64)]).astype(np.uint64)
    slot = np.array([c + gap for c in caps], np.uint64)
    ooff = np.concatenate([[0], np.cumsum(slot[:-1], dtype=np.uint64)]).astype(np.uint64)
    total = int(slot.sum())
    d_comp, d_csize, d_coff, d_ooff = (to_device(a) for a in (comp, csize, coff, ooff))
    d_cap = to_device(np.array(caps, np.uint32))
    d_out = empty_device(total + GUARD)
    d_out.fill_(POISON)
    d_res = empty_device(4 * nb)
    d_res.fill_(POISON)
    ctx.debug_lz4_decode_blocks_device(d_comp.data_ptr(), d_coff.data_ptr(), d_csize.data_ptr(),
                                       d_out.data_ptr(), d_ooff.data_ptr(), d_cap.data_ptr(),
                                       d_res.data_ptr(), nb, launch_stream())
    res = from_device(d_res, np.int32, (nb,))
    out = from_device(d_out, np.uint8, (-1,))
    slots = [out[int(ooff[k]):int(ooff[k] + slot[k])] for k in range(nb)]
    return res, slots, out[total:]


def against_serial(aqz, ctx, named_blocks, caps=None):
    """Device result, bytes and untouched rest of every slot against the
    serial decoder at the same capacity."""
    blocks = [b for _, b in named_blocks]
    if caps is None:
        caps = [len(lc.decode(b)[0]) for b in blocks]
    res, slots, guard = decode_blocks(aqz, ctx, blocks, caps)
    assert (guard == POISON).all(), "guard after the last slot written"
    bad = []
    for k, (name, block) in enumerate(named_blocks):
        want_n, want = aqz.debug_lz4_decode_host(block, caps[k])
        if int(res[k]) != want_n:
            bad.append((name, "result", int(res[k]), want_n))
            continue
        n = max(want_n, 0)
        if want_n >= 0 and not np.array_equal(slots[k][:n], want[:n]):
            at = int(np.flatnonzero(slots[k][:n] != want[:n])[0])
            bad.append((name, "bytes differ from", at, slots[k][at:at + 8].tobytes().hex(),
                        want[at:at + 8].tobytes().hex()))
        if not (slots[k][caps[k]:] == POISON).all():
            bad.append((name, "written past the capacity"))
        if want_n >= 0 and not (slots[k][n:] == POISON).all():
            bad.append((name, "written past the decoded size"))
    if bad:
        pytest.fail(f"{len(bad)} differences, the first:\n" + "\n".join(map(str, bad[:12])))
    return res


@pytest.mark.parametrize("group", sorted(lc.GROUPS))
def test_split_decoder_on_every_encoder_case(aqz, ctx, group):
    named = []
    for name, n, accel, bufs in lc.cases(group, aqz):
        for k, buf in enumerate(bufs):
            csize, block, _ = aqz.debug_lz4_block_host(buf, lc.bound(n), accel)
            named.append((f"{name}[{k}]", block))
    res = against_serial(aqz, ctx, named)
    assert (res > 0).all()


def test_overlapping_matches(aqz, ctx):
    """offset x length over 1 .. 65,535 and 4 + COUNT_EDGES: the copies whose
    sources are the bytes they write.  The 65,535 blocks decode to 65,547
    bytes and more with both matches at the largest distance."""
    cases = bd.overlap_blocks()
    res = against_serial(aqz, ctx, [(name, b) for name, b, _ in cases])
    assert [int(r) for r in res] == [len(w) for _, _, w in cases]
    far = [(b, w) for name, b, w in cases if name.startswith("overlap-o65535-")]
    assert far and all(len(w) >= 65547 and {o for _, o, _ in lc.decode(b)[1]} >= {65535}
                       for b, w in far)


def test_run_lengths_and_tight_capacities(aqz, ctx):
    """Length bytes at their edges; then every overlap block again with a
    capacity one byte short and 5 bytes short: refused as the serial decoder
    refuses, nothing written past the capacity."""
    against_serial(aqz, ctx, [(name, b) for name, b, _ in bd.length_blocks()])
    cases = bd.overlap_blocks()[::3]
    for short in (1, 5):
        named = [(f"{name}-short{short}", b) for name, b, _ in cases]
        res = against_serial(aqz, ctx, named, caps=[len(w) - short for _, _, w in cases])
        assert (res < 0).all()


# ---- 2. unfilter ---------------------------------------------------------------

# the geometries of tests/test_gpu_codecs.py's filter test, restated
UNFILTER_CASES = [
    # (typesize, blocksize, nbytes, n_buffers)
    (2, 65536, 131072, 4),
    (2, 65536, 65536 * 3 + 4096, 2),
    (2, 32768, 1000, 3),
    (1, 4096, 4096 * 5 + 8, 2),
    (4, 16384, 16384 * 4, 3),
    (8, 16384, 16384 * 2 + 48, 2),
    (16, 8192, 8192 * 2, 2),
    (3, 3000, 9000 + 7, 2),
    (2, 4104, 4104 * 2, 1),
    (2, 200, 13, 5),
    (4, 2, 10, 1),
]


@pytest.mark.parametrize("shuffle", [0, 1, 2], ids=["noshuffle", "shuffle", "bitshuffle"])
@pytest.mark.parametrize("case", UNFILTER_CASES, ids=lambda c: f"ts{c[0]}_bs{c[1]}_n{c[2]}x{c[3]}")
def test_unfilter_matches_oracle_and_inverts_the_filter(aqz, oracle, shuffle, case):
    ts, bs, nbytes, nbuf = case
    rng = np.random.default_rng(ts * 1000 + bs + nbytes + shuffle)
    host = rng.integers(0, 256, nbytes * nbuf, dtype=np.uint8)
    d_src = to_device(host)
    d_filt = empty_device(host.size)
    d_back = empty_device(host.size + GUARD)
    d_back.fill_(POISON)
    s = launch_stream()
    aqz.blosc_filter_device(shuffle, ts, bs, d_src.data_ptr(), nbytes, nbuf, d_filt.data_ptr(), s)
    aqz.blosc_unfilter_device(shuffle, ts, bs, d_filt.data_ptr(), nbytes, nbuf,
                              d_back.data_ptr(), s)
    back = from_device(d_back, np.uint8, (-1,))
    assert (back[host.size:] == POISON).all()
    assert np.array_equal(back[:host.size], host), "unfilter(filter(x)) != x"
    # and on bytes that are no filter's output, against the oracle
    d_back.fill_(POISON)
    aqz.blosc_unfilter_device(shuffle, ts, bs, d_src.data_ptr(), nbytes, nbuf, d_back.data_ptr(),
                              launch_stream())
    back = from_device(d_back, np.uint8, (-1,))
    for k in range(nbuf):
        want = oracle.blosc_unfilter(host[k * nbytes:(k + 1) * nbytes], shuffle, ts, bs)
        assert np.array_equal(back[k * nbytes:(k + 1) * nbytes], want), (case, shuffle, k)
    assert (back[host.size:] == POISON).all()


@pytest.mark.parametrize("shuffle", [1, 2])
def test_unfilter_unaligned_buffers(aqz, oracle, shuffle):
    rng = np.random.default_rng(40 + shuffle)
    for ts, bs, nbytes in ((2, 4096, 8192 + 40), (4, 4096 + 32, 3 * (4096 + 32) + 64),
                           (8, 2048, 2048 * 3 + 8)):
        host = rng.integers(0, 256, nbytes, dtype=np.uint8)
        src = empty_device(nbytes + 1)
        src[1:] = to_device(host)
        dst = empty_device(nbytes + 3 + GUARD)
        dst.fill_(POISON)
        aqz.blosc_unfilter_device(shuffle, ts, bs, src.data_ptr() + 1, nbytes, 1,
                                  dst.data_ptr() + 3, launch_stream())
        got = from_device(dst, np.uint8, (-1,))
        assert np.array_equal(got[3:3 + nbytes], oracle.blosc_unfilter(host, shuffle, ts, bs))
        assert (got[:3] == POISON).all() and (got[3 + nbytes:] == POISON).all()


def test_unfilter_errors(aqz):
    p = empty_device(64).data_ptr()
    for args in ((3, 2, 16, p, 32, 1, p + 32), (1, 0, 16, p, 32, 1, p + 32),
                 (1, 2, 0, p, 32, 1, p + 32), (1, 2, 16, 0, 32, 1, p + 32),
                 (1, 2, 16, p, 32, 0, p + 32), (1, 2, 16, p, 1 << 31, 1, p + 32)):
        with pytest.raises(aqz.AqzError):
            aqz.blosc_unfilter_device(*args)


# ---- 3. frames ------------------------------------------------------------------

def shard_image(frames, base, lead=3):
    """Frames packed end to end behind `lead` stray bytes, and their index
    table at file offset `base` (no CRC: it is not read)."""
    image = bytearray(b"\xEE" * lead)
    pairs = []
    for fr in frames:
        pairs += [base + len(image), len(fr)]
        image += fr
    return bytes(image), np.array(pairs, np.uint64)


def decode_frames_both_ways(aqz, ctx, frames, ts, nbytes, dst_gap=19):
    """The frames through the shard form (packed, byte-granular, the table 4
    bytes off 8-byte alignment) and the strided form (with and without the
    size table): (statuses, chunks) of each, outputs poisoned and guarded."""
    n = len(frames)
    out = []
    stride_out = nbytes + dst_gap
    base = (1 << 40) + 12345

    def run(call):
        d_dst = empty_device(n * stride_out + GUARD)
        d_dst.fill_(POISON)
        d_st = empty_device(4 * n + GUARD)
        d_st.fill_(POISON)
        call(d_dst, d_st)
        dst = from_device(d_dst, np.uint8, (-1,))
        st = from_device(d_st, np.uint8, (-1,))
        assert (dst[n * stride_out:] == POISON).all() and (st[4 * n:] == POISON).all()
        chunks = dst[:n * stride_out].reshape(n, stride_out)
        assert (chunks[:, nbytes:] == POISON).all(), "bytes between the chunks written"
        return [int(v) for v in st[:4 * n].copy().view(np.uint32)], chunks[:, :nbytes]

    image, table = shard_image(frames, base)
    d_img = to_device(np.frombuffer(image, np.uint8))
    d_tab = empty_device(table.nbytes + 4)
    d_tab[4:] = to_device(table)
    out.append(run(lambda d, s: ctx.zarr_shard_decompress_device(
        ts, nbytes, d_img.data_ptr(), len(image), base, d_tab.data_ptr() + 4, n, d.data_ptr(),
        stride_out, s.data_ptr(), launch_stream())))
    fstride = max(len(f) for f in frames) + 5
    packed = np.full(n * fstride, 0xEE, np.uint8)
    for k, fr in enumerate(frames):
        packed[k * fstride:k * fstride + len(fr)] = np.frombuffer(fr, np.uint8)
    d_fr = to_device(packed)
    d_sz = to_device(np.array([len(f) for f in frames], np.uint32))
    for sizes in (d_sz.data_ptr(), 0):
        out.append(run(lambda d, s: ctx.lz4_decompress_device(
            ts, nbytes, d_fr.data_ptr(), fstride, sizes, n, d.data_ptr(), stride_out,
            s.data_ptr(), launch_stream())))
    return out


def test_golden_frames(aqz, ctx):
    """c-blosc's own frames, LZ4 and zstd of one input in one call: LZ4 and
    memcpy frames decode to the input, zstd frames are UNSUPPORTED and leave
    their neighbours alone."""
    groups = {}
    for key, fr, src, ts in bd.golden():
        groups.setdefault((key.split("__")[0], ts), []).append((key, fr, src))
    n_lz4 = n_zstd = 0
    for (name, ts), items in groups.items():
        frames = [fr for _, fr, _ in items]
        src = np.frombuffer(items[0][2], np.uint8)
        for statuses, chunks in decode_frames_both_ways(aqz, ctx, frames, ts, src.size):
            for k, (key, fr, _) in enumerate(items):
                if "__zstd__" in key and not fr[2] & 0x2:
                    assert statuses[k] == aqz.FRAME_UNSUPPORTED, key
                    continue
                assert statuses[k] == aqz.FRAME_OK, (key, statuses[k])
                assert np.array_equal(chunks[k], src), key
        n_lz4 += sum("__lz4__" in k for k, _, _ in items)
        n_zstd += sum("__zstd__" in k for k, _, _ in items)
    assert n_lz4 >= 28 + 20 and n_zstd == 28


def chunk_kinds(rng, dtype, nbytes):
    ts = np.dtype(dtype).itemsize
    n = -(-nbytes // ts)
    x = np.arange(n)
    smooth = (1000 + 30 * np.sin(x / 9.0) + rng.normal(0, 2, n)).astype(dtype)
    rand = rng.integers(0, 256, n * ts, dtype=np.uint8)
    mixed = smooth.copy().view(np.uint8)
    mixed[mixed.size // 3:mixed.size // 2] = rng.integers(0, 256, mixed.size // 2 - mixed.size // 3)
    return np.stack([a.view(np.uint8).reshape(-1)[:nbytes]
                     for a in (smooth, rand, np.zeros(n * ts, np.uint8), mixed)])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64],
                         ids=["u8", "u16", "f32", "f64"])
def test_round_trip_through_the_device_encoder(aqz, ctx, dtype):
    """decode(encode(x)) == x with nothing leaving the device: smooth,
    random, zero and mixed chunks of 50 bytes, of a few KiB with a ragged end
    and of two 64 KiB blocks and a leftover, all three shuffles, both probe
    forms of the encoder."""
    ts = np.dtype(dtype).itemsize
    rng = np.random.default_rng(ts)
    for nbytes in (50, 4096 * ts + 24 + ts * 3, 2 * 65536 + 13 * ts + 1):
        chunks = chunk_kinds(rng, dtype, nbytes)
        n = chunks.shape[0]
        d_src = to_device(chunks)
        stride = nbytes + aqz.BLOSC_MAX_OVERHEAD
        for shuffle in (0, 1, 2):
            for flags in (0, aqz.LZ4_PROBE_SERIAL):
                clevel = 1 if flags else 5
                d_frames = empty_device(n * stride)
                d_sizes = empty_device(4 * n)
                d_dst = empty_device(n * nbytes + GUARD)
                d_dst.fill_(POISON)
                d_st = empty_device(4 * n)
                d_st.fill_(POISON)
                s = launch_stream()
                ctx.lz4_frames_device(clevel, shuffle, ts, d_src.data_ptr(), nbytes, n,
                                      d_frames.data_ptr(), stride, d_sizes.data_ptr(), s, flags)
                ctx.lz4_decompress_device(ts, nbytes, d_frames.data_ptr(), stride,
                                          d_sizes.data_ptr(), n, d_dst.data_ptr(), nbytes,
                                          d_st.data_ptr(), s)
                st = from_device(d_st, np.uint32, (n,))
                got = from_device(d_dst, np.uint8, (-1,))
                where = (np.dtype(dtype).name, nbytes, shuffle, flags)
                assert (st == aqz.FRAME_OK).all(), (where, st)
                assert np.array_equal(got[:n * nbytes].reshape(n, nbytes), chunks), where
                assert (got[n * nbytes:] == POISON).all(), where


# ---- 4. shards ------------------------------------------------------------------

def test_shard_round_trip(aqz, oracle, ctx):
    """Level 0 of a 96 x 128 u16 stream into its chunk lattice (3 frames a
    chunk, 32 x 48 chunks: ragged in x) with one chunk all zero; has_data from
    the zero scan; LZ4 frames; 2 x 2-chunk shards (ragged: 4 shards, padding
    slots) with seeded file offsets; tables; then every shard back through its
    own table.  Present chunks equal the lattice bytes; the skipped chunk and
    the padding are ABSENT and read as zeros."""
    torch = torch_cuda()
    geo = tb.halving(128, 96, 2)
    shapes = [(3, 32, 48), (3, 16, 16)]
    rng = np.random.default_rng(12)
    frames = rng.integers(1, 65536, (3, 96, 128), dtype=np.uint16)
    frames[:, 32:64, 48:96] = 0  # chunk (1, 1) = lattice index 4
    ds = aqz.Downsampler(geo, np.uint16, aqz.MEAN, device=0)
    lat = tb.Lattice(oracle, ds, geo, shapes, np.uint16, aqz.MEAN, frames, 0)
    s = launch_stream()
    assert lat.run(ds, s) == [3, 3]
    nt, slots = lat.nt[0], lat.slots[0]
    _, offs, cb, lb, cap = lat.want[0]
    assert nt == 9 and cb == 3 * 32 * 48 * 2 and lb == nt * cb
    d_has = empty_device(nt)
    d_has.fill_(0)
    aqz.zarr_shard_chunk_has_data_device(lat.flags[0].data_ptr(), 3, nt, slots, [0, 0, 0],
                                         d_has.data_ptr(), s)
    stride = cb + aqz.BLOSC_MAX_OVERHEAD
    d_frames, d_sizes = empty_device(nt * stride), empty_device(4 * nt)
    ctx.lz4_frames_device(5, 1, 2, lat.bufs[0].data_ptr(), cb, nt, d_frames.data_ptr(), stride,
                          d_sizes.data_ptr(), s)
    sdims = [(tb.TIME, 0, 3, 1), (tb.SPACE, 96, 32, 2), (tb.SPACE, 128, 48, 2)]
    st = aqz.ZarrShardSet(sdims, 0)
    assert (st.n_shards, st.chunks_per_shard, st.chunks_per_layer) == (4, 4, 9)
    st.begin(s)
    seeds = [1000, 0, (1 << 33) + 5, 77]
    st.debug_set_file_offsets(seeds, s)
    d_out = empty_device(nt * stride)
    d_seg = empty_device(8 * st.segment_words)
    st.append_layer_device(d_frames.data_ptr(), stride, d_out.data_ptr(), nt * stride,
                           d_seg.data_ptr(), d_sizes.data_ptr(), d_has.data_ptr(), s)
    d_tab = empty_device(st.n_shards * st.table_bytes)
    d_taboff = empty_device(8 * st.n_shards)
    st.tables_device(d_tab.data_ptr(), d_taboff.data_ptr(), s)
    seg = from_device(d_seg, np.uint64, (-1,))[:-1].reshape(-1, 3)
    has = from_device(d_has, np.uint8, (-1,))
    assert list(has) == [1, 1, 1, 1, 0, 1, 1, 1, 1]
    lattice = from_device(lat.bufs[0], np.uint8, (-1,))[:lb].reshape(nt, cb)
    _, shard_of, internal_of = aqz.zarr_shard_layout(sdims)
    n_absent = n_ok = 0
    for sh in range(st.n_shards):
        start, nbytes, file_off = (int(v) for v in seg[sh])
        assert file_off == seeds[sh]
        n = st.chunks_per_shard
        d_dst = empty_device(n * cb + GUARD)
        d_dst.fill_(POISON)
        d_st = empty_device(4 * n)
        d_st.fill_(POISON)
        ctx.zarr_shard_decompress_device(2, cb, d_out.data_ptr() + start, nbytes, file_off,
                                         d_tab.data_ptr() + sh * st.table_bytes, n,
                                         d_dst.data_ptr(), cb, d_st.data_ptr(), launch_stream())
        status = from_device(d_st, np.uint32, (n,))
        got = from_device(d_dst, np.uint8, (-1,))
        assert (got[n * cb:] == POISON).all()
        for i in range(n):
            c = [c for c in range(nt) if shard_of[c] == sh and internal_of[c] == i]
            chunk = got[i * cb:(i + 1) * cb]
            if c and has[c[0]]:
                assert status[i] == aqz.FRAME_OK, (sh, i, status[i])
                assert np.array_equal(chunk, lattice[c[0]]), (sh, i)
                n_ok += 1
            else:
                assert status[i] == aqz.FRAME_ABSENT, (sh, i, status[i])
                assert not chunk.any(), (sh, i)
                n_absent += 1
    assert (n_ok, n_absent) == (8, 8)  # 1 skipped chunk, 7 padding slots
    torch.cuda.synchronize()
    st.close()
    ds.close()


def test_shard_table_pairs_outside_the_shard(aqz, ctx):
    """A pair that starts before the base, ends past the shard's bytes or
    wraps around is CORRUPT; its neighbours still decode."""
    key, fr, src, ts = next(g for g in bd.golden() if g[0].startswith("smooth_u16") and
                            "__lz4__5__" in g[0])
    n = len(src)
    base = 5000
    image = b"\x11" * 7 + fr
    pairs = [base + 7, len(fr),
             base - 1, len(fr),
             base + 7, len(fr) + 1,
             base + 7, 0xFFFFFFFFFFFFFFF0,
             0xFFFFFFFFFFFFFFFF, len(fr),
             base + len(image), 0,
             base + 7, len(fr)]
    k = len(pairs) // 2
    d_img = to_device(np.frombuffer(image, np.uint8))
    d_tab = to_device(np.array(pairs, np.uint64))
    d_dst = empty_device(k * n + GUARD)
    d_dst.fill_(POISON)
    d_st = empty_device(4 * k)
    ctx.zarr_shard_decompress_device(ts, n, d_img.data_ptr(), len(image), base, d_tab.data_ptr(),
                                     k, d_dst.data_ptr(), n, d_st.data_ptr(), launch_stream())
    status = list(from_device(d_st, np.uint32, (k,)))
    C, B = aqz.FRAME_CORRUPT, aqz.FRAME_BAD_HEADER
    # the empty frame at the very end of the shard is inside it: a truncated header
    assert status == [aqz.FRAME_OK, C, C, C, C, B, aqz.FRAME_OK]
    got = from_device(d_dst, np.uint8, (-1,))
    want = np.frombuffer(src, np.uint8)
    assert np.array_equal(got[:n], want) and np.array_equal(got[6 * n:7 * n], want)
    assert (got[n:6 * n] == POISON).all() and (got[k * n:] == POISON).all()


# ---- 5. malformed frames ---------------------------------------------------------

MARGIN = 128 << 10


def test_malformed_frames_are_refused_inside_their_ranges(aqz, ctx):
    """Every defect of tests/blosc_decode_cases.defects between good frames,
    frames and chunks inside one poisoned allocation with 128 KiB of owned
    bytes on every side of both: the statuses are the host path's, the good
    neighbours decode, a bad frame's chunk may hold anything, and not a byte
    outside the chunks is touched."""
    cases = [c for c in bd.defects() if (c[2], c[3]) == (1, 4096)]
    assert len(cases) >= 24
    good = cases[0][1]
    want_good = aqz.debug_blosc_decode_host(good, 1, 4096)[1]
    frames, names = [], []
    for name, fr, _, _, _ in cases:
        frames += [fr, good]
        names += [name, "good"]
    n, nbytes = len(frames), 4096
    fstride = 8192 + 3
    assert max(len(f) for f in frames) <= fstride
    dstride = nbytes + 61
    f0, f1 = MARGIN, MARGIN + n * fstride
    o0 = f1 + MARGIN
    o1 = o0 + n * dstride
    host = np.full(o1 + MARGIN, POISON, np.uint8)
    for k, fr in enumerate(frames):
        host[f0 + k * fstride:f0 + k * fstride + len(fr)] = np.frombuffer(fr, np.uint8)
    d_all = to_device(host)
    d_sizes = to_device(np.array([len(f) for f in frames], np.uint32))
    d_st = empty_device(4 * n)
    d_st.fill_(POISON)
    ctx.lz4_decompress_device(1, nbytes, d_all.data_ptr() + f0, fstride, d_sizes.data_ptr(), n,
                              d_all.data_ptr() + o0, dstride, d_st.data_ptr(), launch_stream())
    status = from_device(d_st, np.uint32, (n,))
    after = from_device(d_all, np.uint8, (-1,))
    assert np.array_equal(after[:o0], host[:o0]), "bytes in front of the chunks changed"
    assert (after[o1:] == POISON).all(), "bytes behind the chunks changed"
    chunks = after[o0:o1].reshape(n, dstride)
    assert (chunks[:, nbytes:] == POISON).all(), "bytes between the chunks changed"
    bad = []
    for k, name in enumerate(names):
        want = aqz.debug_blosc_decode_host(frames[k], 1, nbytes)[0]
        if int(status[k]) != want:
            bad.append((k, name, int(status[k]), want))
        elif want == aqz.FRAME_OK and not np.array_equal(chunks[k, :nbytes], want_good):
            bad.append((k, name, "decoded bytes differ"))
    assert not bad, bad
    # the table says what each defect must give, the host path agreed above
    assert [int(s) for s in status[0::2]] == [c[4] for c in cases]


def test_header_that_disagrees_with_the_caller(aqz, ctx):
    """typesize or nbytes not the caller's: BAD_HEADER, nothing written."""
    good = bd.defects()[0][1]
    d_fr = to_device(np.frombuffer(good, np.uint8))
    for ts, nbytes in ((2, 4096), (1, 4097), (1, 4095)):
        d_dst = empty_device(nbytes + GUARD)
        d_dst.fill_(POISON)
        d_st = empty_device(4)
        ctx.lz4_decompress_device(ts, nbytes, d_fr.data_ptr(), len(good), 0, 1, d_dst.data_ptr(),
                                  nbytes, d_st.data_ptr(), launch_stream())
        assert from_device(d_st, np.uint32, (1,))[0] == aqz.FRAME_BAD_HEADER
        assert (from_device(d_dst, np.uint8, (-1,)) == POISON).all()


def test_invalid_arguments(aqz, ctx):
    p = empty_device(256).data_ptr()
    ok = dict(typesize=1, nbytes=64, device_frames=p, frame_stride=80, device_frame_bytes=0,
              n_frames=1, device_dst=p + 128, dst_stride=64, device_status=p + 200)
    for change in (dict(typesize=0), dict(nbytes=0), dict(device_frames=0), dict(n_frames=0),
                   dict(device_dst=0), dict(dst_stride=63), dict(device_status=0),
                   dict(nbytes=(1 << 31) - 16, dst_stride=1 << 31)):
        with pytest.raises(aqz.AqzError):
            ctx.lz4_decompress_device(**{**ok, **change})
    oks = dict(typesize=1, nbytes=64, device_shard_bytes=p, shard_bytes=80, base_file_offset=0,
               device_table=p + 96, n_chunks=1, device_dst=p + 128, dst_stride=64,
               device_status=p + 200)
    for change in (dict(typesize=0), dict(nbytes=0), dict(device_shard_bytes=0),
                   dict(device_table=0), dict(n_chunks=0), dict(device_dst=0),
                   dict(dst_stride=1), dict(device_status=0)):
        with pytest.raises(aqz.AqzError):
            ctx.zarr_shard_decompress_device(**{**oks, **change})
