"""GPU: blosc+LZ4 chunk frames made wholly on the device
(aqz_blosc_lz4_frames_device, aqz_blosc_lz4_compress_device) against the host
path (aqz_blosc_compress_device, pinned to c-blosc by tests/test_gpu_blosc.py)
and, where the image has it, c-blosc 1.21 itself (oracle/blosc_ref.py).

The reference's compress_in_place (zarr.common.cpp:106-137, per chunk from
chunk.cpp:78-105) runs blosc_compress_ctx on every chunk buffer; here filter,
LZ4 and frame layout all run on the GPU and every frame must be the same
bytes.  Every case runs with the batched probe (flags 0) and the serial one
(AQZ_LZ4_PROBE_SERIAL).  Frames are written into device buffers poisoned with
0xA5, at a stride wider than a frame can be, so stale or stray bytes show.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import blosc_ref
import lz4_cases
from gpu_util import empty_device, from_device, launch_stream, to_device, torch_cuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
PAD = 48  # stride beyond nbytes + 16

pytestmark = [pytest.mark.gpu]

FLAGS = [pytest.param(0, id="batch"), pytest.param(1, id="serial")]


@pytest.fixture(scope="module", autouse=True)
def need_lz4(aqz):
    if not re.match(r"lz4 \S+ \(", aqz.blosc_codec_info()):
        pytest.skip("no liblz4 loaded: " + aqz.blosc_codec_info())


@pytest.fixture(scope="module")
def ctx(aqz):
    c = aqz.BloscContext(0, 0)
    yield c
    c.close()


def smooth_chunks(rng, n_chunks, h, w, dtype):
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n_chunks, h, w), dtype)
    for k in range(n_chunks):
        base = 2000 + 500 * np.sin((xx + 13 * k) / 17.0) * np.cos((yy - 5 * k) / 23.0)
        out[k] = (base + rng.normal(0, 4, (h, w))).astype(dtype)
    return out


_EXPECTED = {}


def expected_frames(ctx, key, raw, d_ptr, nbytes, n, clevel, shuffle, ts):
    """The host path's frames of this case, computed once and shared by both
    probe forms; checked against c-blosc itself where the image has it."""
    if key not in _EXPECTED:
        want = ctx.compress_device(clevel, shuffle, ts, "lz4", d_ptr, nbytes, n)
        if blosc_ref.available():
            for k, fr in enumerate(want):
                ref = blosc_ref.compress(raw[k * nbytes:(k + 1) * nbytes], clevel, shuffle, ts,
                                         "lz4")
                assert fr == ref, ("host path differs from c-blosc", key, k)
        _EXPECTED[key] = want
    return _EXPECTED[key]


def device_frames(aqz, ctx, d_ptr, nbytes, n, clevel, shuffle, ts, flags):
    """aqz_blosc_lz4_frames_device into poisoned device memory."""
    stride = nbytes + 16 + PAD
    d_dst = empty_device(n * stride)
    d_dst.fill_(POISON)
    d_sizes = empty_device(4 * n)
    d_sizes.fill_(POISON)
    ctx.lz4_frames_device(clevel, shuffle, ts, d_ptr, nbytes, n, d_dst.data_ptr(), stride,
                          d_sizes.data_ptr(), launch_stream(), flags)
    sizes = from_device(d_sizes, np.uint32, (n,))
    out = from_device(d_dst, np.uint8, (n, stride))
    frames = []
    for k in range(n):
        assert 16 <= sizes[k] <= nbytes + 16, (k, sizes[k])
        assert (out[k, nbytes + 16:] == POISON).all(), f"chunk {k}: bytes written past the frame"
        frames.append(out[k, :sizes[k]].tobytes())
    return frames


def assert_same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, k, len(g), len(w), blosc_ref.header(g), blosc_ref.header(w))


def check_case(aqz, ctx, key, raw, nbytes, n, clevel, shuffle, ts, flags, d=None):
    d = to_device(raw) if d is None else d
    want = expected_frames(ctx, key, raw, d.data_ptr(), nbytes, n, clevel, shuffle, ts)
    got = device_frames(aqz, ctx, d.data_ptr(), nbytes, n, clevel, shuffle, ts, flags)
    assert_same(got, want, key)
    return want


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("clevel", [1, 5, 9])
@pytest.mark.parametrize("shuffle", [0, 1, 2])
def test_u16_chunks(aqz, ctx, clevel, shuffle, flags):
    """6 x 128 KiB: u16-table splits of 32 KiB (clevel 1: blocks of 64 KiB)
    and 64 KiB (clevel 5, 9: one block)."""
    rng = np.random.default_rng(clevel * 7 + shuffle)
    raw = smooth_chunks(rng, 6, 256, 256, np.uint16).view(np.uint8).reshape(-1)
    want = check_case(aqz, ctx, ("u16", clevel, shuffle), raw, 131072, 6, clevel, shuffle, 2,
                      flags)
    if shuffle:  # compressible indeed once the byte planes are apart
        assert all(not f[2] & 0x2 and len(f) < 131072 for f in want)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("clevel,shuffle", [(5, 1), (9, 1), (9, 2)])
def test_u16_large_splits(aqz, ctx, clevel, shuffle, flags):
    """3 x 256 KiB: one block of two 128 KiB splits, past the 65,547-byte
    switch to the u32 table and its distance rule."""
    rng = np.random.default_rng(40 + clevel + shuffle)
    raw = smooth_chunks(rng, 3, 512, 256, np.uint16).view(np.uint8).reshape(-1)
    want = check_case(aqz, ctx, ("u16big", clevel, shuffle), raw, 262144, 3, clevel, shuffle, 2,
                      flags)
    assert all(blosc_ref.header(f)["blocksize"] == 262144 and not f[2] & 0x12 for f in want)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("ts,dtype", [(1, np.uint8), (4, np.float32), (8, np.float64)])
def test_other_typesizes(aqz, ctx, ts, dtype, flags):
    """6 x 100x130: leftover blocks, odd sizes, unaligned payload offsets."""
    rng = np.random.default_rng(ts)
    raw = smooth_chunks(rng, 6, 100, 130, dtype).view(np.uint8).reshape(-1)
    nbytes = 100 * 130 * ts
    d = to_device(raw)
    for clevel, shuffle in ((3, 1), (8, 2), (1, 0)):
        check_case(aqz, ctx, ("ts", ts, clevel, shuffle), raw, nbytes, 6, clevel, shuffle, ts,
                   flags, d)


@pytest.mark.parametrize("flags", FLAGS)
def test_typesize_17_is_never_split(aqz, ctx, flags):
    rng = np.random.default_rng(17)
    nbytes = 100 * 130 * 17
    raw = smooth_chunks(rng, 4, 100, 130 * 17, np.uint8).reshape(-1)
    d = to_device(raw)
    for clevel, shuffle in ((5, 1), (9, 2), (1, 0)):
        want = check_case(aqz, ctx, ("ts17", clevel, shuffle), raw, nbytes, 4, clevel, shuffle,
                          17, flags, d)
        assert all(f[2] & 0x10 for f in want)


@pytest.mark.parametrize("flags", FLAGS)
def test_incompressible_chunks_are_memcpy_frames(aqz, ctx, flags):
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, 12 * 70000, dtype=np.uint8)
    raw[5 * 70000:6 * 70000] = 7  # one compressible chunk among them
    want = check_case(aqz, ctx, ("random",), raw, 70000, 12, 5, 1, 2, flags)
    assert sum(1 for f in want if f[2] & 0x2) == 11
    for k, f in enumerate(want):
        if f[2] & 0x2:  # raw bytes from the unfiltered source
            assert f[16:] == raw[k * 70000:(k + 1) * 70000].tobytes()


@pytest.mark.parametrize("flags", FLAGS)
def test_all_zero_chunks(aqz, ctx, flags):
    raw = np.zeros(3 * 200000, np.uint8)
    d = to_device(raw)
    for clevel, shuffle, ts in ((5, 1, 2), (9, 2, 4), (1, 0, 1)):
        want = check_case(aqz, ctx, ("zero", clevel, shuffle, ts), raw, 200000, 3, clevel,
                          shuffle, ts, flags, d)
        assert all(len(f) < 2000 for f in want)


@pytest.mark.parametrize("flags", FLAGS)
def test_reduced_capacity_split(aqz, ctx, flags):
    """The second split compresses under a cap below its own size: the first
    one (random bytes) is stored raw and leaves 34,988 bytes of the
    destination."""
    raw = np.zeros(70000, np.uint8)
    raw[0::2] = np.random.default_rng(5).integers(0, 256, 35000)
    want = check_case(aqz, ctx, ("reduced",), raw, 70000, 1, 5, 1, 2, flags)
    frame = want[0]
    assert len(frame) == 35176 and frame[2] == 0x21
    (first, _), (second, _) = blosc_ref.stored_splits(frame)[0]
    assert first == 35000 and second == 35176 - 20 - 4 - 35000 - 4
    # what is left for the second split once the first is stored
    assert (70000 + 16) - (20 + 4 + 35000 + 4) == 34988


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("nbytes,clevel", [(100, 5), (64, 5), (5000, 0), (64, 0)])
def test_trivial_frames(aqz, ctx, nbytes, clevel, flags):
    raw = (np.arange(9 * nbytes) % 13).astype(np.uint8)
    want = check_case(aqz, ctx, ("trivial", nbytes, clevel), raw, nbytes, 9, clevel, 2, 2, flags)
    assert all(f[2] & 0x2 and len(f) == nbytes + 16 for f in want)


@pytest.mark.parametrize("flags", FLAGS)
def test_tiled_pyramid_tiles(aqz, ctx, oracle, flags):
    """The tiles aqz_ds_run_device_batch_tiled leaves in HBM for one 1024^2
    u16 frame, compressed where they lie."""
    torch = torch_cuda()
    W = H = 1024
    tile = 256
    dims = [(aqz.TIME, 0, 1, 1), (aqz.SPACE, H, tile, 1), (aqz.SPACE, W, tile, 1)]
    geo = aqz.level_geometry(aqz.plan_levels(dims))
    rng = np.random.default_rng(11)
    frame = smooth_chunks(rng, 1, H, W, np.uint16)[0]
    ds = aqz.Downsampler(geo, np.uint16, aqz.METHODS["mean"], device=0)
    d_in = to_device(frame)
    n_levels = len(geo)
    tiles_per = [0] + [(-(-w // tile)) * (-(-h // tile)) for w, h, _ in geo[1:]]
    outs = [None] + [empty_device(t * tile * tile * 2) for t in tiles_per[1:]]
    ds.run_device_batch_tiled(d_in.data_ptr(), 1, [(tile, tile)] * n_levels,
                              [0] + [o.data_ptr() for o in outs[1:]])
    torch.cuda.synchronize()
    ref = oracle.OracleDownsampler(geo, np.uint16, aqz.METHODS["mean"])
    ref.add_frame(frame)
    nb = tile * tile * 2
    for L in range(1, n_levels):
        want_tiles, _ = oracle.tile_frame(ref.take_frame(L), tile, tile)
        want_tiles = want_tiles.view(np.uint8).reshape(-1)
        check_case(aqz, ctx, ("tiled", L), want_tiles, nb, tiles_per[L], 1, 1, 2, flags,
                   outs[L])
    ds.close()


@pytest.mark.parametrize("flags", FLAGS)
def test_host_delivery_and_pcie_bytes(aqz, ctx, flags):
    """aqz_blosc_lz4_compress_device: the host path's frames and sizes, with
    only the frames and the uint32 size table copied device-to-host."""
    rng = np.random.default_rng(8)
    raw = smooth_chunks(rng, 10, 256, 256, np.uint16).view(np.uint8).reshape(-1).copy()
    raw[3 * 131072:4 * 131072] = rng.integers(0, 256, 131072)  # one memcpy frame
    n, nbytes = 10, 131072
    d = to_device(raw)
    want = expected_frames(ctx, ("pcie",), raw, d.data_ptr(), nbytes, n, 5, 1, 2)
    got = ctx.lz4_compress_device(5, 1, 2, d.data_ptr(), nbytes, n, flags=flags)
    assert_same(got, want, "host delivery")
    total = sum(len(f) for f in want)
    copied = ctx.d2h_bytes()
    # two copies (size table, packed frames), each at most one 16-byte pad off
    assert total + 4 * n <= copied <= total + 4 * n + 2 * 16, (copied, total)
    assert copied < n * nbytes  # less than the filtered volume the host path copies
    # caller's buffer and stride, sizes returned
    stride = nbytes + 16 + 100
    host = np.full(n * stride, POISON, np.uint8)
    sizes = ctx.lz4_compress_device(5, 1, 2, d.data_ptr(), nbytes, n, host_dst=host,
                                    dst_stride=stride, flags=flags)
    assert sizes == [len(f) for f in want]
    for k in range(n):
        assert host[k * stride:k * stride + sizes[k]].tobytes() == want[k]
        assert (host[k * stride + sizes[k]:(k + 1) * stride] == POISON).all()


@pytest.mark.parametrize("flags", FLAGS)
def test_single_split_chunk_at_its_capacity(aqz, ctx, flags):
    """A chunk of one split (typesize 1) has nbytes - 8 bytes for it: 16 of
    header, 4 of block start and 4 of split size out of nbytes + 16.  need ==
    nbytes - 8 is the last packed frame, need == nbytes - 7 the first memcpy
    one; the split's row alone decides."""
    n = 32768
    found = lz4_cases.capacity_scan(aqz, n, 1, 81, wanted=(-8, -7))
    assert sorted(found) == [-8, -7]
    for d in (-8, -7):
        assert aqz.debug_lz4_block_host(found[d], n, 1)[2] == n + d
    raw = np.concatenate([found[-8], found[-7]])
    want = check_case(aqz, ctx, ("onesplit",), raw, n, 2, 9, 0, 1, flags)
    packed, memcpyed = want
    assert blosc_ref.header(packed)["blocksize"] == n and not packed[2] & 0x12
    (((csize, _),),) = blosc_ref.stored_splits(packed)
    assert csize == aqz.debug_lz4_block_host(found[-8], n, 1)[0] and len(packed) == 24 + csize
    assert memcpyed[2] & 0x2 and len(memcpyed) == n + 16
    assert memcpyed[16:] == found[-7].tobytes()


@pytest.mark.parametrize("flags", FLAGS)
def test_split_compressed_to_its_own_size_is_stored_raw(aqz, ctx, flags):
    """csize == split size: c-blosc stores the filtered split, not the
    encoder's output of the same length."""
    n = 32768
    split1 = lz4_cases.capacity_scan(aqz, n, 1, 82, wanted=(0,))[0]
    csize, block, need = aqz.debug_lz4_block_host(split1, n, 1)
    assert csize == need == n and block != split1.tobytes()
    raw = np.zeros(2 * n, np.uint8)
    raw[1::2] = split1  # byte 1 of every element: split 1 once shuffled
    (frame,) = check_case(aqz, ctx, ("rawsplit",), raw, 2 * n, 1, 9, 1, 2, flags)
    assert blosc_ref.header(frame)["blocksize"] == 2 * n and not frame[2] & 0x12
    ((first, _), (second, payload)), = blosc_ref.stored_splits(frame)
    assert first < 200 and second == n
    assert payload == split1.tobytes()


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("r", [1, 3, 12, 13, 17])
def test_short_leftover_blocks(aqz, ctx, r, flags):
    """A leftover block of r bytes behind two full ones: one split below or at
    the encoder's 13-byte minimum, not a multiple of the typesize."""
    bs = aqz.blosc_blocksize(1, 4, 1 << 20, "lz4")
    nbytes = 2 * bs + r
    assert aqz.blosc_blocksize(1, 4, nbytes, "lz4") == bs
    rng = np.random.default_rng(90 + r)
    raw = np.empty(3 * nbytes, np.uint8)
    for k in range(3):
        body = smooth_chunks(rng, 1, 2 * bs // 1024, 256, np.float32)
        raw[k * nbytes:k * nbytes + 2 * bs] = body.view(np.uint8).reshape(-1)
        raw[k * nbytes + 2 * bs:(k + 1) * nbytes] = [7 * k] * r if k else rng.integers(0, 256, r)
    want = check_case(aqz, ctx, ("leftover", r), raw, nbytes, 3, 1, 1, 4, flags)
    for f in want:
        assert not f[2] & 0x2
        blocks = blosc_ref.stored_splits(f)
        assert [len(b) for b in blocks] == [4, 4, 1]


def test_errors(aqz, ctx):
    """Rejected before any launch: the output stays poisoned."""
    d = empty_device(1024)
    out = empty_device(2 * 600)
    out.fill_(POISON)
    sizes = empty_device(8)
    sizes.fill_(POISON)
    host = np.full(2 * 600, POISON, np.uint8)
    bad = [dict(clevel=10), dict(shuffle=3), dict(typesize=0), dict(flags=2), dict(flags=0x80000001),
           dict(dst_stride=520), dict(nbytes=0), dict(n_buffers=0)]
    for change in bad:
        a = dict(clevel=5, shuffle=1, typesize=2, nbytes=512, n_buffers=2, dst_stride=600,
                 flags=0)
        a.update(change)
        with pytest.raises(aqz.AqzError) as e:
            ctx.lz4_frames_device(a["clevel"], a["shuffle"], a["typesize"], d.data_ptr(),
                                  a["nbytes"], a["n_buffers"], out.data_ptr(), a["dst_stride"],
                                  sizes.data_ptr(), 0, a["flags"])
        assert e.value.status == 1, change
        if a["n_buffers"] and a["dst_stride"] >= 528:
            with pytest.raises(aqz.AqzError) as e:
                ctx.lz4_compress_device(a["clevel"], a["shuffle"], a["typesize"], d.data_ptr(),
                                        a["nbytes"], a["n_buffers"], host_dst=host,
                                        dst_stride=a["dst_stride"], flags=a["flags"])
            assert e.value.status == 1, change
    with pytest.raises(aqz.AqzError):  # stride too small, host delivery
        ctx.lz4_compress_device(5, 1, 2, d.data_ptr(), 512, 2, host_dst=host, dst_stride=520)
    for null in ("src", "dst", "sizes"):
        with pytest.raises(aqz.AqzError):
            ctx.lz4_frames_device(5, 1, 2, None if null == "src" else d.data_ptr(), 512, 2,
                                  None if null == "dst" else out.data_ptr(), 600,
                                  None if null == "sizes" else sizes.data_ptr())
    assert (from_device(out, np.uint8, (-1,)) == POISON).all()
    assert (from_device(sizes, np.uint8, (-1,)) == POISON).all()
    assert (host == POISON).all()


def test_launch_log():
    """One fresh process with the launch log on: the family=lz4 lines carry
    the probe form asked for and the table form the split size implies."""
    env = dict(os.environ)
    env["AQZ_LAUNCH_LOG"] = "1"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "lz4_launch_child.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    runs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [(x["flags"], x["want_table"]) for x in runs] == [(0, "u16"), (1, "u16"), (0, "u32"),
                                                             (1, "u32")]
    for x in runs:
        assert x["equal"], x
        lz4 = [rec for rec in x["launches"] if rec.get("family") == "lz4"]
        assert len(lz4) == 1, x["launches"]
        rec = lz4[0]
        assert rec["probe"] == ("serial" if x["flags"] else "batch")
        assert rec["table"] == x["want_table"]
        # two chunks of one block of two splits: four streams, one wave each
        assert rec["streams"] == 4 and rec["grid"] == 4 and rec["block"] == 64
