"""Child process of tests/test_gpu_large_batch.py and
tests/test_gpu_large_codecs.py: runs one group of the large-batch cases on the
GPU with the launch log on ($AQZ_LAUNCH_LOG=1 is read once, at the library's
first launch, so it needs a process of its own) and prints one JSON object
per case:

  {"case": id, "seconds": s, "launches": [...], "kind": k,
   "error": null | text, "skip": null | text}

A failed comparison (AssertionError) is the case's "error" and the next case
runs.  Anything else (a HIP error, a fault reported by the runtime) ends the
child at once with status 3, so nothing more is launched on that card.

Usage: large_batch_child.py --group row|volume|deep|tiled|volume_tiled|filter|crc|lz4
"""
import argparse
import json
import os
import re
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402  (binds the HIP runtime before the library loads)

import aqz_pkg  # noqa: E402
import large_batch as lb  # noqa: E402
import oracle  # noqa: E402
from gpu_util import launch_stream  # noqa: E402

POISON, PAD = lb.POISON, lb.PAD
FILTER_TS, FILTER_BS, FILTER_CASES = lb.FILTER_TS, lb.FILTER_BS, lb.FILTER_CASES
filter_nbytes, filter_windows = lb.filter_nbytes, lb.filter_windows
CRC_CASES, CRC_LIMIT = lb.CRC_CASES, lb.CRC_LIMIT
LZ4_CHUNK, LZ4_PROTOS, LZ4_CASES, lz4_chunks = lb.LZ4_CHUNK, lb.LZ4_PROTOS, lb.LZ4_CASES, lb.lz4_chunks


class Skip(Exception):
    pass


def need_memory(need):
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        raise Skip(f"needs {need} bytes of device memory, {free} free")


def poison_kept(buf, size, what):
    assert bool((buf[size:] == POISON).all()), f"{what}: bytes behind the output were written"


# ---- pyramid cases ------------------------------------------------------------

def dev_level(case, arr):
    return lb.to_view(torch, arr, case.dtype)


def run_pyramid(aqz, case):
    """row, volume and zpath: aqz_ds_run_device_batch."""
    n = lb.frames_for(case)
    need_memory(lb.need_bytes(case))
    e = lb.expected_levels(oracle, case)
    d_in = lb.build_batch(torch, case, n)
    nl = len(case.geo)
    sizes = [0] + [lb.level_frames(case, L, n) * lb.frame_bytes(case, L) for L in range(1, nl)]
    outs = [None] + [lb.poisoned(torch, sizes[L]) for L in range(1, nl)]
    ds = aqz.Downsampler(case.geo, case.dtype, case.method)
    try:
        aqz.debug_launch_log()
        counts = ds.run_device_batch(d_in.data_ptr(), n, [0] + [o.data_ptr() for o in outs[1:]],
                                     launch_stream())
        torch.cuda.synchronize()
        kind = ds.last_batch_kind()
    finally:
        ds.close()
    launches = aqz.debug_launch_log()
    del d_in
    vt = lb.torch_view_dtype(torch, case.dtype)
    tags = lb.device_tags(torch, case, n // lb.group_planes(case))
    for L in range(1, nl):
        w, h, _ = case.geo[L]
        nf = lb.level_frames(case, L, n)
        assert counts[L] == nf, f"level {L}: {counts[L]} frames, expected {nf}"
        poison_kept(outs[L], sizes[L], f"level {L}")
        got = outs[L][:sizes[L]].view(vt).view(nf, h, w)
        lb.compare_frames(torch, got, dev_level(case, e[L]), None, tags, lb.per_group(case, L),
                          f"{case.id} level {L}")
    return kind, launches


def tiled_expected(case, e, L):
    """(tiles of tag 0, 0/1 mask of the level's own elements, flags of tag 0,
    flags of any tag above 0), on the device."""
    t0, f0 = lb.tiled_expectation(oracle, case, L, e[L][0], 0)
    t1, f1 = lb.tiled_expectation(oracle, case, L, e[L][0], 1)
    mask = (t1 != t0).astype(case.dtype)
    return (dev_level(case, t0), dev_level(case, mask),
            torch.from_numpy(f0.copy()).to("cuda"), torch.from_numpy(f1.copy()).to("cuda"))


def run_tiled(aqz, case):
    n = lb.frames_for(case)
    need_memory(lb.need_bytes(case))
    e = lb.expected_levels(oracle, case)
    tr, tc = case.tile
    nl = len(case.geo)
    d_in = lb.build_batch(torch, case, n)
    ds = aqz.Downsampler(case.geo, case.dtype, case.method)
    try:
        nts, slots, sizes, fsizes, outs, flags = [0], [0], [0], [0], [None], [None]
        for L in range(1, nl):
            w, h, _ = case.geo[L]
            nt = (-(-h // tr)) * (-(-w // tc))
            s = ds.tiled_flag_slots(L, tr, tc)
            assert s >= 1 and nt * tr * tc == lb.frame_elems(case, L)
            assert nt * s <= lb.flag_bytes_bound(case, L)
            nts.append(nt)
            slots.append(s)
            sizes.append(n * lb.frame_bytes(case, L))
            fsizes.append(n * nt * s)
            outs.append(lb.poisoned(torch, sizes[L]))
            flags.append(lb.poisoned(torch, fsizes[L]))
        aqz.debug_launch_log()
        counts = ds.run_device_batch_tiled(
            d_in.data_ptr(), n, [None] + [(tr, tc)] * (nl - 1),
            [0] + [o.data_ptr() for o in outs[1:]], [0] + [f.data_ptr() for f in flags[1:]],
            launch_stream())
        torch.cuda.synchronize()
        kind = ds.last_batch_kind()
    finally:
        ds.close()
    launches = aqz.debug_launch_log()
    del d_in
    assert counts == [n] * nl, counts
    vt = lb.torch_view_dtype(torch, case.dtype)
    tags = lb.device_tags(torch, case, n)
    for L in range(1, nl):
        t0, mask, f0, f1 = tiled_expected(case, e, L)
        poison_kept(outs[L], sizes[L], f"level {L} tiles")
        poison_kept(flags[L], fsizes[L], f"level {L} flags")
        got = outs[L][:sizes[L]].view(vt).view(n, nts[L], tr, tc)
        lb.compare_frames(torch, got, t0.unsqueeze(0), mask.unsqueeze(0), tags, 1,
                          f"{case.id} level {L} tiles")
        fl = flags[L][:fsizes[L]].view(n, nts[L], slots[L])
        assert bool((fl <= 1).all()), f"level {L}: flag slot left unwritten"
        nz = (fl != 0).any(-1)
        want = torch.where((tags == 0).view(-1, 1), f0.view(1, -1), f1.view(1, -1))
        bad = (nz != want).any(1)
        if bool(bad.any()):
            k = int(torch.nonzero(bad)[0])
            raise AssertionError(f"{case.id} level {L}: zero-scan flags of {int(bad.sum())} frames "
                                 f"differ, first frame {k} (tag {int(tags[k])})")
    return kind, launches


def run_lattice(aqz, case):
    from test_gpu_lattice import level_dims
    n = lb.frames_for(case)
    need_memory(lb.need_bytes(case))
    e = lb.expected_levels(oracle, case)
    tr, tc = case.tile
    tf = lb.LATTICE_DIMS[0][2]          # frames per chunk
    nl = len(case.geo)
    b = lb.bpp(case)
    assert n % tf == 0
    lats, bufs, caps, nts = [None], [None], [0], [0]
    for L in range(1, nl):
        # oracle addressing (array.dimensions.cpp:232-314), never the product's
        o, cb, layer = oracle.chunk_frame_offsets(level_dims(lb.LATTICE_DIMS, case.geo, L), b, 0, n)
        w, h, _ = case.geo[L]
        nt = (-(-h // tr)) * (-(-w // tc))
        assert cb == tf * tr * tc * b and layer == nt * cb
        # frame k: layer k // tf, place k % tf inside each chunk
        assert o == [(k // tf) * layer + (k % tf) * tr * tc * b for k in range(n)]
        cap = (max(o) // layer + 1) * layer
        assert cap == n * lb.frame_bytes(case, L)
        caps.append(cap)
        nts.append(nt)
        bufs.append(lb.poisoned(torch, cap))
        lats.append((bufs[L].data_ptr(), cap, tr, tc, cb, o))
    assert caps[1] > 1 << 32
    d_in = lb.build_batch(torch, case, n)
    ds = aqz.Downsampler(case.geo, case.dtype, case.method, device=0)
    try:
        aqz.debug_launch_log()
        counts = ds.run_device_batch_chunked(d_in.data_ptr(), n, lats, None, launch_stream())
        torch.cuda.synchronize()
        kind = ds.last_batch_kind()
    finally:
        ds.close()
    launches = aqz.debug_launch_log()
    del d_in
    assert counts == [n] * nl, counts
    vt = lb.torch_view_dtype(torch, case.dtype)
    # one chunk layer as a group: (chunk, frame in chunk, rows, cols)
    tags = lb.device_tags(torch, case, n).view(n // tf, 1, 1, tf, 1, 1)
    for L in range(1, nl):
        t0, mask, _, _ = tiled_expected(case, e, L)
        poison_kept(bufs[L], caps[L], f"level {L}")
        got = bufs[L][:caps[L]].view(vt).view(n // tf, nts[L], tf, tr, tc)
        lb.compare_frames(torch, got, t0.view(1, nts[L], 1, tr, tc), mask.view(1, nts[L], 1, tr, tc),
                          tags, 1, f"{case.id} level {L} lattice")
    return kind, launches


def volume_tiled_expected(case, e, L):
    """tiled_expected for the level's planes of one plane group: (per, nt, tr,
    tc) tiles of tag 0 and mask, (per, nt) flags of tag 0 and of any tag above."""
    per = lb.per_group(case, L)
    t0, f0, t1, f1 = [], [], [], []
    for j in range(per):
        a, fa = lb.tiled_expectation(oracle, case, L, e[L][j], 0)
        b, fb = lb.tiled_expectation(oracle, case, L, e[L][j], 1)
        t0.append(a), f0.append(fa), t1.append(b), f1.append(fb)
    t0, t1 = np.stack(t0), np.stack(t1)
    mask = (t1 != t0).astype(case.dtype)
    return (dev_level(case, t0), dev_level(case, mask),
            torch.from_numpy(np.stack(f0)).to("cuda"), torch.from_numpy(np.stack(f1)).to("cuda"))


def run_volume_tiled(aqz, case):
    """aqz_ds_run_device_volume_tiled with flags: level L's n >> L planes,
    a plane group's planes sharing its tag."""
    n = lb.frames_for(case)
    need_memory(lb.need_bytes(case))
    e = lb.expected_levels(oracle, case)
    tr, tc = case.tile
    nl = len(case.geo)
    gp = lb.group_planes(case)
    assert n % gp == 0
    d_in = lb.build_batch(torch, case, n)
    nts, sizes, fsizes, outs, flags = [0], [0], [0], [None], [None]
    for L in range(1, nl):
        w, h, _ = case.geo[L]
        nt = (-(-h // tr)) * (-(-w // tc))
        assert nt * tr * tc == lb.frame_elems(case, L) and lb.level_frames(case, L, n) == n >> L
        nts.append(nt)
        sizes.append((n >> L) * lb.frame_bytes(case, L))
        fsizes.append((n >> L) * nt)
        outs.append(lb.poisoned(torch, sizes[L]))
        flags.append(lb.poisoned(torch, fsizes[L]))
    ds = aqz.Downsampler(case.geo, case.dtype, case.method)
    try:
        aqz.debug_launch_log()
        counts = ds.run_device_volume_tiled(
            d_in.data_ptr(), n, [None] + [(tr, tc)] * (nl - 1),
            [0] + [o.data_ptr() for o in outs[1:]], [0] + [f.data_ptr() for f in flags[1:]],
            launch_stream())
        torch.cuda.synchronize()
        kind = ds.last_batch_kind()
    finally:
        ds.close()
    launches = aqz.debug_launch_log()
    del d_in
    assert counts == [n >> L for L in range(nl)], counts
    vt = lb.torch_view_dtype(torch, case.dtype)
    tags = lb.device_tags(torch, case, n // gp)
    for L in range(1, nl):
        per = lb.per_group(case, L)
        t0, mask, f0, f1 = volume_tiled_expected(case, e, L)
        poison_kept(outs[L], sizes[L], f"level {L} tiles")
        poison_kept(flags[L], fsizes[L], f"level {L} flags")
        got = outs[L][:sizes[L]].view(vt).view(n >> L, nts[L], tr, tc)
        lb.compare_frames(torch, got, t0, mask, tags, per, f"{case.id} level {L} tiles")
        fl = flags[L][:fsizes[L]].view(n // gp, per, nts[L])
        assert bool((fl <= 1).all()), f"level {L}: a flag byte is neither 0 nor 1"
        want = torch.where((tags == 0).view(-1, 1, 1), f0.unsqueeze(0), f1.unsqueeze(0))
        bad = ((fl != 0) != want).flatten(1).any(1)
        if bool(bad.any()):
            k = int(torch.nonzero(bad)[0])
            raise AssertionError(f"{case.id} level {L}: zero-scan flags of {int(bad.sum())} plane "
                                 f"groups differ, first group {k} (tag {int(tags[k])})")
    return kind, launches


def run_volume_lattice(aqz, case):
    """aqz_ds_run_device_volume_chunked into whole chunk layers: every byte of
    every lattice is owned by a plane of the batch."""
    import volume_tiled_cases as vc
    n = lb.frames_for(case)
    need_memory(lb.need_bytes(case))
    e = lb.expected_levels(oracle, case)
    nl = len(case.geo)
    b = lb.bpp(case)
    gp = lb.group_planes(case)
    shapes = lb.VOLUME_LATTICE_SHAPES
    lats, bufs, caps, nts = [None], [None], [0], [0]
    for L in range(1, nl):
        cz, tr, tc = shapes[L]
        nf = n >> L
        # oracle addressing (array.dimensions.cpp:232-314), never the product's
        o, cb, layer = oracle.chunk_frame_offsets(vc.chunk_dims(L, case.geo, shapes), b, 0, nf)
        w, h, _ = case.geo[L]
        nt = (-(-h // tr)) * (-(-w // tc))
        assert cb == cz * tr * tc * b and layer == nt * cb and nf % cz == 0
        assert o == [(k // cz) * layer + (k % cz) * tr * tc * b for k in range(nf)]
        cap = (max(o) // layer + 1) * layer
        assert cap == nf * lb.frame_bytes(case, L)
        caps.append(cap)
        nts.append(nt)
        bufs.append(lb.poisoned(torch, cap))
        lats.append((bufs[L].data_ptr(), cap, tr, tc, cb, o))
    assert caps[1] > 1 << 32
    d_in = lb.build_batch(torch, case, n)
    ds = aqz.Downsampler(case.geo, case.dtype, case.method, device=0)
    try:
        aqz.debug_launch_log()
        counts = ds.run_device_volume_chunked(d_in.data_ptr(), n, lats, None, launch_stream())
        torch.cuda.synchronize()
        kind = ds.last_batch_kind()
    finally:
        ds.close()
    launches = aqz.debug_launch_log()
    del d_in
    assert counts == [n >> L for L in range(nl)], counts
    vt = lb.torch_view_dtype(torch, case.dtype)
    for L in range(1, nl):
        cz, tr, tc = shapes[L]
        per = lb.per_group(case, L)
        assert cz % per == 0
        q = cz // per                      # plane groups per chunk layer
        layers = (n >> L) // cz
        t0, mask, _, _ = volume_tiled_expected(case, e, L)
        poison_kept(bufs[L], caps[L], f"level {L}")
        # a layer: (chunk, group in chunk, plane of the group, rows, cols)
        got = bufs[L][:caps[L]].view(vt).view(layers, nts[L], q, per, tr, tc)
        tags = lb.device_tags(torch, case, n // gp).view(layers, 1, 1, q, 1, 1, 1)
        want0 = t0.permute(1, 0, 2, 3).reshape(1, nts[L], 1, per, tr, tc)
        m = mask.permute(1, 0, 2, 3).reshape(1, nts[L], 1, per, tr, tc)
        lb.compare_frames(torch, got, want0, m, tags, 1, f"{case.id} level {L} lattice")
    return kind, launches


def run_case(aqz, case):
    if case.family == "tiled":
        return run_tiled(aqz, case)
    if case.family == "lattice":
        return run_lattice(aqz, case)
    if case.family == "volume_tiled":
        return run_volume_tiled(aqz, case)
    if case.family == "volume_lattice":
        return run_volume_lattice(aqz, case)
    return run_pyramid(aqz, case)


PYRAMID_GROUPS = {
    "row": lambda: lb.select("row", "shallow"),
    "volume": lambda: lb.select("volume", "shallow"),
    "deep": lambda: lb.select("row", "deep") + lb.select("volume", "deep") + lb.select("zpath"),
    "tiled": lambda: lb.select("tiled") + lb.select("lattice"),
    "volume_tiled": lambda: lb.select("volume_tiled") + lb.select("volume_lattice"),
}


# ---- codec cases --------------------------------------------------------------

def run_filter(aqz, name):
    shuffle, nbuf = FILTER_CASES[name]
    nbytes = filter_nbytes(nbuf)
    ts, bs = FILTER_TS, FILTER_BS
    need_memory(2 * nbuf * nbytes + (1 << 30))
    g = torch.Generator(device="cuda").manual_seed(1000 + 10 * shuffle + nbuf)
    src = torch.randint(0, 256, (nbuf * nbytes,), dtype=torch.uint8, device="cuda", generator=g)
    dst = lb.poisoned(torch, nbuf * nbytes)
    aqz.debug_launch_log()
    aqz.blosc_filter_device(shuffle, ts, bs, src.data_ptr(), nbytes, nbuf, dst.data_ptr(),
                            launch_stream())
    torch.cuda.synchronize()
    launches = aqz.debug_launch_log()
    poison_kept(dst, nbuf * nbytes, name)
    win, cap, per, total = filter_windows(nbuf)

    def check(what, off, length):
        host = src[off:off + length].cpu().numpy()
        got = dst[off:off + length].cpu().numpy()
        want = oracle.blosc_filter(host, shuffle, ts, bs)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{name} {what}: {bad.size} of {length} bytes differ, first at "
                                 f"byte {off + int(bad[0])}: got {got[bad[0]]}, oracle "
                                 f"{want[bad[0]]}")

    for what, g0, nb in win:
        for blk in range(g0, g0 + nb):      # block by block: a window may span two buffers
            check(f"{what} (block {blk})", (blk // per) * nbytes + (blk % per) * bs, bs)
    left = nbytes - per * bs
    assert 0 < left < bs
    for k in range(nbuf):
        check(f"leftover of buffer {k}", k * nbytes + per * bs, left)
    if shuffle == 0:
        assert torch.equal(dst[:nbuf * nbytes], src), f"{name}: the copy differs somewhere"
    return None, launches


def run_crc(aqz, name):
    nbytes = CRC_CASES[name]
    nbuf, stride = 2, nbytes + 13
    need_memory(nbuf * stride + (1 << 28))
    g = torch.Generator(device="cuda").manual_seed(nbytes % 1000003)
    data = torch.randint(0, 256, (nbuf * stride,), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.full((nbuf + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    aqz.crc32c_device(data.data_ptr(), nbytes, stride, nbuf, out.data_ptr(), launch_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert all(int(x) == 0x5A5A5A5A for x in got[nbuf:]), "words behind the checksums written"
    for k in range(nbuf):
        want = lb.oracle_crc32c_parts(oracle, data[k * stride:k * stride + nbytes].cpu().numpy())
        assert int(got[k]) == want, f"{name} buffer {k}: {int(got[k]):#x}, oracle {want:#x}"
    return None, []


def run_crc_limit(aqz, name):
    """2^16 workgroups a buffer: refused before any launch (the buffer is
    there in full all the same)."""
    nbytes = 65536 * 16384
    need_memory(nbytes + (1 << 28))
    d = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    try:
        aqz.crc32c_device(d.data_ptr(), nbytes, nbytes, 1, out.data_ptr(), launch_stream())
    except aqz.AqzError:
        torch.cuda.synchronize()
        assert all(int(x) == 0x5A5A5A5A for x in out.cpu().numpy()), "output touched"
        return None, []
    raise AssertionError("nbytes = 65536 * 16384 was accepted")


_LZ4 = {}


def lz4_setup(aqz):
    """Context, the 5 prototype chunks and the host path's frames of them
    (aqz_blosc_compress_device, pinned to c-blosc by tests/test_gpu_blosc.py)."""
    if not _LZ4:
        from test_gpu_blosc_lz4 import smooth_chunks
        ctx = aqz.BloscContext(0, 0)
        rng = np.random.default_rng(4096)
        protos = smooth_chunks(rng, LZ4_PROTOS, 256, 256, np.uint16).view(np.uint8)
        protos = protos.reshape(LZ4_PROTOS, LZ4_CHUNK)
        d = torch.from_numpy(protos.copy()).to("cuda")
        want = ctx.compress_device(5, 1, 2, "lz4", d.data_ptr(), LZ4_CHUNK, LZ4_PROTOS)
        assert len({bytes(w) for w in want}) == LZ4_PROTOS
        _LZ4.update(ctx=ctx, protos=d, want=want)
    return _LZ4["ctx"], _LZ4["protos"], _LZ4["want"]


def run_lz4(aqz, name):
    if not re.match(r"lz4 \S+ \(", aqz.blosc_codec_info()):
        raise Skip("no liblz4 loaded: " + aqz.blosc_codec_info())
    flags = LZ4_CASES[name]
    n = lz4_chunks()
    stride = LZ4_CHUNK + 16 + 48
    need_memory(n * (LZ4_CHUNK + stride) + (1 << 30))
    ctx, protos, want = lz4_setup(aqz)
    src = torch.empty((n, LZ4_CHUNK), dtype=torch.uint8, device="cuda")
    for p in range(LZ4_PROTOS):
        src[p::LZ4_PROTOS] = protos[p]
    dst = lb.poisoned(torch, n * stride)
    sizes = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    aqz.debug_launch_log()
    ctx.lz4_frames_device(5, 1, 2, src.data_ptr(), LZ4_CHUNK, n, dst.data_ptr(), stride,
                          sizes.data_ptr(), launch_stream(), flags)
    torch.cuda.synchronize()
    launches = aqz.debug_launch_log()
    poison_kept(dst, n * stride, name)
    assert bool((sizes[n:] == 0x5A5A5A5A).all()), "words behind the sizes written"
    frames = dst[:n * stride].view(n, stride)
    for p in range(LZ4_PROTOS):
        w = torch.from_numpy(np.frombuffer(want[p], np.uint8).copy()).to("cuda")
        rows = frames[p::LZ4_PROTOS]
        sz = sizes[:n][p::LZ4_PROTOS]
        bad = sz != len(want[p])
        assert not bool(bad.any()), (f"{name}: chunk {p + LZ4_PROTOS * int(torch.nonzero(bad)[0])}"
                                     f" has another size than the host path's {len(want[p])}")
        bad = (rows[:, :len(want[p])] != w.view(1, -1)).any(1)
        assert not bool(bad.any()), (f"{name}: frame bytes of {int(bad.sum())} chunks of prototype "
                                     f"{p} differ, first chunk "
                                     f"{p + LZ4_PROTOS * int(torch.nonzero(bad)[0])}")
        assert bool((rows[:, LZ4_CHUNK + 16:] == POISON).all()), \
            f"{name}: bytes written past a frame of prototype {p}"
    return None, launches


CODEC_GROUPS = {
    "filter": (list(FILTER_CASES), run_filter),
    "crc": (list(CRC_CASES), run_crc),
    "lz4": (list(LZ4_CASES), run_lz4),
}
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", required=True)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    aqz = aqz_pkg.load()
    if args.group in PYRAMID_GROUPS:
        work = [(c.id, lambda c=c: run_case(aqz, c)) for c in PYRAMID_GROUPS[args.group]()]
    else:
        names, run = CODEC_GROUPS[args.group]
        work = [(name, lambda name=name: run(aqz, name)) for name in names]
        if args.group == "crc":
            work.append((CRC_LIMIT, lambda: run_crc_limit(aqz, CRC_LIMIT)))
    for cid, job in work:
        rec = {"case": cid, "seconds": 0.0, "launches": [], "kind": None, "error": None,
               "skip": None}
        t0 = time.perf_counter()
        fatal = False
        try:
            rec["kind"], rec["launches"] = job()
        except Skip as s:
            rec["skip"] = str(s)
        except AssertionError as a:
            rec["error"] = str(a) or traceback.format_exc()[-1500:]
        except Exception:  # a HIP error: nothing more runs on this card
            rec["error"] = traceback.format_exc()[-3000:]
            fatal = True
        rec["seconds"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(rec), flush=True)
        if fatal:
            return 3
        try:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
        except Exception:
            print(json.dumps({"case": None, "error": traceback.format_exc()[-3000:]}), flush=True)
            return 3
    print("DONE", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
