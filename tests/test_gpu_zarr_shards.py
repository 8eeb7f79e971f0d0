"""GPU: Zarr v3 shards assembled on the device (include/aqz_shard.h).

Every case fills `device_out` and the tables with a poison byte and keeps a
guard region behind them: every output byte is checked, everything past
`total` and the guard must keep the poison, and the segment rows must be the
model's.  The expected offsets are plain Python sums (zarr_shard_model.py);
the expected tables come from oracle.shard_index_table, the restatement of
Shard::write_table_.  Inputs are seeded random bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import zarr_shard_model as zm
from gpu_util import torch_cuda

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_shard_kats.json")))
POISON = 0xA5
GUARD = 4096
SENT = zm.SENTINEL


def dev_bytes(n, fill=POISON):
    torch = torch_cuda()
    return torch.full((max(int(n), 1),), fill, dtype=torch.uint8, device="cuda")


def dev_from(arr):
    torch = torch_cuda()
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to("cuda")


class Rig:
    """One shard set with its model and poisoned device outputs."""

    def __init__(self, aqz, dims, out_capacity, dst_off=0):
        self.aqz = aqz
        self.set = aqz.ZarrShardSet(dims, 0)
        self.model = zm.ShardModel(dims)
        m = self.model
        assert (self.set.n_shards, self.set.chunks_per_shard, self.set.chunks_per_layer,
                self.set.layers_per_shard) == (m.n_shards, m.cps, m.cpl, m.lps)
        self.cap = out_capacity
        self.dst_off = dst_off
        self.out = dev_bytes(dst_off + out_capacity + GUARD)
        self.seg = dev_bytes(8 * self.set.segment_words + GUARD)
        self.tab = dev_bytes(self.set.table_bytes * m.n_shards + GUARD)
        self.tab_off = dev_bytes(8 * m.n_shards + GUARD)

    def close(self):
        self.set.close()

    def append(self, oracle, frames_host, src_off, stride, sizes, has, d_frames, sizes_given=True,
               has_given=True):
        """frames_host: the host copy of the device buffer d_frames; frame c
        at src_off + c * stride.  Checks rows, every out byte and the poison."""
        torch = torch_cuda()
        m = self.model
        self.out.fill_(POISON)
        self.seg.fill_(POISON)
        d_sizes = dev_from(np.asarray(sizes, np.uint32)) if sizes_given else None
        d_has = dev_from(np.asarray(has, np.uint8)) if has_given else None
        self.set.append_layer_device(
            d_frames.data_ptr() + src_off, stride, self.out.data_ptr() + self.dst_off, self.cap,
            self.seg.data_ptr(), d_sizes.data_ptr() if sizes_given else 0,
            d_has.data_ptr() if has_given else 0)
        torch.cuda.synchronize()
        rows, total, place = m.append(sizes, has)
        seg = self.seg.cpu().numpy()
        got = seg[:8 * self.set.segment_words].view(np.uint64)
        want = np.array([v for r in rows for v in r] + [total], np.uint64)
        assert np.array_equal(got, want), (got, want)
        assert np.all(seg[8 * self.set.segment_words:] == POISON)
        expect = np.full(self.out.numel(), POISON, np.uint8)
        for c in range(m.cpl):
            if place[c] is not None:
                a = src_off + c * stride
                at = self.dst_off + place[c]
                expect[at:at + sizes[c]] = frames_host[a:a + sizes[c]]
        out = self.out.cpu().numpy()
        if not np.array_equal(out, expect):
            bad = np.flatnonzero(out != expect)
            raise AssertionError(f"{bad.size} output bytes differ, first at {bad[0]} "
                                 f"(dst_off {self.dst_off}, total {total})")
        return rows, total, place

    def tables(self, oracle):
        torch = torch_cuda()
        m = self.model
        self.tab.fill_(POISON)
        self.tab_off.fill_(POISON)
        self.set.tables_device(self.tab.data_ptr(), self.tab_off.data_ptr())
        torch.cuda.synchronize()
        tb = self.set.table_bytes
        tab = self.tab.cpu().numpy()
        off = self.tab_off.cpu().numpy()
        for s in range(m.n_shards):
            want = oracle.shard_index_table(m.offsets[s], m.extents[s])
            assert np.array_equal(tab[s * tb:(s + 1) * tb], want), f"table of shard {s}"
        assert np.all(tab[m.n_shards * tb:] == POISON)
        assert np.array_equal(off[:8 * m.n_shards].view(np.uint64),
                              np.array(m.file_off, np.uint64))
        assert np.all(off[8 * m.n_shards:] == POISON)
        return tab[:m.n_shards * tb].reshape(m.n_shards, tb)


# ---- 1. piece and alignment sweep ------------------------------------------

def sweep_sizes(aqz):
    P = aqz.ZARR_SHARD_PACK_PIECE
    stride = 2 * P + 64
    sizes = (list(range(0, 34)) + [63, 64, 65, 255, 256, 257, 4095, 4096, 4097,
                                   P - 1, P, P + 1, 2 * P + 3, stride])
    return sizes, stride


_SWEEP = {}


def sweep_input(aqz):
    """The frames of the sweep, made once and left unchanged."""
    if not _SWEEP:
        sizes, stride = sweep_sizes(aqz)
        host = np.random.default_rng(1).integers(0, 256, len(sizes) * stride + 16, dtype=np.uint8)
        _SWEEP.update(host=host, dev=dev_from(host))
    return _SWEEP["host"], _SWEEP["dev"]


HAS_PATTERNS = {
    "all": lambda n: [1] * n,
    "none": lambda n: [0] * n,
    "alternating": lambda n: [i % 2 for i in range(n)],
    "first": lambda n: [1] + [0] * (n - 1),
    "last": lambda n: [0] * (n - 1) + [1],
}


@pytest.mark.parametrize("offsets", [(1, 0), (3, 5), (15, 9)], ids=lambda o: f"src{o[0]}dst{o[1]}")
@pytest.mark.parametrize("pattern", list(HAS_PATTERNS))
def test_piece_and_alignment_sweep(aqz, oracle, pattern, offsets):
    src_off, dst_off = offsets
    sizes, stride = sweep_sizes(aqz)
    n = len(sizes)
    host, dev = sweep_input(aqz)
    has = HAS_PATTERNS[pattern](n)
    rig = Rig(aqz, zm.one_shard_dims(n), n * stride, dst_off)
    rows, total, place = rig.append(oracle, host, src_off, stride, sizes, has, dev)
    if pattern == "all":
        assert total == sum(sizes)
        # every destination alignment occurs, by construction of the sizes
        base = rig.out.data_ptr() + dst_off
        seen = {(base + place[c]) % 16 for c in range(n) if sizes[c]}
        assert seen == set(range(16)), seen
        # and the odd source base makes source and destination disagree mod 16
        assert any((dev.data_ptr() + src_off + c * stride - base - place[c]) % 16
                   for c in range(n))
    rig.tables(oracle)
    rig.close()


def test_uncompressed_frames_need_no_size_table(aqz, oracle):
    """device_frame_bytes NULL: every frame is frame_stride bytes; has_data
    NULL: every chunk present."""
    n, stride = 5, 1000
    host = np.random.default_rng(2).integers(0, 256, n * stride, dtype=np.uint8)
    rig = Rig(aqz, zm.one_shard_dims(n), n * stride)
    rows, total, _ = rig.append(oracle, host, 0, stride, [stride] * n, [1] * n, dev_from(host),
                                sizes_given=False, has_given=False)
    assert total == n * stride
    rig.tables(oracle)
    rig.close()


# ---- 2. scan widths --------------------------------------------------------

def scan_case(aqz, oracle, dims, seed):
    stride = 100
    n = zm.layout(dims)[2]
    sizes = [1 + (7 * i) % 97 for i in range(n)]
    has = [0 if i % 5 == 3 else 1 for i in range(n)]
    host = np.random.default_rng(seed).integers(0, 256, n * stride, dtype=np.uint8)
    rig = Rig(aqz, dims, n * stride)
    rows, total, _ = rig.append(oracle, host, 0, stride, sizes, has, dev_from(host))
    assert total == sum(s for s, h in zip(sizes, has) if h)
    rig.tables(oracle)
    rig.close()


@pytest.mark.parametrize("slots", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 4099])
def test_scan_over_slots(aqz, oracle, slots):
    scan_case(aqz, oracle, zm.one_shard_dims(slots), slots)


@pytest.mark.parametrize("shards", [1, 2, 65, 300])
def test_scan_over_shards(aqz, oracle, shards):
    scan_case(aqz, oracle, zm.many_shard_dims(shards, 3), 1000 + shards)


# ---- 3. ragged shards and layers -------------------------------------------

@pytest.mark.parametrize("case", KATS["addressing"], ids=lambda c: c["name"])
def test_ragged_shards_and_layers(aqz, oracle, case):
    dims = [tuple(d) for d in case["dims"]]
    stride = 200
    rng = np.random.default_rng(len(dims))
    _, _, n, lps, _, _ = zm.layout(dims)
    rig = Rig(aqz, dims, n * stride)
    m = rig.model
    if len(dims) == 3:
        assert (m.n_shards, m.cps, lps) == (4, 6, 1) and n < m.n_shards * m.cps  # ragged
    else:
        assert lps == 2
    for file_no in range(2):
        running = [0] * m.n_shards
        for layer in range(lps):
            sizes = [int(v) for v in rng.integers(0, stride + 1, n)]
            has = [int(v) for v in rng.integers(0, 4, n) > 0]
            host = rng.integers(0, 256, n * stride, dtype=np.uint8)
            rows, total, place = rig.append(oracle, host, 0, stride, sizes, has, dev_from(host))
            # file offsets continue across the layers of a file, from 0
            assert [r[2] for r in rows] == running
            running = [r[2] + r[1] for r in rows]
            tab = rig.tables(oracle)
            pairs = tab[:, :-4].copy().view(np.uint64).reshape(m.n_shards, m.cps, 2)
            for s in range(m.n_shards):
                real = {layer * m.spl + int(m.slot_of[c]): c for c in range(n)
                        if m.shard_of[c] == s}
                for i in range(m.cps):
                    li = i // m.spl
                    if li > layer:
                        assert tuple(pairs[s, i]) == (SENT, SENT)  # never appended
                    elif li == layer and (i not in real or not has[real[i]]):
                        assert tuple(pairs[s, i]) == (SENT, SENT)  # ragged or skipped
                    elif li == layer:
                        assert pairs[s, i, 1] == sizes[real[i]]
        # the shards are full: one more layer is refused, nothing changes
        with pytest.raises(aqz.AqzError) as e:
            rig.set.append_layer_device(rig.out.data_ptr(), stride, rig.out.data_ptr(),
                                        n * stride, rig.seg.data_ptr())
        assert e.value.status == 1
        rig.tables(oracle)
        rig.set.begin()
        m.begin()
    rig.tables(oracle)  # a fresh set of shards: all sentinel, offsets 0
    assert m.file_off == [0] * m.n_shards
    rig.close()


# ---- 4. shard-finalize.cpp's cases -----------------------------------------

def test_shard_finalize_cases(aqz, oracle):
    fin = KATS["finalize"]
    assert fin["chunks_per_shard"] == 2 and fin["bytes_per_chunk"] == 32
    nb = fin["bytes_per_chunk"]
    dims = zm.one_shard_dims(1, layers=2)  # 2 chunks per shard, one a layer
    rig = Rig(aqz, dims, nb)
    assert rig.set.chunks_per_shard == 2
    host = np.full(nb, fin["fill_byte"], np.uint8)
    dev = dev_from(host)
    written = 0
    for k in (1, 2):
        rows, total, _ = rig.append(oracle, host, 0, nb, [nb], [1], dev, sizes_given=False,
                                    has_given=False)
        written += total
        tab = rig.tables(oracle)
        pairs = tab[0, :-4].copy().view(np.uint64).reshape(2, 2)
        assert tuple(pairs[0]) == (0, nb)
        assert tuple(pairs[1]) == ((SENT, SENT) if k == 1 else (nb, nb))
        # the file: written chunk data + index table + crc32 (shard-finalize.cpp:14-20)
        assert written + tab.shape[1] == fin["expected_shard_size"][str(k)]
        assert rig.model.file_off[0] == written  # where the table goes
    rig.close()


# ---- 5. end to end ---------------------------------------------------------

def test_pyramid_level_to_shards(aqz, oracle):
    """The geometry of test_gpu_lattice.py::test_completed_layer_compresses_in_place
    (512x512 u16, 128-pixel chunks, 4 frames a chunk, 8 frames): level 1 goes
    into its chunk lattice with some tiles all zero, then has_data from the
    zero scan, LZ4 frames on the device, the shards to the host.  The test
    walks each shard's image by its own table."""
    torch = torch_cuda()
    dims = [(zm.TIME, 0, 4, 1), (zm.SPACE, 512, 128, 1), (zm.SPACE, 512, 128, 1)]
    geo = aqz.level_geometry(aqz.plan_levels(dims))
    n_frames, tile = 8, 128
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 65536, (n_frames, 512, 512), dtype=np.uint16)
    frames[:, :256, 256:] = 0   # level-1 tile 1 of every frame: chunk 1 empty in both layers
    frames[4:, 256:, :256] = 0  # and tile 2 in the second layer
    ds = aqz.Downsampler(geo, np.uint16, aqz.METHODS["mean"], device=0)
    d_in = dev_from(frames)
    lats, bufs, flags, info = [None], [None], [None], [None]
    for L in range(1, len(geo)):
        w, h, _ = geo[L]
        ld = [dims[0], (zm.SPACE, h, tile, 1), (zm.SPACE, w, tile, 1)]
        o, cb, lb = aqz.chunk_frame_offsets(ld, 2, 0, n_frames)
        cap = (max(o) // lb + 1) * lb
        buf = dev_bytes(cap, 0)
        S = ds.tiled_flag_slots(L, tile, tile)
        nt = (-(-h // tile)) * (-(-w // tile))
        fl = dev_bytes(n_frames * nt * S, 0)
        lats.append((buf.data_ptr(), cap, tile, tile, cb, o))
        bufs.append(buf)
        flags.append(fl)
        info.append((cb, lb, nt, S))
    ds.run_device_batch_chunked(d_in.data_ptr(), n_frames, lats,
                                device_nonzero=[None] + [f.data_ptr() for f in flags[1:]])
    torch.cuda.synchronize()
    cb, lb, nt, S = info[1]
    assert nt == 4 and lb == 4 * cb
    # level 1 as an array of 2 x 2 chunks a layer, two layers to a shard,
    # shards of 2 x 1 chunks: 2 shards of 4 chunks
    sdims = [(zm.TIME, 0, 4, 2), (zm.SPACE, 256, tile, 2), (zm.SPACE, 256, tile, 1)]
    st = aqz.ZarrShardSet(sdims, 0)
    m = zm.ShardModel(sdims)
    assert (st.n_shards, st.chunks_per_shard, st.chunks_per_layer, st.layers_per_shard) == \
        (2, 4, 4, 2)
    ctx = aqz.BloscContext(0, 2)
    lattice = bufs[1].cpu().numpy()
    stride = cb + aqz.BLOSC_MAX_OVERHEAD
    d_frames = dev_bytes(nt * stride)
    d_sizes = dev_bytes(4 * nt)
    d_has = dev_bytes(nt)
    images = [bytearray() for _ in range(st.n_shards)]
    ref = []
    for layer in range(2):
        src = bufs[1].data_ptr() + layer * lb
        d_has.fill_(0)
        # 3-D dims: tile_group_offset is 0 for every frame (array.dimensions.cpp:264-282)
        aqz.zarr_shard_chunk_has_data_device(flags[1].data_ptr() + layer * 4 * nt * S, 4, nt, S,
                                             [0] * 4, d_has.data_ptr())
        ctx.lz4_frames_device(1, 1, 2, src, cb, nt, d_frames.data_ptr(), stride,
                              d_sizes.data_ptr())
        rows, total, data = st.append_layer(d_frames.data_ptr(), stride, d_sizes.data_ptr(),
                                            d_has.data_ptr())
        assert st.d2h_bytes() == total + 24 * st.n_shards + 8
        has = d_has.cpu().numpy()
        chunks = lattice[layer * lb:(layer + 1) * lb].reshape(nt, cb)
        assert list(has) == [int(chunks[c].any()) for c in range(nt)]
        assert list(has) == ([1, 0, 1, 1] if layer == 0 else [1, 0, 0, 1])
        ref.append(ctx.lz4_compress_device(1, 1, 2, src, cb, nt))
        for s in range(st.n_shards):
            start, nbytes, file_off = (int(v) for v in rows[s])
            assert file_off == len(images[s])  # segments continue the file
            images[s] += data[start:start + nbytes].tobytes()
        assert sum(int(r[1]) for r in rows) == total == data.size
    tab, tab_off = st.tables()
    for s in range(st.n_shards):
        assert int(tab_off[s]) == len(images[s])
        pairs = tab[s, :-4].copy().view(np.uint64).reshape(st.chunks_per_shard, 2)
        assert int(tab[s, -4:].copy().view(np.uint32)[0]) == oracle.crc32c(tab[s, :-4])
        used = 0
        for layer in range(2):
            for c in range(nt):
                if m.shard_of[c] != s:
                    continue
                off, ext = (int(v) for v in pairs[layer * m.spl + int(m.slot_of[c])])
                chunk = lattice[layer * lb + c * cb:layer * lb + (c + 1) * cb]
                if not chunk.any():
                    assert (off, ext) == (SENT, SENT)  # occupies no bytes
                    continue
                assert bytes(images[s][off:off + ext]) == ref[layer][c], (s, layer, c)
                used += ext
        assert used == len(images[s])
    ctx.close()
    st.close()
    ds.close()


# ---- 6. past 2^32 ----------------------------------------------------------

def test_file_offsets_past_4gib(aqz, oracle):
    """Running offsets seeded just below 2^32: table offsets and segment rows
    carry past it."""
    dims = zm.many_shard_dims(2, 3)
    stride = 64
    rig = Rig(aqz, dims, 6 * stride)
    seed = [(1 << 32) - 5, (1 << 33) - 1]
    rig.set.debug_set_file_offsets(seed)
    rig.model.file_off = list(seed)
    host = np.random.default_rng(6).integers(0, 256, 6 * stride, dtype=np.uint8)
    sizes = [3, 4, 5, 1, 0, 9]
    rows, total, _ = rig.append(oracle, host, 0, stride, sizes, [1] * 6, dev_from(host))
    assert [r[2] for r in rows] == seed
    tab = rig.tables(oracle)
    pairs = tab[:, :-4].copy().view(np.uint64).reshape(2, 3, 2)
    assert [int(v) for v in pairs[0, :, 0]] == [(1 << 32) - 5, (1 << 32) - 2, (1 << 32) + 2]
    assert [int(v) for v in pairs[1, :, 0]] == [(1 << 33) - 1, 1 << 33, 1 << 33]
    assert rig.model.file_off == [(1 << 32) + 7, (1 << 33) + 9]
    rig.close()


def test_output_past_4gib(aqz):
    """Three frames of about 1.5 GiB into one 4.5 GiB output, made and
    compared on the device: the last frame lies across output position 2^32."""
    torch = torch_cuda()
    G = 3 << 29  # 1.5 GiB
    stride = G + 4096
    sizes = [G - 7, G - 1, G]
    total = sum(sizes)
    assert sizes[0] + sizes[1] < 1 << 32 < total
    src = torch.empty(3 * stride, dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(64)
    step = 1 << 28
    for a in range(0, src.numel(), step):
        b = min(a + step, src.numel())
        src[a:b] = torch.randint(0, 256, (b - a,), dtype=torch.uint8, device="cuda",
                                 generator=gen)
    cap = 3 * stride
    out = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    seg = dev_bytes(8 * 4)
    st = aqz.ZarrShardSet(zm.one_shard_dims(3), 0)
    d_sizes = dev_from(np.asarray(sizes, np.uint32))
    st.append_layer_device(src.data_ptr(), stride, out.data_ptr(), cap, seg.data_ptr(),
                           d_sizes.data_ptr())
    torch.cuda.synchronize()
    rows = seg.cpu().numpy().view(np.uint64)
    assert [int(v) for v in rows] == [0, total, 0, total]
    at = 0
    for c in range(3):
        assert torch.equal(out[at:at + sizes[c]], src[c * stride:c * stride + sizes[c]]), c
        at += sizes[c]
    # the bytes either side of output position 2^32, named on their own
    edge = 1 << 32
    a = edge - (sizes[0] + sizes[1])  # their place in frame 2
    assert torch.equal(out[edge - 64:edge + 64], src[2 * stride + a - 64:2 * stride + a + 64])
    assert bool((out[total:] == POISON).all())
    tab, off = st.tables()
    pairs = tab[0, :-4].copy().view(np.uint64).reshape(3, 2)
    assert [tuple(int(v) for v in p) for p in pairs] == [
        (0, sizes[0]), (sizes[0], sizes[1]), (sizes[0] + sizes[1], sizes[2])]
    assert int(off[0]) == total
    st.close()


# ---- 7. launch form --------------------------------------------------------

def test_launch_log():
    """One fresh process with the launch log on: the _device calls record
    their kernels and nothing else — no copy to the host, no second pass."""
    env = dict(os.environ)
    env["AQZ_LAUNCH_LOG"] = "1"
    r = subprocess.run([sys.executable, "-u",
                        os.path.join(ROOT, "tests", "zarr_shard_launch_child.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    P = rec["piece"]
    stride = rec["stride"]
    pieces = -(-stride // P)
    assert pieces == 2
    common = {"family": "shard", "block": 256, "slots": 3, "shards": 2}
    assert rec["append"] == [
        dict(common, kernel="scan_slots", grid=2, piece=0),
        dict(common, kernel="scan_shards", grid=1, piece=0),
        dict(common, kernel="pack_nt", grid=6 * pieces, piece=P),
    ]
    # 2 tables of 4 * 3 + 1 words: one workgroup
    assert rec["tables"] == [dict(common, kernel="tables", grid=1, piece=0)]
    assert rec["begin"] == []
    # 70 frames of 300 tiles: two launches of 64 and 6 frames, 2 workgroups a frame
    assert rec["has_data"] == [
        {"family": "shard", "kernel": "chunk_flags", "grid": 128, "block": 256, "slots": 2,
         "shards": 0, "piece": 0},
        {"family": "shard", "kernel": "chunk_flags", "grid": 12, "block": 256, "slots": 2,
         "shards": 0, "piece": 0}]
    assert rec["has_data_ok"] is True


def test_refusals(aqz):
    dims = zm.one_shard_dims(4)
    st = aqz.ZarrShardSet(dims, 0)
    buf = dev_bytes(4096)
    p = buf.data_ptr()
    bad = [
        dict(device_frames=0, frame_stride=16, device_out=p, out_capacity=64, device_segments=p),
        dict(device_frames=p, frame_stride=16, device_out=0, out_capacity=64, device_segments=p),
        dict(device_frames=p, frame_stride=16, device_out=p, out_capacity=64, device_segments=0),
        dict(device_frames=p, frame_stride=0, device_out=p, out_capacity=64, device_segments=p),
        dict(device_frames=p, frame_stride=16, device_out=p, out_capacity=63, device_segments=p),
        # sizes are uint32: a stride of 2^32 with a size table
        dict(device_frames=p, frame_stride=1 << 32, device_out=p, out_capacity=1 << 34,
             device_segments=p, device_frame_bytes=p),
        # 4 chunks x 2^29 pieces: a grid of 2^31 workgroups
        dict(device_frames=p, frame_stride=aqz.ZARR_SHARD_PACK_PIECE << 29, device_out=p,
             out_capacity=1 << 62, device_segments=p),
    ]
    for kw in bad:
        with pytest.raises(aqz.AqzError) as e:
            st.append_layer_device(**kw)
        assert e.value.status == 1, kw
    with pytest.raises(aqz.AqzError):
        st.tables_device(0, p)
    with pytest.raises(aqz.AqzError):
        st.tables_device(p, 0)
    # none of the refused calls counted as a layer
    st.append_layer_device(p, 16, p + 1024, 64, p + 2048)
    torch_cuda().cuda.synchronize()
    st.close()
