#!/usr/bin/env python3
"""Time the Zarr v3 shard pack step and its host delivery.

  python tools/zarr_shard_bench.py [--reps 15] [--warmup 3] [--out FILE]

Workloads, each over 1 and 16 shards:

  smooth, random  256 chunks of 128 KiB u16 through aqz_blosc_lz4_frames_device
                  (clevel 1, byte shuffle): §12.9's compressible and
                  incompressible inputs, frames of different sizes
  raw             64 uncompressed chunks of 2 MiB (no size table)

Pack variants, on the placement one aqz_zarr_shard_set_append_layer_device
left, the variants taking turns inside every repeat, timed with events around
a batch of rotated buffer sets that together read at least 1 GiB (so nothing
is served from a cache):

  pack_<piece>[_nt]  the product's pack kernel at that piece, plain or
                     nontemporal loads and stores
  legacy             pack_frames_kernel (one workgroup per frame) on the same
                     offsets
  memcpy             hipMemcpyDtoDAsync of the same total bytes: the ceiling

End to end (smooth, random; host clock, each call ends synchronised):
aqz_blosc_lz4_frames_device + aqz_zarr_shard_set_append_layer against
aqz_blosc_lz4_compress_device, with the bytes each copied device-to-host.

One JSON line per (workload, shards): per variant ms per batch (min, median,
and the spread max - min over the repeats) and GB/s of bytes moved (read +
written) at the median.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from blosc_lz4_bench import smooth  # noqa: E402

PIECES = (16 << 10, 64 << 10, 256 << 10)
GIB = 1 << 30


def shard_dims(aqz, n_shards, n_chunks):
    return [(aqz.TIME, 0, 1, 1), (aqz.SPACE, 1, 1, 1),
            (aqz.SPACE, n_chunks, 1, n_chunks // n_shards)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    import aqz_pkg
    aqz = aqz_pkg.load()
    if not torch.cuda.is_available():
        sys.exit("zarr_shard_bench needs a GPU")
    torch.cuda.set_device(0)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.c_void_p]

    def u8(n, fill=None):
        if fill is None:
            return torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda")
        return torch.full((max(int(n), 1),), fill, dtype=torch.uint8, device="cuda")

    ctx = aqz.BloscContext(0, 16)
    NB = 256 * 256 * 2
    lz4_stride = NB + aqz.BLOSC_MAX_OVERHEAD
    raw = {
        "smooth": torch.from_numpy(smooth(np.random.default_rng(5), 256, 256, 256)
                                   .view(np.uint8).reshape(-1)).to("cuda"),
        "random": torch.from_numpy(np.random.default_rng(7).integers(
            0, 256, 256 * NB, dtype=np.uint8)).to("cuda"),
    }
    lines = []
    for name in ("smooth", "random", "raw"):
        if name == "raw":
            n, stride = 64, 2 << 20
            frames0 = torch.from_numpy(np.random.default_rng(8).integers(
                0, 256, n * stride, dtype=np.uint8)).to("cuda")
            sizes_h = np.full(n, stride, np.uint32)
            d_sizes = torch.from_numpy(sizes_h.view(np.uint8)).to("cuda")
            size_ptr = 0  # the product path takes no size table here
        else:
            n, stride = 256, lz4_stride
            frames0 = u8(n * stride, 0)
            d_sizes = u8(4 * n, 0)
            ctx.lz4_frames_device(1, aqz.SHUFFLE, 2, raw[name].data_ptr(), NB, n,
                                  frames0.data_ptr(), stride, d_sizes.data_ptr())
            torch.cuda.synchronize()
            sizes_h = d_sizes.cpu().numpy().view(np.uint32).copy()
            size_ptr = d_sizes.data_ptr()
        total = int(sizes_h.sum())
        rot = max(2, -(-GIB // total))
        srcs = [frames0] + [frames0.clone() for _ in range(rot - 1)]
        outs = [u8(n * stride, 0) for _ in range(rot)]
        flat_src, flat_dst = u8(total, 1), u8(total, 0)
        flats = [(flat_src.clone(), flat_dst.clone()) for _ in range(rot)]
        for n_shards in (1, 16):
            dims = shard_dims(aqz, n_shards, n)
            st = aqz.ZarrShardSet(dims, 0)
            seg = u8(8 * st.segment_words, 0)
            st.append_layer_device(frames0.data_ptr(), stride, outs[0].data_ptr(), n * stride,
                                   seg.data_ptr(), size_ptr)
            torch.cuda.synchronize()
            want = outs[0][:total].clone()
            rows = seg.cpu().numpy().view(np.uint64)
            assert int(rows[-1]) == total
            # the same placement for pack_frames_kernel: ascending internal
            # index within a shard, shards end to end
            _, shard_of, internal_of = aqz.zarr_shard_layout(dims)
            order = np.lexsort((internal_of, shard_of))
            offs = np.zeros(n, np.uint64)
            offs[order] = np.concatenate(([0], np.cumsum(sizes_h[order].astype(np.uint64))[:-1]))
            d_offs = torch.from_numpy(offs.view(np.uint8)).to("cuda")

            def pack(piece, policy):
                def run(r):
                    st.debug_pack_device(srcs[r].data_ptr(), stride, outs[r].data_ptr(),
                                         seg.data_ptr(), piece, policy,
                                         device_frame_bytes=size_ptr)
                return run

            def legacy(r):
                st.debug_pack_device(srcs[r].data_ptr(), stride, outs[r].data_ptr(), 0, 0, 0,
                                     device_frame_bytes=d_sizes.data_ptr(),
                                     device_offsets=d_offs.data_ptr())

            def memcpy(r):
                hip.hipMemcpyDtoDAsync(flats[r][1].data_ptr(), flats[r][0].data_ptr(), total, None)

            variants = {}
            for p in PIECES:
                variants[f"pack_{p >> 10}k"] = pack(p, 0)
                variants[f"pack_{p >> 10}k_nt"] = pack(p, 1)
            variants["legacy"] = legacy
            variants["memcpy"] = memcpy
            same = True
            for v, run in variants.items():
                if v == "memcpy":
                    continue
                outs[1].zero_()
                run(1)
                torch.cuda.synchronize()
                same = same and bool(torch.equal(outs[1][:total], want))
            times = {v: [] for v in variants}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for rep in range(args.warmup + args.reps):
                for v, run in variants.items():  # taking turns, so drift hits all alike
                    e0.record()
                    for r in range(rot):
                        run(r)
                    e1.record()
                    e1.synchronize()
                    if rep >= args.warmup:
                        times[v].append(e0.elapsed_time(e1))
            rec = {"workload": name, "shards": n_shards, "chunks": n, "frame_stride": stride,
                   "packed_bytes": total, "rotations": rot, "batch_bytes_read": total * rot,
                   "reps": args.reps, "warmup": args.warmup, "bytes_identical": same}
            for v in variants:
                med = statistics.median(times[v])
                rec[v] = {"ms_min": round(min(times[v]), 4), "ms_median": round(med, 4),
                          "ms_spread": round(max(times[v]) - min(times[v]), 4),
                          "GBps_moved_median": round(2 * total * rot / med / 1e6, 1)}
            if name != "raw":
                host_new = np.empty(n * stride, np.uint8)
                host_old = np.empty(n * stride, np.uint8)

                def new():
                    st.begin()
                    ctx.lz4_frames_device(1, aqz.SHUFFLE, 2, raw[name].data_ptr(), NB, n,
                                          srcs[1].data_ptr(), stride, d_sizes.data_ptr())
                    return st.append_layer(srcs[1].data_ptr(), stride, d_sizes.data_ptr(),
                                           host_out=host_new)

                def old():
                    return ctx.lz4_compress_device(1, aqz.SHUFFLE, 2, raw[name].data_ptr(), NB, n,
                                                   host_dst=host_old, dst_stride=stride)

                e2e = {"shards_append_layer": [], "lz4_compress_device": []}
                for rep in range(args.warmup + args.reps):
                    for v, fn in (("shards_append_layer", new), ("lz4_compress_device", old)):
                        t0 = time.perf_counter()
                        fn()
                        dt = time.perf_counter() - t0
                        if rep >= args.warmup:
                            e2e[v].append(dt * 1e3)
                rec["end_to_end"] = {
                    v: {"ms_min": round(min(t), 3), "ms_median": round(statistics.median(t), 3),
                        "ms_spread": round(max(t) - min(t), 3)} for v, t in e2e.items()}
                rec["end_to_end"]["shards_append_layer"]["d2h_bytes"] = int(st.d2h_bytes())
                rec["end_to_end"]["lz4_compress_device"]["d2h_bytes"] = int(ctx.d2h_bytes())
            st.close()
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
