#!/usr/bin/env python3
"""Time reading blosc+LZ4 chunk frames back on the device.

  python tools/blosc_lz4_decode_bench.py [--reps 15] [--warmup 3] [--threads 16] [--out FILE]

The method of tools/blosc_lz4_bench.py: per workload and clevel (lz4, byte
shuffle, typesize 2, 256 chunks of 128 KiB made into frames on the device by
aqz_blosc_lz4_frames_device), in one process, the variants taking turns inside
every repeat, 3 warm-ups, the median of 15:

  decode     aqz_blosc_lz4_decompress_device: header parse, split decode,
             raw and memcpy copies, unfilter
  splits     the split decoder alone (aqz_debug_lz4_decode_blocks_device) on
             the frames' LZ4 splits, found once by a host walk of the frames
  unfilter   aqz_blosc_unfilter_device alone (byte unshuffle) on the filtered bytes
  unbitshuffle  the same call with the bit unshuffle, on the same bytes
  filter     the forward byte shuffle, aqz_blosc_filter_device, for comparison
  copy       a device-to-device copy of as many bytes (the yardstick of DESIGN
             §4.6).  32 MiB in and out stay inside the last-level cache: these
             four are cache-resident rates, comparable with each other only
  cblosc     blosc_decompress_ctx on `threads` host threads from
             host-resident frames, where the image has libblosc (a Python
             thread pool over ctypes calls: its overhead is in the figure)

Device variants are timed with HIP events on the stream they are queued on;
cblosc with the host clock.  Workloads: "smooth" and "tiles" as in
tools/blosc_lz4_bench.py, and "random" (every chunk a memcpy frame: no split
to decode).  One JSON line per (workload, clevel): ms (min, median, max) and
GB/s of decoded bytes at the median per variant, the frames' ratio, how many
splits are LZ4 streams, and whether the decoded bytes equal the input.
"""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]

from blosc_lz4_bench import N_CHUNKS, NB, TILE, pyramid_tiles, smooth  # noqa: E402


def lz4_splits(frames, sizes, stride):
    """(offset in `frames`, csize, offset in the decoded buffer, decoded size)
    of every split stored as an LZ4 stream."""
    out = []
    for k in range(N_CHUNKS):
        fr = frames[k * stride:k * stride + sizes[k]]
        flags, ts = int(fr[2]), int(fr[3])
        nbytes, bs, _ = struct.unpack_from("<III", fr, 4)
        if flags & 0x2:
            continue
        split = not flags & 0x10 and ts <= 16 and bs // ts >= 128
        nb = -(-nbytes // bs)
        starts = struct.unpack_from(f"<{nb}i", fr, 16)
        for b, p in enumerate(starts):
            bsize = min(bs, nbytes - b * bs)
            nsp = ts if split and bsize == bs else 1
            neb = bsize // nsp
            for j in range(nsp):
                (c,) = struct.unpack_from("<i", fr, p)
                if c != neb:
                    out.append((k * stride + p + 4, c, k * NB + b * bs + j * neb, neb))
                p += 4 + c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    import aqz_pkg
    import blosc_ref
    aqz = aqz_pkg.load()
    if not torch.cuda.is_available():
        sys.exit("blosc_lz4_decode_bench needs a GPU")
    torch.cuda.set_device(0)
    stride = NB + aqz.BLOSC_MAX_OVERHEAD
    workloads = {
        "smooth": torch.from_numpy(smooth(np.random.default_rng(5), N_CHUNKS, TILE, TILE)
                                   .view(np.uint8).reshape(-1)).to("cuda"),
        "tiles": pyramid_tiles(aqz, torch),
        "random": torch.from_numpy(np.random.default_rng(7).integers(
            0, 256, N_CHUNKS * NB, dtype=np.uint8)).to("cuda"),
    }
    torch.cuda.synchronize()
    ctx = aqz.BloscContext(0, args.threads)
    stream = torch.cuda.current_stream().cuda_stream
    have_blosc = blosc_ref.available()
    pool = ThreadPoolExecutor(args.threads) if have_blosc else None
    lines = []
    total = N_CHUNKS * NB
    for name, d in workloads.items():
        for clevel in (1, 5):
            d_frames = torch.zeros(N_CHUNKS * stride, dtype=torch.uint8, device="cuda")
            d_sizes = torch.zeros(N_CHUNKS, dtype=torch.int32, device="cuda")
            ctx.lz4_frames_device(clevel, aqz.SHUFFLE, 2, d.data_ptr(), NB, N_CHUNKS,
                                  d_frames.data_ptr(), stride, d_sizes.data_ptr(), stream)
            torch.cuda.synchronize()
            frames = d_frames.cpu().numpy()
            sizes = d_sizes.cpu().numpy()
            bs = aqz.blosc_blocksize(clevel, 2, NB, "lz4")
            splits = lz4_splits(frames, sizes, stride)
            d_dst = torch.empty(total, dtype=torch.uint8, device="cuda")
            d_filt = torch.empty(total, dtype=torch.uint8, device="cuda")
            d_tmp = torch.empty(total, dtype=torch.uint8, device="cuda")
            d_status = torch.empty(N_CHUNKS, dtype=torch.int32, device="cuda")
            aqz.blosc_filter_device(aqz.SHUFFLE, 2, bs, d.data_ptr(), NB, N_CHUNKS,
                                    d_filt.data_ptr(), stream)
            if splits:
                cols = list(zip(*splits))
                d_coff = torch.from_numpy(np.array(cols[0], np.uint64).view(np.int64)).to("cuda")
                d_csz = torch.from_numpy(np.array(cols[1], np.uint32).view(np.int32)).to("cuda")
                d_ooff = torch.from_numpy(np.array(cols[2], np.uint64).view(np.int64)).to("cuda")
                d_cap = torch.from_numpy(np.array(cols[3], np.uint32).view(np.int32)).to("cuda")
                d_res = torch.empty(len(splits), dtype=torch.int32, device="cuda")
            host_frames = [frames[k * stride:k * stride + sizes[k]].copy() for k in range(N_CHUNKS)]
            host_out = np.empty((N_CHUNKS, NB), np.uint8)

            def one(k):
                return blosc_ref.lib().blosc_decompress_ctx(host_frames[k].ctypes.data,
                                                            host_out[k].ctypes.data, NB, 1)

            def run(v):
                if v == "decode":
                    ctx.lz4_decompress_device(2, NB, d_frames.data_ptr(), stride,
                                              d_sizes.data_ptr(), N_CHUNKS, d_dst.data_ptr(), NB,
                                              d_status.data_ptr(), stream)
                elif v == "splits":
                    ctx.debug_lz4_decode_blocks_device(
                        d_frames.data_ptr(), d_coff.data_ptr(), d_csz.data_ptr(),
                        d_tmp.data_ptr(), d_ooff.data_ptr(), d_cap.data_ptr(), d_res.data_ptr(),
                        len(splits), stream)
                elif v == "unfilter":
                    aqz.blosc_unfilter_device(aqz.SHUFFLE, 2, bs, d_filt.data_ptr(), NB, N_CHUNKS,
                                              d_tmp.data_ptr(), stream)
                elif v == "unbitshuffle":
                    aqz.blosc_unfilter_device(aqz.BITSHUFFLE, 2, bs, d_filt.data_ptr(), NB,
                                              N_CHUNKS, d_tmp.data_ptr(), stream)
                elif v == "filter":
                    aqz.blosc_filter_device(aqz.SHUFFLE, 2, bs, d_dst.data_ptr(), NB, N_CHUNKS,
                                            d_tmp.data_ptr(), stream)
                elif v == "copy":
                    d_tmp.copy_(d_filt)
                else:
                    assert all(r == NB for r in pool.map(one, range(N_CHUNKS)))

            variants = ["decode"] + (["splits"] if splits else []) + \
                ["unfilter", "unbitshuffle", "filter", "copy"] + (["cblosc"] if have_blosc else [])
            times = {v: [] for v in variants}
            for rep in range(args.warmup + args.reps):
                for v in variants:  # taking turns, so drift hits all alike
                    if v == "cblosc":
                        t0 = time.perf_counter()
                        run(v)
                        ms = (time.perf_counter() - t0) * 1e3
                    else:
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record()
                        run(v)
                        e1.record()
                        e1.synchronize()
                        ms = e0.elapsed_time(e1)
                    if rep >= args.warmup:
                        times[v].append(ms)
            torch.cuda.synchronize()
            ok = bool((d_status == 0).all()) and torch.equal(d_dst, d)
            if have_blosc:
                ok = ok and np.array_equal(host_out.reshape(-1), d.cpu().numpy())
            if splits:
                ok = ok and bool((d_res == d_cap).all())
            lz4_bytes = int(sum(s[3] for s in splits))
            rec = {"workload": name, "chunks": N_CHUNKS, "chunk_bytes": NB,
                   "codec": f"lz4 clevel {clevel} shuffle", "threads": args.threads,
                   "reps": args.reps, "warmup": args.warmup, "blocksize": bs,
                   "ratio": round(int(sizes.sum()) / total, 4),
                   "lz4_splits": len(splits), "lz4_split_bytes": lz4_bytes,
                   "decoded_equals_input": ok}
            for v in variants:
                med = statistics.median(times[v])
                nbytes = lz4_bytes if v == "splits" else total
                rec[v] = {"ms_min": round(min(times[v]), 4), "ms_median": round(med, 4),
                          "ms_max": round(max(times[v]), 4),
                          "GBps_out_median": round(nbytes / med / 1e6, 3)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
