#!/usr/bin/env python3
"""Time the chunk -> frame gather.

  python tools/chunk_gather_bench.py [--reps 15] [--warmup 3] [--frames 64] [--out FILE]
                                     [--only NAME]

Workloads: batches of `--frames` frames from 256 x 256 tiles, one frame a
chunk: 4096^2 u16, 4096^2 f32, 3000^2 u16 (rows are 16-byte multiples) and
3001^2 u16 (they are not: every row end straddles a vector); and 4096^2 u8
from 256 x 8 tiles, whose rows no vector fits (the element form).  Every timed
launch reads at least 1 GiB, so nothing is served from a cache.
Variants, taking turns inside every repeat, one process and one stream, timed
with events:

  gather        aqz_chunk_gather_frames_device, identity slots
  gather_table  the same through a permuted slot table
  copy          hipMemcpyDtoDAsync of the frames' bytes
  forward       aqz_tile_frame_device_sliced once per frame: the tiling the
                gather inverts (unchanged code)

One JSON line per workload: per variant ms per batch (min, median, spread
max - min over the repeats), GB/s of bytes read plus bytes written, the
gather's median as a fraction of the copy's and of the forward pass's, and
whether gather(forward(frames)) gave the frames back.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

TILE = 256
WORKLOADS = [
    ("u16_4096", np.uint16, 4096, TILE),
    ("f32_4096", np.float32, 4096, TILE),
    ("u16_3000", np.uint16, 3000, TILE),
    ("u16_3001", np.uint16, 3001, TILE),
    # not one of the 256 x 256 workloads: tile rows of 8 bytes, which no vector
    # fits, so that the element form has a figure too
    ("u8_4096_cols8", np.uint8, 4096, 8),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--only")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    import aqz_pkg
    aqz = aqz_pkg.load()
    if not torch.cuda.is_available():
        sys.exit("chunk_gather_bench needs a GPU")
    torch.cuda.set_device(0)
    L = aqz.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.c_void_p]
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    st = ctypes.c_void_p(stream.cuda_stream)
    n = args.frames

    lines = []
    for name, dtype, side, tcols in WORKLOADS:
        if args.only and args.only != name:
            continue
        bpp = np.dtype(dtype).itemsize
        code = aqz.dtype_code(np.dtype(dtype))
        frame = side * side * bpp
        nt = -(-side // TILE) * -(-side // tcols)
        tile_bytes = TILE * tcols * bpp
        assert n * frame >= 1 << 30, "a timed launch must read at least 1 GiB"
        g = torch.Generator(device="cuda").manual_seed(14)
        frames = torch.randint(0, 256, (n * frame,), dtype=torch.uint8, device="cuda", generator=g)
        tiles = torch.empty(n * nt * tile_bytes, dtype=torch.uint8, device="cuda")
        shuffled = torch.empty_like(tiles)
        back = torch.empty_like(frames)
        copy_dst = torch.empty_like(frames)
        slices = L.aqz_tile_slices(TILE, tcols)
        flags = torch.empty(n * nt * slices, dtype=torch.uint8, device="cuda")
        base = (np.arange(n, dtype=np.uint32) * nt).astype(np.uint32)
        internal = np.zeros(n, np.uint64)
        perm = np.random.default_rng(14).permutation(n * nt).astype(np.uint32)
        d_perm = torch.from_numpy(perm.view(np.int32)).to("cuda")
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        f_args = [(code, frames.data_ptr() + k * frame, side, side, TILE, tcols,
                   tiles.data_ptr() + k * nt * tile_bytes, flags.data_ptr() + k * nt * slices, st)
                  for k in range(n)]

        def gather_args(src, table):
            return (code, side, side, TILE, tcols, src.data_ptr(), tile_bytes, n * nt,
                    table.data_ptr() if table is not None else None, n * nt, base.ctypes.data,
                    internal.ctypes.data, n, back.data_ptr(), frame, d_bad.data_ptr(), st)

        g_args, t_args = gather_args(tiles, None), gather_args(shuffled, d_perm)

        def forward():
            for c in f_args:
                rc = L.aqz_tile_frame_device_sliced(*c)
                assert rc == 0, rc

        def gather():
            rc = L.aqz_chunk_gather_frames_device(*g_args)
            assert rc == 0, L.aqz_last_error()

        def gather_table():
            rc = L.aqz_chunk_gather_frames_device(*t_args)
            assert rc == 0, L.aqz_last_error()

        def copy():
            rc = hip.hipMemcpyDtoDAsync(copy_dst.data_ptr(), frames.data_ptr(), n * frame, st)
            assert rc == 0, rc

        # the round trip, through both tables
        forward()
        shuffled.view(n * nt, tile_bytes)[d_perm.to(torch.int64) & 0xFFFFFFFF] = \
            tiles.view(n * nt, tile_bytes)
        same = []
        for run in (gather, gather_table):
            back.fill_(0x5A)
            run()
            torch.cuda.synchronize()
            same.append(bool(torch.equal(back, frames)))
        assert int(d_bad.cpu()[0]) == 0

        variants = {"gather": gather, "gather_table": gather_table, "copy": copy,
                    "forward": forward}
        times = {v: [] for v in variants}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rep in range(args.warmup + args.reps):
            for v, run in variants.items():  # taking turns, so drift hits all alike
                e0.record(stream)
                run()
                e1.record(stream)
                e1.synchronize()
                if rep >= args.warmup:
                    times[v].append(e0.elapsed_time(e1))
        moved = {"gather": 2 * n * frame, "gather_table": 2 * n * frame, "copy": 2 * n * frame,
                 "forward": n * frame + n * nt * tile_bytes}
        rec = {"workload": name, "dtype": np.dtype(dtype).name, "side": side, "tile": [TILE, tcols],
               "frames": n, "frame_bytes": n * frame, "tile_bytes": n * nt * tile_bytes,
               "row_bytes": side * bpp, "form": "vec" if tcols * bpp >= 16 else "elem",
               "frames_per_launch": aqz.CHUNK_GATHER_FRAMES,
               "reps": args.reps, "warmup": args.warmup, "frames_came_back": same,
               "version": L.aqz_version().decode()}
        for v in variants:
            med = statistics.median(times[v])
            rec[v] = {"ms_min": round(min(times[v]), 4), "ms_median": round(med, 4),
                      "ms_max": round(max(times[v]), 4),
                      "ms_spread": round(max(times[v]) - min(times[v]), 4),
                      "gb_per_s": round(moved[v] / med / 1e6, 1)}
        for v in ("gather", "gather_table"):
            rec[f"{v}_over_copy"] = round(rec[v]["ms_median"] / rec["copy"]["ms_median"], 3)
            rec[f"{v}_over_forward"] = round(rec[v]["ms_median"] / rec["forward"]["ms_median"], 3)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del frames, tiles, shuffled, back, copy_dst, flags
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
