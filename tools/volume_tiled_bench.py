#!/usr/bin/env python3
"""Time the fused volume kernel writing chunk tiles.

  python tools/volume_tiled_bench.py [--reps 15] [--warmup 3] [--volumes 4] [--out FILE]

Workload: BASELINE config V (1024 x 1024 x 256 u16, 3 levels halving X, Y and
Z), `--volumes` volumes per launch, Mean and Decimate, tiles 64x64 and 256x256.
Variants, taking turns inside every repeat, one process and one stream, timed with events
around a batch of rotated buffer sets that together read at least 1 GiB (so
nothing is served from a cache):

  volume_tiled   aqz_ds_run_device_volume_tiled, with zero-scan flags
  row_major      aqz_ds_run_device_batch alone (kind 2): a floor for context
  row_then_tile  row_major, then aqz_tile_frame_device on every emitted plane:
                 the only route to tiles before the fused call

One JSON line per (method, tile): per variant ms per launch (min, median, and
the spread max - min over the repeats), whether volume_tiled's median lies
below row_then_tile's by more than the larger spread, and whether the two
produced the same tiles.
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

GIB = 1 << 30
W = H = 1024
PLANES = 256
LEVELS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--volumes", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    import aqz_pkg
    aqz = aqz_pkg.load()
    if not torch.cuda.is_available():
        sys.exit("volume_tiled_bench needs a GPU")
    torch.cuda.set_device(0)
    L = aqz.lib()
    # one stream for every call and both events: a NULL stream would put the
    # batch calls on their handles' own streams, outside the events
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    st = ctypes.c_void_p(stream.cuda_stream)
    dtype, bpp = np.uint16, 2
    code = aqz.dtype_code(np.dtype(dtype))
    geo = [(W >> l, H >> l, PLANES >> l) for l in range(LEVELS)]
    n = PLANES * args.volumes
    in_bytes = n * W * H * bpp

    def u8(nbytes):
        return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")

    lines = []
    for method in ("mean", "decimate"):
        # Decimate reads every other row of every other plane: a quarter
        read = in_bytes if method == "mean" else in_bytes // 4
        rot = max(2, -(-GIB // read))
        g = torch.Generator(device="cuda").manual_seed(3)
        ins = [torch.randint(0, 256, (in_bytes,), dtype=torch.uint8, device="cuda", generator=g)
               for _ in range(rot)]
        rows = [[None] + [u8((n >> l) * (W >> l) * (H >> l) * bpp) for l in range(1, LEVELS)]
                for _ in range(rot)]
        for tile in (64, 256):
            nt = [None] + [((H >> l) // tile) * ((W >> l) // tile) for l in range(1, LEVELS)]
            tiled = [[None] + [u8((n >> l) * (W >> l) * (H >> l) * bpp) for l in range(1, LEVELS)]
                     for _ in range(rot)]
            flags = [[None] + [u8((n >> l) * nt[l]) for l in range(1, LEVELS)] for _ in range(rot)]
            # the tile pass's own outputs and its u32 flags
            tiled_c = [None] + [u8((n >> l) * (W >> l) * (H >> l) * bpp) for l in range(1, LEVELS)]
            flags_c = [None] + [u8(4 * (n >> l) * nt[l]) for l in range(1, LEVELS)]
            ds = {v: aqz.Downsampler(geo, dtype, aqz.METHODS[method], device=0)
                  for v in ("volume_tiled", "row_major")}
            tiles = [None] + [(tile, tile)] * (LEVELS - 1)
            tr = (ctypes.c_uint32 * LEVELS)(0, tile, tile)
            counts = (ctypes.c_uint32 * LEVELS)()

            def ptrs(bufs):
                return (ctypes.c_void_p * LEVELS)(*[b.data_ptr() if b is not None else 0
                                                    for b in bufs])

            a_args = [(ds["volume_tiled"]._h, ins[r].data_ptr(), n, tr, tr, ptrs(tiled[r]),
                       ptrs(flags[r]), counts, st) for r in range(rot)]
            b_args = [(ds["row_major"]._h, ins[r].data_ptr(), n, ptrs(rows[r]), counts, st)
                      for r in range(rot)]
            # one aqz_tile_frame_device call per emitted plane, arguments prepared
            c_args = []
            for r in range(rot):
                calls = []
                for l in range(1, LEVELS):
                    w, h = W >> l, H >> l
                    for k in range(n >> l):
                        calls.append((code, rows[r][l].data_ptr() + k * w * h * bpp, w, h, tile,
                                      tile, tiled_c[l].data_ptr() + k * w * h * bpp,
                                      flags_c[l].data_ptr() + 4 * k * nt[l], st))
                c_args.append(calls)

            def volume_tiled(r):
                rc = L.aqz_ds_run_device_volume_tiled(*a_args[r])
                assert rc == 0, ds["volume_tiled"]._check(rc)

            def row_major(r):
                rc = L.aqz_ds_run_device_batch(*b_args[r])
                assert rc == 0, ds["row_major"]._check(rc)

            def row_then_tile(r):
                row_major(r)
                for c in c_args[r]:
                    rc = L.aqz_tile_frame_device(*c)
                    assert rc == 0, rc

            variants = {"volume_tiled": volume_tiled, "row_major": row_major,
                        "row_then_tile": row_then_tile}
            # same tiles from both routes, and the kinds the handles report
            volume_tiled(0)
            row_then_tile(0)
            torch.cuda.synchronize()
            same = all(bool(torch.equal(tiled[0][l], tiled_c[l])) for l in range(1, LEVELS))
            kinds = [ds["volume_tiled"].last_batch_kind(), ds["row_major"].last_batch_kind()]
            assert kinds == [5, 2], kinds
            times = {v: [] for v in variants}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for rep in range(args.warmup + args.reps):
                for v, run in variants.items():  # taking turns, so drift hits all alike
                    e0.record(stream)
                    for r in range(rot):
                        run(r)
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= args.warmup:
                        times[v].append(e0.elapsed_time(e1) / rot)
            out_bytes = sum((n >> l) * (W >> l) * (H >> l) * bpp for l in range(1, LEVELS))
            rec = {"config": "V", "dtype": "uint16", "method": method, "tile": tile,
                   "volumes": args.volumes, "planes": n, "rotations": rot,
                   "bytes_read_per_launch": read, "bytes_written_per_launch": out_bytes,
                   "tile_launches_per_call": len(c_args[0]), "reps": args.reps,
                   "warmup": args.warmup, "tiles_identical": same}
            for v in variants:
                med = statistics.median(times[v])
                rec[v] = {"ms_min": round(min(times[v]), 4), "ms_median": round(med, 4),
                          "ms_spread": round(max(times[v]) - min(times[v]), 4)}
            spread = max(rec["volume_tiled"]["ms_spread"], rec["row_then_tile"]["ms_spread"])
            rec["larger_spread_ms"] = spread
            rec["tiled_below_row_then_tile_by_more_than_spread"] = bool(
                rec["volume_tiled"]["ms_median"] < rec["row_then_tile"]["ms_median"] - spread)
            rec["tiled_over_row_major"] = round(
                rec["volume_tiled"]["ms_median"] / rec["row_major"]["ms_median"], 3)
            for d in ds.values():
                d.close()
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del tiled, flags, tiled_c, flags_c
        del ins, rows
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
