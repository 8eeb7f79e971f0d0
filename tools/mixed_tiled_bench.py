#!/usr/bin/env python3
"""Time aqz_ds_run_device_mixed_tiled against the two-pass way to chunk tiles
(DESIGN.md §12.16).

  python tools/mixed_tiled_bench.py [--reps 15] [--warmup 3] [--out FILE]

Workloads A, B and C of tools/mixed_batch_bench.py (u16, Mean and Decimate),
256 x 256 tiles at every level.  Routes, taking turns inside every repeat, one
process and one stream, timed with events around a batch of rotated buffer
sets that together read at least 1 GiB:
  tiled      aqz_ds_run_device_mixed_tiled (aqz_ds_last_batch_kind 8)
  two_pass   aqz_ds_run_device_batch (kind 7) into row-major buffers, then one
             aqz_tile_frame_device_sliced per emitted plane per level: the way
             to chunk tiles before the call existed
  row_major  kind 7 alone: the floor (no tiles are made)

The tiles of `tiled` and `two_pass` are compared on the device before timing,
and `row_major`'s levels are those `two_pass` tiles.  One JSON line per
(workload, method): per route ms per batch (min, median, max, spread = max -
min over the repeats), tiled / two_pass and tiled / row_major with the larger
spread of each pair, and whether tiled's median lies below two_pass's by more
than that spread.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from mixed_batch_bench import BPP, GIB, WORKLOADS, traffic  # noqa: E402

TILE = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default="A,B,C")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    import aqz_pkg
    aqz = aqz_pkg.load()
    if not torch.cuda.is_available():
        sys.exit("mixed_tiled_bench needs a GPU")
    torch.cuda.set_device(0)
    L = aqz.lib()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    st = ctypes.c_void_p(stream.cuda_stream)
    slices = aqz.tile_slices(TILE, TILE)

    def u8(nbytes):
        return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")

    lines = []
    for wl in args.workloads.split(","):
        geo, stacks = WORKLOADS[wl]
        nl = len(geo)
        n = geo[0][2] * stacks
        in_bytes = n * geo[0][0] * geo[0][1] * BPP
        frames = [n]
        for l in range(1, nl):
            frames.append(frames[-1] >> (geo[l][2] < geo[l - 1][2]))
        nt = [0] + [(-(-geo[l][1] // TILE)) * (-(-geo[l][0] // TILE)) for l in range(1, nl)]
        tiled_bytes = [0] + [frames[l] * nt[l] * TILE * TILE * BPP for l in range(1, nl)]
        for method in ("mean", "decimate"):
            read, written = traffic(geo, n, method == "decimate")
            rot = max(2, -(-GIB // read))
            g = torch.Generator(device="cuda").manual_seed(3)
            ins = [torch.randint(0, 256, (in_bytes,), dtype=torch.uint8, device="cuda",
                                 generator=g) for _ in range(rot)]
            ds = aqz.Downsampler(geo, np.uint16, aqz.METHODS[method], device=0)
            slots = [0] + [ds.mixed_flag_slots(l, TILE, TILE) for l in range(1, nl)]
            rows = [[None] + [u8(frames[l] * geo[l][0] * geo[l][1] * BPP) for l in range(1, nl)]
                    for _ in range(rot)]
            t_new = [[None] + [u8(tiled_bytes[l]) for l in range(1, nl)] for _ in range(rot)]
            f_new = [[None] + [u8(frames[l] * nt[l] * slots[l]) for l in range(1, nl)]
                     for _ in range(rot)]
            t_two = [[None] + [u8(tiled_bytes[l]) for l in range(1, nl)] for _ in range(rot)]
            f_two = [[None] + [u8(frames[l] * nt[l] * slices) for l in range(1, nl)]
                     for _ in range(rot)]
            counts = (ctypes.c_uint32 * nl)()

            def ptrs(bufs):
                return (ctypes.c_void_p * nl)(*[b.data_ptr() if b is not None else 0
                                                for b in bufs])

            tr = (ctypes.c_uint32 * nl)(*([0] + [TILE] * (nl - 1)))
            call_rows = [(ds._h, ins[r].data_ptr(), n, ptrs(rows[r]), counts, st)
                         for r in range(rot)]
            call_new = [(ds._h, ins[r].data_ptr(), n, tr, tr, ptrs(t_new[r]), ptrs(f_new[r]),
                         counts, st) for r in range(rot)]
            code = aqz.dtype_code(np.uint16)
            # the per-plane tiling calls of two_pass, arguments built once
            call_tile = []
            for r in range(rot):
                c = []
                for l in range(1, nl):
                    w, h, _ = geo[l]
                    fb, tb, sb = w * h * BPP, nt[l] * TILE * TILE * BPP, nt[l] * slices
                    for k in range(frames[l]):
                        c.append((code, rows[r][l].data_ptr() + k * fb, w, h, TILE, TILE,
                                  t_two[r][l].data_ptr() + k * tb,
                                  f_two[r][l].data_ptr() + k * sb, st))
                call_tile.append(c)

            def tiled(r):
                rc = L.aqz_ds_run_device_mixed_tiled(*call_new[r])
                assert rc == 0, ds._check(rc)

            def row_major(r):
                rc = L.aqz_ds_run_device_batch(*call_rows[r])
                assert rc == 0, ds._check(rc)

            def two_pass(r):
                row_major(r)
                for c in call_tile[r]:
                    rc = L.aqz_tile_frame_device_sliced(*c)
                    assert rc == 0, rc

            variants = {"tiled": tiled, "two_pass": two_pass, "row_major": row_major}
            tiled(0)
            kinds = [ds.last_batch_kind()]
            two_pass(0)
            kinds.append(ds.last_batch_kind())
            torch.cuda.synchronize()
            assert kinds == [8, 7], kinds
            same = all(bool(torch.equal(t_new[0][l], t_two[0][l])) for l in range(1, nl))
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
            rec = {"workload": wl, "geometry": geo, "stacks": stacks, "dtype": "uint16",
                   "method": method, "frames": n, "tile": [TILE, TILE], "rotations": rot,
                   "bytes_read_per_batch": read, "bytes_written_row_major": written,
                   "bytes_written_tiled": sum(tiled_bytes), "reps": args.reps,
                   "warmup": args.warmup, "tile_launches_two_pass": len(call_tile[0]),
                   "tiles_identical": same}
            for v in variants:
                med = statistics.median(times[v])
                rec[v] = {"ms_min": round(min(times[v]), 4), "ms_median": round(med, 4),
                          "ms_max": round(max(times[v]), 4),
                          "ms_spread": round(max(times[v]) - min(times[v]), 4)}
            for other in ("two_pass", "row_major"):
                spread = max(rec["tiled"]["ms_spread"], rec[other]["ms_spread"])
                rec[f"tiled_over_{other}"] = round(
                    rec["tiled"]["ms_median"] / rec[other]["ms_median"], 3)
                rec[f"larger_spread_ms_{other}"] = spread
            rec["tiled_below_two_pass_by_more_than_spread"] = bool(
                rec["tiled"]["ms_median"] <
                rec["two_pass"]["ms_median"] - rec["larger_spread_ms_two_pass"])
            ds.close()
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del ins, rows, t_new, f_new, t_two, f_two, call_tile
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
