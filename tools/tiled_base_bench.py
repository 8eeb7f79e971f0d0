#!/usr/bin/env python3
"""Time the fused tiled cascade writing level 0's chunk tiles too.

  python tools/tiled_base_bench.py [--reps 15] [--warmup 3] [--frames 64] [--out FILE]
                                   [--only NAME]

Workloads: 4096^2 u16 (Mean and Decimate), 3000^2 u16 (ragged tiles, Mean),
4096^2 f32 (Mean, 16 bytes a lane) and 3000^2 f32 (Mean, 32 bytes a lane), 5 levels, 256 x 256 tiles at every level, `--frames` frames
per batch.  Variants, taking turns inside every repeat, one process and one
stream, timed with events around a batch of rotated buffer sets that together
read at least 1 GiB (so nothing is served from a cache):

  base       aqz_ds_run_device_batch_tiled_base, with zero-scan flags
  tiled      aqz_ds_run_device_batch_tiled alone (levels >= 1): a floor
  tiled_then_tile
             tiled, then aqz_tile_frame_device_sliced on every frame: the only
             route to level 0's tiles before the fused call
  copy       a device-to-device copy of the batch: what moving level 0's bytes
             once costs, beside base - tiled

One JSON line per (workload, method): per variant ms per batch (min, median,
and the spread max - min over the repeats), whether base's median lies below
tiled_then_tile's by more than the larger spread, and whether the two produced
the same level-0 tiles.
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
LEVELS = 5
TILE = 256
WORKLOADS = [
    ("u16_4096_mean", np.uint16, 4096, "mean"),
    ("u16_4096_decimate", np.uint16, 4096, "decimate"),
    ("u16_3000_mean", np.uint16, 3000, "mean"),
    ("f32_4096_mean", np.float32, 4096, "mean"),
    ("f32_3000_mean", np.float32, 3000, "mean"),  # rows not whole KiB: 32 bytes a lane
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
        sys.exit("tiled_base_bench needs a GPU")
    torch.cuda.set_device(0)
    L = aqz.lib()
    # one stream for every call and both events: a NULL stream would put the
    # batch calls on their handles' own streams, outside the events
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    st = ctypes.c_void_p(stream.cuda_stream)
    n = args.frames

    def u8(nbytes):
        return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")

    lines = []
    for name, dtype, side, method in WORKLOADS:
        if args.only and args.only != name:
            continue
        bpp = np.dtype(dtype).itemsize
        code = aqz.dtype_code(np.dtype(dtype))
        geo = [(side, side, 1)]
        for _ in range(1, LEVELS):
            geo.append(((geo[-1][0] + 1) // 2, (geo[-1][1] + 1) // 2, 1))
        nt = [(-(-h // TILE)) * (-(-w // TILE)) for w, h, _ in geo]
        tbytes = [n * t * TILE * TILE * bpp for t in nt]
        in_bytes = n * side * side * bpp
        rot = max(2, -(-GIB // in_bytes))
        g = torch.Generator(device="cuda").manual_seed(3)
        # bytes below 128: finite floats, no NaN for the f32 Mean to carry around
        ins = [torch.randint(0, 128, (in_bytes,), dtype=torch.uint8, device="cuda", generator=g)
               for _ in range(rot)]
        ds = {v: aqz.Downsampler(geo, dtype, aqz.METHODS[method], device=0)
              for v in ("base", "tiled")}
        slots = [ds["base"].tiled_base_flag_slots(TILE, TILE)] + \
            [ds["base"].tiled_flag_slots(l, TILE, TILE) for l in range(1, LEVELS)]
        slices = L.aqz_tile_slices(TILE, TILE)
        outs_a = [[u8(tbytes[l]) for l in range(LEVELS)] for _ in range(rot)]
        flags_a = [[u8(n * nt[l] * slots[l]) for l in range(LEVELS)] for _ in range(rot)]
        outs_b = [[None] + [u8(tbytes[l]) for l in range(1, LEVELS)] for _ in range(rot)]
        flags_b = [[None] + [u8(n * nt[l] * slots[l]) for l in range(1, LEVELS)]
                   for _ in range(rot)]
        base_c = [u8(tbytes[0]) for _ in range(rot)]  # the tile pass's own outputs
        flags_c = u8(n * nt[0] * slices)
        copy_dst = u8(in_bytes)
        tr = (ctypes.c_uint32 * LEVELS)(*([TILE] * LEVELS))
        counts = (ctypes.c_uint32 * LEVELS)()

        def ptrs(bufs):
            return (ctypes.c_void_p * LEVELS)(*[b.data_ptr() if b is not None else 0
                                                for b in bufs])

        a_args = [(ds["base"]._h, ins[r].data_ptr(), n, tr, tr, ptrs(outs_a[r]),
                   ptrs(flags_a[r]), counts, st) for r in range(rot)]
        b_args = [(ds["tiled"]._h, ins[r].data_ptr(), n, tr, tr, ptrs(outs_b[r]),
                   ptrs(flags_b[r]), counts, st) for r in range(rot)]
        frame = side * side * bpp
        tframe = nt[0] * TILE * TILE * bpp
        c_args = [[(code, ins[r].data_ptr() + k * frame, side, side, TILE, TILE,
                    base_c[r].data_ptr() + k * tframe, flags_c.data_ptr() + k * nt[0] * slices, st)
                   for k in range(n)] for r in range(rot)]

        def base(r):
            rc = L.aqz_ds_run_device_batch_tiled_base(*a_args[r])
            assert rc == 0, ds["base"]._check(rc)

        def tiled(r):
            rc = L.aqz_ds_run_device_batch_tiled(*b_args[r])
            assert rc == 0, ds["tiled"]._check(rc)

        def tiled_then_tile(r):
            tiled(r)
            for c in c_args[r]:
                rc = L.aqz_tile_frame_device_sliced(*c)
                assert rc == 0, rc

        def copy(r):
            copy_dst.copy_(ins[r], non_blocking=True)

        variants = {"base": base, "tiled": tiled, "tiled_then_tile": tiled_then_tile,
                    "copy": copy}
        # same bytes from both routes, and the kinds the handles report
        base(0)
        tiled_then_tile(0)
        torch.cuda.synchronize()
        same = bool(torch.equal(outs_a[0][0], base_c[0])) and \
            all(bool(torch.equal(outs_a[0][l], outs_b[0][l])) and
                bool(torch.equal(flags_a[0][l], flags_b[0][l])) for l in range(1, LEVELS))
        kinds = [ds["base"].last_batch_kind(), ds["tiled"].last_batch_kind()]
        assert kinds == [6, 4], kinds
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
        rec = {"workload": name, "dtype": np.dtype(dtype).name, "side": side, "method": method,
               "tile": TILE, "levels": LEVELS, "frames": n, "rotations": rot,
               "input_bytes": in_bytes, "base_tile_bytes": tbytes[0],
               "level_tile_bytes": sum(tbytes[1:]), "base_flag_slots": slots[0],
               "tile_launches_per_batch": n, "reps": args.reps, "warmup": args.warmup,
               "bytes_identical": same, "version": L.aqz_version().decode()}
        for v in variants:
            med = statistics.median(times[v])
            rec[v] = {"ms_min": round(min(times[v]), 4), "ms_median": round(med, 4),
                      "ms_spread": round(max(times[v]) - min(times[v]), 4)}
        spread = max(rec["base"]["ms_spread"], rec["tiled_then_tile"]["ms_spread"])
        rec["larger_spread_ms"] = spread
        rec["base_below_tiled_then_tile_by_more_than_spread"] = bool(
            rec["base"]["ms_median"] < rec["tiled_then_tile"]["ms_median"] - spread)
        rec["base_minus_tiled_ms"] = round(rec["base"]["ms_median"] - rec["tiled"]["ms_median"], 4)
        for d in ds.values():
            d.close()
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del ins, outs_a, flags_a, outs_b, flags_b, base_c, flags_c, copy_dst
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
