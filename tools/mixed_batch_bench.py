#!/usr/bin/env python3
"""Time aqz_ds_run_device_batch on mixed 3-D pyramids.

  python tools/mixed_batch_bench.py [--reps 15] [--warmup 3] [--out FILE]

Workloads, u16, Mean and Decimate:
  A  2048^2 x 64 under 256 x 256 x 16 chunks: two XYZ levels, one XY level;
     4 stacks a batch
  B  512^2 x 1024 under 256 x 256 x 64 chunks: one XYZ level, three Z-only
     levels; 2 stacks
  C  Z only: 1024^2 x 256 paired down three times; 2 stacks
Variants, taking turns inside every repeat, one process and one stream, timed
with events around a batch of rotated buffer sets that together read at least
1 GiB (so nothing is served from a cache):
  fused      the batched route (aqz_ds_last_batch_kind 7)
  per_frame  the same handle with aqz_debug_ds_force_per_frame_batch(1): the
             per-frame state machine (kind 0), the only route before
  copy       (C only) hipMemcpyDtoDAsync of (bytes read + bytes written) / 2:
             a copy reads and writes each byte once

Both routes' outputs are compared on the device before timing.  One JSON line
per (workload, method): per variant ms per batch (min, median, spread = max -
min over the repeats), whether fused's median lies below per_frame's by more
than the larger spread, and for C the TB/s (read + written) of fused and copy.
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
WORKLOADS = {
    "A": ([(2048, 2048, 64), (1024, 1024, 32), (512, 512, 16), (256, 256, 16)], 4),
    "B": ([(512, 512, 1024), (256, 256, 512), (256, 256, 256), (256, 256, 128),
           (256, 256, 64)], 2),
    "C": ([(1024, 1024, 256), (1024, 1024, 128), (1024, 1024, 64), (1024, 1024, 32)], 2),
}
BPP = 2


def traffic(geo, n, decimate):
    """(bytes read, bytes written) of the fused route: every run reads its
    input level once (Decimate: a quarter of it where XY halves — every other
    row of every other plane, or of every plane — and the even planes where Z
    alone does) and writes each of its levels once."""
    frames, read, written = [n], 0, 0
    for l in range(1, len(geo)):
        frames.append(frames[-1] >> (geo[l][2] < geo[l - 1][2]))
        written += frames[l] * geo[l][0] * geo[l][1] * BPP

    def cls(l):
        return (geo[l][0] < geo[l - 1][0], geo[l][2] < geo[l - 1][2])
    l = 1
    while l < len(geo):
        xy, z = cls(l)
        depth = 2 if xy and z else 4 if xy else 3
        k = 1
        while l + k < len(geo) and k < depth and cls(l + k) == (xy, z):
            k += 1
        level_bytes = frames[l - 1] * geo[l - 1][0] * geo[l - 1][1] * BPP
        read += level_bytes // ((4 if xy else 2) if decimate else 1)
        l += k
    return read, written


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
        sys.exit("mixed_batch_bench needs a GPU")
    torch.cuda.set_device(0)
    L = aqz.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.c_void_p]
    # one stream for every call and both events: a NULL stream would put the
    # batch calls on their handles' own streams, outside the events
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    st = ctypes.c_void_p(stream.cuda_stream)

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
        for method in ("mean", "decimate"):
            read, written = traffic(geo, n, method == "decimate")
            rot = max(2, -(-GIB // read))
            g = torch.Generator(device="cuda").manual_seed(3)
            ins = [torch.randint(0, 256, (in_bytes,), dtype=torch.uint8, device="cuda",
                                 generator=g) for _ in range(rot)]
            sets = {v: [[None] + [u8(frames[l] * geo[l][0] * geo[l][1] * BPP)
                                  for l in range(1, nl)] for _ in range(rot)]
                    for v in ("fused", "per_frame")}
            ds = aqz.Downsampler(geo, np.uint16, aqz.METHODS[method], device=0)
            counts = (ctypes.c_uint32 * nl)()

            def ptrs(bufs):
                return (ctypes.c_void_p * nl)(*[b.data_ptr() if b is not None else 0
                                                for b in bufs])

            call = {v: [(ds._h, ins[r].data_ptr(), n, ptrs(sets[v][r]), counts, st)
                        for r in range(rot)] for v in sets}

            def fused(r):
                rc = L.aqz_ds_run_device_batch(*call["fused"][r])
                assert rc == 0, ds._check(rc)

            def per_frame(r):
                ds.debug_force_per_frame_batch(1)
                rc = L.aqz_ds_run_device_batch(*call["per_frame"][r])
                ds.debug_force_per_frame_batch(0)
                assert rc == 0, ds._check(rc)

            variants = {"fused": fused, "per_frame": per_frame}
            copy_bytes = (read + written) // 2
            if wl == "C":
                csrc = [u8(copy_bytes) for _ in range(rot)]
                cdst = [u8(copy_bytes) for _ in range(rot)]

                def copy(r):
                    rc = hip.hipMemcpyDtoDAsync(cdst[r].data_ptr(), csrc[r].data_ptr(), copy_bytes,
                                                st)
                    assert rc == 0, rc
                variants["copy"] = copy

            # the same bytes from both routes, and the kinds the handle reports
            fused(0)
            kinds = [ds.last_batch_kind()]
            per_frame(0)
            kinds.append(ds.last_batch_kind())
            torch.cuda.synchronize()
            assert kinds == [7, 0], kinds
            same = all(bool(torch.equal(sets["fused"][0][l], sets["per_frame"][0][l]))
                       for l in range(1, nl))
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
                   "method": method, "frames": n, "rotations": rot, "bytes_read_per_batch": read,
                   "bytes_written_per_batch": written, "reps": args.reps, "warmup": args.warmup,
                   "outputs_identical": same}
            for v in variants:
                med = statistics.median(times[v])
                rec[v] = {"ms_min": round(min(times[v]), 4), "ms_median": round(med, 4),
                          "ms_max": round(max(times[v]), 4),
                          "ms_spread": round(max(times[v]) - min(times[v]), 4)}
            spread = max(rec["fused"]["ms_spread"], rec["per_frame"]["ms_spread"])
            rec["larger_spread_ms"] = spread
            rec["fused_below_per_frame_by_more_than_spread"] = bool(
                rec["fused"]["ms_median"] < rec["per_frame"]["ms_median"] - spread)
            rec["per_frame_over_fused"] = round(
                rec["per_frame"]["ms_median"] / rec["fused"]["ms_median"], 2)
            if wl == "C":
                def tbs(nbytes, v, key):
                    return round(nbytes / (rec[v][key] * 1e-3) / 1e12, 3)
                rec["copy_bytes"] = copy_bytes
                rec["fused_tb_s"] = {"median": tbs(read + written, "fused", "ms_median"),
                                     "min": tbs(read + written, "fused", "ms_max"),
                                     "max": tbs(read + written, "fused", "ms_min")}
                rec["copy_tb_s"] = {"median": tbs(2 * copy_bytes, "copy", "ms_median"),
                                    "min": tbs(2 * copy_bytes, "copy", "ms_max"),
                                    "max": tbs(2 * copy_bytes, "copy", "ms_min")}
                rec["fused_over_copy_tb_s"] = round(
                    rec["fused_tb_s"]["median"] / rec["copy_tb_s"]["median"], 3)
                del csrc, cdst
            ds.close()
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del ins, sets
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
