#!/usr/bin/env python3
"""Time blosc+LZ4 chunk frames made on the device against the host path.

  python tools/blosc_lz4_bench.py [--reps 15] [--warmup 3] [--threads 16] [--out FILE]

Per workload and clevel (lz4, byte shuffle, typesize 2), in one process, the
variants taking turns inside every repeat:

  device_batch   aqz_blosc_lz4_compress_device, flags 0 (64 probes per step)
  device_serial  aqz_blosc_lz4_compress_device, AQZ_LZ4_PROBE_SERIAL
  host           aqz_blosc_compress_device on `threads` host threads (the
                 path without this entry point: filtered chunks cross PCIe)
  cblosc         c-blosc itself on `threads` threads from host-resident
                 chunks (oracle/libblosc_cpu.so), where the image has it

Workloads: the 256 smooth 256x256 u16 chunks bench.py's measure_blosc_frames
uses ("smooth"), and 256 level-1 tiles the tiled pyramid kernel leaves in HBM
for 64 such 1024x1024 frames ("tiles"); beside them the same image without
noise ("noiseless") and noise alone ("random"), the two ends of
compressibility.  A call is timed with the host clock
around it; every call ends in a stream synchronise.  One JSON line per
(workload, clevel): ms per batch (min and median), GB/s of input, bytes copied
device-to-host, and whether all variants wrote the same bytes.
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

N_CHUNKS = 256
TILE = 256
NB = TILE * TILE * 2


def smooth(rng, n, h, w, noise=4.0):
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w), np.uint16)
    for k in range(n):
        out[k] = (2000 + 500 * np.sin((xx + 13 * k) / 17.0) * np.cos((yy - 5 * k) / 23.0)
                  + rng.normal(0, noise, (h, w))).astype(np.uint16)
    return out


def pyramid_tiles(aqz, torch):
    """Level-1 tiles of 64 smooth 1024^2 frames, as aqz_ds_run_device_batch_tiled
    lays them out: 256 chunk buffers of 128 KiB, left on the device."""
    frames = smooth(np.random.default_rng(6), 64, 1024, 1024)
    dims = [(aqz.TIME, 0, 1, 1), (aqz.SPACE, 1024, TILE, 1), (aqz.SPACE, 1024, TILE, 1)]
    geo = aqz.level_geometry(aqz.plan_levels(dims))[:2]
    ds = aqz.Downsampler(geo, np.uint16, aqz.METHODS["mean"], device=0)
    d_in = torch.from_numpy(frames.view(np.uint8).reshape(-1)).to("cuda")
    out = torch.empty(N_CHUNKS * NB, dtype=torch.uint8, device="cuda")
    ds.run_device_batch_tiled(d_in.data_ptr(), 64, [(TILE, TILE)] * 2, [0, out.data_ptr()])
    torch.cuda.synchronize()
    ds.close()
    return out


def cblosc_lib():
    path = os.path.join(ROOT, "oracle", "libblosc_cpu.so")
    import blosc_ref
    if not (os.path.exists(path) and blosc_ref.available()):
        return None
    cpu = ctypes.CDLL(path)
    cpu.cblosc_compress_chunks.restype = ctypes.c_double
    cpu.cblosc_compress_chunks.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    return cpu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    import aqz_pkg
    aqz = aqz_pkg.load()
    if not torch.cuda.is_available():
        sys.exit("blosc_lz4_bench needs a GPU")
    torch.cuda.set_device(0)
    cpu = cblosc_lib()
    stride = NB + aqz.BLOSC_MAX_OVERHEAD
    workloads = {
        "smooth": torch.from_numpy(smooth(np.random.default_rng(5), N_CHUNKS, TILE, TILE)
                                   .view(np.uint8).reshape(-1)).to("cuda"),
        "tiles": pyramid_tiles(aqz, torch),
        # the two ends of compressibility: the same image without noise, and
        # noise alone (every chunk becomes a memcpy frame)
        "noiseless": torch.from_numpy(smooth(np.random.default_rng(5), N_CHUNKS, TILE, TILE, 0.0)
                                      .view(np.uint8).reshape(-1)).to("cuda"),
        "random": torch.from_numpy(np.random.default_rng(7).integers(
            0, 256, N_CHUNKS * NB, dtype=np.uint8)).to("cuda"),
    }
    torch.cuda.synchronize()
    ctx = aqz.BloscContext(0, args.threads)
    lines = []
    for name, d in workloads.items():
        host_raw = d.cpu().numpy()
        for clevel in (1, 5):
            bufs = {v: np.empty(N_CHUNKS * stride, np.uint8)
                    for v in ("device_batch", "device_serial", "host", "cblosc")}
            csz = (ctypes.c_size_t * N_CHUNKS)()

            def run(v):
                if v == "host":
                    return ctx.compress_device(clevel, aqz.SHUFFLE, 2, "lz4", d.data_ptr(), NB,
                                               N_CHUNKS, host_dst=bufs[v], dst_stride=stride)
                if v == "cblosc":
                    cpu.cblosc_compress_chunks(host_raw.ctypes.data, NB, N_CHUNKS, clevel, 1, 2,
                                               b"lz4", args.threads, bufs[v].ctypes.data, stride,
                                               csz, 1)
                    return list(csz)
                return ctx.lz4_compress_device(
                    clevel, aqz.SHUFFLE, 2, d.data_ptr(), NB, N_CHUNKS, host_dst=bufs[v],
                    dst_stride=stride, flags=aqz.LZ4_PROBE_SERIAL if v == "device_serial" else 0)

            variants = ["device_batch", "device_serial", "host"] + (["cblosc"] if cpu else [])
            times = {v: [] for v in variants}
            sizes = {}
            for rep in range(args.warmup + args.reps):
                for v in variants:  # taking turns, so drift hits all alike
                    t0 = time.perf_counter()
                    sizes[v] = run(v)
                    dt = time.perf_counter() - t0
                    if rep >= args.warmup:
                        times[v].append(dt)
            ctx.lz4_compress_device(clevel, aqz.SHUFFLE, 2, d.data_ptr(), NB, N_CHUNKS,
                                    host_dst=bufs["device_batch"], dst_stride=stride)
            d2h_device = ctx.d2h_bytes()
            ref = sizes["host"]
            same = all(
                list(sizes[v]) == list(ref) and all(
                    np.array_equal(bufs[v][k * stride:k * stride + ref[k]],
                                   bufs["host"][k * stride:k * stride + ref[k]])
                    for k in range(N_CHUNKS))
                for v in variants)
            memcpy_frames = sum(1 for k in range(N_CHUNKS) if bufs["host"][k * stride + 2] & 0x2)
            d2h_host = N_CHUNKS * NB + memcpy_frames * NB
            total_in = N_CHUNKS * NB
            rec = {"workload": name, "chunks": N_CHUNKS, "chunk_bytes": NB,
                   "codec": f"lz4 clevel {clevel} shuffle", "threads": args.threads,
                   "reps": args.reps, "warmup": args.warmup,
                   "ratio": round(sum(ref) / total_in, 4),
                   "frames_identical": bool(same),
                   "d2h_bytes_device": int(d2h_device), "d2h_bytes_host": int(d2h_host),
                   "d2h_ratio": round(d2h_device / d2h_host, 4)}
            for v in variants:
                best, med = min(times[v]), statistics.median(times[v])
                rec[v] = {"ms_min": round(best * 1e3, 3), "ms_median": round(med * 1e3, 3),
                          "GBps_in_median": round(total_in / med / 1e9, 3)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
