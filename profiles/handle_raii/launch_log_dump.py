"""Drain the launch log of a short streaming script into a file (one JSON
record per launch, phase headers between)."""
import json
import os
import sys

os.environ["AQZ_LAUNCH_LOG"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (binds the HIP runtime first, as the tests do)
import aqz_pkg

aqz = aqz_pkg.load()
out = open(sys.argv[1], "w")


def drain(tag):
    for rec in aqz.debug_launch_log():
        out.write(f"{tag} " + json.dumps(rec, sort_keys=True) + "\n")


def run(name, geo, tile):
    w, h, _ = geo[0]
    rng = np.random.default_rng(5)
    for tiled in (False, True):
        ds = aqz.Downsampler(geo, np.uint16, 1, device=0)
        if tiled:
            for L in range(1, len(geo)):
                ds.set_level_tiling(L, *tile)
        for i in range(3):
            f = rng.integers(0, 65536, (h, w), dtype=np.uint16)
            ds.add_frame(f)
            drain(f"{name} tiled={int(tiled)} frame={i} add")
            for L in range(1, len(geo)):
                got = ds.take_frame_tiled(L, *tile) if tiled else ds.take_frame(L)
                drain(f"{name} tiled={int(tiled)} frame={i} take L{L} has={int(got is not None)}")
        out.write(f"{name} tiled={int(tiled)} stream_tiled_runs={ds.stream_tiled_runs()} "
                  f"device_bytes={ds.device_memory_usage()}\n")
        ds.close()


geo2d = [(1000, 601, 1)]
for _ in range(3):
    w, h, _z = geo2d[-1]
    geo2d.append(((w + 1) // 2, (h + 1) // 2, 1))
run("1000x601_u16_4lv", geo2d, (64, 64))
run("64x48xz6_u16", [(64, 48, 6), (32, 24, 3), (16, 12, 2)], (8, 8))
out.close()
print("launch log written:", sys.argv[1], sum(1 for _ in open(sys.argv[1])), "lines")
