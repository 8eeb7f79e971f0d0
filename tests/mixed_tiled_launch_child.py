"""Runner for tests/test_gpu_mixed_tiled.py::test_launch_log_names_the_runs (not
a test module).

The launch log is switched on by $AQZ_LAUNCH_LOG=1 at the library's first use,
so it is read in a process of its own, started fresh by the test.  Every fixed
shape of mixed_batch_cases goes through run_device_mixed_tiled once under each
of its tile shapes (mixed_tiled_cases.FIXED_TILES), then two calls it refuses
(an odd stack, frames off the multiple); the log is drained after each and
everything printed as one JSON object."""
import json
import os
import sys

import numpy as np
import torch  # before the native library: both share one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import aqz_pkg  # noqa: E402
import mixed_batch_cases as mc  # noqa: E402
import mixed_tiled_cases as tc  # noqa: E402


def one(aqz, geo, n, dtype, tiles):
    bpp = np.dtype(dtype).itemsize
    counts = mc.emitted(geo, n) if mc.runs_of(geo, n) else [n] * len(geo)
    d_in = torch.zeros(n * geo[0][0] * geo[0][1] * bpp, dtype=torch.uint8, device="cuda")
    ds = aqz.Downsampler(geo, dtype, 1)
    outs, flags = [None], [None]
    for L in range(1, len(geo)):
        tr, tcol = tiles[L]
        nt = tc.n_tiles(geo, L, tiles[L])
        slots = max(1, ds.mixed_flag_slots(L, tr, tcol))
        outs.append(torch.zeros(max(1, counts[L] * nt * tr * tcol * bpp), dtype=torch.uint8,
                                device="cuda"))
        flags.append(torch.zeros(max(1, counts[L] * nt * slots), dtype=torch.uint8,
                                 device="cuda"))
    aqz.debug_launch_log()
    status = 0
    try:
        ds.run_device_mixed_tiled(d_in.data_ptr(), n, tiles,
                                  [0] + [o.data_ptr() for o in outs[1:]],
                                  [0] + [f.data_ptr() for f in flags[1:]])
    except aqz.AqzError as e:
        status = e.status
    kind = ds.last_batch_kind()
    log = aqz.debug_launch_log()
    torch.cuda.synchronize()
    ds.close()
    rec = {"kind": kind, "log": log}
    if status:
        rec["status"] = status
    return rec


def main():
    aqz = aqz_pkg.load()
    rec = {}
    for name, spec in tc.FIXED_CASES:
        geo, n, dtype, _ = mc.FIXED[name]
        rec[f"{name}-{tc.tiles_id(spec)}"] = one(aqz, geo, n, dtype, tc.tiles_for(geo, spec))
    odd = [(256, 128, 6), (128, 64, 3), (64, 32, 2)]
    rec["refused_odd_stack"] = one(aqz, odd, 12, np.uint16, tc.tiles_for(odd, (32, 64)))
    first = mc.FIXED["volume2_cascade2"]
    rec["refused_six_frames"] = one(aqz, first[0], 6, first[2], tc.tiles_for(first[0], (32, 64)))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
