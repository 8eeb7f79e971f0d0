"""Runner for tests/test_gpu_tiled_base.py::test_launch_log_shows_full_and_half_width_tiles
(not a test module).

The launch log is switched on by $AQZ_LAUNCH_LOG=1 at the library's first use,
so it is read in a process of its own, started fresh by the test.  Each of
tiled_base_cases.COLS_CASES (f32 and f64 at a width that takes the full tile
and one that takes the half-width tile) goes through
run_device_batch_tiled_base; the log is drained after each and printed as one
JSON list."""
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
import tiled_base_cases as tb  # noqa: E402


def main():
    aqz = aqz_pkg.load()
    out = []
    aqz.debug_launch_log()
    for dtype, w, _ in tb.COLS_CASES:
        h, levels, tile = tb.SWEEP["h"], tb.SWEEP["levels"], tb.SWEEP["tile"]
        geo = tb.halving(w, h, levels)
        d_in = torch.zeros(w * h * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
        outs = [torch.zeros(1 << 21, dtype=torch.uint8, device="cuda") for _ in geo]
        ds = aqz.Downsampler(geo, dtype, 1)
        ds.run_device_batch_tiled_base(d_in.data_ptr(), 1, [tile] * levels,
                                       [o.data_ptr() for o in outs])
        torch.cuda.synchronize()
        out.append(dict(dtype=np.dtype(dtype).name, w=w, kind=ds.last_batch_kind(),
                        log=aqz.debug_launch_log()))
        ds.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
