"""Runner for tests/test_gpu_volume_tiled.py::test_launch_log_names_both_families
(not a test module).

The launch log is switched on by $AQZ_LAUNCH_LOG=1 at the library's first use,
so it is read in a process of its own, started fresh by the test.  One volume
(520x22x8 f32, 3 levels) goes through run_device_batch and through
run_device_volume_tiled; the log is drained after each and printed as one JSON
object."""
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
import volume_tiled_cases as vc  # noqa: E402


def main():
    aqz = aqz_pkg.load()
    w, h, planes, levels, dtype, tr, tc, _ = vc.CASES[3]
    geo = vc.volume_geo(w, h, planes, levels)
    d_in = torch.zeros(planes * h * w * 4, dtype=torch.uint8, device="cuda")
    outs = [torch.zeros(1 << 20, dtype=torch.uint8, device="cuda") for _ in geo]
    ptrs = [0] + [o.data_ptr() for o in outs[1:]]
    rec, kinds = {}, []
    aqz.debug_launch_log()
    ds = aqz.Downsampler(geo, dtype, 1)
    ds.run_device_batch(d_in.data_ptr(), planes, ptrs)
    kinds.append(ds.last_batch_kind())
    rec["row_major"] = aqz.debug_launch_log()
    ds.close()
    ds = aqz.Downsampler(geo, dtype, 1)
    ds.run_device_volume_tiled(d_in.data_ptr(), planes, [None] + [(tr, tc)] * (levels - 1), ptrs)
    kinds.append(ds.last_batch_kind())
    rec["tiled"] = aqz.debug_launch_log()
    torch.cuda.synchronize()
    ds.close()
    rec["kinds"] = kinds
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
