"""Runner for tests/test_gpu_mixed_batch.py::test_launch_log_names_the_runs (not
a test module).

The launch log is switched on by $AQZ_LAUNCH_LOG=1 at the library's first use,
so it is read in a process of its own, started fresh by the test.  Every fixed
shape of mixed_batch_cases goes through run_device_batch once, then two
batches the route refuses (an odd stack, frames off the multiple); the log is
drained after each and everything printed as one JSON object."""
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


def one(aqz, geo, n, dtype):
    bpp = np.dtype(dtype).itemsize
    counts = mc.emitted(geo, n) if mc.runs_of(geo, n) else [n] * len(geo)
    d_in = torch.zeros(n * geo[0][0] * geo[0][1] * bpp, dtype=torch.uint8, device="cuda")
    outs = [None] + [torch.zeros(max(1, counts[L] * geo[L][0] * geo[L][1] * bpp),
                                 dtype=torch.uint8, device="cuda") for L in range(1, len(geo))]
    ds = aqz.Downsampler(geo, dtype, 1)
    aqz.debug_launch_log()
    ds.run_device_batch(d_in.data_ptr(), n, [0] + [o.data_ptr() for o in outs[1:]])
    kind = ds.last_batch_kind()
    log = aqz.debug_launch_log()
    torch.cuda.synchronize()
    ds.close()
    return {"kind": kind, "log": log}


def main():
    aqz = aqz_pkg.load()
    rec = {name: one(aqz, geo, n, dtype) for name, (geo, n, dtype, _) in mc.FIXED.items()}
    rec["refused_odd_stack"] = one(aqz, [(256, 128, 6), (128, 64, 3), (64, 32, 2)], 12, np.uint16)
    first = mc.FIXED["volume2_cascade2"]
    rec["refused_six_frames"] = one(aqz, first[0], 6, first[2])
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
