"""Runner for tests/test_gpu_chunk_gather.py::test_launch_log_pins_the_form
(not a test module).

The launch log is switched on by $AQZ_LAUNCH_LOG=1 at the library's first use,
so it is read in a process of its own, started fresh by the test.  Every fixed
shape of tests/chunk_gather_cases.py goes through
aqz_chunk_gather_frames_device as the GPU test runs it (3 frames from frame 1,
2 frames a chunk), then the 76 frames of the reference's KAT dimensions, one
aqz_untile_frame_device and one refused call; the log is drained after each
and printed as one JSON object."""
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
import chunk_gather_cases as cg  # noqa: E402
import kat_runner  # noqa: E402


def run(aqz, dims, dtype, first, n):
    bpp = np.dtype(dtype).itemsize
    h, w, tr, tc = dims[-2][1], dims[-1][1], dims[-2][2], dims[-1][2]
    base, internal, cb, cpl = aqz.chunk_frame_places(dims, bpp, first, n)
    n_chunks = (int(base.max()) // cpl + 1) * cpl
    chunks = torch.zeros(n_chunks * cb, dtype=torch.uint8, device="cuda")
    frames = torch.zeros(n * w * h * bpp, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    aqz.chunk_gather_frames_device(dtype, w, h, tr, tc, chunks.data_ptr(), cb, n_chunks, 0,
                                   n_chunks, base, internal, frames.data_ptr(), w * h * bpp)
    torch.cuda.synchronize()
    return aqz.debug_launch_log()


def main():
    aqz = aqz_pkg.load()
    aqz.debug_launch_log()
    rec = {}
    for name, w, h, tile, dtype, _ in cg.FIXED:
        rec[name] = run(aqz, cg.tyx(w, h, tile, 2), dtype, 1, 3)
    kat = [tuple(d) for d in kat_runner.load()["addressing"][0]["dims"]]
    rec["kat_76"] = run(aqz, kat, np.uint16, 0, 76)
    tiles = torch.zeros(4 * 16 * 16 * 2, dtype=torch.uint8, device="cuda")
    frame = torch.zeros(30 * 20 * 2, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    aqz.untile_frame_device(np.uint16, tiles.data_ptr(), 30, 20, 16, 16, frame.data_ptr())
    torch.cuda.synchronize()
    rec["untile"] = aqz.debug_launch_log()
    try:
        aqz.untile_frame_device(np.uint16, tiles.data_ptr(), 30, 20, 0, 16, frame.data_ptr())
    except aqz.AqzError:
        pass
    rec["refused"] = aqz.debug_launch_log()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
