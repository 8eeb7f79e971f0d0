"""Runner for tests/test_gpu_blosc_lz4.py::test_launch_log (not a test module).

The launch log is switched on by $AQZ_LAUNCH_LOG=1 at the library's first use,
so it is read in a process of its own, started fresh by the test.  For each
probe form and each table form, two small chunks go through
aqz_blosc_lz4_compress_device; one JSON object per run is printed:

  {"flags": f, "want_table": "u16"|"u32", "equal": frames equal the host
   path's, "launches": [the launch lines, as dicts]}
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]


def main():
    import torch
    import aqz_pkg
    from gpu_util import to_device

    aqz = aqz_pkg.load()
    torch.cuda.set_device(0)
    ctx = aqz.BloscContext(0, 2)
    rng = np.random.default_rng(21)
    # clevel 5, typesize 2: a 64 KiB chunk is one block of two 32 KiB splits
    # (u16 table), a 256 KiB chunk one block of two 128 KiB splits (u32 table)
    for nbytes, table in ((65536, "u16"), (262144, "u32")):
        vals = (1000 + 200 * np.sin(np.arange(nbytes) / 31.0) + rng.normal(0, 3, nbytes))
        raw = vals.astype(np.uint16).view(np.uint8).reshape(-1)[:2 * nbytes].copy()
        d = to_device(raw)
        want = ctx.compress_device(5, 1, 2, "lz4", d.data_ptr(), nbytes, 2)
        aqz.debug_launch_log()
        for flags in (0, aqz.LZ4_PROBE_SERIAL):
            got = ctx.lz4_compress_device(5, 1, 2, d.data_ptr(), nbytes, 2, flags=flags)
            print(json.dumps({"flags": flags, "want_table": table, "equal": got == want,
                              "launches": aqz.debug_launch_log()}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
