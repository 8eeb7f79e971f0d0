"""Runner for tests/test_gpu_decode_mutations.py::test_header_named_blocksizes_launch_log
(not a test module).

The launch log is switched on by $AQZ_LAUNCH_LOG=1 at the library's first use,
so it is read in a process of its own, started fresh by the test.  The two
frames of decode_mutation_cases.LAUNCH_LOG_SEEDS (typesize 4 with blocksize
4098, typesize 3 with blocksize 1200: blocksizes only a header names) go
through aqz_blosc_lz4_decompress_device; one JSON object per frame is printed:

  {"name": seed, "status": s, "equal": chunk equals the source,
   "launches": [the launch lines, as dicts]}
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
    import decode_mutation_cases as dm
    from gpu_util import empty_device, from_device, to_device

    aqz = aqz_pkg.load()
    torch.cuda.set_device(0)
    ctx = aqz.BloscContext(0, 0)
    for name in dm.LAUNCH_LOG_SEEDS:
        _, seed, _ = dm.seed_named(aqz, name)
        n = len(seed.src)
        d_fr = to_device(np.frombuffer(seed.frame, np.uint8))
        d_dst = empty_device(n)
        d_st = empty_device(4)
        torch.cuda.synchronize()
        aqz.debug_launch_log()
        ctx.lz4_decompress_device(seed.ts, n, d_fr.data_ptr(), len(seed.frame), 0, 1,
                                  d_dst.data_ptr(), n, d_st.data_ptr())
        status = int(from_device(d_st, np.uint32, (1,))[0])
        got = from_device(d_dst, np.uint8, (-1,))[:n].tobytes()
        print(json.dumps({"name": name, "status": status, "equal": got == seed.src,
                          "launches": aqz.debug_launch_log()}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
