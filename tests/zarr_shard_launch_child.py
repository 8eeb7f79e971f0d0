"""Runner for tests/test_gpu_zarr_shards.py::test_launch_log (not a test module).

The launch log is switched on by $AQZ_LAUNCH_LOG=1 at the library's first use,
so it is read in a process of its own, started fresh by the test.  A fixed
geometry (2 shards of 3 slots, frames of 100,000 bytes) goes through begin,
append_layer_device and tables_device, and 70 frames of 300 tiles through
chunk_has_data_device; the log is drained after each and printed as one JSON
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
import zarr_shard_model as zm  # noqa: E402


def main():
    aqz = aqz_pkg.load()
    stride = 100_000
    st = aqz.ZarrShardSet(zm.many_shard_dims(2, 3), 0)
    frames = torch.zeros(6 * stride, dtype=torch.uint8, device="cuda")
    out = torch.zeros(6 * stride, dtype=torch.uint8, device="cuda")
    seg = torch.zeros(8 * st.segment_words, dtype=torch.uint8, device="cuda")
    tab = torch.zeros(st.table_bytes * 2 + 16, dtype=torch.uint8, device="cuda")
    aqz.debug_launch_log()
    rec = {"piece": aqz.ZARR_SHARD_PACK_PIECE, "stride": stride}
    st.begin()
    rec["begin"] = aqz.debug_launch_log()
    st.append_layer_device(frames.data_ptr(), stride, out.data_ptr(), 6 * stride, seg.data_ptr())
    rec["append"] = aqz.debug_launch_log()
    st.tables_device(tab.data_ptr(), tab.data_ptr() + st.table_bytes * 2)
    rec["tables"] = aqz.debug_launch_log()
    torch.cuda.synchronize()

    n_frames, n_tiles, S = 70, 300, 2
    rng = np.random.default_rng(7)
    flags = (rng.integers(0, 40, (n_frames, n_tiles, S)) == 0).astype(np.uint8)
    base = [int(b) for b in rng.integers(0, 5, n_frames) * n_tiles]
    want = np.zeros(5 * n_tiles, np.uint8)
    for k in range(n_frames):
        want[base[k]:base[k] + n_tiles] |= flags[k].any(axis=1)
    d_flags = torch.from_numpy(flags.reshape(-1)).to("cuda")
    d_has = torch.zeros(5 * n_tiles, dtype=torch.uint8, device="cuda")
    aqz.zarr_shard_chunk_has_data_device(d_flags.data_ptr(), n_frames, n_tiles, S, base,
                                         d_has.data_ptr())
    rec["has_data"] = aqz.debug_launch_log()
    torch.cuda.synchronize()
    rec["has_data_ok"] = bool(np.array_equal(d_has.cpu().numpy(), want))
    st.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
