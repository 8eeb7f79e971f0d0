"""GPU: aqz_ds_run_device_batch's mixed-pyramid route (kind 7) between pending
work on the caller's stream (tests/stream_order.py, imported as it is).  The
route owns no scratch and joins no other stream: the unstalled first run is
the handle's first use and is checked like the stalled one, which must return
while the stall runs, read its inputs and write its outputs in stream order."""
import numpy as np
import pytest

import mixed_batch_cases as mc
from stream_order import Sandwich

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", mc.OFFSET_SHAPES)
def test_mixed_batch_behind_a_stall(aqz, oracle, name):
    geo, n, dtype, runs = mc.FIXED[name]
    frames = mc.fixed_frames(name, seed=1)
    want = mc.oracle_levels(oracle, geo, dtype, mc.MEAN, frames)
    sw = Sandwich(f"run_device_batch mixed {name}")
    d_in = sw.input(frames)
    outs = [None] + [sw.output(want[L].nbytes,
                               np.ascontiguousarray(want[L]).view(np.uint8).reshape(-1),
                               name=f"level {L}") for L in range(1, len(geo))]
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    counts = []

    def call(sw):
        counts.append(ds.run_device_batch(d_in.data_ptr(), n,
                                          [0] + [o.data_ptr() for o in outs[1:]], sw.hip_stream))
        assert ds.last_batch_kind() == 7

    try:
        sw.run(call)   # check_dry: the first use is checked too
        assert counts == [mc.emitted(geo, n)] * 2
    finally:
        ds.close()
