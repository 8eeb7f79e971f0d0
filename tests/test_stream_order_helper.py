"""CPU: the parts of tests/stream_order.py that need no GPU."""
import numpy as np

import stream_order as so


def test_poisons_and_bounds():
    assert so.POISON == 0xA5 and so.LATE_POISON == 0x5A and so.POISON != so.LATE_POISON
    # every stall ends by itself, within what a test may take
    assert 0 < so.STALL_FLOOR_MS <= so.STALL_CAP_MS <= 2000
    assert so.STALL_MULTIPLE >= 2


def test_decoy_differs_everywhere_and_is_never_zero():
    rng = np.random.default_rng(0)
    for arr in (np.zeros(4096, np.uint8), np.full(4096, 0xFF, np.uint8),
                rng.integers(0, 256, 70000, dtype=np.uint8),
                rng.standard_normal((33, 17)).astype(np.float32)):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        d = so.decoy_like(arr, seed=3)
        assert d.dtype == np.uint8 and d.size == raw.size
        assert (d != raw).all() and (d != 0).all()
        assert np.array_equal(d, so.decoy_like(arr, seed=3))  # seeded
