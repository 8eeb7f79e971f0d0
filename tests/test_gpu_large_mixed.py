"""GPU: a Z run past 4 GiB.  u8 1031 x 517 planes through three Z-only levels
in one launch, by the shift rule of tests/large_batch.py: plane k of the batch
is a base plane group's plane k mod 8 plus tag(k div 8), so level L's frames
of group g must be the oracle's levels of the base group plus tag(g), and one
oracle run serves every size.  Every frame of every level is compared on the
device.  The smaller batch's input passes 2^32 bytes, the larger one's passes
2^33, so that its level 1 passes 2^32 as well: the kernel's element offsets of
both the loads and the stores are past 32 bits."""
import numpy as np
import pytest

import large_batch as lb
from gpu_util import launch_stream, torch_cuda

pytestmark = pytest.mark.gpu

W, H, LEVELS = 1031, 517, 4
GROUP = 1 << (LEVELS - 1)


def planes_past(nbytes):
    """The first multiple of 8 planes whose bytes pass `nbytes`."""
    n = nbytes // (W * H) + 1
    return -(-n // GROUP) * GROUP


SIZES = {"input_past_4GiB": planes_past(1 << 32), "level1_past_4GiB": planes_past(1 << 33)}


def case_of(planes, method):
    geo = [(W, H, planes >> L) for L in range(LEVELS)]
    return lb.Case(f"mixed-z3-{planes}-m{method}", "volume", "mixed_z3", geo, np.uint8, method, 7,
                   "shallow", None)


def test_sizes():
    a, b = SIZES["input_past_4GiB"], SIZES["level1_past_4GiB"]
    assert (a - GROUP) * W * H <= 1 << 32 < a * W * H and a % GROUP == 0
    assert b * W * H > 1 << 33 and (b >> 1) * W * H > 1 << 32 and b % GROUP == 0


@pytest.mark.parametrize("method", [1, 0], ids=["mean", "decimate"])
@pytest.mark.parametrize("size", list(SIZES))
def test_zrun_past_4gib(aqz, oracle, size, method):
    torch = torch_cuda()
    planes = SIZES[size]
    case = case_of(planes, method)
    assert lb.group_planes(case) == GROUP
    need = sum(lb.level_frames(case, L, planes) * W * H for L in range(LEVELS)) + 5 * lb.SLAB_BYTES
    free, _ = torch.cuda.mem_get_info()
    assert free > need, f"{need >> 20} MiB of device memory needed, {free >> 20} free"
    expected = lb.expected_levels(oracle, case)
    d_in = lb.build_batch(torch, case, planes)
    outs = [None] + [lb.poisoned(torch, (planes >> L) * W * H) for L in range(1, LEVELS)]
    ds = aqz.Downsampler(case.geo, case.dtype, method)
    try:
        counts = ds.run_device_batch(d_in.data_ptr(), planes,
                                     [0] + [o.data_ptr() for o in outs[1:]], launch_stream())
        torch.cuda.synchronize()
        assert ds.last_batch_kind() == 7
    finally:
        ds.close()
    assert counts == [planes >> L for L in range(LEVELS)]
    tags = lb.device_tags(torch, case, planes // GROUP)
    vt = lb.torch_view_dtype(torch, case.dtype)
    for L in range(1, LEVELS):
        n = planes >> L
        raw = outs[L]
        assert bool((raw[n * W * H:] == lb.POISON).all()), f"L{L}: bytes past the level written"
        got = raw[: n * W * H].view(vt).view(n, H, W)
        want0 = lb.to_view(torch, expected[L], case.dtype)
        lb.compare_frames(torch, got, want0, None, tags, GROUP >> L, f"{case.id} L{L}")
