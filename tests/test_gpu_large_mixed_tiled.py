"""GPU: the tiled Z run's 64-bit offsets.

Destination: a lattice buffer just over 4 GiB is allocated but not filled; the
offsets put a level's frames on both sides of byte 2^32, and only the regions
written and their guards are checked.

Source: tests/test_gpu_large_mixed.py's conventions — u8 1031 x 517 planes,
three Z-only levels, Mean, by the shift rule of tests/large_batch.py (plane k
is a base group's plane k mod 8 plus tag(k div 8), so one oracle run serves
every group) — with the input past 2^32 bytes and the levels written as
128 x 256 tiles, un-tiled and compared on the device."""
import numpy as np
import pytest

import large_batch as lb
import mixed_batch_cases as mc
import mixed_tiled_cases as tc
from gpu_util import launch_stream, random_frames, to_device, torch_cuda

pytestmark = pytest.mark.gpu

GUARD = 64


def test_destination_offsets_past_4gib(aqz, oracle):
    torch = torch_cuda()
    name = "volume1_zrun3"
    geo, n, dtype, _ = mc.FIXED[name]
    frames = mc.fixed_frames(name)
    levels = mc.oracle_levels(oracle, geo, dtype, mc.MEAN, frames)
    counts = mc.emitted(geo, n)
    tile = (16, 12)
    tiles = tc.tiles_for(geo, tile)
    want = tc.expected_tiled(oracle, levels, tiles)
    cap = (1 << 32) + (64 << 20)
    free, _ = torch.cuda.mem_get_info()
    assert free > cap + (1 << 30), f"{cap >> 20} MiB of device memory needed, {free >> 20} free"
    big = torch.empty(cap, dtype=torch.uint8, device="cuda")   # not filled
    small = {}
    lats = [None]
    placed = {}
    for L in range(1, len(geo)):
        t, _ = want[L]
        nt, fb = t.shape[1], t[0].nbytes
        cb = tile[0] * tile[1] * 4
        if L in (2, 3):
            # frames alternately below and above byte 2^32, level 2's first
            # one straddling it
            d = (L - 2) << 20
            offs = [(1 << 32) - d - (k + 1) * 2 * fb if k % 2 else (1 << 32) + d + k * 2 * fb
                    for k in range(counts[L])]
            if L == 2:
                offs[0] = (1 << 32) - fb // 2 // 4 * 4
            lats.append((big.data_ptr(), cap, tile[0], tile[1], cb, offs))
            placed[L] = offs
        else:
            small[L] = torch.full((counts[L] * fb,), tc.POISON, dtype=torch.uint8, device="cuda")
            lats.append((small[L].data_ptr(), counts[L] * fb, tile[0], tile[1], cb,
                         [k * fb for k in range(counts[L])]))
        assert nt * cb == fb
    for L, offs in placed.items():
        fb = want[L][0][0].nbytes
        assert min(offs) + fb < 1 << 32 < max(offs)
        assert L != 2 or offs[0] < 1 << 32 < offs[0] + fb
        for o in offs:      # poison each frame's place and its guards
            big[o - GUARD: o + fb + GUARD] = tc.POISON
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        d_in = to_device(frames)
        assert ds.run_device_mixed_chunked(d_in.data_ptr(), n, lats, None,
                                           launch_stream()) == counts
        torch.cuda.synchronize()
        assert ds.last_batch_kind() == 8
    finally:
        ds.close()
    for L, offs in placed.items():
        t = want[L][0]
        fb = t[0].nbytes
        for k, o in enumerate(offs):
            got = big[o - GUARD: o + fb + GUARD].cpu().numpy()
            assert (got[:GUARD] == tc.POISON).all() and (got[-GUARD:] == tc.POISON).all(), (L, k)
            assert got[GUARD:-GUARD].tobytes() == t[k].tobytes(), f"L{L} frame {k} at {o}"
    for L, d in small.items():
        assert d.cpu().numpy().tobytes() == want[L][0].tobytes(), f"L{L}"


W, H, LEVELS = 1031, 517, 4
GROUP = 1 << (LEVELS - 1)
TILE = (128, 256)


def test_source_offsets_past_4gib(aqz, oracle):
    torch = torch_cuda()
    planes = -(-((1 << 32) // (W * H) + 1) // GROUP) * GROUP
    assert (planes - GROUP) * W * H <= 1 << 32 < planes * W * H
    geo = [(W, H, planes >> L) for L in range(LEVELS)]
    case = lb.Case(f"mixed-tiled-z3-{planes}", "volume", "mixed_z3", geo, np.uint8, 1, 8,
                   "shallow", None)
    assert lb.group_planes(case) == GROUP
    nty, ntx = -(-H // TILE[0]), -(-W // TILE[1])
    ph, pw = nty * TILE[0], ntx * TILE[1]
    need = planes * W * H + 3 * planes * ph * pw + 5 * lb.SLAB_BYTES
    free, _ = torch.cuda.mem_get_info()
    assert free > need, f"{need >> 20} MiB of device memory needed, {free >> 20} free"
    expected = lb.expected_levels(oracle, case)
    d_in = lb.build_batch(torch, case, planes)
    outs = [None] + [lb.poisoned(torch, (planes >> L) * ph * pw) for L in range(1, LEVELS)]
    flags = [None] + [lb.poisoned(torch, (planes >> L) * nty * ntx) for L in range(1, LEVELS)]
    ds = aqz.Downsampler(geo, np.uint8, 1)
    try:
        counts = ds.run_device_mixed_tiled(d_in.data_ptr(), planes, [None] + [TILE] * (LEVELS - 1),
                                           [0] + [o.data_ptr() for o in outs[1:]],
                                           [0] + [f.data_ptr() for f in flags[1:]],
                                           launch_stream())
        torch.cuda.synchronize()
        assert ds.last_batch_kind() == 8
    finally:
        ds.close()
    assert counts == [planes >> L for L in range(LEVELS)]
    tags = lb.device_tags(torch, case, planes // GROUP)
    for L in range(1, LEVELS):
        n = planes >> L
        raw = outs[L]
        assert bool((raw[n * ph * pw:] == lb.POISON).all()), f"L{L}: bytes past the tiles written"
        padded = raw[: n * ph * pw].view(n, nty, ntx, TILE[0], TILE[1]).permute(0, 1, 3, 2, 4) \
            .reshape(n, ph, pw)
        assert not bool(padded[:, H:, :].any()) and not bool(padded[:, :, W:].any()), \
            f"L{L}: the overhang is not zero"
        got = padded[:, :H, :W].contiguous()
        want0 = lb.to_view(torch, expected[L], case.dtype)
        lb.compare_frames(torch, got, want0, None, tags, GROUP >> L, f"{case.id} L{L}")
        f = flags[L][: n * nty * ntx]
        assert bool(((f == 0) | (f == 1)).all()), f"L{L}: a flag byte is neither 0 nor 1"
        assert bool((flags[L][n * nty * ntx:] == lb.POISON).all())
        del padded, got
