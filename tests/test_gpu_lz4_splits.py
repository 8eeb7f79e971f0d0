"""GPU: the wave-cooperative LZ4 split encoder (lz4_split_kernel,
csrc/codec_kernels.hip) against the serial encoder it restates
(csrc/lz4_block.hh, pinned to liblz4 by tests/test_lz4_block.py), split by
split, through aqz_debug_lz4_splits_device: no filter, no frame, no liblz4.

c-blosc compresses every split of a chunk with LZ4_compress_fast into at most
the split's own size (blosc_compress_ctx, zarr.common.cpp:106-137); the frame
kernel decides from each split's (csize, need) row, so the rows are compared as
well as the bytes.  The inputs are those of tests/lz4_cases.py, one test per
hazard; tests/test_lz4_split_cases.py shows on the CPU that each input does
reach its hazard.  Every case runs with the batched probe (flags 0) and the
serial one (AQZ_LZ4_PROBE_SERIAL).

Slots lie back to back, each of the split's own size, poisoned with 0xA5 with a
256-byte guard after the last: a fitting split leaves the rest of its slot and
the guard untouched.
"""
import numpy as np
import pytest

import lz4_cases as lc
from gpu_util import empty_device, from_device, launch_stream, to_device

POISON = 0xA5
GUARD = 256

pytestmark = [pytest.mark.gpu]

FLAGS = [pytest.param(0, id="batch"), pytest.param(1, id="serial")]


@pytest.fixture(scope="module")
def ctx(aqz):
    c = aqz.BloscContext(0, 0)
    yield c
    c.close()


def run_case(aqz, ctx, case, flags, stream):
    """One launch for the buffers of a case; a list of what differs."""
    name, n, accel, bufs = case
    nb = len(bufs)
    d_src = to_device(np.concatenate(bufs))
    d_comp = empty_device(nb * n + GUARD)
    d_comp.fill_(POISON)
    d_rows = empty_device(8 * nb)
    d_rows.fill_(POISON)
    ctx.debug_lz4_splits_device(d_src.data_ptr(), n, nb, accel, d_comp.data_ptr(),
                                d_rows.data_ptr(), stream, flags)
    rows = from_device(d_rows, np.uint32, (nb, 2))
    comp = from_device(d_comp, np.uint8, (-1,))
    bad = []
    if not (comp[nb * n:] == POISON).all():
        bad.append((name, "guard after the last slot written"))
    for k, (buf, (csize, block, need)) in enumerate(zip(bufs, lc.expected(aqz, case))):
        slot = comp[k * n:(k + 1) * n]
        if (int(rows[k, 0]), int(rows[k, 1])) != (csize, need):
            bad.append((name, k, "row", tuple(int(x) for x in rows[k]), (csize, need)))
            continue
        got = slot[:csize].tobytes()
        if got != block:
            at = next(i for i in range(csize) if got[i] != block[i])
            bad.append((name, k, "bytes differ from", at, got[at:at + 8].hex(),
                        block[at:at + 8].hex()))
        if csize:
            if not (slot[csize:] == POISON).all():
                bad.append((name, k, "slot written past csize",
                            csize + int(np.flatnonzero(slot[csize:] != POISON)[0])))
            try:
                ok = lc.decode(got)[0] == buf.tobytes()
            except (AssertionError, IndexError):
                ok = False
            if not ok:
                bad.append((name, k, "does not decode to the input"))
    return bad


def run_group(aqz, ctx, group, flags):
    stream = launch_stream()
    bad = []
    cases = lc.cases(group, aqz)
    for case in cases:
        bad += run_case(aqz, ctx, case, flags, stream)
    if bad:
        pytest.fail(f"{len(bad)} differences, the first:\n" + "\n".join(map(str, bad[:12])))
    return cases


@pytest.mark.parametrize("flags", FLAGS)
def test_small_and_end_of_input(aqz, ctx, flags):
    """Lengths 1..160: literals only below 13 bytes, every count of valid
    lanes in the last batch, matches that run into the last five bytes."""
    assert len(run_group(aqz, ctx, "small", flags)) == 480


@pytest.mark.parametrize("flags", FLAGS)
def test_in_batch_candidate(aqz, ctx, flags):
    """A hit inside a batch; a candidate that is another lane of the batch;
    only the lanes up to the hit store, the latest of a bucket winning."""
    run_group(aqz, ctx, "in_batch", flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_distance_rule(aqz, ctx, flags):
    """u32 table: a candidate further than 65,535 behind is turned down."""
    run_group(aqz, ctx, "distance", flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_backward_extension(aqz, ctx, flags):
    """Several 64-byte steps back; stops at candidate 0 and at the anchor."""
    run_group(aqz, ctx, "backward", flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_match_counter(aqz, ctx, flags):
    """Match lengths around the counter's 256-byte steps, offsets 1..300."""
    run_group(aqz, ctx, "counter", flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_length_bytes(aqz, ctx, flags):
    """Run lengths around one and 64 length bytes, and beyond 64."""
    run_group(aqz, ctx, "length", flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_capacity_boundary(aqz, ctx, flags):
    """need one below, at and one above the split size."""
    cases = run_group(aqz, ctx, "capacity", flags)
    assert "capacity-n32768-a1-m0p" in [c[0] for c in cases]


@pytest.mark.parametrize("flags", FLAGS)
def test_unaligned_slots(aqz, ctx, flags):
    """Odd split lengths: slots 1..4 start on odd addresses."""
    run_group(aqz, ctx, "unaligned", flags)


def test_errors(aqz, ctx):
    """Rejected before any launch: comp and rows stay poisoned."""
    d_src = to_device(np.zeros(1024, np.uint8))
    d_comp = empty_device(1024 + GUARD)
    d_comp.fill_(POISON)
    d_rows = empty_device(16)
    d_rows.fill_(POISON)
    ok = dict(src=d_src.data_ptr(), split_bytes=512, n_splits=2, comp=d_comp.data_ptr(),
              rows=d_rows.data_ptr(), flags=0)
    bad = [dict(flags=2), dict(flags=0x80000001), dict(split_bytes=0), dict(n_splits=0),
           dict(split_bytes=0x7E000001), dict(src=None), dict(comp=None), dict(rows=None)]
    for change in bad:
        a = dict(ok)
        a.update(change)
        with pytest.raises(aqz.AqzError) as e:
            ctx.debug_lz4_splits_device(a["src"], a["split_bytes"], a["n_splits"], 1, a["comp"],
                                        a["rows"], 0, a["flags"])
        assert e.value.status == 1, change
    rc = aqz.lib().aqz_debug_lz4_splits_device(None, ok["src"], 512, 2, 1, ok["comp"], ok["rows"],
                                               None, 0)
    assert rc == 1
    assert (from_device(d_comp, np.uint8, (-1,)) == POISON).all()
    assert (from_device(d_rows, np.uint8, (-1,)) == POISON).all()
    # and the accepted call does run
    ctx.debug_lz4_splits_device(ok["src"], 512, 2, 1, ok["comp"], ok["rows"], 0, 0)
    rows = from_device(d_rows, np.uint32, (2, 2))
    want = aqz.debug_lz4_block_host(np.zeros(512, np.uint8), 512, 1)
    assert [tuple(int(x) for x in r) for r in rows] == [(want[0], want[2])] * 2
