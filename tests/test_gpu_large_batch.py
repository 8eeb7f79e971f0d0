"""GPU: batches past 4 GiB through every launch form of the device batch calls,
every frame of every level checked (tests/large_batch.py: the shift rule, the
case table, what each case crosses; tests/test_large_batch_cases.py shows all
of that on the CPU).

Geometries are BATCH_GEOMETRIES' and TILED_CASES' own, the suite's smallest
shape per launch scheme; only the frame count grows, to ceil(2^32 / frame
bytes) + 2 (deep cases: of level 1's frames), so that 32-bit frame offsets,
byte offsets and unit-to-frame decompositions that had only ever seen 24
frames run past 2^32 bytes, and for u8 and u16 past 2^32 and 2^31 elements:

* row-major batches (aqz_ds_run_device_batch, kind 1): 13 geometries x
  {u8, u16, f32} x {Decimate, Mean}, about 5.5 GiB each;
* fused volumes (kind 2), the same dtypes and methods, plane groups fastest
  for Decimate;
* four deep cases whose level 1 passes 2^32 bytes (fused cascade, the same at
  an odd width, volume, band spans), and the per-frame Z path (kind 0);
* a 7-pixel u8 row, which the fused cascade refuses (under one 8-byte load):
  every level is one batched xy_generic_kernel launch (kind 3, family=generic
  in the log), its thread index running over more than 2^32 level-1 outputs;
* chunk-tiled batches with zero-scan flags, tag 0 leaving whole zero tiles,
  and one chunk lattice whose level-1 capacity passes 2^32 bytes, its frame
  offsets from the oracle's addressing;
* the same two forms from the fused volume kernel (kind 5, family=volume_tiled
  in the log): row overhang and column zero-fill shapes past 2^32 input bytes,
  64 x 64 tiles whose level-1 output passes 2^32 bytes, and a Z/Y/X chunk
  lattice whose level-1 capacity does.

The batch is built on the device (frame k = base + k mod M), the library runs
once, and level L's frame k must equal E[L] + k mod M in bits, E from one
oracle run of the base.  Outputs are poisoned with 0xA5 and carry 64 poisoned
bytes behind them.  The cases of a group run in one child process
(tests/large_batch_child.py), which has the launch log on: each case asserts
last_batch_kind() and, where tests/test_gpu_launch_rules.py pins its scheme,
the launch-log form, so a case cannot quietly take another kernel.  A case
skips only when the device reports less free memory than need_bytes(case).
"""
import numpy as np
import pytest

import large_batch as lb
import test_gpu_launch_rules as rules

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.id for c in cases]


def pinned_fields(case):
    """The launch-log fields DEFAULT_PINS pins for this geometry, dtype and
    method (the pins do not depend on the frame count: ds_plan.cpp)."""
    cid = f"{case.name}/{np.dtype(case.dtype).name}/m{case.method}/al"
    return [fields for fields, ids in rules.DEFAULT_PINS["cascade"] if cid in ids]


def check_generic(rec, case):
    """Every level one batched single-level launch, none fused."""
    assert rec["kind"] == case.kind == 3
    fams = [r.get("family") for r in rec["launches"]]
    assert fams == ["generic"] * (len(case.geo) - 1), rec["launches"]
    assert all(r["dtype"] == lb.bpp(case) and r["method"] == case.method
               for r in rec["launches"])
    # a grid-stride loop: the grid is capped far under the 2^32 outputs
    n1 = lb.level_frames(case, 1) * lb.frame_elems(case, 1)
    assert n1 > 1 << 32 and rec["launches"][0]["grid"] * 256 < n1


def check_row(rec, case):
    if case.kind == 3:
        return check_generic(rec, case)
    assert rec["kind"] == case.kind == 1
    n = lb.frames_for(case)
    runs = [r for r in rec["launches"] if r.get("family") in ("cascade", "band")]
    assert runs, f"no cascade launch in the log: {rec['launches']}"
    # the first fused run's units are whole frames of this batch
    assert runs[0]["units"] % n == 0 and runs[0]["dtype"] == lb.bpp(case)
    for fields in pinned_fields(case):
        assert lb.shows(rec["launches"], fields), f"{fields} not in {rec['launches']}"


@pytest.mark.parametrize("cid", _ids(lb.select("row", "shallow")))
def test_row_major_batch(cid):
    check_row(lb.record_of("row", cid), lb.BY_ID[cid])


def test_pins_reach_the_large_cases():
    """The schemes with a pin are among the cases above."""
    pinned = [c.id for c in lb.select("row") if pinned_fields(c)]
    assert len(pinned) == 18 and "2d_narrow-uint8-m0" in pinned
    assert "deep-2d_band8_aligned-uint16-m1" in pinned


def check_volume(rec, case):
    assert rec["kind"] == 2
    groups = lb.frames_for(case) // lb.group_planes(case)
    assert groups >= 128
    # launch_volume: Decimate goes two units per wave and, from 128 plane
    # groups on, plane groups fastest; other methods one unit, columns fastest
    dec = case.method == 0
    want = {"family": "volume", "zfast": int(dec), "UPW": 2 if dec else 1, "ntl": 1}
    assert lb.shows(rec["launches"], want), f"{want} not in {rec['launches']}"
    vol = [r for r in rec["launches"] if r.get("family") == "volume"]
    assert vol[0]["units"] % groups == 0


@pytest.mark.parametrize("cid", _ids(lb.select("volume", "shallow")))
def test_volume_batch(cid):
    check_volume(lb.record_of("volume", cid), lb.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids(lb.select("row", "deep") + lb.select("volume", "deep")))
def test_deep_batch(cid):
    case = lb.BY_ID[cid]
    rec = lb.record_of("deep", cid)
    if case.family == "volume":
        check_volume(rec, case)
    else:
        check_row(rec, case)


@pytest.mark.parametrize("cid", _ids(lb.select("zpath")))
def test_per_frame_z_path(cid):
    case = lb.BY_ID[cid]
    rec = lb.record_of("deep", cid)
    assert rec["kind"] == case.kind == 0


@pytest.mark.parametrize("cid", _ids(lb.select("tiled")))
def test_tiled_batch(cid):
    case = lb.BY_ID[cid]
    rec = lb.record_of("tiled", cid)
    assert rec["kind"] == case.kind == 4
    tiled = [r for r in rec["launches"] if r.get("family") == "tiled"]
    assert tiled and tiled[0]["units"] % lb.frames_for(case) == 0
    assert tiled[0]["zwaves"] > 0       # these shapes have an overhang to zero-fill


@pytest.mark.parametrize("cid", _ids(lb.select("lattice")))
def test_chunk_lattice_batch(cid):
    case = lb.BY_ID[cid]
    rec = lb.record_of("tiled", cid)
    assert rec["kind"] == case.kind == 4
    tiled = [r for r in rec["launches"] if r.get("family") == "tiled"]
    assert tiled and tiled[0]["units"] % lb.frames_for(case) == 0
    assert tiled[0]["dtype"] == lb.bpp(case)


def check_volume_tiled(rec, case):
    """Kind 5 from the tiled volume kernel: family=volume_tiled in the log,
    zero-fill waves (every shape here has padding the units do not reach), and
    units in whole plane groups."""
    assert rec["kind"] == case.kind == 5
    groups = lb.frames_for(case) // lb.group_planes(case)
    runs = [r for r in rec["launches"] if r.get("family") == "volume_tiled"]
    assert len(runs) == 1 and len(rec["launches"]) == 1, rec["launches"]
    r = runs[0]
    assert r["dtype"] == lb.bpp(case) and r["method"] == case.method
    assert r["zwaves"] > 0 and r["zitems"] > 0
    assert r["units"] % groups == 0 and r["units"] // groups == r["units_x"] * r["units_y"]


@pytest.mark.parametrize("cid", _ids(lb.select("volume_tiled")))
def test_volume_tiled_batch(cid):
    check_volume_tiled(lb.record_of("volume_tiled", cid), lb.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids(lb.select("volume_lattice")))
def test_volume_lattice_batch(cid):
    check_volume_tiled(lb.record_of("volume_tiled", cid), lb.BY_ID[cid])
