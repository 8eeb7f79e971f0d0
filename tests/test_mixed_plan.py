"""CPU: plan_pyramid_runs and plan_zrun (acquire-zarr_amd/csrc/ds_plan.cpp), the
plans behind aqz_ds_run_device_batch's mixed-pyramid route (kind 7).

tests/cpp/mixed_plan_probe.cpp links ds_plan.cpp alone and is built as a
stand-alone program with the host compiler under ASan + UBSan
(mixed_batch_cases.plan_probe).  The expectations are restated from the rule:
maximal stretches of one class cut into pieces of 2 (XYZ), 4 (XY) and 3 (Z)
levels; a Z-run unit is one plane group of 2^n_out planes by one span of
64 lanes x 2 vectors x 16 bytes, spans fastest, four waves a workgroup."""
import numpy as np
import pytest

import mixed_batch_cases as mc

Z4 = [(9, 5, 16 >> l) for l in range(5)]     # four Z levels
Z5 = [(9, 5, 32 >> l) for l in range(6)]     # five
FIRST, FIRST_N = mc.FIXED["volume2_cascade2"][0], mc.FIXED["volume2_cascade2"][1]

REFUSALS = {
    # BATCH_GEOMETRIES["3d_odd_stack"]: three planes in front of level 2
    "odd planes": mc.runs_request([(256, 128, 6), (128, 64, 3), (64, 32, 2)], 12),
    "odd planes at a Z-only level": mc.runs_request([(8, 8, 6), (8, 8, 3), (8, 8, 1)], 12),
    "stored plane": mc.runs_request(FIRST, FIRST_N, holds=(1,)),
    "stored plane at a Z-only level": mc.runs_request(mc.FIXED["z_then_xy"][0], 8, holds=(1,)),
    "frames off the multiple": mc.runs_request(FIRST, 6),
    "no frames": mc.runs_request(FIRST, 0),
    "classless level": mc.runs_request([(64, 32, 4), (32, 16, 2), (32, 16, 2)], 8),
    "one level": mc.runs_request([(64, 32, 4)], 8),
}
ACCEPTED = {
    "four Z levels cut 3 + 1": (mc.runs_request(Z4, 32), [("Z", 1, 3, 32), ("Z", 4, 1, 4)]),
    "five Z levels cut 3 + 2": (mc.runs_request(Z5, 32), [("Z", 1, 3, 32), ("Z", 4, 2, 4)]),
    # a plane held by an XY-only level is no concern of the pairing
    "plane bit on an XY level": (mc.runs_request(FIRST, FIRST_N, holds=(3,)),
                                 mc.FIXED["volume2_cascade2"][3]),
    "five XY levels cut 4 + 1 behind a Z level": (
        mc.runs_request([(96, 96, 2), (96, 96, 1), (48, 48, 1), (24, 24, 1), (12, 12, 1),
                         (6, 6, 1), (3, 3, 1)], 4),
        [("Z", 1, 1, 4), ("XY", 2, 4, 2), ("XY", 6, 1, 2)]),
    "three XYZ levels cut 2 + 1": (
        mc.runs_request([(64, 64, 8), (32, 32, 4), (16, 16, 2), (8, 8, 1), (4, 4, 1)], 8),
        [("XYZ", 1, 2, 8), ("XYZ", 3, 1, 2), ("XY", 4, 1, 1)]),
}


def zrun_request(dtype, method, elems, n_out, planes, extra=""):
    return f"zrun {mc.DTYPES.index(dtype)} {method} {elems} {n_out} {planes} {extra}".strip()


def fixed_zruns():
    """Every Z run of the fixed shapes: id -> (request, (bpp, elems, n_out, planes))."""
    req = {}
    for name, (geo, n, dtype, runs) in mc.FIXED.items():
        for i, (cls, first, k, frames) in enumerate(runs):
            if cls == "Z":
                w, h, _ = geo[first - 1]
                req[f"{name}/run{i}"] = (zrun_request(dtype, 1, w * h, k, frames),
                                         (np.dtype(dtype).itemsize, w * h, k, frames))
    return req


ZRUNS = fixed_zruns()
# u8 planes of one span: units = groups = planes / 2
LIMITS = {
    "units just below 2^31": (zrun_request(np.uint8, 1, 2048, 1, (1 << 32) - 4), True),
    "units at 2^31": (zrun_request(np.uint8, 1, 2049, 1, 1 << 31), False),
    "spans alone at 2^31": (zrun_request(np.uint8, 1, 1 << 42, 1, 2), False),
    "n_out 0": (zrun_request(np.uint8, 1, 64, 0, 8), False),
    "n_out 4": (zrun_request(np.uint8, 1, 64, 4, 16), False),
    "no planes": (zrun_request(np.uint8, 1, 64, 1, 0), False),
    "planes not a multiple of 2^n_out": (zrun_request(np.uint8, 1, 64, 3, 12), False),
    "planes a multiple of 2^n_out": (zrun_request(np.uint8, 1, 64, 3, 16), True),
    "source stride below a plane": (zrun_request(np.uint16, 1, 64, 1, 4, "sstride=63"), False),
    "level stride below a plane": (zrun_request(np.uint16, 1, 64, 1, 4, "ostride=63"), False),
    "strides above a plane": (zrun_request(np.uint16, 1, 64, 1, 4, "sstride=70 ostride=65"), True),
    "source off the element grid": (zrun_request(np.uint16, 1, 64, 1, 4, "soff=1"), False),
    "level off the element grid": (zrun_request(np.float64, 1, 64, 1, 4, "ooff=4"), False),
    "element-aligned at odd elements": (zrun_request(np.uint16, 1, 64, 1, 4, "soff=2 ooff=6"),
                                        True),
    "no elements": (zrun_request(np.uint8, 1, 0, 1, 4), False),
    "bad method": (zrun_request(np.uint8, 4, 64, 1, 4), False),
    "bad dtype": ("zrun 10 1 64 1 4", False),
}


@pytest.fixture(scope="module")
def answers():
    requests = sorted({mc.runs_request(g, n) for g, n, _, _ in mc.FIXED.values()} |
                      set(REFUSALS.values()) | {r for r, _ in ACCEPTED.values()} |
                      {r for r, _ in ZRUNS.values()} | {r for r, _ in LIMITS.values()})
    return dict(zip(requests, mc.plan_probe()(requests)))


@pytest.mark.parametrize("name", mc.FIXED_NAMES)
def test_fixed_shape_runs(answers, name):
    geo, n, _, runs = mc.FIXED[name]
    assert mc.runs_of(geo, n) == runs, "the table disagrees with the rule"
    assert mc.parse_runs(answers[mc.runs_request(geo, n)]) == runs


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(answers, name):
    line = answers[REFUSALS[name]]
    assert mc.parse_runs(line) is None, f"{name}: {line}"


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_cuts(answers, name):
    req, runs = ACCEPTED[name]
    assert mc.parse_runs(answers[req]) == runs


def test_zrun_lines_restate_the_unit_shape(answers):
    assert len(ZRUNS) == 9   # 1 + 2 + 1 + 1 + 1 + 1 + 1 + 1 over the fixed shapes
    for cid, (req, (bpp, elems, k, planes)) in ZRUNS.items():
        assert answers[req] != "invalid", cid
        rec = mc.parse_line(answers[req])
        groups, spans, grid = mc.zrun_shape(elems, bpp, k, planes)
        assert (rec["family"], rec["dtype"], rec["method"], rec["n_out"]) == ("zrun", bpp, 1, k)
        assert (rec["planes"], rec["elems"], rec["block"]) == (planes, elems, 256), cid
        assert (rec["groups"], rec["spans"], rec["grid"]) == (groups, spans, grid), cid


def test_named_zruns(answers):
    """851 u8 elements are one span with a 3-byte tail; 2049 bytes are two
    spans, the second without a vector; 2047 one; one u16 element one."""
    spans = {cid: mc.parse_line(answers[req])["spans"] for cid, (req, _) in ZRUNS.items()}
    assert spans["zrun3_zrun2_851/run0"] == 1 and spans["zrun3_zrun2_851/run1"] == 1
    assert (spans["span_plus_1/run0"], spans["span_minus_1/run0"]) == (2, 1)
    assert spans["one_element/run0"] == 1
    many = mc.parse_line(answers[ZRUNS["many_tiny_groups/run0"][0]])
    assert (many["groups"], many["grid"]) == (1024, 256)   # 2048 planes in pairs


@pytest.mark.parametrize("name", list(LIMITS))
def test_limits(answers, name):
    req, valid = LIMITS[name]
    assert (answers[req] != "invalid") == valid, f"{name}: {answers[req]}"
    if name == "units just below 2^31":
        rec = mc.parse_line(answers[req])
        assert rec["groups"] * rec["spans"] == (1 << 31) - 2 and rec["grid"] == 1 << 29
