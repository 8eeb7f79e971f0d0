"""CPU: plan_volume_tiled (acquire-zarr_amd/csrc/ds_plan.cpp), the plan behind
aqz_ds_run_device_volume_tiled / _chunked.

tests/cpp/volume_tiled_plan_probe.cpp links ds_plan.cpp alone, is built as a
stand-alone program with the host compiler under ASan + UBSan
(volume_tiled_cases.plan_probe), and prints the
plan line of every fused run of the cases tests/test_gpu_volume_tiled.py runs
on the GPU.  The expectations here are restated from the kernel's unit shape:
a volume unit is 64 lanes x (16 / bytes per pixel) columns x 2^k rows x 2^k
planes for a run of k <= 2 levels."""
import numpy as np
import pytest

import volume_tiled_cases as vc

DTYPE_CODE = {"uint8": 0, "uint16": 1, "uint32": 2, "uint64": 3, "int8": 4, "int16": 5,
              "int32": 6, "int64": 7, "float32": 8, "float64": 9}
SWEEP = (520, 21, 4, 3, None, 6, 40, 2)  # the dtype and method sweep's shape


def runs(case):
    """(W, H, k, planes) of each fused run of up to two levels."""
    w, h, planes, levels, _, _, _, volumes = case
    out, n, L = [], planes * volumes, 1
    while L < levels:
        k = min(levels - L, 2)
        out.append((w, h, k, n))
        for _ in range(k):
            w, h = (w + 1) // 2, (h + 1) // 2
        n >>= k
        L += k
    return out


def request(dtype, w, h, k, n, tile, extra=""):
    return f"{DTYPE_CODE[np.dtype(dtype).name]} 1 {w} {h} {k} {n} tile={tile[0]}x{tile[1]} {extra}" \
        .strip()


def case_requests():
    req = {}
    cases = list(vc.CASES) + [SWEEP[:4] + (dt,) + SWEEP[5:] for dt in
                              (np.uint8, np.int16, np.uint32, np.int64, np.float32, np.float64)]
    cases += [c for c, _, _ in vc.BRANCH_CASES]
    for c in cases:
        for i, (w, h, k, n) in enumerate(runs(c)):
            req[f"{vc.case_id(c)}/run{i}"] = (request(c[4], w, h, k, n, (c[5], c[6])),
                                              (np.dtype(c[4]).itemsize, w, h, k, n, c[5], c[6]))
    return req


REQ = case_requests()

U8_1024 = "0 1 1024 4 1"  # one unit across, two down: units = 2 * groups
LIMITS = {
    "units just below 2^31": (f"{U8_1024} {(1 << 31) - 2} tile=2x512", True),
    "units at 2^31": (f"{U8_1024} {1 << 31} tile=2x512", False),
    # level 1 is 512 x 1 under 4096-row tiles: 4095 zero-fill rows a plane
    "zero-fill items below 2^32": (f"0 1 1024 2 1 {1 << 21} tile=4096x512", True),
    "zero-fill items past 2^32": (f"0 1 1024 2 1 {1 << 22} tile=4096x512", False),
    "padded width at 2^31": (f"0 1 1024 2 1 2 tile=1x{1 << 31}", False),
    "padded height at 2^31": (f"0 1 1024 2 1 2 tile={1 << 31}x1", False),
    "zero tile rows": ("1 1 512 8 2 4 tile=0x128", False),
    "zero tile columns": ("1 1 512 8 2 4 tile=2x0", False),
    "misaligned tile buffer": ("1 1 512 8 2 4 tile=2x128 toff=1", False),
    "aligned tile buffer at an odd pixel": ("1 1 512 8 2 4 tile=2x128 toff=2", True),
    "lattice stride of one tile": ("1 1 512 8 2 4 tile=2x128 stride=256", True),
    "lattice stride below one tile": ("1 1 512 8 2 4 tile=2x128 stride=255", False),
    "planes not a multiple of 2^k": ("1 1 512 8 2 6 tile=2x128", False),
    "no planes": ("1 1 512 8 2 0 tile=2x128", False),
    "three levels in one run": ("1 1 512 8 3 8 tile=2x128", False),
    "narrower than one vector load": ("1 1 7 8 1 2 tile=2x128", False),
    "bad method": ("1 9 512 8 2 4 tile=2x128", False),
    "no flags": ("1 1 512 8 2 4 tile=2x128 flags=0", True),
}


@pytest.fixture(scope="module")
def plans():
    requests = sorted({r for r, _ in REQ.values()} | {r for r, _ in LIMITS.values()} |
                      set(zero_fill_rule_requests().values()))
    return dict(zip(requests, vc.plan_probe()(requests)))


def test_every_run_of_the_gpu_cases_is_planned(plans):
    # five single runs, 2 + 1, 2 + 2, the sweep; the branch table's seven single runs and 3
    assert len(REQ) == 5 + 2 + 2 + 6 + 7 + 3
    for cid, (req, (bpp, w, h, k, n, tr, tc)) in REQ.items():
        rec = plans[req]
        assert rec is not None, f"{cid}: invalid"
        cols = 64 * (16 // bpp)  # a unit's columns at level 0
        ux, uy, groups = -(-w // cols), -(-h // (1 << k)), n >> k
        assert (rec["family"], rec["dtype"], rec["n_out"]) == ("volume_tiled", bpp, k), cid
        assert (rec["units_x"], rec["units_y"], rec["units"]) == (ux, uy, ux * uy * groups), cid
        assert rec["block"] == 64 * rec["wpb"]
        assert rec["main_blocks"] * rec["wpb"] >= rec["units"] > (rec["main_blocks"] - 1) * \
            rec["wpb"], cid
        assert rec["zwaves"] % (8 * rec["wpb"]) == 0
        assert rec["grid"] == rec["zwaves"] // rec["wpb"] + rec["main_blocks"], cid
        zitems = 0
        lw, lh = w, h
        for L in range(1, k + 1):
            lw, lh = (lw + 1) // 2, (lh + 1) // 2
            ntx, nty = -(-lw // tc), -(-lh // tr)
            got = tuple(rec[f"{f}{L}"] for f in ("ntx", "nty", "pw", "ph", "cov_w", "cov_h"))
            assert got == (ntx, nty, ntx * tc, nty * tr, ux * (cols >> L), uy * ((1 << k) >> L)), \
                f"{cid} level {L}: {got}"
            assert rec[f"clear{L}"] == 1
            zitems += rec[f"zrows{L}"] << (k - L)
        assert rec["zitems"] == zitems, cid
        assert (rec["zwaves"] > 0) == (zitems > 0), cid


def test_named_shapes_reach_their_paths(plans):
    """The first table case has interior units only (one across, two down)
    and nothing to zero-fill; the lone-edge case is one unit wide, past the
    frame's right-hand side."""
    a = plans[REQ[vc.case_id(vc.CASES[0]) + "/run0"][0]]
    assert (a["units_x"], a["units"], a["zitems"], a["zwaves"]) == (1, 2, 0, 0)
    assert (a["pw1"], a["ph1"], a["cov_w1"], a["cov_h1"]) == (256, 4, 256, 4)
    b = plans[REQ[vc.case_id(vc.CASES[1]) + "/run0"][0]]
    assert (b["units_x"], b["units_y"], b["units"]) == (1, 12, 24)  # two plane groups
    c = plans[REQ[vc.case_id(vc.CASES[2]) + "/run0"][0]]
    assert (c["units_x"], c["pw1"], c["ph1"]) == (2, 576, 24)  # 515 x 19 under 8 x 64 tiles
    d = plans[REQ[vc.case_id(vc.CASES[5]) + "/run1"][0]]
    assert (d["n_out"], d["units"]) == (1, 3)  # 66 x 6 x 2: the second run's source


def test_zero_fill_and_units_cover_the_padding_exactly_once(plans):
    """Replay the zero-fill items of one plane on a numpy count of the padded
    level: with the area the units reach, every padded element is written
    exactly once."""
    for cid, (req, (bpp, w, h, k, n, tr, tc)) in REQ.items():
        rec = plans[req]
        for L in range(1, k + 1):
            pw, ph = rec[f"pw{L}"], rec[f"ph{L}"]
            cw, ch = min(rec[f"cov_w{L}"], pw), min(rec[f"cov_h{L}"], ph)
            count = np.zeros((ph, pw), np.int32)
            count[:ch, :cw] += 1
            for item in range(rec[f"zrows{L}"]):
                row = item if cw < pw else ch + item
                count[row, (0 if row >= ch else cw):] += 1
            assert (count == 1).all(), f"{cid} level {L}: {np.argwhere(count != 1)[:4]}"
            assert rec[f"zrows{L}"] * pw >= pw * ph - cw * ch  # whole rows at the most


def zero_fill_rule_requests():
    """The launch-rule child's two cases under $AQZ_TILED_ZROWS_PER_WAVE unset,
    0 and 1."""
    req = {}
    for c in vc.ZROWS_CASES:
        (w, h, k, n), = runs(c)
        for zi in (None, 0, 1):
            req[(vc.case_id(c), zi)] = request(c[4], w, h, k, n, (c[5], c[6]),
                                               "" if zi is None else f"zi={zi}")
    return req


def test_branch_cases_zero_fill_as_their_table_says(plans):
    """The planner's own zrows on the column zero-fill shapes: every padded
    row where cov_w < pw, none where the units cover the level."""
    both = plans[REQ[vc.case_id(vc.BRANCH_CASES[0][0]) + "/run0"][0]]
    assert (both["cov_w1"], both["pw1"], both["zrows1"], both["ph1"]) == (256, 384, 4, 4)
    assert (both["cov_w2"], both["pw2"], both["zrows2"], both["ph2"]) == (128, 384, 2, 2)
    assert both["units"] == 4 and both["zitems"] == 4 * 2 + 2
    second = plans[REQ[vc.case_id(vc.BRANCH_CASES[1][0]) + "/run0"][0]]
    assert second["zrows1"] == 0 and second["cov_w1"] >= second["pw1"]
    assert (second["cov_w2"], second["pw2"], second["zrows2"]) == (128, 200, second["ph2"])
    deep = [plans[REQ[vc.case_id(vc.BRANCH_CASES[5][0]) + f"/run{i}"][0]] for i in range(3)]
    assert [d["n_out"] for d in deep] == [2, 2, 2]


def test_zero_fill_switch_pins_hold_on_the_plan(plans):
    """The zwaves tests/test_gpu_launch_rules.py pins for the volume_tiled
    family (volume_tiled_cases.ZROWS_PINS), on the planner's own output."""
    req = zero_fill_rule_requests()
    assert sorted(vc.ZROWS_PINS, key=str) == [0, 1, None]
    for zi, pins in vc.ZROWS_PINS.items():
        for c, fields in zip(vc.ZROWS_CASES, pins):
            rec = plans[req[(vc.case_id(c), zi)]]
            assert all(rec.get(k) == v for k, v in fields.items()), (zi, c, fields, rec)


@pytest.mark.parametrize("name", list(LIMITS))
def test_limits(plans, name):
    req, valid = LIMITS[name]
    rec = plans[req]
    assert (rec is not None) == valid, f"{name}: {rec}"
    if name == "no flags":
        assert rec["clear1"] == 0 and rec["clear2"] == 0
