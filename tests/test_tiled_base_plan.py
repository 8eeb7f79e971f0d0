"""CPU: plan_cascade_tiled with a base level (acquire-zarr_amd/csrc/ds_plan.cpp),
the plan behind aqz_ds_run_device_batch_tiled_base / _chunked_base.

tests/cpp/tiled_base_plan_probe.cpp links ds_plan.cpp alone, is built as a
stand-alone program with the host compiler under ASan + UBSan
(tiled_base_cases.plan_probe), and prints the plan of the first fused run —
the one that writes level 0 — of every case tests/test_gpu_tiled_base.py runs
on the GPU.  A unit is 64 lanes x `cols` columns x 2^k rows for a run of k
levels; at level 0 it covers units_x * 64 * cols by units_y * 2^k pixels."""
import numpy as np
import pytest

import tiled_base_cases as tb


def all_cases():
    cases = [c for c, _ in tb.CASES]
    for dt in tb.DTYPES:
        cases.append(tb.case(f"sweep_{np.dtype(dt).name}", tb.SWEEP["w"], tb.SWEEP["h"],
                             tb.SWEEP["levels"], dt, [tb.SWEEP["tile"]]))
    for dt, w, _ in tb.COLS_CASES:
        cases.append(tb.case(f"cols_{np.dtype(dt).name}_{w}", w, tb.SWEEP["h"],
                             tb.SWEEP["levels"], dt, [tb.SWEEP["tile"]]))
    cases += [tb.fuzz_tiled_params(i) for i in range(tb.N_FUZZ_TILED)]
    cases += [tb.fuzz_chunked_params(i) for i in range(tb.N_FUZZ_CHUNKED)]
    return cases


ALL = all_cases()

U8 = "0 1 1024 2 1"  # u8 1024 x 2, one level: one unit a frame
LIMITS = {
    # (request, valid with the base, valid without)
    "units just below 2^30": (f"{U8} {(1 << 30) - 1} tiles=2x1024,1x512", True, True),
    "units at 2^30": (f"{U8} {1 << 30} tiles=2x1024,1x512", False, False),
    # the base under 4096-row tiles: 4094 zero-fill rows a frame, level 1 none
    "base zero-fill items below 2^32": (f"{U8} {1 << 20} tiles=4096x1024,1x512", True, True),
    "base zero-fill items past 2^32": (f"{U8} {1 << 21} tiles=4096x1024,1x512", False, True),
    "padded base width at 2^31": (f"{U8} 2 tiles=2x{1 << 31},1x512", False, True),
    "padded base height at 2^31": (f"{U8} 2 tiles={1 << 31}x1024,1x512", False, True),
    "padded base width just below 2^31": (f"{U8} 2 tiles=2x{(1 << 31) - 1},1x512", True, True),
    "zero base tile rows": (f"{U8} 2 tiles=0x1024,1x512", False, True),
    "zero base tile columns": (f"{U8} 2 tiles=2x0,1x512", False, True),
    "misaligned tile buffers": ("1 1 512 8 2 4 tiles=2x128 toff=1", False, False),
    "lattice stride of one base tile": ("1 1 512 8 2 4 tiles=4x128,1x64 stride=512", True, True),
    "lattice stride below one base tile": ("1 1 512 8 2 4 tiles=4x128,1x64 stride=511",
                                           False, True),
    "no frames": (f"{U8} 0 tiles=2x1024,1x512", False, False),
}

# format_plan(TiledPlan) of the parent commit for three launches without a
# base (made with that commit's ds_plan.cpp): the line a launch without a base
# must still print, byte for byte
PARENT_LINES = {
    "1 1 4096 4096 4 64 tiles=256x256 base=0":
        "family=tiled dtype=2 method=1 n_out=4 grid=32768 block=256 units=131072"
        " units_x=8 cols=8 nt=1 remap=0 seg_w=0 wpb=4 zwaves=0 nested=1 main_blocks=32768",
    "8 0 3000 3000 4 2 tiles=256x256 base=0":
        "family=tiled dtype=4 method=0 n_out=4 grid=1160 block=128 units=2256"
        " units_x=6 cols=8 nt=0 remap=0 seg_w=0 wpb=2 zwaves=64 nested=1 main_blocks=1128",
    "0 1 300 7 1 3 tiles=4x128 base=0":
        "family=tiled dtype=1 method=1 n_out=1 grid=6 block=128 units=12"
        " units_x=1 cols=8 nt=0 remap=0 seg_w=0 wpb=2 zwaves=0 nested=1 main_blocks=6",
}


@pytest.fixture(scope="module")
def lines():
    req = {tb.request(c) for c in ALL} | {tb.request(c, extra="base=0") for c in ALL}
    for r, _, _ in LIMITS.values():
        req |= {r, r + " base=0"}
    req |= set(PARENT_LINES)
    req = sorted(req)
    return dict(zip(req, tb.plan_probe()(req)))


def plan(lines, c, extra=""):
    rec = tb.parse_plan(lines[tb.request(c, extra=extra)])
    assert rec is not None, f"{c['name']}: invalid"
    return rec


def test_units_and_zero_fill_cover_the_padded_base_exactly_once(lines):
    """Replay one frame's zero-fill items of every level of the run, the base
    first, on a numpy count of the padded level: with the area the units
    reach, every padded element is written exactly once."""
    for c in ALL:
        rec = plan(lines, c)
        k = rec["n_out"]
        assert rec["base"] == 1 and rec["family"] == "tiled", c["name"]
        cols = rec["cols"]
        ux, uy = -(-c["w"] // (64 * cols)), -(-c["h"] // (1 << k))
        assert (rec["units_x"], rec["units"]) == (ux, ux * uy * c["n"]), c["name"]
        assert (rec["cov_w0"], rec["cov_h0"]) == (ux * 64 * cols, uy << k), c["name"]
        assert rec["cov_w0"] >= c["w"] and rec["cov_h0"] >= c["h"]
        assert rec["zitems"] == sum(rec[f"zrows{L}"] for L in range(1, k + 1)), c["name"]
        assert rec["base_slots"] == rec["slots0"] and rec["base_zrows"] == rec["zrows0"]
        lw, lh = c["w"], c["h"]
        for L in range(k + 1):
            tr, tc = c["tiles"][L]
            pw, ph = rec[f"pw{L}"], rec[f"ph{L}"]
            assert (pw, ph) == (-(-lw // tc) * tc, -(-lh // tr) * tr), (c["name"], L)
            cw, ch = min(rec[f"cov_w{L}"], pw), min(rec[f"cov_h{L}"], ph)
            count = np.zeros((ph, pw), np.int8)
            count[:ch, :cw] += 1
            for item in range(rec[f"zrows{L}"]):
                row = item if cw < pw else ch + item
                count[row, (0 if row >= ch else cw):] += 1
            assert (count == 1).all(), f"{c['name']} level {L}: {np.argwhere(count != 1)[:4]}"
            lw, lh = (lw + 1) // 2, (lh + 1) // 2


def test_named_shapes_reach_their_paths(lines):
    for c, want in tb.CASES:
        rec = plan(lines, c)
        got = tb.paths_of(rec)
        assert want <= got, f"{c['name']}: {got}"
    stale = plan(lines, tb.CASE["stale"])
    assert (stale["pw0"], stale["cov_w0"], stale["ph0"], stale["cov_h0"]) == (1088, 1536, 576, 528)
    a = plan(lines, tb.CASE["colfill_base"])
    assert (a["cov_w0"], a["pw0"], a["zrows0"], a["ph0"], a["zrows1"]) == (512, 600, 8, 8, 0)
    b = plan(lines, tb.CASE["colfill_level1"])
    assert (b["zrows0"], b["cov_w1"], b["pw1"], b["zrows1"]) == (0, 256, 300, 4)
    r = plan(lines, tb.CASE["rowfill"])
    assert (r["cov_h0"], r["ph0"], r["zrows0"], r["slots0"], r["clear0"]) == (40, 48, 8, 0, 1)
    for name, slots in tb.SLOT_CASES.items():
        rec = plan(lines, tb.CASE[name])
        assert max(rec["slots0"], 1) == slots and rec["clear0"] == (rec["slots0"] == 0), name
        assert rec["nested"] == (0 if "gen" in name or "none" in name else 1), name
    s = plan(lines, tb.CASE["slots_rowfill"])
    assert (s["cov_h0"], s["ph0"], s["slots0"], s["slots_x0"]) == (48, 64, 2, 1)
    for dt, w, cols in tb.COLS_CASES:
        c = next(c for c in ALL if c["name"] == f"cols_{np.dtype(dt).name}_{w}")
        assert plan(lines, c)["cols"] == cols, c["name"]


def test_the_fuzz_reaches_every_path_four_times(lines):
    count = dict.fromkeys(tb.PATHS, 0)
    modes = {0: 0, 1: 0}
    for i in range(tb.N_FUZZ_TILED):
        c = tb.fuzz_tiled_params(i)
        rec = plan(lines, c)
        for p in tb.paths_of(rec, c["flags"]):
            count[p] += 1
        modes[rec["nested"]] += 1
        for L, (tr, tc) in enumerate(c["tiles"]):
            lw, lh, _ = c["geo"][L]
            assert c["n"] * (-(-lh // tr) * tr) * (-(-lw // tc) * tc) * \
                np.dtype(c["dtype"]).itemsize <= tb.FUZZ_LEVEL_BYTES
    assert all(v >= 4 for v in count.values()), count
    assert modes[0] >= 4 and modes[1] >= 4, modes
    n_flags = sum(tb.fuzz_tiled_params(i)["flags"] for i in range(tb.N_FUZZ_TILED))
    assert tb.N_FUZZ_TILED // 2 < n_flags < tb.N_FUZZ_TILED


def test_a_plan_without_a_base_prints_the_line_it_always_did(lines):
    for req, want in PARENT_LINES.items():
        assert lines[req].startswith(want + " zitems="), req
    for c in ALL:
        with_base, without = lines[tb.request(c)], lines[tb.request(c, extra="base=0")]
        assert " base=" not in without, c["name"]
        rec, old = tb.parse_plan(with_base), tb.parse_plan(without)
        assert list(old)[:17] == ["family", "dtype", "method", "n_out", "grid", "block", "units",
                                  "units_x", "cols", "nt", "remap", "seg_w", "wpb", "zwaves",
                                  "nested", "main_blocks", "zitems"], c["name"]
        # the base changes the zero-fill waves and `nested` at the most, and
        # nothing of the levels
        for k, v in old.items():
            if k not in ("grid", "zwaves", "nested"):
                assert rec[k] == v, (c["name"], k)
        assert rec["grid"] - old["grid"] == (rec["zwaves"] - old["zwaves"]) // rec["wpb"]


@pytest.mark.parametrize("name", list(LIMITS))
def test_limits(lines, name):
    req, valid, valid_without = LIMITS[name]
    assert (lines[req] != "invalid") == valid, f"{name}: {lines[req]}"
    assert (lines[req + " base=0"] != "invalid") == valid_without, name
