"""Every A/B switch of the kernel launchers against the oracle, and the
scheme each fixed geometry takes under the default launch.

The library ships many kernel instantiations the default launch never
reaches, selected by the $AQZ_* switches that launch_cascade,
launch_cascade_tiled, launch_volume and launch_volume_tiled (planned in
csrc/ds_plan.cpp) and the blosc
filter dispatch (csrc/codec_kernels.hip) read.  Each is one default flip away
from being the product, so each rule of RULES below runs its family's case
list (tests/launch_rule_child.py: the smallest shapes at which each store
scheme triggers, four dtypes, four methods, poisoned outputs) and must match
the oracle byte for byte.  The switches are static locals, so every rule is
one child process (started, never exec'd), one at a time.

A rule that changed nothing proves nothing: the child runs with
AQZ_LAUNCH_LOG=1 and returns the launch log of every case, and each rule
names the log fields that must show its value on a named case.  The expected
values are derived from the launcher source, not from a run.

test_default_launch_* run the default launch the same way and pin the scheme
each named geometry of BATCH_GEOMETRIES (tests/test_gpu_parity.py) takes, so
that a threshold moving in the launcher cannot silently leave a scheme
without its fixed case.

Values outside what the launcher's comments document are not run;
AQZ_TILED_ZWAVES=0 is documented to leave the tile overhang unwritten.
tests/test_launch_rules_table.py (CPU) checks that every switch the sources
read is in RULES or exempt for a stated reason; tests/test_launch_plan.py
(CPU) asserts the pins and proofs below on the planner's own output.
"""
import json
import os
import re
import subprocess
import sys

import pytest

import volume_tiled_cases as vc
from test_gpu_divergent import ROUND5_LAUNCH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 240  # as tests/test_gpu_divergent.py


def rule(family, env, *proofs):
    """proofs: (fields that must all show on one launch line, case ids on at
    least one of which such a line must appear)."""
    rid = family + ":" + ",".join(f"{k}={v}" for k, v in env.items())
    return pytest.param(family, env, proofs, id=rid)


U16_2D = ["2d/uint16/m1/al"]                 # 1024 px: 2 tiles, aligned, plain cascade
I64_2D = ["2d/int64/m1/al"]                  # 1024 px: 8 narrow tiles, aligned, 4 levels
U16_STAGED = ["2d_band_staged/uint16/m1/al"]  # 1500 px: 3 tiles, misaligned, staged
F32_STAGED = ["2d_band_staged/float32/m1/al"]
U16_BAND8 = ["2d_band8_aligned/uint16/m1/al"]  # 4096 px: 8 tiles, aligned
U16_BAND6 = ["2d_band6_edge_rows/uint16/m1/al"]  # 3072 px: 6 tiles, aligned
U16_8TILE = ["2d_complete_8tile/uint16/m1/al"]  # 3900 px: 8 tiles, misaligned
U16_MISSEG = ["2d_mis_segments/uint16/m1/al"]  # 4700 px: 10 tiles, misaligned
F32_TILED = ["1000x600_float32_64x128/m1"]   # 2 wide tiles per band
U16_TILED_SPLIT = ["1500x90_uint16_64x128/m1"]  # 3000-B rows split 128-B lines, 3 tiles
U8_TILED_OVERHANG = ["600x40_uint8_256x1024/m1"]  # 2560 overhang rows
VOL_U16_DEC = ["3d_fused/uint16/m0"]         # 64 units, Decimate
VOL_U16_MEAN = ["3d_fused/uint16/m1"]
U8_VOLUME_TILED = vc.ZROWS_CASE_IDS[:1]     # 1030 x 37 u8, 8 x 64: rows past cov_h to zero
U16_VOLUME_TILED = vc.ZROWS_CASE_IDS[1:]    # 512 x 8 u16, 2 x 384: columns past cov_w to zero
U16_BITSHUFFLE = ["ts2_bs65536_n131072x4/bitshuffle"]
U8_BITSHUFFLE = ["ts1_bs4096_n20480x2/bitshuffle"]

RULES = [
    # ---- row-major cascade (launch_cascade, cascade_pick_cols).  First the
    # eight settings the round-6 fuzz runs had covered.
    rule("cascade", dict(ROUND5_LAUNCH),
         ({"family": "cascade", "upw": 2}, U16_2D), ({"cols": 4}, F32_STAGED)),
    rule("cascade", {"AQZ_CASCADE_NARROW": "1"}, ({"cols": 4}, F32_STAGED)),
    rule("cascade", {"AQZ_CASCADE_NARROW": "0"},
         ({"cols": 8}, ["2d_band8_aligned/float32/m1/al"])),
    rule("cascade", {"AQZ_BAND_STAGING": "0"}, ({"family": "cascade"}, U16_STAGED)),
    rule("cascade", {"AQZ_BAND_LAST": "2"}, ({"family": "band", "band_last": 2}, U16_STAGED)),
    rule("cascade", {"AQZ_UNITS_PER_WAVE": "4"}, ({"family": "cascade", "upw": 4}, U16_2D)),
    rule("cascade", {"AQZ_CASCADE_WAVES": "8"}, ({"family": "cascade", "block": 512}, U16_2D)),
    rule("cascade", {"AQZ_XCD_REMAP": "1"}, ({"family": "cascade", "remap": 1}, U16_2D)),
    rule("cascade", {"AQZ_BAND_LAST": "0"}, ({"family": "band", "band_last": 0}, U16_STAGED)),
    rule("cascade", {"AQZ_UNITS_PER_WAVE": "2"}, ({"family": "cascade", "upw": 2}, U16_2D)),
    rule("cascade", {"AQZ_UNITS_PER_WAVE": "8"}, ({"family": "cascade", "upw": 8}, U16_2D)),
    rule("cascade", {"AQZ_CASCADE_WAVES": "1"}, ({"family": "cascade", "block": 64}, U16_2D)),
    rule("cascade", {"AQZ_UNIT_ORDER": "1"}, ({"family": "cascade", "order": 1}, U16_2D)),
    rule("cascade", {"AQZ_UNIT_ORDER": "2"}, ({"family": "cascade", "order": 2}, U16_2D)),
    rule("cascade", {"AQZ_LOAD_NT": "0"}, ({"nt": 0}, U16_2D)),
    rule("cascade", {"AQZ_LOAD_NT": "1"}, ({"nt": 1}, U16_STAGED)),
    rule("cascade", {"AQZ_STORE_WB": "15"}, ({"family": "cascade", "wb": 15}, U16_2D)),
    rule("cascade", {"AQZ_SPLIT_LOADS": "1"}, ({"family": "band", "split": 1}, F32_STAGED)),
    rule("cascade", {"AQZ_BAND_ALIGNED": "0"}, ({"family": "cascade"}, U16_BAND6)),
    rule("cascade", {"AQZ_BAND_SEGMENTS": "0"},
         ({"family": "cascade"}, ["2d_band_segments/uint16/m1/al"])),
    rule("cascade", {"AQZ_BAND_SEG4": "0"},
         ({"family": "band", "seg_tiles": 0, "block": 512}, U16_BAND8)),
    rule("cascade", {"AQZ_BAND_SEG4": "1"}, ({"family": "band", "seg_tiles": 3}, U16_BAND6)),
    rule("cascade", {"AQZ_BAND_SEGN": "2"}, ({"family": "band", "seg_tiles": 2}, U16_BAND8)),
    rule("cascade", {"AQZ_BAND_FORCE": "15"}, ({"family": "band", "stage_mask": 15}, U16_2D)),
    rule("cascade", {"AQZ_BAND_MIS_MAX": "0"}, ({"family": "cascade"}, U16_STAGED)),
    rule("cascade", {"AQZ_BAND_MIS_MAX": "8"},
         ({"family": "band", "seg_tiles": 0, "band_last": 1, "block": 512}, U16_8TILE)),
    rule("cascade", {"AQZ_BAND_MIS_SEG": "0"}, ({"family": "cascade", "seg_w": 5}, U16_MISSEG)),
    rule("cascade", {"AQZ_BAND_MIS_SEG": "2"},
         ({"family": "band", "seg_rowwise": 1, "seg_tiles": 2}, U16_MISSEG)),
    rule("cascade", {"AQZ_BAND_WG": "0"}, ({"family": "cascade", "seg_w": 0}, U16_8TILE)),
    rule("cascade", {"AQZ_BAND_LDS_CAP": "32768"}, ({"family": "cascade"}, I64_2D)),
    # ---- chunk-tiled cascade (launch_cascade_tiled, cascade_tiled_cols)
    rule("tiled", {"AQZ_TILED_NARROW": "0"}, ({"cols": 4}, ["512x512_float64_3x5/m1"])),
    rule("tiled", {"AQZ_TILED_NARROW": "1"}, ({"cols": 4}, F32_TILED)),
    rule("tiled", {"AQZ_TILED_WAVES": "1"}, ({"wpb": 1, "block": 64}, F32_TILED)),
    rule("tiled", {"AQZ_TILED_WAVES": "3"}, ({"wpb": 3, "block": 192}, F32_TILED)),
    rule("tiled", {"AQZ_TILED_WAVES": "8"}, ({"wpb": 8, "block": 512}, F32_TILED)),
    rule("tiled", {"AQZ_TILED_BAND_WG": "1"}, ({"seg_w": 3, "wpb": 3}, U16_TILED_SPLIT)),
    rule("tiled", {"AQZ_TILED_ZROWS_PER_WAVE": "0"}, ({"zwaves": 64}, U8_TILED_OVERHANG)),
    rule("tiled", {"AQZ_TILED_ZROWS_PER_WAVE": "1"}, ({"zwaves": 240}, U16_TILED_SPLIT)),
    rule("tiled", {"AQZ_TILED_ZWAVES": "64"}, ({"zwaves": 64}, U8_TILED_OVERHANG)),
    rule("tiled", {"AQZ_XCD_REMAP": "1"}, ({"remap": 1}, F32_TILED)),
    rule("tiled", {"AQZ_LOAD_NT": "0"}, ({"nt": 0}, ["64x48_uint16_16x16/m1"])),
    # ---- fused volume (launch_volume).  Four units per wave exist only
    # with nontemporal loads: with AQZ_VOLUME_NT=0 the request is clamped to
    # two (until round 6 the grid was sized for four and the one-unit kernel
    # ran, leaving three quarters of the units unwritten).
    rule("volume", {"AQZ_VOLUME_NT": "0"}, ({"ntl": 0}, VOL_U16_MEAN)),
    rule("volume", {"AQZ_VOLUME_UPW": "1"}, ({"UPW": 1, "ntl": 1}, VOL_U16_DEC)),
    rule("volume", {"AQZ_VOLUME_UPW": "2"}, ({"UPW": 2, "ntl": 1}, VOL_U16_DEC)),
    rule("volume", {"AQZ_VOLUME_UPW": "4"}, ({"UPW": 4, "ntl": 1}, VOL_U16_DEC)),
    rule("volume", {"AQZ_VOLUME_UPW": "1", "AQZ_VOLUME_NT": "0"},
         ({"UPW": 1, "ntl": 0}, VOL_U16_DEC)),
    rule("volume", {"AQZ_VOLUME_UPW": "2", "AQZ_VOLUME_NT": "0"},
         ({"UPW": 2, "ntl": 0}, VOL_U16_DEC)),
    rule("volume", {"AQZ_VOLUME_UPW": "4", "AQZ_VOLUME_NT": "0"},
         ({"UPW": 2, "upw": 2, "ntl": 0}, VOL_U16_DEC)),
    rule("volume", {"AQZ_VOLUME_ZFAST": "0"},
         ({"zfast": 0}, ["3d_fused_many_groups/uint16/m0"])),
    rule("volume", {"AQZ_VOLUME_ZFAST": "1"}, ({"zfast": 1}, VOL_U16_DEC)),
    # ---- chunk-tiled volume (plan_volume_tiled): the zwaves of
    # volume_tiled_cases.ZROWS_PINS, worked by hand there
    rule("volume_tiled", {"AQZ_TILED_ZROWS_PER_WAVE": "0"},
         (vc.ZROWS_PINS[0][0], U8_VOLUME_TILED), (vc.ZROWS_PINS[0][1], U16_VOLUME_TILED)),
    rule("volume_tiled", {"AQZ_TILED_ZROWS_PER_WAVE": "1"},
         (vc.ZROWS_PINS[1][0], U8_VOLUME_TILED), (vc.ZROWS_PINS[1][1], U16_VOLUME_TILED)),
    # ---- blosc bit shuffle (filter_run)
    rule("codec", {"AQZ_BITSHUFFLE_WAVES": "1"}, ({"form": "vec", "waves": 1}, U16_BITSHUFFLE)),
    rule("codec", {"AQZ_BITSHUFFLE_WAVES": "2"}, ({"form": "vec", "waves": 2}, U16_BITSHUFFLE)),
    rule("codec", {"AQZ_BITSHUFFLE_WAVES": "4"}, ({"form": "vec", "waves": 4}, U8_BITSHUFFLE)),
    rule("codec", {"AQZ_BITSHUFFLE_BYTES": "1"}, ({"form": "bytes", "waves": 1}, U16_BITSHUFFLE)),
]

RULE_SWITCHES = sorted({k for p in RULES for k in p.values[1]})

# The scheme each fixed geometry takes under the default launch: what the
# comments of BATCH_GEOMETRIES claim, as the launcher source gives it.
# Tiles are 64 lanes x cols: u16 512 px; f32 512 px, or 256 px (cols 4) on
# rows of whole KiB (narrow_rows).
DEFAULT_PINS = {
    "cascade": [
        # 1500 px, 3 tiles, every level's rows split bursts: the whole band
        # staged, stored by its last wave
        ({"family": "band", "band_last": 1, "seg_tiles": 0, "seg_rowwise": 0, "block": 192},
         ["2d_band_staged/uint16/m1/al", "2d_band_staged/float32/m1/al"]),
        # 2600 px, 6 misaligned tiles: 2-byte tiles stage up to 6 (one
        # storing wave), 4-byte wide tiles only 4 and store directly from one
        # 6-wave workgroup per band
        ({"family": "band", "band_last": 1, "seg_tiles": 0, "block": 384},
         ["2d_wide_misaligned/uint16/m1/al"]),
        ({"family": "cascade", "seg_w": 6, "block": 384}, ["2d_wide_misaligned/float32/m1/al"]),
        # 4096 px aligned: u16 8 tiles, staged in 3-tile segments (2-byte
        # Mean); f32 16 narrow tiles, staged in 8-tile segments
        ({"family": "band", "stage_mask": 7, "band_last": 0, "seg_tiles": 3, "block": 192},
         ["2d_band8_aligned/uint16/m1/al"]),
        ({"family": "band", "stage_mask": 7, "band_last": 0, "seg_tiles": 8, "cols": 4},
         ["2d_band8_aligned/float32/m1/al"]),
        # 1024 px i64: 8 narrow tiles (128 px), four levels, staged in 4-tile
        # segments; the whole band's 43.5 KiB of LDS is what the rule's
        # condition weighs ($AQZ_BAND_LDS_CAP)
        ({"family": "band", "stage_mask": 15, "band_last": 0, "seg_tiles": 4, "cols": 2,
          "block": 256}, I64_2D),
        # 3072 px aligned: u16 6 tiles, the whole band staged behind a
        # barrier by a 6-wave workgroup; f32 12 narrow tiles in 8-tile segments
        ({"family": "band", "stage_mask": 7, "band_last": 0, "seg_tiles": 0, "block": 384},
         ["2d_band6_edge_rows/uint16/m1/al"]),
        ({"family": "band", "stage_mask": 7, "band_last": 0, "seg_tiles": 8, "cols": 4},
         ["2d_band6_edge_rows/float32/m1/al"]),
        # 8704 px aligned (u16 17 tiles, f32 34 narrow ones): 8-tile segments
        ({"family": "band", "seg_tiles": 8, "seg_rowwise": 0, "band_last": 0, "block": 512},
         ["2d_band_segments/uint16/m1/al"]),
        ({"family": "band", "seg_tiles": 8, "seg_rowwise": 0, "band_last": 0, "block": 512},
         ["2d_band_segments/float32/m1/al"]),
        # 4700 px, 10 misaligned tiles: balanced 4-tile segments, one LDS
        # slot per level row, stored by the last two waves (level 1 splits
        # bursts)
        ({"family": "band", "seg_rowwise": 1, "seg_tiles": 4, "band_last": 2, "block": 256},
         ["2d_mis_segments/uint16/m1/al"]),
        ({"family": "band", "seg_rowwise": 1, "seg_tiles": 4, "band_last": 2, "block": 256},
         ["2d_mis_segments/float32/m1/al"]),
        # 3900 px, 8 misaligned tiles: direct stores, one 8-wave workgroup per band
        ({"family": "cascade", "seg_w": 8, "block": 512}, ["2d_complete_8tile/uint16/m1/al"]),
        ({"family": "cascade", "seg_w": 8, "block": 512}, ["2d_complete_8tile/float32/m1/al"]),
        # 2570 px, 6 misaligned tiles, the last 10 px wide: staged whole for
        # u16 (<= 6 tiles), direct stores from a 6-wave workgroup for f32
        ({"family": "band", "band_last": 1, "seg_tiles": 0, "block": 384},
         ["2d_complete_short_last/uint16/m1/al"]),
        ({"family": "cascade", "seg_w": 6, "block": 384},
         ["2d_complete_short_last/float32/m1/al"]),
        # 512 px u8 Decimate: 1 KiB read per unit, four units per wave
        ({"family": "cascade", "upw": 4, "cols": 8}, ["2d_narrow/uint8/m0/al"]),
    ],
    "volume": [
        # 128 and 130 plane groups: plane groups fastest, two units per wave
        ({"zfast": 1, "UPW": 2, "ntl": 1}, ["3d_fused_many_groups/uint16/m0"]),
        ({"zfast": 1, "UPW": 2, "ntl": 1}, ["3d_fused_many_groups_edge/uint16/m0"]),
        ({"zfast": 1, "UPW": 2, "ntl": 1}, ["3d_fused_many_groups/float32/m0"]),
        # 2 plane groups: columns fastest; other methods one unit per wave
        ({"zfast": 0, "UPW": 2, "ntl": 1}, VOL_U16_DEC),
        ({"zfast": 0, "UPW": 1, "ntl": 1}, VOL_U16_MEAN),
    ],
    "tiled": [
        ({"cols": 8, "wpb": 2, "seg_w": 0, "remap": 0}, F32_TILED),
        ({"cols": 2}, ["512x512_float64_3x5/m1"]),
        ({"zwaves": 64, "seg_w": 0, "nt": 0}, U16_TILED_SPLIT),
        # 1-byte types: at most 32 overhang rows per zero-fill wave
        ({"zwaves": 80}, U8_TILED_OVERHANG),
    ],
    "volume_tiled": [
        # 1-byte types: 32 rows per wave, ceil(112 / 32) = 4 waves, so the 64
        # every launch has; the u16 case: the byte rule alone
        (vc.ZROWS_PINS[None][0], U8_VOLUME_TILED),
        (vc.ZROWS_PINS[None][1], U16_VOLUME_TILED),
    ],
    "codec": [
        ({"family": "bitshuffle", "form": "vec", "waves": 4}, U16_BITSHUFFLE),
        ({"family": "bitshuffle", "form": "vec", "waves": 1}, U8_BITSHUFFLE),
        ({"family": "bitshuffle", "form": "generic"}, ["ts3_bs3000_n9007x2/bitshuffle"]),
        ({"family": "shuffle", "form": "vec"}, ["ts2_bs65536_n131072x4/shuffle"]),
    ],
}

# Set once a child ends by signal, abort or timeout: every later rule then
# fails at once without starting a child, so the suite never goes on
# launching on a card a child has just faulted.
_LATCH = {"reason": None}


def run_rule(family, env_extra):
    if _LATCH["reason"]:
        pytest.fail(f"not started: an earlier launch-rule child {_LATCH['reason']}")
    env = {k: v for k, v in os.environ.items() if k not in RULE_SWITCHES}
    env.update(env_extra)
    env["AQZ_LAUNCH_LOG"] = "1"
    what = f"{family} {env_extra}"
    try:
        r = subprocess.run([sys.executable, "-u",
                            os.path.join(ROOT, "tests", "launch_rule_child.py"),
                            "--family", family], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _LATCH["reason"] = f"timed out ({what})"
        pytest.fail(_LATCH["reason"])
    if r.returncode < 0 or r.returncode in (134, 139):
        _LATCH["reason"] = f"ended with status {r.returncode} ({what})"
        pytest.fail(_LATCH["reason"] + "\n" + r.stdout[-1500:] + r.stderr[-1500:])
    dump = os.environ.get("AQZ_LAUNCH_RULES_DUMP")  # one-off runs: keep every child's lines
    if dump:
        name = re.sub(r"\W+", "_", what).strip("_")
        with open(os.path.join(dump, name + ".jsonl"), "w") as f:
            f.write(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"^TOTAL (\d+) differing", r.stdout, re.M)
    assert m, r.stdout[-2000:]
    cases = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert cases, "the child ran no case"
    short = [{k: v for k, v in c.items() if k != "launches"} for c in cases
             if c["differing"] or c["poison"] or c["stray"] or c["launch_errors"]
             or not c["launches"]]
    assert not short, f"{len(short)} of {len(cases)} cases: " + json.dumps(short[:8])
    assert int(m.group(1)) == 0
    return {c["case"]: c["launches"] for c in cases}


def assert_proofs(launches, proofs):
    for fields, case_ids in proofs:
        for cid in case_ids:
            assert cid in launches, f"no case {cid}"
        shown = [cid for cid in case_ids
                 if any(all(rec.get(k) == v for k, v in fields.items())
                        for rec in launches[cid])]
        assert shown, (f"{fields} on none of {case_ids}: " +
                       json.dumps({cid: launches[cid] for cid in case_ids}))


@pytest.mark.parametrize("family,env,proofs", RULES)
def test_launch_rule(family, env, proofs):
    """The family's cases are byte-exact under the rule, every output byte is
    written, every case launched, each launch's grid covers its units, and
    the rule's switch shows in the launch log."""
    assert_proofs(run_rule(family, env), proofs)


@pytest.mark.parametrize("family", sorted(DEFAULT_PINS))
def test_default_launch_schemes(family):
    """The default launch is exact on the same cases, and every pinned
    geometry takes the scheme it is in the suite for: on each listed case
    some launch shows all the pinned fields."""
    launches = run_rule(family, {})
    for fields, case_ids in DEFAULT_PINS[family]:
        for cid in case_ids:
            assert_proofs(launches, [(fields, [cid])])
