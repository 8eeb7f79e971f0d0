"""CPU: every environment switch the native sources read has a parity rule in
tests/test_gpu_launch_rules.py, or is exempt here for a stated reason — so a
new launch switch cannot be added without a rule that runs it against the
oracle.  Also: the launch log of a fresh process is empty."""
import glob
import os
import re

import test_gpu_launch_rules as rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acquire-zarr_amd", "csrc")

# switches that select no kernel, or that other tests already run both ways
EXEMPT = {
    "AQZ_GPU_DEVICE": "device choice, not a launch rule (test_gpu_parity.py: "
                      "test_spread_device_policy, test_bad_device_ordinal_is_invalid_argument)",
    "AQZ_NODE_STAGE_MB": "staging size of the node path, covered by test_gpu_node_device.py",
    "AQZ_LZ4_LIB": "path of the host LZ4 library (blosc_frame.cpp), no kernel",
    "AQZ_ZSTD_LIB": "path of the host zstd library (blosc_frame.cpp), no kernel",
    "AQZ_PINNED_STAGING": "parametrised in test_gpu_parity.py::test_host_staging_modes",
    "AQZ_STREAM_TILE_PASS": "parametrised in test_gpu_parity.py "
                            "(test_take_frame_tiled, test_eager_tiling_follows_the_cached_frame)",
    "AQZ_EAGER_READBACK": "parametrised in test_gpu_parity.py::test_take_frame_tiled",
    "AQZ_LAUNCH_LOG": "the launch log itself; every rule runs with it on",
}


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))
    assert len(files) >= 8
    return {f: open(f).read() for f in files}


def test_every_switch_has_a_rule_or_a_reason():
    read_by_call, literals = set(), set()
    for text in sources().values():
        read_by_call |= set(re.findall(
            r"\b(?:getenv|int_env|env_flag|open_first)\(\s*\"(AQZ_[A-Z0-9_]+)\"", text))
        # any other helper that takes a switch name still names it in a string
        literals |= set(re.findall(r"\"(AQZ_[A-Z0-9_]+)\"", text))
    # the scan itself: the launchers alone read some thirty switches
    assert len(read_by_call) >= 30, sorted(read_by_call)
    assert {"AQZ_VOLUME_UPW", "AQZ_BAND_MIS_SEG", "AQZ_TILED_BAND_WG",
            "AQZ_BITSHUFFLE_WAVES", "AQZ_LAUNCH_LOG"} <= read_by_call
    known = set(rules.RULE_SWITCHES) | set(EXEMPT)
    missing = sorted((read_by_call | literals) - known)
    assert not missing, (f"{missing}: add a rule to tests/test_gpu_launch_rules.py "
                         "(or an EXEMPT reason here)")
    # no stale entries either: a rule or exemption for a switch nobody reads
    stale = sorted(known - (read_by_call | literals))
    assert not stale, f"{stale} are read nowhere in {CSRC}"
    assert not set(rules.RULE_SWITCHES) & set(EXEMPT)


def test_rule_table_is_well_formed():
    ids = [p.id for p in rules.RULES]
    assert len(ids) == len(set(ids))
    for p in rules.RULES:
        family, env, proofs = p.values
        assert family in rules.DEFAULT_PINS
        assert env and proofs
        for fields, case_ids in proofs:
            assert fields and case_ids
    # one switch at a time, except round 5's launch and the volume pairs
    multi = [p.id for p in rules.RULES if len(p.values[1]) > 1]
    assert len(multi) == 4, multi


def test_launch_log_of_a_fresh_process_is_empty(aqz):
    """aqz_debug_launch_log before any launch: status OK and no lines (no
    device call is made); a null buffer is an invalid argument."""
    assert aqz.debug_launch_log() == []
    assert aqz.lib().aqz_debug_launch_log(None, 0) == 1
