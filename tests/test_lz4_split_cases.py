"""CPU: the inputs of tests/lz4_cases.py do what their names say.

tests/test_gpu_lz4_splits.py runs these cases through the wave-cooperative
encoder (lz4_split_kernel) and compares with the serial one
(csrc/lz4_block.hh).  A case only tests its hazard if the parse really goes
where the case was built to send it, so every condition is asserted here, on
the serial encoder's output alone (decoded), with no GPU: the first sequence
of an in-batch case, the rejected far candidate, the backward extension's
length and stop, the match lengths around the counter's 256-byte steps, the
length-byte edges and the capacity boundary.  Where liblz4 is loaded the
expected bytes are also LZ4_compress_fast's, as c-blosc would get them
(blosc_compress_ctx, zarr.common.cpp:106-137).
"""
import ctypes
import re

import numpy as np
import pytest

import lz4_cases as lc


@pytest.fixture(scope="module")
def lz4(aqz):
    """LZ4_compress_fast of the liblz4 the frame writer loaded, or None."""
    m = re.match(r"lz4 \S+ \(([^)]+)\)", aqz.blosc_codec_info())
    if not m:
        return None
    fn = ctypes.CDLL(m.group(1)).LZ4_compress_fast
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]

    def compress(data, cap, accel):
        dst = np.zeros(cap + 1, np.uint8)
        n = fn(data.ctypes.data, dst.ctypes.data, data.size, cap, accel)
        return n, dst[:n].tobytes()

    return compress


def check_expected(aqz, lz4, case):
    """What the GPU test compares against: decodes to the input where it
    fits, csize and need agree, and liblz4 says the same."""
    name, n, accel, bufs = case
    for k, (buf, (csize, block, need)) in enumerate(zip(bufs, lc.expected(aqz, case))):
        assert (csize != 0) == (need <= n), (name, k, csize, need)
        assert len(block) == csize
        if csize:
            assert lc.decode(block)[0] == buf.tobytes(), (name, k)
        if lz4 is not None:
            want_n, want = lz4(np.ascontiguousarray(buf), n, accel)
            assert (want_n, want) == (csize, block), (name, k, want_n, csize)


def parses(aqz, case):
    """Per buffer: (sequences of the serial encoder, trace events, far
    candidates); the trace must tell the same sequences."""
    name, n, accel, bufs = case
    out = []
    for k, buf in enumerate(bufs):
        seqs = lc.reference_parse(aqz, buf, accel)
        events, far = lc.trace(buf, accel)
        assert [(e["lit"], e["off"], e["ml"]) for e in events] == seqs[:-1], (name, k)
        out.append((seqs, events, far))
    return out


def by_name(cases):
    return {c[0]: c for c in cases}


def test_decoder_and_schedule():
    # token 0x17: one literal, match length 4 + 7 at offset 1; then five literals
    data, seqs = lc.decode(bytes([0x17, 65, 1, 0, 0x50, 1, 2, 3, 4, 5]))
    assert data == b"A" * 12 + bytes([1, 2, 3, 4, 5])
    assert seqs == [(1, 1, 11), (5, 0, 0)]
    # length bytes: 15 + 255 + 3 literals
    lit = bytes(range(256)) + bytes(17)
    data, seqs = lc.decode(bytes([0xF0, 255, 3]) + lit)
    assert data == lit and seqs == [(273, 0, 0)]
    s = lc.schedule(1, 1, 100)
    assert s[:4] == [1, 2, 3, 4] and s[65] == 66 and s[66] == 68 and s[72] == 80
    s = lc.schedule(1, 9, 700)
    assert s[:4] == [1, 2, 11, 20] and s[66] - s[65] == 10
    assert lc.lane_of(7) == (0, 7) and lc.lane_of(8) == (1, 0) and lc.lane_of(71) == (1, 63)
    assert lc.lane_of(72) == (2, 0)


def test_small_and_end_of_input(aqz, lz4):
    cases = lc.cases("small")
    assert len(cases) == 480
    assert sorted({c[1] for c in cases}) == list(range(1, 161))
    ends_at_limit = zero = 0
    for case in cases:
        name, n, accel, bufs = case
        assert len(bufs) == 11
        check_expected(aqz, lz4, case)
        zero += sum(1 for csize, _, _ in lc.expected(aqz, case) if csize == 0)
        for buf in bufs:
            seqs = lc.reference_parse(aqz, buf, accel)
            if n < lc.MIN_INPUT:
                assert seqs == [(n, 0, 0)], name
            starts = lc.match_starts(seqs)
            ends_at_limit += sum(1 for (lit, off, ml), at in zip(seqs, starts)
                                 if ml and at + ml == n - lc.LAST_LITERALS)
    assert ends_at_limit > 100 and zero > 100, (ends_at_limit, zero)


def test_in_batch_candidate(aqz, lz4):
    cases = by_name(lc.cases("in_batch"))
    for case in cases.values():
        check_expected(aqz, lz4, case)
    first = {name: parses(aqz, case)[0] for name, case in cases.items()}

    seqs, events, _ = first["inbatch-a"]
    assert seqs[0] == (40, 20, 16)
    # probe index 39 hits; its candidate, position 20, is probe 19 of the same batch
    assert (events[0]["probe"], events[0]["cand"], events[0]["back"]) == (39, 20, 0)
    assert lc.lane_of(39)[0] == lc.lane_of(19)[0] == 1

    for name in ("inbatch-b", "inbatch-b-reuse"):
        seqs, events, _ = first[name]
        assert seqs[0] == (35, 15, 31), name
        assert (events[0]["probe"], events[0]["cand"]) == (34, 20)
    # found again at 130: the bucket holds 35 (the hit), not 50 (a later lane)
    seqs, events, _ = first["inbatch-b-reuse"]
    assert (130, 95) in [(at, s[1]) for s, at in zip(seqs, lc.match_starts(seqs))]
    seqs, events, _ = first["inbatch-b-reuse-L72"]
    assert seqs[0] == (80, 14, 30)
    assert (events[0]["probe"], events[0]["cand"]) == (72, 66)
    assert (160, 80) in [(at, s[1]) for s, at in zip(seqs, lc.match_starts(seqs))]

    seen = set()
    for name, (seqs, events, _) in first.items():
        m = re.match(r"inbatch-(pair|short|a9)-L(\d+)-E(\d+)$", name)
        if not m:
            continue
        accel = cases[name][2]
        later, earlier = int(m.group(2)), int(m.group(3))
        s = lc.schedule(1, accel, cases[name][1])
        assert seqs[0][0] == s[later], (name, seqs[0])
        assert (events[0]["probe"], events[0]["cand"], events[0]["back"]) == (later, s[earlier], 0)
        assert lc.lane_of(later)[0] >= 1
        seen.add((accel, lc.lane_of(later), lc.lane_of(later)[0] == lc.lane_of(earlier)[0]))
    assert first["inbatch-short-L71-E30"][0][0] == (78, 47, 5)
    # first lane of the first batch, its last lane, first lane of the second;
    # candidate from the same batch and from the table
    assert {(1, (1, 0), False), (1, (1, 63), True), (1, (1, 63), False), (1, (2, 0), False)} <= seen
    assert any(a == 9 and same for a, _, same in seen)
    assert any(a == 9 and not same for a, _, same in seen)


def test_distance_rule(aqz, lz4):
    cases = by_name(lc.cases("distance"))
    for case in cases.values():
        check_expected(aqz, lz4, case)
    seqs, events, far = parses(aqz, cases["distance-rule"])[0]
    assert max(off for _, off, _ in seqs) <= lc.MAX_DISTANCE
    starts = lc.match_starts(seqs)
    for (lit, off, ml), at in zip(seqs, starts):
        assert not (ml and at < 70064 and at + ml > 70000), "70000..70063 must be literals"
    assert any(off == 200 for _, off, _ in seqs)
    # a probe inside the block at 70000 found the block at 16 in its bucket
    # and was turned down for the distance alone
    assert any(70000 <= p < 70064 and p - cand == 69984 for p, cand in far), far
    for name in ("distance-far-repeat-n65546", "distance-far-repeat-n65547"):
        for seqs, _, _ in parses(aqz, cases[name]):
            assert max(off for _, off, _ in seqs) <= lc.MAX_DISTANCE and len(seqs) > 100


def test_backward_extension(aqz, lz4):
    cases = by_name(lc.cases("backward"))
    for case in cases.values():
        check_expected(aqz, lz4, case)
    start = lc.backward_start()
    seqs, events, _ = parses(aqz, cases["backward-steps"])[0]
    assert seqs[0] == (start, 30000, 20000)
    # the probe that hit lay far past the start: two or more whole 64-byte steps
    assert events[0]["back"] >= 128 and events[0]["stop"] == "byte", events[0]
    for seqs, events, _ in parses(aqz, cases["backward-zero"]):
        starts = lc.match_starts(seqs)
        assert any(lit > 0 and ml and at - off == 0 for (lit, off, ml), at in zip(seqs, starts))
        assert any(e["stop"] == "zero" and e["back"] > 0 and e["lit"] > 0 for e in events)
    for name in ("backward-anchor", "backward-anchor-a5"):
        n_anchor = 0
        for seqs, events, _ in parses(aqz, cases[name]):
            hits = [e for e in events if e["probe"] is not None and e["lit"] == 0]
            assert all(e["stop"] == "anchor" and e["back"] > 0 for e in hits)
            n_anchor += len(hits)
        assert n_anchor > 0, name


def test_match_counter(aqz, lz4):
    cases = lc.cases("counter")
    assert [c[0] for c in cases] == [f"counter-o{o}" for o in lc.COUNTER_OFFSETS]
    for case, o in zip(cases, lc.COUNTER_OFFSETS):
        name, n, accel, bufs = case
        check_expected(aqz, lz4, case)
        found, to_limit = set(), 0
        for seqs, _, _ in parses(aqz, case):
            for (lit, off, ml), at in zip(seqs, lc.match_starts(seqs)):
                if off == o:
                    found.add(ml)
                    to_limit += at + ml == n - lc.LAST_LITERALS
        want = {4 + c for c in lc.COUNT_EDGES}
        assert want <= found, (name, sorted(want - found))
        assert to_limit >= 1, name


def test_length_bytes(aqz, lz4):
    (case,) = lc.cases("length")
    check_expected(aqz, lz4, case)
    all_seqs = [seqs for seqs, _, _ in parses(aqz, case)]
    for e, seqs in zip(lc.LENGTH_EDGES, all_seqs):
        assert seqs[0][0] == e and seqs[0][2] == 4 + e, (e, seqs[0])
        assert seqs[-1] == (e, 0, 0), (e, seqs[-1])
    # more 255s than the wave has lanes: (17000 - 15) // 255 = 66
    assert all_seqs[-1][0][:2] == (17000, 300), all_seqs[-1][0]
    assert 15 + 255 * 64 in lc.LENGTH_EDGES


def test_capacity_boundary(aqz, lz4):
    cases = lc.cases("capacity", aqz)
    names = [c[0] for c in cases]
    assert "capacity-n32768-a1-m0p" in names, names
    assert any(n.startswith("capacity-n70000-") for n in names), names
    assert any(n.startswith("capacity-n32768-a9-") for n in names), names
    for case in cases:
        name, n, accel, bufs = case
        check_expected(aqz, lz4, case)
        kinds = name.rsplit("-", 1)[1]
        assert len(kinds) == len(bufs)
        for kind, (csize, _, need) in zip(kinds, lc.expected(aqz, case)):
            assert need - n == "m0p".index(kind) - 1, (name, kind, need)
            assert csize == (0 if kind == "p" else n if kind == "0" else csize)
            if kind == "m":
                assert 0 < csize < n


def test_unaligned_slots(aqz, lz4):
    cases = lc.cases("unaligned")
    assert [c[1] for c in cases] == [13, 4097, 65547]
    for case in cases:
        assert len(case[3]) == 5 and case[1] % 2 == 1
        check_expected(aqz, lz4, case)
