"""Inputs that steer the LZ4 split encoders down named paths (a plain helper,
shared by tests/test_lz4_split_cases.py on the CPU and
tests/test_gpu_lz4_splits.py on the GPU).

c-blosc hands every split to LZ4_compress_fast (blosc_compress_ctx, reached
from zarr.common.cpp:106-137); csrc/lz4_block.hh states that call serially and
lz4_split_kernel (csrc/codec_kernels.hip) restates it for a wave.  The kernel
has parts the serial statement lacks: a 64-wide probe batch behind eight serial
lead probes, an in-batch bucket conflict rule, a 256-byte match counter, a
64-byte backward extension and wave-wide length bytes.  Each builder below
makes inputs for one of them.

Three pieces:
  decode(block)           an LZ4 block decoder: (bytes, [(literals, offset,
                          match length)]), the last run as (literals, 0, 0);
  schedule(ip, accel, upto)  the probe positions of one search from `ip`;
  *_cases()               the case builders; a case is
                          (name, len, accel, [buffers of len bytes]).
trace(buf, accel) is the serial parse again in Python, kept only to say *why* a
sequence came out (which probe hit, how far it went back, whether the distance
rule turned a candidate down); test_lz4_split_cases.py holds it to the serial
encoder's own sequences.

Every seed is fixed.  The conditions a case must meet are asserted by
tests/test_lz4_split_cases.py on the serial encoder's output alone.

Capacity scans (capacity_cases) that found no input here: none; every scan
found need - len of -1, 0 and +1.
"""
import numpy as np

MIN_INPUT = 13      # lz4::kMinInput
MF_LIMIT = 11       # lz4::kMfLimit
LAST_LITERALS = 5   # lz4::kLastLiterals
U16_LIMIT = 65547   # lz4::kU16Limit
MAX_DISTANCE = 65535
SERIAL_LEAD = 8     # kSerialLead of codec_kernels.hip: probes before the first batch
BATCH = 64

LENGTH_EDGES = [14, 15, 16, 269, 270, 271, 16334, 16335, 16336]
COUNT_EDGES = [0, 3, 4, 251, 252, 253, 255, 256, 257, 511, 512, 513]
COUNTER_OFFSETS = [1, 2, 3, 4, 7, 300]


def bound(n):
    """A capacity every parse of n bytes fits into."""
    return n + n // 255 + 16


# ---- decoder ------------------------------------------------------------------

def decode(block):
    """The bytes an LZ4 block stands for and its sequences (literals, offset,
    match length); the closing literal run is (literals, 0, 0)."""
    b = bytes(block)
    out = bytearray()
    seqs = []
    i, n = 0, len(b)
    while True:
        token = b[i]
        i += 1
        lit = token >> 4
        if lit == 15:
            while True:
                x = b[i]
                i += 1
                lit += x
                if x != 255:
                    break
        assert i + lit <= n, "literals past the end of the block"
        out += b[i:i + lit]
        i += lit
        if i == n:
            seqs.append((lit, 0, 0))
            return bytes(out), seqs
        off = b[i] | (b[i + 1] << 8)
        i += 2
        assert 0 < off <= len(out), ("offset outside the output", off, len(out))
        ml = token & 15
        if ml == 15:
            while True:
                x = b[i]
                i += 1
                ml += x
                if x != 255:
                    break
        ml += 4
        start = len(out) - off
        if off >= ml:
            out += out[start:start + ml]
        else:
            pattern = bytes(out[start:])
            out += (pattern * (ml // off + 1))[:ml]
        seqs.append((lit, off, ml))


def match_starts(seqs):
    """Input position at which each sequence's match begins."""
    pos, starts = 0, []
    for lit, off, ml in seqs:
        pos += lit
        starts.append(pos)
        pos += ml
    return starts


# ---- probe schedule -----------------------------------------------------------

def schedule(ip, accel, upto):
    """Positions one search from `ip` probes, while they stay below `upto`:
    the first step is 1, then step = nb++ >> 6 with nb starting at accel << 6.
    Index 0..7 are the kernel's serial lead, 8..71 its first batch, 72..135
    the second."""
    out = []
    nxt, step, nb = ip, 1, accel << 6
    while nxt < upto:
        out.append(nxt)
        nxt += step
        step = nb >> 6
        nb += 1
    return out


def lane_of(index):
    """(batch number from 1, lane) of a probe index; batch 0 is the lead."""
    if index < SERIAL_LEAD:
        return 0, index
    return 1 + (index - SERIAL_LEAD) // BATCH, (index - SERIAL_LEAD) % BATCH


# ---- the serial parse, traced -------------------------------------------------

def _hash(b, p, u16):
    if u16:
        v = int.from_bytes(b[p:p + 4], "little")
        return ((v * 2654435761) & 0xFFFFFFFF) >> 19
    v = int.from_bytes(b[p:p + 8], "little")
    return ((((v << 24) & 0xFFFFFFFFFFFFFFFF) * 889523592379) & 0xFFFFFFFFFFFFFFFF) >> 52


def _common(a, x, y, limit):
    """Equal bytes of a[x...] and a[y...] (y < x) while x stays below limit."""
    total = 0
    while x + total < limit:
        step = min(4096, limit - x - total)
        ne = np.flatnonzero(a[x + total:x + total + step] != a[y + total:y + total + step])
        if ne.size:
            return total + int(ne[0])
        total += step
    return total


def trace(buf, accel):
    """csrc/lz4_block.hh's parse with its reasons.  Returns (events, far):
    one event per match, dict(lit, off, ml, probe, p, cand, back, stop) with
      probe  index of the probe that hit within its search, None for the test
             of ip right after a match (the immediate re-match);
      p, cand  where that probe hit, before the backward extension;
      back   bytes the backward extension took; stop: "anchor", "zero"
             (candidate position 0) or "byte";
    and `far`, the probes whose bucket held equal bytes further than 65,535
    behind (u32 table only)."""
    a = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    b = a.tobytes()
    n = a.size
    u16 = n < U16_LIMIT
    table = {}
    events, far = [], []
    if n < MIN_INPUT:
        return events, far
    mflimit1, matchlimit = n - MF_LIMIT, n - LAST_LITERALS
    anchor, ip = 0, 1

    def usable(cand, p):
        if b[cand:cand + 4] != b[p:p + 4]:
            return False
        if not u16 and cand + MAX_DISTANCE < p:
            far.append((p, cand))
            return False
        return True

    while True:
        nxt, step, nb = ip, 1, accel << 6
        g, found = 0, False
        while True:
            p = nxt
            nxt += step
            step = nb >> 6
            nb += 1
            if nxt > mflimit1:
                break
            h = _hash(b, p, u16)
            cand = table.get(h, 0)
            table[h] = p
            if usable(cand, p):
                found = True
                break
            g += 1
        if not found:
            break
        hit_p, hit_c, probe = p, cand, g
        while p > anchor and cand > 0 and b[p - 1] == b[cand - 1]:
            p -= 1
            cand -= 1
        stop = "anchor" if p == anchor else ("zero" if cand == 0 else "byte")
        lit = p - anchor
        while True:
            count = _common(a, p + 4, cand + 4, matchlimit)
            events.append(dict(lit=lit, off=p - cand, ml=4 + count, probe=probe, p=hit_p,
                               cand=hit_c, back=hit_p - p, stop=stop))
            anchor = ip = p + 4 + count
            if ip >= mflimit1:
                break
            table[_hash(b, ip - 2, u16)] = ip - 2
            h = _hash(b, ip, u16)
            cand = table.get(h, 0)
            table[h] = ip
            if not usable(cand, ip):
                break
            p, lit, probe, hit_p, hit_c, stop = ip, 0, None, ip, cand, "anchor"
        if ip >= mflimit1:
            break
        ip += 1
    return events, far


# ---- data kinds ---------------------------------------------------------------

def make_data(rng, kind, n):
    """tests/test_lz4_block.py's five adversarial kinds."""
    from test_lz4_block import make_data as md
    return md(rng, kind, n)


def _random(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def _sparse(rng, n):
    v = _random(rng, n)
    v[rng.integers(0, 16, n) != 0] = 0
    return v


def _planted_tail(rng, n):
    """Random bytes whose start recurs late enough that the match runs into
    the last five bytes (matches stop at n - 5)."""
    v = _random(rng, n)
    if n >= MIN_INPUT:
        a = n - 21 if n >= 37 else max(1, min(n // 2, n - 12))
        v[a:] = v[:n - a].copy()
    return v


# ---- cases --------------------------------------------------------------------

def small_cases():
    """Every length 1..160 at accelerations 1, 5, 9: below 13 bytes literals
    only; consecutive lengths give the last batch every count of valid lanes."""
    cases = []
    for accel in (1, 5, 9):
        for n in range(1, 161):
            rng = np.random.default_rng(1000 * accel + n)
            bufs = [_random(rng, n), np.zeros(n, np.uint8)]
            bufs += [(np.arange(n) % p).astype(np.uint8) for p in range(1, 8)]
            bufs += [_sparse(rng, n), _planted_tail(rng, n)]
            cases.append((f"small-n{n}-a{accel}", n, accel, bufs))
    return cases


def _pair(seed, n, later, earlier, third=None, again=None, size=16):
    """Random bytes with the `size` bytes at `earlier` planted at `later` (and at
    `third`, `again`), one after the other: where `later` is less than 16
    past `earlier` the next copy carries the overlap on, periodically."""
    v = _random(np.random.default_rng(seed), n)
    for at in (later, third, again):
        if at is not None:
            v[at:at + size] = v[earlier:earlier + size].copy()
    return v


def in_batch_cases():
    """A hit inside a 64-wide batch whose candidate is another lane of the
    same batch, or comes from the table (stored by the lead or by the batch
    before).  Names carry the probe indices: L later, E earlier position."""
    cases = [
        # (a): probe index 39 hits, its candidate is index 19 of the same batch
        ("inbatch-a", 200, 1, [_pair(11, 200, 40, 20)]),
        # (b): three lanes of one bucket; the first hit wins, the third must not store
        ("inbatch-b", 200, 1, [_pair(12, 200, 35, 20, 50)]),
        # (b) with the block once more, far on: the bucket must still hold 35, not 50
        ("inbatch-b-reuse", 200, 1, [_pair(13, 200, 35, 20, 50, 130)]),
    ]
    s1 = schedule(1, 1, 400)
    # later position: first lane of the first batch, its last lane, first lane of the second
    for later, earliers in ((8, [3]), (71, [30, 3]), (72, [40, 3])):
        for earlier in earliers:
            pl, pe = s1[later], s1[earlier]
            n = 200
            cases.append((f"inbatch-pair-L{later}-E{earlier}", n, 1,
                          [_pair(100 + later + earlier, n, pl, pe)]))
    # the last lane again with five bytes only: at step 2 no later probe can
    # find the pair and walk back to it
    cases.append(("inbatch-short-L71-E30", 200, 1, [_pair(15, 200, s1[71], s1[30], size=5)]))
    # (b)-reuse across two batches: earlier 66 is lane 57 of the first batch (from
    # the table), later 80 and third 94 are lanes 0 and 7 of the second; found
    # again at 160, the bucket must hold 80, not 94
    assert (s1[65], s1[72], s1[79]) == (66, 80, 94)
    cases.append(("inbatch-b-reuse-L72", 200, 1, [_pair(14, 200, 80, 66, 94, 160)]))
    s9 = schedule(1, 9, 1000)
    for later, earlier in ((39, 19), (39, 3), (71, 30), (72, 40)):
        cases.append((f"inbatch-a9-L{later}-E{earlier}", 1000, 9,
                      [_pair(300 + later + earlier, 1000, s9[later], s9[earlier])]))
    return cases


def distance_cases():
    """u32 table: a candidate 65,536 or more behind is turned down.  In
    "distance-rule" a block at 16 recurs at 70000 (too far: literals) and at
    70200 (offset 200).  By 70000 a search through random bytes steps 47 at a
    time, and no two of its probes lie 200 apart; a run of zeros up to 69990
    gives a match there, so the next search probes 69991..70056 one by one:
    every one of them finds the block at 16 in its bucket unless a later probe
    took it, and the probes into 70200.. find those positions."""
    n = 140000
    v = _random(np.random.default_rng(21), n)
    v[69800:69990] = 0
    block = v[16:80].copy()
    v[70000:70064] = block
    v[70200:70264] = block
    cases = [("distance-rule", n, 1, [v])]
    for m in (65546, 65547):
        rng = np.random.default_rng(22)
        cases.append((f"distance-far-repeat-n{m}", m, 1,
                      [make_data(rng, "far_repeat", m) for _ in range(2)]))
    return cases


def backward_start():
    """Where "backward-steps" plants its copy: one past the first probe whose
    successor is 66 or more bytes on (acceleration 9)."""
    s = schedule(1, 9, 170000)
    i = next(i for i in range(len(s) - 1) if s[i + 1] - s[i] >= 66)
    return s[i] + 1


def backward_cases():
    """The backward extension: two or more 64-byte steps, a stop at candidate
    position 0, a stop at the anchor."""
    n = 170000
    d = _random(np.random.default_rng(2), n)
    start = backward_start()
    d[start:start + 20000] = d[start - 30000:start - 10000].copy()
    cases = [("backward-steps", n, 9, [d])]
    # the buffer's first bytes recur where no probe lands: the probe after it
    # hits r bytes into the block and the extension walks back to position 0
    bufs = []
    s = schedule(1, 1, 4000)
    for seed, gap in ((31, 2), (32, 3), (33, 5), (34, 8)):
        v = _random(np.random.default_rng(seed), 4000)
        i = next(i for i in range(len(s) - 1) if s[i + 1] - s[i] >= gap)
        q = s[i] + 1
        v[q:q + 64] = v[0:64].copy()
        bufs.append(v)
    cases.append(("backward-zero", 4000, 1, bufs))
    # periodic data with noise: searches that hit past the anchor and walk back to it
    rng = np.random.default_rng(35)
    cases.append(("backward-anchor", 6000, 1, [make_data(rng, "periodic", 6000) for _ in range(4)]))
    cases.append(("backward-anchor-a5", 6000, 5,
                  [make_data(rng, "periodic", 6000) for _ in range(4)]))
    return cases


def _counter_buffers(rng, n, o, mls):
    """Buffers of n bytes holding, for every ml of `mls`, o fresh bytes
    repeated with period o for o + ml bytes and then one differing byte (a
    match of ml at offset o); the last buffer ends inside such a run."""
    bufs = []
    v, at = _random(rng, n), 8
    todo = list(mls)
    while todo:
        ml = todo[0]
        if at + o + ml + 9 > n - 64:
            bufs.append(v)
            v, at = _random(rng, n), 8
            continue
        todo.pop(0)
        unit = _random(rng, o)
        if o > 1 and len(set(unit.tolist())) < min(o, 4):
            unit = (np.arange(o) * 37 + 11).astype(np.uint8)
        run = np.resize(unit, o + ml)
        v[at:at + o + ml] = run
        v[at - 1] = unit[-1] ^ 0x5A                  # no backward extension before it
        v[at + o + ml] = unit[ml % o] ^ 0xFF         # the differing byte
        at += o + ml + 9
    # to the end of input: the count stops at matchlimit = n - 5
    unit = (np.arange(o) * 29 + 3).astype(np.uint8)
    v[at:] = np.resize(unit, n - at)
    v[at - 1] = unit[-1] ^ 0x5A
    bufs.append(v)
    return bufs


def counter_cases():
    """wave_count: match lengths that end on, just before and just after its
    256-byte steps, by a differing byte or at matchlimit, at offsets that
    overlap the match (1-3), equal a lane's word (4), and lie far back."""
    cases = []
    for o in COUNTER_OFFSETS:
        rng = np.random.default_rng(40 + o)
        cases.append((f"counter-o{o}", 4096, 1,
                      _counter_buffers(rng, 4096, o, [4 + c for c in COUNT_EDGES])))
    return cases


def _length_buffer(rng, n, lit, count, last):
    """`lit` random bytes, then those bytes again with period `lit` for a
    match of 4 + count, a run of one byte, and `last` random bytes."""
    v = _random(rng, n)
    ml = 4 + count
    v[lit:lit + ml] = np.resize(v[:lit].copy(), lit + ml)[lit:]
    v[lit + ml] = v[ml] ^ 0xFF
    run0 = lit + ml + 9
    fill = (int(v[run0 - 1]) + 77) & 0xFF
    v[run0:n - last] = fill
    v[n - last] = fill ^ 0xFF
    return v


def length_cases():
    """wave_put_length: literal runs before a match, match counts and last
    runs on both sides of one and of 64 length bytes (15 + 255 * 64 = 16335);
    and 17000 literals before a match, more 255s than the wave has lanes."""
    n = 60000
    rng = np.random.default_rng(50)
    bufs = [_length_buffer(rng, n, e, e, e) for e in LENGTH_EDGES]
    v = _random(rng, n)
    v[17000:] = np.resize(v[16700:17000].copy(), n - 16700)[300:]
    bufs.append(v)
    return [("length-bytes", n, 1, bufs)]


def _head_tail(seed, n, k):
    v = np.zeros(n, np.uint8)
    v[:k] = _random(np.random.default_rng(seed), k)
    return v


def capacity_scan(aqz, n, accel, seed, wanted=(-1, 0, 1)):
    """A random head of k bytes and zeros after, k scanned down from n: the
    inputs whose need (serial encoder, cap = n) is n + d for the d of
    `wanted`, as {d: buffer}."""
    found = {}
    for k in range(n, max(n - 600, 0), -1):
        v = _head_tail(seed, n, k)
        csize, _, need = aqz.debug_lz4_block_host(v, n, accel)
        d = need - n
        if d in wanted and d not in found:
            assert (csize != 0) == (d <= 0)
            found[d] = v
        if d < min(wanted) - 40 or len(found) == len(wanted):
            break
    return found


def capacity_cases(aqz):
    """The (csize, need) rows at the capacity a split has in a frame, its own
    size: need one below it, equal to it (csize == len, which c-blosc stores
    raw) and one above it (csize 0)."""
    cases = []
    for n, accel, seed in ((32768, 1, 61), (70000, 1, 62), (32768, 9, 63), (70000, 9, 64)):
        found = capacity_scan(aqz, n, accel, seed)
        if found:
            cases.append((f"capacity-n{n}-a{accel}-" + "".join("m0p"[d + 1] for d in sorted(found)),
                          n, accel, [found[d] for d in sorted(found)]))
    return cases


def unaligned_cases():
    """Five buffers of an odd length: slots 1..4 start on odd addresses."""
    cases = []
    for n in (13, 4097, 65547):
        rng = np.random.default_rng(70 + n % 97)
        bufs = [make_data(rng, kind, n) for kind in ("periodic", "sparse", "runs", "far_repeat")]
        bufs.insert(2, np.zeros(n, np.uint8))
        cases.append((f"unaligned-n{n}", n, 1, bufs))
    return cases


GROUPS = {
    "small": small_cases,
    "in_batch": in_batch_cases,
    "distance": distance_cases,
    "backward": backward_cases,
    "counter": counter_cases,
    "length": length_cases,
    "capacity": capacity_cases,
    "unaligned": unaligned_cases,
}

_BUILT = {}


def cases(group, aqz=None):
    """The cases of one group, built once a process."""
    if group not in _BUILT:
        fn = GROUPS[group]
        out = fn(aqz) if group == "capacity" else fn()
        for name, n, accel, bufs in out:
            for b in bufs:
                assert b.dtype == np.uint8 and b.shape == (n,), name
                b.setflags(write=False)
        _BUILT[group] = out
    return _BUILT[group]


_EXPECTED = {}


def expected(aqz, case):
    """Per buffer of a case: the serial encoder at cap = len, what a slot must
    hold: (csize, bytes, need)."""
    name, n, accel, bufs = case
    if name not in _EXPECTED:
        _EXPECTED[name] = [aqz.debug_lz4_block_host(b, n, accel) for b in bufs]
    return _EXPECTED[name]


def reference_parse(aqz, buf, accel):
    """The serial encoder's whole parse (cap = bound(len)), decoded."""
    n = buf.size
    csize, block, need = aqz.debug_lz4_block_host(buf, bound(n), accel)
    assert csize > 0 and need <= bound(n)
    data, seqs = decode(block)
    assert data == buf.tobytes()
    return seqs
