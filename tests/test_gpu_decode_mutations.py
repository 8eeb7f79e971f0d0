"""GPU: the wave decoder (wave_decode_block, blosc_decode_kernel and the
unfilter it hands a header's blocksize to, csrc/codec_kernels.hip) against the
serial decoder of csrc/blosc_decode.hh on the mutation corpus of
tests/decode_mutation_cases.py: about 3,000 mutated blocks and about 24
mutants of every frame seed, split, filtered, multi-block and multi-wave
frames among them.

The expectation is the serial decoder's answer on the same bytes
(tests/test_decode_mutation_cases.py holds the corpus to its counts on the
CPU; tests/cpp/blosc_decode_sweep.cpp takes the same kinds of input under the
host sanitizers).  The aim is agreement, not a fault: every launch reads and
writes inside one allocation of the test's own,

    [M poison | inputs | M poison | outputs | M poison]

with M the margin decode_mutation_cases states, so whatever a missing check
could touch is owned, poisoned memory and shows as a failed assertion.  The
margins are compared on the device.  (The scratch a filtered frame decodes
into is the context's own and is not part of the layout.)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import decode_mutation_cases as dm
from gpu_util import empty_device, from_device, launch_stream, to_device, torch_cuda

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = dm.POISON
GAP = 37          # between block slots, as decode_blocks of test_gpu_blosc_decode.py
CHUNK_GAP = 61    # between chunks
NAMES = {0: "OK", 1: "ABSENT", 2: "BAD_HEADER", 3: "UNSUPPORTED", 4: "CORRUPT"}


@pytest.fixture(scope="module")
def ctx(aqz):
    c = aqz.BloscContext(0, 0)
    yield c
    c.close()


class Arena:
    """[M | inputs | M | outputs | M] in one device allocation, all poison but
    the inputs."""

    def __init__(self, margin, inputs, out_bytes):
        torch = torch_cuda()
        self.m, self.n_in, self.n_out = margin, len(inputs), out_bytes
        self.all = torch.full((3 * margin + self.n_in + out_bytes,), POISON, dtype=torch.uint8,
                              device="cuda")
        self.uploaded = to_device(inputs) if self.n_in else None
        if self.n_in:
            self.all[margin:margin + self.n_in] = self.uploaded
        self.in_ptr = self.all.data_ptr() + margin
        self.out0 = 2 * margin + self.n_in
        self.out_ptr = self.all.data_ptr() + self.out0

    def check_untouched(self, where):
        """The three margins still poison, the inputs still what was
        uploaded, compared on the device; returns the outputs."""
        torch = torch_cuda()
        torch.cuda.synchronize()
        a, m = self.all, self.m
        assert bool((a[:m] == POISON).all()), f"{where}: the margin before the inputs was written"
        assert bool((a[m + self.n_in:self.out0] == POISON).all()), \
            f"{where}: the margin between inputs and outputs was written"
        assert bool((a[self.out0 + self.n_out:] == POISON).all()), \
            f"{where}: the margin behind the outputs was written"
        if self.n_in:
            assert torch.equal(a[m:m + self.n_in], self.uploaded), f"{where}: the inputs changed"
        return a[self.out0:self.out0 + self.n_out].cpu().numpy()


def fail_with(bad, what):
    if bad:
        pytest.fail(f"{len(bad)} {what} differ from the serial decoder, the first:\n" +
                    "\n".join(map(str, bad[:12])))


# ---- blocks ---------------------------------------------------------------------

def decode_blocks(ctx, muts, margin):
    """One launch over `muts`: blocks packed byte-granular, slot k of cap +
    GAP bytes.  Returns (results, slots)."""
    nb = len(muts)
    comp = np.frombuffer(b"".join(m.block for m in muts), np.uint8)
    csize = np.array([len(m.block) for m in muts], np.uint32)
    coff = np.concatenate([[0], np.cumsum(csize[:-1], dtype=np.uint64)]).astype(np.uint64)
    slot = np.array([m.cap + GAP for m in muts], np.uint64)
    ooff = np.concatenate([[0], np.cumsum(slot[:-1], dtype=np.uint64)]).astype(np.uint64)
    arena = Arena(margin, comp, int(slot.sum()))
    d_csize, d_coff, d_ooff = (to_device(a) for a in (csize, coff, ooff))
    d_cap = to_device(np.array([m.cap for m in muts], np.uint32))
    d_res = empty_device(4 * nb)
    d_res.fill_(POISON)
    ctx.debug_lz4_decode_blocks_device(arena.in_ptr, d_coff.data_ptr(), d_csize.data_ptr(),
                                       arena.out_ptr, d_ooff.data_ptr(), d_cap.data_ptr(),
                                       d_res.data_ptr(), nb, launch_stream())
    out = arena.check_untouched(f"blocks {muts[0].name} .. {muts[-1].name}")
    res = from_device(d_res, np.int32, (nb,))
    return res, [out[int(ooff[k]):int(ooff[k] + slot[k])] for k in range(nb)]


def test_block_mutants_against_the_serial_decoder(aqz, ctx):
    """The whole block corpus in four launches: the exact result, negative
    codes included; the decoded bytes; poison behind the decoded size, or
    behind the capacity where the block is refused."""
    c = dm.corpus(aqz)
    muts, want = c["block_mutants"], dm.block_expectations(aqz)
    assert any(len(m.block) == 0 for m in muts) and any(m.cap == 0 for m in muts)
    bad = []
    part = -(-len(muts) // 4)
    for lo in range(0, len(muts), part):
        res, slots = decode_blocks(ctx, muts[lo:lo + part], c["M_blocks"])
        for k, m in enumerate(muts[lo:lo + part]):
            want_n, want_out = want[lo + k]
            got_n, slot = int(res[k]), slots[k]
            if got_n != want_n:
                bad.append((m.name, "result", got_n, "serial", want_n))
                continue
            if want_n >= 0:
                if not np.array_equal(slot[:want_n], want_out[:want_n]):
                    at = int(np.flatnonzero(slot[:want_n] != want_out[:want_n])[0])
                    bad.append((m.name, "bytes differ from", at, slot[at:at + 8].tobytes().hex(),
                                want_out[at:at + 8].tobytes().hex()))
                if not (slot[want_n:] == POISON).all():
                    bad.append((m.name, "written past the decoded size"))
            elif not (slot[m.cap:] == POISON).all():
                bad.append((m.name, "written past the capacity"))
    fail_with(bad, "block mutants")


# ---- frames, strided ------------------------------------------------------------

def check_chunks(aqz, names, status, chunks, nbytes, want, good_src, bad):
    """Statuses and bytes of one launch against the host path's."""
    for k, name in enumerate(names):
        want_st, want_out = want[k]
        got = int(status[k])
        chunk = chunks[k, :nbytes]
        if got != want_st:
            bad.append((name, "status", NAMES.get(got, got), "serial", NAMES[want_st]))
        elif want_st == dm.OK and not np.array_equal(chunk, want_out):
            at = int(np.flatnonzero(chunk != want_out)[0])
            bad.append((name, "bytes differ from", at))
        elif want_st == dm.ABSENT and chunk.any():
            bad.append((name, "an absent chunk is not zeros"))
        elif want_st in (dm.BAD_HEADER, dm.UNSUPPORTED) and not (chunk == POISON).all():
            bad.append((name, "a chunk refused by its header was written"))
        if name.endswith("good neighbour") and not (got == dm.OK and np.array_equal(chunk, good_src)):
            bad.append((name, "status", NAMES.get(got, got), "or bytes of a valid frame"))


@pytest.mark.parametrize("form", ["sizes", "header"])
def test_frame_mutants_strided(aqz, ctx, form):
    """One launch a seed: mutant, good seed, mutant, good seed ... at a
    byte-odd frame stride, chunks nbytes + 61 apart; extents from the uint32
    size table or from the headers."""
    c = dm.corpus(aqz)
    expect = dm.frame_expectations(aqz, form)
    margin = c["M_frames"]
    bad = []
    for seed, muts, exp in zip(c["frame_seeds"], c["frame_mutants"], expect):
        nbytes = len(seed.src)
        src = np.frombuffer(seed.src, np.uint8)
        stride = dm.frame_stride(seed, muts)
        assert stride % 2 == 1 and stride <= c["B_frames"]
        frames, names, want = [], [], []
        for m, e in zip(muts, exp):
            frames += [m.frame, seed.frame]
            names += [f"{m.name} [{form}]", f"{seed.name} after {m.kind}: good neighbour"]
            want += [e, (dm.OK, src)]
        n = len(frames)
        host = np.full(n * stride, POISON, np.uint8)
        for k, fr in enumerate(frames):
            host[k * stride:k * stride + len(fr)] = np.frombuffer(fr, np.uint8)
        dstride = nbytes + CHUNK_GAP
        arena = Arena(margin, host, n * dstride)
        d_sizes = to_device(np.array([len(f) for f in frames], np.uint32))
        d_st = empty_device(4 * n + 64)
        d_st.fill_(POISON)
        ctx.lz4_decompress_device(seed.ts, nbytes, arena.in_ptr, stride,
                                  d_sizes.data_ptr() if form == "sizes" else 0, n, arena.out_ptr,
                                  dstride, d_st.data_ptr(), launch_stream())
        out = arena.check_untouched(f"{seed.name} [{form}]")
        st = from_device(d_st, np.uint8, (-1,))
        assert (st[4 * n:] == POISON).all(), seed.name
        status = st[:4 * n].copy().view(np.uint32)
        chunks = out.reshape(n, dstride)
        assert (chunks[:, nbytes:] == POISON).all(), f"{seed.name}: bytes between the chunks written"
        check_chunks(aqz, names, status, chunks, nbytes, want, src, bad)
    fail_with(bad, "frames")


# ---- frames, through a shard ----------------------------------------------------

def test_frame_mutants_through_a_shard(aqz, ctx):
    """The mutants of three seeds (unsplit; split and byte-shuffled;
    multi-block and bit-shuffled with a leftover) packed end to end into one
    shard image, a sentinel pair every seventh slot, ten pairs 1 to 16 bytes
    short or long; the table at a non-zero base, 4 bytes off 8-byte
    alignment.  The image is decoded once with every seed's typesize and
    nbytes: a frame of another seed is then refused by its header."""
    c = dm.corpus(aqz)
    picked = [dm.seed_named(aqz, name) for name in dm.SHARD_SEEDS]
    frames, names = [], []
    for _, seed, muts in picked:
        frames += [seed.frame] + [m.frame for m in muts]
        names += [seed.name] + [m.name for m in muts]
    assert max(len(f) for f in frames) + 16 <= c["B_frames"]
    rng = dm.rng_of("shard-lengths")
    base = (1 << 40) + 12345
    image = bytearray(b"\xEE" * 3)
    pairs, slot_names, wrong = [], [], 0
    todo = list(zip(names, frames))
    while todo:
        if len(slot_names) % 7 == 6:
            pairs += [0xFFFFFFFFFFFFFFFF] * 2
            slot_names.append("sentinel")
            continue
        name, fr = todo.pop(0)
        length = len(fr)
        if len(todo) % 5 == 2 and wrong < 10:
            delta = int(rng.integers(1, 17)) * (1 if rng.integers(0, 2) else -1)
            length = max(length + delta, 0)
            name += f" length{delta:+d}"
            wrong += 1
        pairs += [base + len(image), length]
        slot_names.append(name)
        image += fr
    assert wrong == 10 and slot_names.count("sentinel") >= 10
    image += b"\xEE" * 16  # a pair 16 bytes long still ends inside the shard
    image = bytes(image)
    n = len(slot_names)
    table = np.array(pairs, np.uint64)
    d_tab = empty_device(table.nbytes + 4)
    d_tab[4:] = to_device(table)
    bad = []
    for _, seed, _ in picked:
        nbytes = len(seed.src)
        want = []
        for k in range(n):
            off, length = pairs[2 * k], pairs[2 * k + 1]
            if off == length == 0xFFFFFFFFFFFFFFFF:
                want.append((dm.ABSENT, None))
                continue
            assert off >= base and off - base + length <= len(image)  # span_shard's checks pass
            want.append(aqz.debug_blosc_decode_host(image[off - base:off - base + length], seed.ts,
                                                    nbytes))
        assert sum(st == dm.OK for st, _ in want) >= 3 and sum(st == dm.CORRUPT for st, _ in want) >= 3
        dstride = nbytes + CHUNK_GAP
        arena = Arena(c["M_frames"], np.frombuffer(image, np.uint8), n * dstride)
        d_st = empty_device(4 * n)
        d_st.fill_(POISON)
        ctx.zarr_shard_decompress_device(seed.ts, nbytes, arena.in_ptr, len(image), base,
                                         d_tab.data_ptr() + 4, n, arena.out_ptr, dstride,
                                         d_st.data_ptr(), launch_stream())
        out = arena.check_untouched(f"shard as {seed.name}")
        status = from_device(d_st, np.uint32, (n,))
        chunks = out.reshape(n, dstride)
        assert (chunks[:, nbytes:] == POISON).all(), f"{seed.name}: bytes between the chunks written"
        check_chunks(aqz, [f"{s} [shard as {seed.name}]" for s in slot_names], status, chunks,
                     nbytes, want, None, bad)
    fail_with(bad, "shard chunks")


# ---- blocksizes only a header names ---------------------------------------------

def test_header_named_blocksizes_decode(aqz, ctx):
    """The frames written from the format (blocksizes c-blosc would not
    choose: 1, 100, 1200, 2064, 4098, nbytes) decode OK to their sources: the
    blocksize goes from the header through `meta` into blosc_unfilter_kernel."""
    c = dm.corpus(aqz)
    seeds = [s for s in c["frame_seeds"] if s.written]
    assert len(seeds) >= 24
    bad = []
    for seed in seeds:
        n = len(seed.src)
        d_fr = to_device(np.frombuffer(seed.frame, np.uint8))
        d_dst = empty_device(n + 256)
        d_dst.fill_(POISON)
        d_st = empty_device(4)
        d_st.fill_(POISON)
        ctx.lz4_decompress_device(seed.ts, n, d_fr.data_ptr(), len(seed.frame), 0, 1,
                                  d_dst.data_ptr(), n, d_st.data_ptr(), launch_stream())
        status = int(from_device(d_st, np.uint32, (1,))[0])
        got = from_device(d_dst, np.uint8, (-1,))
        if status != dm.OK or got[:n].tobytes() != seed.src or not (got[n:] == POISON).all():
            bad.append((seed.name, NAMES.get(status, status)))
    fail_with(bad, "written frames")


def test_header_named_blocksizes_launch_log(aqz):
    """In a fresh process: typesize 4 with blocksize 4098 goes through the
    vector unfilter, typesize 3 with blocksize 1200 through the generic one,
    both with the blocksize per frame (per_frame=1)."""
    env = dict(os.environ)
    env["AQZ_LAUNCH_LOG"] = "1"
    r = subprocess.run([sys.executable, "-u",
                        os.path.join(ROOT, "tests", "decode_mutation_launch_child.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    runs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [x["name"] for x in runs] == dm.LAUNCH_LOG_SEEDS
    for x, (ts, form) in zip(runs, ((4, "vec"), (3, "generic"))):
        assert x["status"] == dm.OK and x["equal"], x
        dec = [rec for rec in x["launches"] if rec.get("family") == "blosc_decode"]
        unf = [rec for rec in x["launches"] if rec.get("family") == "unfilter"]
        assert len(dec) == 1 and len(unf) == 1, x["launches"]
        assert dec[0]["dtype"] == ts and dec[0]["waves"] == 1 and dec[0]["shard"] == 0
        assert unf[0]["dtype"] == ts and unf[0]["form"] == form and unf[0]["per_frame"] == 1
