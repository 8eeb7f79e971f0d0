"""CPU: the gather's case table and numpy model (tests/chunk_gather_cases.py).

The model must invert the oracle's forward placement on every case the GPU
tests run — else they would hold the kernels to a wrong statement — each case
must reach the kernel form it is named for, from geometry alone, and the fuzz
generator must reach every form.
"""
import collections

import numpy as np
import pytest

import chunk_gather_cases as cg


def model_of(src):
    return cg.gather_model(src.chunks, src.table, src.n_slots, src.base, src.internal, src.dtype,
                           src.w, src.h, src.tr, src.tc)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("case", cg.FIXED, ids=lambda c: c[0])
def test_model_inverts_the_forward_placement(oracle, case):
    name, w, h, tile, dtype, _ = case
    rng = np.random.default_rng(len(name) * 131 + w)
    frames = cg.random_bytes_frames(rng, dtype, (3, h, w))
    src = cg.Source(oracle, cg.tyx(w, h, tile, t_chunk=2), frames, 1)
    got, bad = model_of(src)
    assert bad == 0
    assert np.array_equal(bits(got), bits(frames))
    # the poison is there to be found: the chunks hold more than the frames
    ragged = w % tile[1] or h % tile[0]
    assert (src.chunks == cg.POISON).sum() >= (1 if ragged else 0)
    assert src.chunks.size > frames.nbytes  # frame 0's place, outside the batch


@pytest.mark.parametrize("i", range(cg.N_FUZZ))
def test_model_inverts_the_fuzz_cases(oracle, i):
    c = cg.fuzz_case(i)
    src = cg.fuzz_source(oracle, c)
    got, bad = model_of(src)
    assert bad == 0
    assert np.array_equal(bits(got), bits(src.frames)), c
    assert np.array_equal(bits(src.expected()), bits(src.frames))


def test_model_reads_absent_and_bad_slots_as_zeros(oracle):
    w, h, tile = 40, 9, (4, 8)
    frames = cg.random_bytes_frames(np.random.default_rng(3), np.uint16, (2, h, w)) | 1
    n_chunks = 2 * 3 * 5
    table = np.arange(n_chunks, dtype=np.uint32)
    table[[2, 17]] = cg.ABSENT
    src = cg.Source(oracle, cg.tyx(w, h, tile), frames, 0, table, n_chunks)
    got, bad = model_of(src)
    assert bad == 0 and src.bad() == 0
    want = src.expected()
    assert np.array_equal(got, want)
    assert not want[0, 0:4, 16:24].any() and not want[1, 0:4, 16:24].any()
    assert (got != frames).sum() == 2 * 4 * 8
    table[5] = n_chunks + 3
    src = cg.Source(oracle, cg.tyx(w, h, tile), frames, 0, table, n_chunks)
    got, bad = model_of(src)
    assert bad == 1 and src.bad() == 1
    assert np.array_equal(got, src.expected())
    assert not got[0, 4:8, 0:8].any()


@pytest.mark.parametrize("case", cg.FIXED, ids=lambda c: c[0])
def test_fixed_cases_reach_the_form_they_are_named_for(case):
    name, w, h, tile, dtype, want = case
    bpp = np.dtype(dtype).itemsize
    assert cg.form(w, tile[1], bpp) == want
    assert name.startswith(cg.log_form(want))
    # from first principles: does any aligned 16-byte vector of the frame hold
    # elements of two tile rows (another tile, or another frame row)?
    if tile[1] * bpp < 16:
        assert want == "elem"
        return
    px = np.arange(w * h)
    key = (px // w) * (w + 1) + (px % w) // tile[1]  # (row, tile column) of a pixel
    per = 16 // bpp
    whole = key[:len(px) // per * per].reshape(-1, per)
    straddles = bool((whole != whole[:, :1]).any())
    assert want == ("vec_straddle" if straddles else "vec")


def test_form_follows_the_destination_offset():
    assert cg.form(64, 16, 2) == "vec"
    assert cg.form(64, 16, 2, dst_off_bytes=2) == "vec_straddle"
    assert cg.form(64, 16, 2, dst_off_bytes=16) == "vec"
    assert cg.form(64, 7, 2) == "elem" and cg.form(64, 8, 2) == "vec"
    assert cg.form(1 << 30, 8, 2) == "elem"  # rows of 2^31 bytes


def test_fuzz_reaches_every_form_and_every_shape_of_batch():
    cases = [cg.fuzz_case(i) for i in range(cg.N_FUZZ)]
    forms = collections.Counter(c["form"] for c in cases)
    assert set(forms) == set(cg.FORMS)
    assert min(forms.values()) >= 4, forms
    assert {len(c["dims"]) for c in cases} == {3, 4, 5}
    assert {np.dtype(c["dtype"]).name for c in cases} == {np.dtype(d).name for d in cg.DTYPES}
    assert sum(c["permute"] for c in cases) == cg.N_FUZZ // 2
    assert max(c["n"] for c in cases) == 12 and max(c["w"] for c in cases) > 80
    larger = [c for c in cases if c["dims"][-1][2] > c["w"] and c["dims"][-2][2] > c["h"]]
    one_px = [c for c in cases if c["dims"][-1][2] == 1 or c["dims"][-2][2] == 1]
    assert larger and one_px
    assert cases == [cg.fuzz_case(i) for i in range(cg.N_FUZZ)]  # seeded
