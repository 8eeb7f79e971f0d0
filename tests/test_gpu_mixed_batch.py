"""GPU: aqz_ds_run_device_batch on mixed pyramids — levels that halve XY and
Z, XY alone or Z alone in any order — as a chain of batched runs on the
caller's stream (aqz_ds_last_batch_kind 7): fused volume, fused cascade (or
batched single-level XY kernels) and the Z-run kernel.

Expected values are oracle.OracleDownsampler's, streaming the same frames:
integers bit for bit, floats bit for bit NaN payloads included.  Every batch
runs into poisoned outputs with 64 guard bytes on both sides."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import float_cases as fc
import mixed_batch_cases as mc
from gpu_util import random_frames, torch_cuda
from test_gpu_float_classes import assert_bits, edge_stack
from test_gpu_parity import BATCH_GEOMETRIES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WANT = {}


def name_of(dtype):
    return np.dtype(dtype).name


def fixed_case(oracle, name, dtype=None, method=mc.MEAN):
    """(geo, n, dtype, frames, oracle levels) of a fixed shape: one oracle run
    per (shape, dtype, method), shared and left unchanged."""
    geo, n, dt, _ = mc.FIXED[name]
    dtype = dt if dtype is None else dtype
    key = (name, name_of(dtype), method)
    if key not in _WANT:
        frames = mc.fixed_frames(name, dtype)
        want = mc.oracle_levels(oracle, geo, dtype, method, frames)
        for a in [frames] + want[1:]:
            a.setflags(write=False)
        _WANT[key] = (frames, want)
    return (geo, n, dtype) + _WANT[key]


def run_checked(aqz, geo, dtype, method, frames, want, kind, ctx, offs=None, force=False):
    """One batch on a fresh handle into poisoned buffers: kind, counts, bytes."""
    counts = [len(frames)] + [len(w) for w in want[1:]]
    b = mc.Batch(geo, dtype, frames, counts, offs)
    ds = aqz.Downsampler(geo, dtype, method)
    try:
        if force:
            ds.debug_force_per_frame_batch(1)
        got_counts = b.run(ds)
        torch_cuda().cuda.synchronize()
        assert ds.last_batch_kind() == kind, f"{ctx}: kind {ds.last_batch_kind()}"
    finally:
        ds.close()
    assert got_counts == counts, f"{ctx}: counts {got_counts}"
    return b.check(want, ctx)


@pytest.mark.parametrize("name", mc.FIXED_NAMES)
def test_fixed_shapes(aqz, oracle, name):
    geo, n, dtype, frames, want = fixed_case(oracle, name)
    assert [len(w) for w in want[1:]] == mc.emitted(geo, n)[1:]
    run_checked(aqz, geo, dtype, mc.MEAN, frames, want, 7, name)


@pytest.mark.parametrize("name", mc.FIXED_NAMES)
def test_same_bytes_as_the_per_frame_route(aqz, oracle, name):
    """A second handle with the batched routes off: kind 0, the same counts and
    bytes (both compared with the oracle's, and with each other)."""
    geo, n, dtype, frames, want = fixed_case(oracle, name)
    fused = run_checked(aqz, geo, dtype, mc.MEAN, frames, want, 7, f"{name} fused")
    per_frame = run_checked(aqz, geo, dtype, mc.MEAN, frames, want, 0, f"{name} per frame",
                            force=True)
    for L in range(1, len(geo)):
        assert fused[L].tobytes() == per_frame[L].tobytes(), f"{name} L{L}"


@pytest.mark.parametrize("method", mc.METHODS)
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=name_of)
@pytest.mark.parametrize("name", mc.SWEEP_SHAPES)
def test_every_dtype_and_method(aqz, oracle, name, dtype, method):
    geo, n, dtype, frames, want = fixed_case(oracle, name, dtype, method)
    run_checked(aqz, geo, dtype, method, frames, want, 7, f"{name} {name_of(dtype)} m{method}")


@pytest.mark.parametrize("off", range(1, 8))
@pytest.mark.parametrize("name", mc.OFFSET_SHAPES)
def test_element_offsets(aqz, oracle, name, off):
    """The input `off` elements off its buffer's start, every level at an
    offset of its own (1-7 elements, in turn)."""
    geo, n, dtype, frames, want = fixed_case(oracle, name)
    offs = [off] + [1 + (off + L) % 7 for L in range(1, len(geo))]
    run_checked(aqz, geo, dtype, mc.MEAN, frames, want, 7, f"{name} offsets {offs}", offs=offs)


@pytest.mark.parametrize("method", mc.METHODS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=name_of)
@pytest.mark.parametrize("name", mc.FLOAT_SHAPES)
def test_float_classes(aqz, oracle, name, dtype, method):
    """Stacks built from float_cases: every planted class of every level, bit
    for bit.  851 elements a plane end each plane in a partial wave (f32: 212
    whole vectors and three elements; f64: 425 and one)."""
    geo, n, _, _ = mc.FIXED[name]
    frames = edge_stack(dtype, geo, n)
    want = mc.oracle_levels(oracle, geo, dtype, method, frames)
    ctx = f"{name} {name_of(dtype)} m{method}"
    got = run_checked(aqz, geo, dtype, method, frames, want, 7, ctx)
    for L in range(1, len(geo)):
        assert_bits(got[L], want[L], dtype, geo, n, method, L, ctx)
    # the Z-only levels carry Z-pair windows of the method's classes
    last = len(geo) - 1
    assert fc.claimed(dtype, geo, method, last), "nothing planted at the last level"


def test_state_after_a_mixed_batch(aqz, oracle):
    """A kind-7 batch, one more stack streamed through add_frame / take_frame
    on the same handle, then a second kind-7 batch: the oracle fed the same
    frames in the same order gives every level of all three."""
    name = "volume1_zrun3"
    geo, n, dtype, _ = mc.FIXED[name]
    rng = np.random.default_rng(7)
    stack = geo[0][2]
    first, streamed, second = (random_frames(rng, dtype, (k, geo[0][1], geo[0][0]))
                               for k in (n, stack, n))
    ref = oracle.OracleDownsampler(geo, dtype, mc.MEAN)
    wants = [mc.oracle_levels(oracle, geo, dtype, mc.MEAN, f, ref=ref)
             for f in (first, streamed, second)]
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        counts = [n] + [len(w) for w in wants[0][1:]]
        a = mc.Batch(geo, dtype, first, counts)
        assert a.run(ds) == counts and ds.last_batch_kind() == 7
        a.check(wants[0], "first batch")
        got = [[] for _ in geo]
        for fr in streamed:
            ds.add_frame(fr)
            for L in range(1, len(geo)):
                p = ds.take_frame(L)
                if p is not None:
                    got[L].append(p)
        for L in range(1, len(geo)):
            assert len(got[L]) == len(wants[1][L]), f"streamed L{L}: {len(got[L])} frames"
            mc.assert_parity(np.stack(got[L]), wants[1][L], f"streamed L{L}")
        b = mc.Batch(geo, dtype, second, counts)
        assert b.run(ds) == counts and ds.last_batch_kind() == 7
        b.check(wants[2], "second batch")
    finally:
        ds.close()


def test_refused_batches_keep_the_per_frame_route(aqz, oracle):
    """An odd plane count, n_frames off the multiple and a stored plane: kind
    0, the oracle's bytes."""
    geo, n, _ = BATCH_GEOMETRIES["3d_odd_stack"]
    frames = random_frames(np.random.default_rng(1), np.uint16, (n, geo[0][1], geo[0][0]))
    want = mc.oracle_levels(oracle, geo, np.uint16, mc.MEAN, frames)
    run_checked(aqz, geo, np.uint16, mc.MEAN, frames, want, 0, "3d_odd_stack")

    geo, _, dtype, frames, _ = fixed_case(oracle, "volume2_cascade2")
    six = frames[:6]
    want = mc.oracle_levels(oracle, geo, dtype, mc.MEAN, six)
    run_checked(aqz, geo, dtype, mc.MEAN, six, want, 0, "six frames")

    # one add_frame first: level 1 holds the earlier plane of its first pair
    ref = oracle.OracleDownsampler(geo, dtype, mc.MEAN)
    mc.oracle_levels(oracle, geo, dtype, mc.MEAN, frames[:1], ref=ref)
    rest = frames[1:]
    want = mc.oracle_levels(oracle, geo, dtype, mc.MEAN, rest, ref=ref)
    counts = [len(rest)] + [len(w) for w in want[1:]]
    ds = aqz.Downsampler(geo, dtype, mc.MEAN)
    try:
        ds.add_frame(frames[0])
        assert all(ds.take_frame(L) is None for L in range(1, len(geo)))
        b = mc.Batch(geo, dtype, rest, counts)
        assert b.run(ds) == counts
        torch_cuda().cuda.synchronize()
        assert ds.last_batch_kind() == 0
        b.check(want, "stored plane")
    finally:
        ds.close()


@pytest.mark.parametrize("name,kind", [("2d_odd", 1), ("3d_fused", 2)])
def test_pure_pyramids_keep_their_kinds(aqz, name, kind):
    geo, n, k = BATCH_GEOMETRIES[name]
    assert k == kind
    frames = np.zeros((n, geo[0][1], geo[0][0]), np.uint16)
    counts = [n >> L if kind == 2 else n for L in range(len(geo))]
    b = mc.Batch(geo, np.uint16, frames, counts)
    ds = aqz.Downsampler(geo, np.uint16, mc.MEAN)
    try:
        assert b.run(ds) == counts
        assert ds.last_batch_kind() == kind
        ds.debug_force_per_frame_batch(1)
        assert b.run(ds) == counts
        assert ds.last_batch_kind() == 0
        ds.debug_force_per_frame_batch(0)
        assert b.run(ds) == counts
        assert ds.last_batch_kind() == kind
        torch_cuda().cuda.synchronize()
    finally:
        ds.close()


@pytest.mark.parametrize("i", range(mc.N_FUZZ))
def test_fuzz(aqz, oracle, i):
    c = mc.fuzz_case(i)
    geo, dtype, method = c["geo"], c["dtype"], c["method"]
    frames = random_frames(c["rng"], dtype, (c["n"], geo[0][1], geo[0][0]))
    want = mc.oracle_levels(oracle, geo, dtype, method, frames)
    assert [len(w) for w in want[1:]] == mc.emitted(geo, c["n"])[1:]
    run_checked(aqz, geo, dtype, method, frames, want, 7,
                f"fuzz {i} {geo} x {c['n']} {name_of(dtype)} m{method} offs {c['offs']}",
                offs=c["offs"])


def test_launch_log_names_the_runs():
    """In one fresh process with the log on: each fixed shape records the
    families of its runs in order, each zrun line the planned shape; a refused
    pyramid records no zrun line."""
    env = dict(os.environ, AQZ_LAUNCH_LOG="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mixed_batch_launch_child.py")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    xy_families = {"cascade", "band", "generic"}
    for name, (geo, n, dtype, runs) in mc.FIXED.items():
        lines, kind = rec[name]["log"], rec[name]["kind"]
        assert kind == 7, name
        bpp = np.dtype(dtype).itemsize
        at = 0
        for cls, first, k, frames in runs:
            line = lines[at]
            if cls == "XYZ":
                assert (line["family"], line["n_out"]) == ("volume", k), (name, line)
            elif cls == "Z":
                w, h, _ = geo[first - 1]
                groups, spans, grid = mc.zrun_shape(w * h, bpp, k, frames)
                assert line["family"] == "zrun", (name, line)
                assert (line["dtype"], line["n_out"], line["planes"], line["groups"], line["spans"],
                        line["grid"], line["elems"]) == (bpp, k, frames, groups, spans, grid,
                                                         w * h), (name, line)
            else:
                assert line["family"] in xy_families, (name, line)
                if line["family"] == "generic":   # one launch a level
                    assert all(l["family"] == "generic" for l in lines[at: at + k]), name
                    at += k - 1
                else:
                    assert line["n_out"] == k, (name, line)
            at += 1
        assert at == len(lines), f"{name}: {len(lines) - at} launches past the runs"
    for name in ("refused_odd_stack", "refused_six_frames"):
        assert rec[name]["kind"] == 0
        fams = {l["family"] for l in rec[name]["log"]}
        assert fams and "zrun" not in fams and "volume" not in fams, (name, fams)
