"""CPU: the cases tests/test_gpu_mixed_batch.py runs on the GPU
(tests/mixed_batch_cases.py).  The fuzz generator yields only pyramids the
planner accepts and reaches every order of classes; the oracle accepts the
fixed shapes, emits n >> zcount(l) frames a level, and equals the
level-by-level model "XY-reduce every plane, then pair consecutive planes"."""
import numpy as np
import pytest

import mixed_batch_cases as mc


@pytest.fixture(scope="module")
def fuzz():
    return [mc.fuzz_case(i) for i in range(mc.N_FUZZ)]


def test_fuzz_yields_only_accepted_pyramids(fuzz):
    ask = mc.plan_probe()
    lines = ask([mc.runs_request(c["geo"], c["n"]) for c in fuzz])
    for i, (c, line) in enumerate(zip(fuzz, lines)):
        runs = mc.parse_runs(line)
        assert runs is not None, f"case {i} {c['geo']} x {c['n']}: {line}"
        assert runs == mc.runs_of(c["geo"], c["n"]), f"case {i}"
        assert {r[0] for r in runs} != {"XY"} and {r[0] for r in runs} != {"XYZ"}, \
            f"case {i} is a pure pyramid (kinds 1 and 2)"
        bpp = np.dtype(c["dtype"]).itemsize
        for cls, first, _, _ in runs:   # a fused-volume source row holds one 16-byte load
            assert cls != "XYZ" or c["geo"][first - 1][0] * bpp >= 16, f"case {i}"


def test_fuzz_shape_limits(fuzz):
    for i, c in enumerate(fuzz):
        geo = c["geo"]
        assert 2 <= len(geo) <= 6 and max(geo[0][:2]) <= 96 and 1 <= geo[-1][2] <= 3, i
        assert c["n"] % geo[0][2] == 0 and 1 <= c["n"] // geo[0][2] <= 3, i
        assert any(c["offs"]) == (i % 4 >= 2), i
    assert {np.dtype(c["dtype"]).name for c in fuzz} == {np.dtype(d).name for d in mc.DTYPES}
    assert {c["method"] for c in fuzz} == set(mc.METHODS)
    assert {len(c["geo"]) for c in fuzz} == {2, 3, 4, 5, 6}


def test_fuzz_reaches_every_order_of_classes(fuzz):
    count = {k: 0 for k in mc.CATEGORIES}
    for c in fuzz:
        for k in mc.fuzz_categories(c):
            count[k] += 1
    assert all(v >= 4 for v in count.values()), count


@pytest.mark.parametrize("name", mc.FIXED_NAMES)
def test_model_equals_the_oracle_on_the_fixed_shapes(oracle, name):
    geo, n, _, _ = mc.FIXED[name]
    for dtype in (np.uint8, np.float32):
        rng = np.random.default_rng(len(name))
        if dtype is np.uint8:
            frames = rng.integers(0, 256, (n, geo[0][1], geo[0][0]), dtype=np.uint8)
        else:   # finite, of mixed magnitude and sign
            frames = (rng.standard_normal((n, geo[0][1], geo[0][0])) *
                      np.exp(rng.uniform(-8, 8, (n, geo[0][1], geo[0][0])))).astype(np.float32)
        for method in mc.METHODS:
            want = mc.oracle_levels(oracle, geo, dtype, method, frames)
            model = mc.model_levels(geo, dtype, method, frames)
            counts = mc.emitted(geo, n)
            for L in range(1, len(geo)):
                ctx = f"{name} {np.dtype(dtype).name} m{method} L{L}"
                assert want[L].shape[0] == counts[L], ctx
                assert np.array_equal(want[L].view(f"u{want[L].itemsize}"),
                                      model[L].view(f"u{model[L].itemsize}")), ctx
