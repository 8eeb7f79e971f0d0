"""CPU: tests/float_cases.py reaches what it names, and the oracle gives the
reference's bits there.

* Census: the edge frames through the oracle; every class the module claims
  for a (method, level) occurs, and every planted output holds the bits this
  file works out from the operands on its own (numpy scalar arithmetic, a
  compare chain in Python, and tables written out below), so the oracle is
  checked and not echoed.
* gpu_util.random_frames reaches none of it (why the module exists).
* The launch planner gives float64 the schemes tests/test_gpu_float_classes.py
  counts on at the suite's fixed geometries, and float32 the ones
  test_gpu_launch_rules.DEFAULT_PINS states, so a threshold that moves cannot
  leave a scheme without its float edge case.
* The reference-made fixture (tests/golden/reference_float_classes.npz, made
  by make_reference_vectors.py --float-classes) replays through the oracle
  byte for byte.
"""
import os
import subprocess

import numpy as np
import pytest

import float_cases as fc
import refvec as rv
import test_gpu_launch_rules as rules
from gpu_util import random_frames
from test_gpu_parity import BATCH_GEOMETRIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acquire-zarr_amd", "csrc")
FLOATS = [np.float32, np.float64]
METHODS = [fc.DECIMATE, fc.MEAN, fc.MIN, fc.MAX]

# name: (h, w, levels, planes, frames)
CENSUS = {
    "1024x64": (64, 1024, 4, 1, 3),       # 4 levels, two tiles per band and more
    "1001x33": (33, 1001, 3, 1, 3),       # odd everywhere
    "stack_64x48x7": (48, 64, 3, 7, 14),  # [(64,48,7),(32,24,4),(16,12,2)], two stacks
}

# sum = k x smallest subnormal -> sum/4 in units of the smallest subnormal,
# round to nearest even: 0.25 0.5 0.75 1 1.25 1.5 1.75
SUB_ROUND_4 = {1: 0, 2: 0, 3: 1, 4: 1, 5: 1, 6: 2, 7: 2}
# sum/2: 0.5 1 1.5
SUB_ROUND_2 = {1: 0, 2: 1, 3: 2}
# B + 1 == B (B = 1e8 in float32, 1e17 in float64): the left-to-right mean.
# A pairwise sum, (a + b) + (c + d), gives 0, 0, 0.5, 0.5, 0, 0.
ABSORB = {("B", "1", "-B", "1"): 0.25, ("1", "B", "-B", "1"): 0.25, ("1", "1", "B", "-B"): 0.0,
          ("B", "-B", "1", "1"): 0.5, ("-B", "1", "B", "1"): 0.25, ("B", "1", "1", "-B"): 0.0}


def oracle_levels(oracle, geo, dtype, method, frames):
    """{level: the frames the oracle emits, in order}."""
    ref = oracle.OracleDownsampler(geo, dtype, method)
    out = {L: [] for L in range(1, len(geo))}
    for fr in frames:
        ref.add_frame(fr)
        for L in out:
            r = ref.take_frame(L)
            if r is not None:
                out[L].append(r)
    return out


# ---- the expected bits, worked out here ---------------------------------------

def _value(f, b):
    return np.array(b, f.ut).view(f.dt)[()]


def _bits(f, v):
    return int(np.array(v, f.dt).view(f.ut))


def rne_div(k, n):
    """k / n to the nearest integer, ties to even (k >= 0)."""
    q, r = divmod(k, n)
    return q + (1 if 2 * r > n or (2 * r == n and q % 2) else 0)


def x86_add(f, x, y):
    """addss / addsd on bit patterns: the first NaN operand quieted, the
    negative default NaN for an invalid sum."""
    if f.is_nan(x):
        return x | f.quiet
    if f.is_nan(y):
        return y | f.quiet
    with np.errstate(all="ignore"):
        s = _value(f, x) + _value(f, y)
    return f.default_nan if np.isnan(s) else _bits(f, s)


def expect_mean(f, ops):
    if len(ops) == 1:   # the last plane of an odd stack passes through
        return ops[0]
    acc = ops[0]
    for b in ops[1:]:
        acc = x86_add(f, acc, b)
    if f.is_nan(acc):
        return acc
    with np.errstate(all="ignore"):
        return _bits(f, _value(f, acc) / f.dt.type(len(ops)))


def expect_select(f, ops, greater):
    """min4 / max4: a chain seeded with a; min2 / max2: `a < b ? a : b`."""
    def beats(x, y):
        x, y = float(_value(f, x)), float(_value(f, y))   # exact in a double
        return x > y if greater else x < y
    if len(ops) == 2:
        return ops[0] if beats(ops[0], ops[1]) else ops[1]
    v = ops[0]
    for b in ops[1:]:
        if beats(b, v):
            v = b
    return v


def expected_bits(f, method, ops):
    if method == fc.DECIMATE:
        return ops[0]
    if method == fc.MEAN:
        return expect_mean(f, ops)
    return expect_select(f, ops, method == fc.MAX)


def sub_count(f, b):
    """A subnormal's (or zero's) signed count of smallest subnormals."""
    assert (b & ~f.sign) < f.tiny, hex(b)
    return -(b & ~f.sign) if b & f.sign else b


def check_defining_bits(f, method, p, got):
    """What the class says about the result, from the operands alone."""
    ops, ctx = p.ops, f"{p.name} {[hex(b) for b in p.ops]} -> {got:#x}"
    nan = [b for b in ops if f.is_nan(b)]
    if len(ops) == 1:   # passed through: no reduce step ran on it
        assert got == ops[0], ctx
    elif p.name == "neg_zero":
        assert all(b == f.nz for b in ops) and got == f.nz, ctx
    elif p.name == "mixed_zero":
        assert got == f.pz, ctx
    elif p.name == "sub_exact":
        assert 0 < (got & ~f.sign) < f.tiny, ctx
        assert float(_value(f, got)) * len(ops) == sum(float(_value(f, b)) for b in ops), ctx
    elif p.name == "sub_round":
        k = sum(sub_count(f, b) for b in ops)
        table = SUB_ROUND_4 if len(ops) == 4 else SUB_ROUND_2
        want = table.get(abs(k), rne_div(abs(k), len(ops)))
        assert got == (want | (f.sign if k < 0 else 0)), f"{ctx}: k = {k}"
    elif p.name == "overflow":
        assert all((b & ~f.sign) < f.inf for b in ops), ctx
        assert got in (f.inf, f.ninf), ctx
    elif p.name == "absorb":
        big = 1e8 if f.dt.itemsize == 4 else 1e17
        sym = tuple({big: "B", -big: "-B", 1.0: "1"}[float(_value(f, b))] for b in ops)
        assert got == f.val(ABSORB[sym]), ctx
    elif p.name == "nan_first":
        assert nan and got == nan[0] | f.quiet, ctx
    elif p.name == "nan_default":
        assert got == f.default_nan, ctx
    elif p.name == "zero_tie":
        assert all(b in (f.pz, f.nz) for b in ops), ctx
        assert got == (ops[1] if len(ops) == 2 else ops[0]), ctx
    elif p.name == "sub_cmp":
        k = [sub_count(f, b) for b in ops]
        want = max(k) if method == fc.MAX else min(k)
        assert sub_count(f, got) == want, ctx
    elif p.name == "nan_a":
        assert f.is_nan(ops[0]), ctx
        assert got == (ops[1] if len(ops) == 2 else ops[0]), ctx
    elif p.name == "nan_later":
        assert not f.is_nan(ops[0]) and nan, ctx
        if len(ops) == 2:
            assert got == ops[1], ctx   # `a < b ? a : b` hands back b, bits unchanged
        else:
            assert not f.is_nan(got), ctx
    elif p.name == "inf_max":
        want = f.inf if method == fc.MAX else f.ninf
        if want in ops:
            assert got == want, ctx
    elif p.name == "pass_bits":
        assert got == ops[0], ctx
    else:
        raise AssertionError(f"unknown class {p.name}")


def test_tables_agree_with_round_to_nearest_even():
    assert {k: rne_div(k, 4) for k in range(1, 8)} == SUB_ROUND_4
    assert {k: rne_div(k, 2) for k in range(1, 4)} == SUB_ROUND_2


# ---- census ---------------------------------------------------------------------

@pytest.mark.parametrize("geom", sorted(CENSUS))
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", FLOATS, ids=["f32", "f64"])
def test_census(oracle, dtype, method, geom):
    h, w, nl, planes, n = CENSUS[geom]
    geo = fc.pyramid(h, w, nl, planes)
    f = fc.Fmt(dtype)
    frames = fc.edge_frames(dtype, n, h, w, nl, planes)
    assert frames.shape == (n, h, w) and frames.dtype == f.dt
    out = oracle_levels(oracle, geo, dtype, method, frames)
    for L in range(1, nl):
        gw, gh, gp = geo[L]
        assert len(out[L]) == n // planes * gp
        plants = fc.planted(dtype, n, h, w, nl, method, L, planes)
        claimed = fc.claimed(dtype, geo, method, L)
        assert claimed and claimed <= set(fc.CLASSES[method])
        if L == 1:
            assert claimed == set(fc.CLASSES[method])
        elif method == fc.MEAN:   # the level-1-only class, by arithmetic
            assert claimed == set(fc.CLASSES[method]) - {"overflow"}
        assert {p.name for p in plants} == claimed, f"level {L}"
        for p in plants:
            got = int(out[L][p.frame].view(f.ut)[p.y, p.x])
            ctx = f"level {L} frame {p.frame} ({p.y}, {p.x})"
            want = expected_bits(f, method, p.ops)
            assert got == want, f"{ctx}: {p.name} {[hex(b) for b in p.ops]}: " \
                                f"{got:#x}, expected {want:#x}"
            check_defining_bits(f, method, p, got)
        # signalling NaNs reach the reduce step wherever the class needs them
        if method != fc.MEAN or L == 1:
            assert any(f.is_nan(b) and not b & f.quiet for p in plants for b in p.ops)
        # odd parents: the classes that keep their meaning sit on the
        # replicated last column and row
        pw, ph, _ = geo[L - 1]
        edge = set(fc.EDGE_CLASSES) & claimed
        if pw % 2:
            assert {p.name for p in plants if p.x == gw - 1} >= edge, f"level {L} last column"
        if ph % 2:
            assert {p.name for p in plants if p.y == gh - 1} >= edge, f"level {L} last row"
        # wide frames: every class in the first 512 px, in the last 256 px
        # (the last tile of a band) and in the last band of rows
        if w >= 1024:
            band = -(-h // (1 << (nl - 1))) - 1
            for what, inside in (
                    ("first 512 px", lambda p: (p.x + 1) << L <= 512),
                    ("last 256 px", lambda p: p.x << L >= w - 256),
                    ("last band", lambda p: (p.y << L) >> (nl - 1) == band)):
                assert {p.name for p in plants if inside(p)} == claimed, f"level {L} {what}"


@pytest.mark.parametrize("dtype", FLOATS, ids=["f32", "f64"])
def test_every_variant_is_planted_somewhere(dtype):
    """Over the census geometries and the Z-only stack (the one place where a
    pair meets raw operands) every catalogue entry is reached."""
    cat = fc.catalogue(dtype)
    seen = set()
    geos = [(n, tuple(fc.pyramid(h, w, nl, planes))) for h, w, nl, planes, n in CENSUS.values()]
    for n, geo in geos + [(6, ((40, 30, 6), (40, 30, 3), (40, 30, 2)))]:
        for recs in fc._layout(np.dtype(dtype).name, n, geo)[1].values():
            for rec in recs:
                seen |= set(np.unique(rec[3]).tolist())
    assert seen == set(range(len(cat)))
    assert {e.name for e in cat if e.raw_only} == {"overflow", "nan_first"}


def test_class_map_names_the_planted_outputs():
    h, w, nl, planes, n = CENSUS["stack_64x48x7"]
    cm = fc.class_map(np.float32, n, h, w, nl, fc.MEAN, 2, planes)
    assert cm.shape == (4, 12, 16)
    plants = fc.planted(np.float32, n, h, w, nl, fc.MEAN, 2, planes)
    assert sum(v is not None for v in cm.reshape(-1)) == len(plants) > 0
    assert all(cm[p.frame, p.y, p.x] == p.name for p in plants)


def test_z_only_stack_pairs_raw_operands(oracle):
    """Where Z halves alone, the pair classes see their operands raw, the
    signalling NaNs and max + max included, and the last plane of the odd
    level passes through."""
    geo = [(40, 30, 6), (40, 30, 3), (40, 30, 2)]
    for dtype in FLOATS:
        f = fc.Fmt(dtype)
        frames = fc.edge_frames(dtype, 6, 30, 40, 3, 6, geometry=geo)
        for method in METHODS:
            out = oracle_levels(oracle, geo, dtype, method, frames)
            assert fc.claimed(dtype, geo, method, 1) == set(fc.CLASSES[method]) - {"absorb"}
            for L in (1, 2):
                plants = fc.planted(dtype, 6, 30, 40, 3, method, L, 6, geometry=geo)
                assert {p.name for p in plants} == fc.claimed(dtype, geo, method, L)
                assert all(len(p.ops) <= 2 for p in plants)
                assert (L == 2) == any(len(p.ops) == 1 for p in plants)
                for p in plants:
                    got = int(out[L][p.frame].view(f.ut)[p.y, p.x])
                    assert got == expected_bits(f, method, p.ops), (L, p)
                    check_defining_bits(f, method, p, got)


# ---- the classes tell the mutations apart -----------------------------------------

@pytest.mark.parametrize("dtype", FLOATS, ids=["f32", "f64"])
def test_classes_distinguish_the_known_mutations(dtype):
    """absorb: a pairwise sum gives other bits than the left-to-right one;
    zero_tie: `<=` in the select chain gives other bits than `<`;
    nan_first: an unquieted signalling NaN differs from the quieted one."""
    f = fc.Fmt(dtype)
    cat = fc.catalogue(dtype)
    with np.errstate(all="ignore"):
        pairwise = [e for e in cat if e.name == "absorb" and expect_mean(f, e.ops) != _bits(
            f, ((_value(f, e.ops[0]) + _value(f, e.ops[1])) +
                (_value(f, e.ops[2]) + _value(f, e.ops[3]))) / f.dt.type(4))]
    assert len(pairwise) >= 3
    big = f.val(1e8 if dtype is np.float32 else 1e17)
    one = f.val(1.0)
    assert expect_mean(f, (big, one, f.neg(big), one)) == f.val(0.25)
    assert expect_mean(f, (one, one, big, f.neg(big))) == f.pz

    def min_le(ops):
        v = ops[0]
        for b in ops[1:]:
            if float(_value(f, b)) <= float(_value(f, v)):
                v = b
        return v
    ties = [e for e in cat if e.name == "zero_tie" and e.kind == 4]
    assert len(ties) == 14
    assert sum(min_le(e.ops) != expect_select(f, e.ops, False) for e in ties) >= 8
    snan = [e for e in cat if e.name == "nan_first" and e.raw_only and e.kind == 4]
    assert len(snan) == 8
    for e in snan:
        first = next(b for b in e.ops if f.is_nan(b))
        assert not first & f.quiet and expect_mean(f, e.ops) == first | f.quiet


# ---- random frames reach none of it ---------------------------------------------------

def test_random_frames_reach_none_of_it(oracle):
    """8 frames of 384 x 512, 4 levels below them, Mean: 522240 outputs per
    dtype, none of them -0.0, subnormal or an overflow from finite operands."""
    for dtype in FLOATS:
        f = fc.Fmt(dtype)
        rng = np.random.default_rng(384512)
        frames = random_frames(rng, dtype, (8, 384, 512))
        n_out = neg_zero = subnormal = overflow = 0
        for fr in frames:
            prev = fr
            for lv in oracle.cascade_2d(fr, 5, fc.MEAN):
                b = lv.view(f.ut)
                mag = b & f.ut.type(f.sign - 1)
                n_out += lv.size
                neg_zero += int((b == f.ut.type(f.nz)).sum())
                subnormal += int(((mag > 0) & (mag < f.ut.type(f.tiny))).sum())
                finite = np.isfinite(prev)
                finite4 = (finite[0::2, 0::2] & finite[0::2, 1::2] &
                           finite[1::2, 0::2] & finite[1::2, 1::2])
                overflow += int((np.isinf(lv) & finite4).sum())
                prev = lv
        assert n_out == 522240
        assert (neg_zero, subnormal, overflow) == (0, 0, 0), np.dtype(dtype).name


# ---- scheme pins on the planner ---------------------------------------------------------

# float64 Mean, the default launch of the `al` pass (ds_plan.cpp, plan_cascade).
# 8-byte tiles are 64 lanes x 4 columns (256 px), or 2 columns (128 px) on
# rows of whole KiB (narrow_rows); bands of 8-byte tiles stage at most 4
# misaligned tiles (mis_max) and have no rowwise segments (2- and 4-byte only).
F64_PINS = {
    # 12000-B rows: 6 wide tiles, level rows split bursts, 6 > mis_max:
    # direct stores from one 6-wave workgroup per band
    "2d_band_staged": {"family": "cascade", "seg_w": 6, "block": 384, "cols": 4},
    # 19 wide tiles, misaligned: ceil(19 / 8) = 3 pieces of ceil(19 / 3) = 7
    # waves, a workgroup size no pinned u16 / f32 case takes
    "2d_mis_segments": {"family": "cascade", "seg_w": 7, "block": 448, "cols": 4},
    # 8192-B rows: 8 narrow tiles, aligned: all four levels staged, a band
    # of exactly 8 goes in 4-tile segments (Mean of a type that is not 2-byte)
    "2d": {"family": "band", "stage_mask": 15, "band_last": 0, "seg_tiles": 4, "cols": 2,
           "block": 256},
    # 4096-B rows: 4 narrow tiles, aligned: the whole band behind a barrier
    "2d_narrow": {"family": "band", "stage_mask": 3, "band_last": 0, "seg_tiles": 0, "cols": 2,
                  "block": 256},
    # 8008-B rows: 4 wide tiles, misaligned, 4 <= mis_max: staged whole and
    # stored by the last wave
    "2d_generic": {"family": "band", "band_last": 1, "seg_tiles": 0, "seg_rowwise": 0,
                   "cols": 4, "block": 256},
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/cpp/plan_probe.cpp, built as tests/test_launch_plan.py builds it."""
    exe = str(tmp_path_factory.mktemp("plan_probe_float") / "plan_probe")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "plan_probe.cpp"),
                    os.path.join(CSRC, "ds_plan.cpp"), "-o", exe], check=True)

    def run(requests):
        env = {k: v for k, v in os.environ.items() if not k.startswith("AQZ_")}
        r = subprocess.run([exe], input="\n".join(requests) + "\n", env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(requests)
        recs = []
        for line in lines:
            assert line != "invalid"
            recs.append({k: int(v) if v.lstrip("-").isdigit() else v
                         for k, _, v in (kv.partition("=") for kv in line.split())})
        return recs
    return run


def _request(name, dtype_code):
    geo, n, _ = BATCH_GEOMETRIES[name]
    w, h, _ = geo[0]
    return f"cascade {dtype_code} 1 {w} {h} {min(4, len(geo) - 1)} {min(n, 2)}"


def test_float64_default_schemes_on_the_plan(probe):
    names = sorted(F64_PINS)
    for name, rec in zip(names, probe([_request(n, 9) for n in names])):
        assert rec["dtype"] == 8   # the line prints the element size
        for k, v in F64_PINS[name].items():
            assert rec[k] == v, f"{name}: {k}={rec[k]}, pinned {v}: {rec}"


def test_float32_default_pins_on_the_plan(probe):
    pins = [(fields, cid.split("/")[0]) for fields, ids in rules.DEFAULT_PINS["cascade"]
            for cid in ids if cid.endswith("/float32/m1/al")]
    assert len(pins) >= 8
    for (fields, name), rec in zip(pins, probe([_request(n, 8) for _, n in pins])):
        for k, v in fields.items():
            assert rec[k] == v, f"{name}: {k}={rec[k]}, pinned {v}: {rec}"


# ---- the reference-made fixture ---------------------------------------------------------

def _oracle_make(oracle):
    def make(dims, dt, method):
        return oracle.OracleDownsampler(oracle.level_geometry(oracle.plan_levels(dims)), dt,
                                        method)
    return make


def test_float_class_fixture_holds_the_edge_frames():
    """The fixture's inputs are edge_frames of its geometries, bit for bit,
    and it stays small."""
    vec = np.load(rv.FLOAT_NPZ, allow_pickle=False)
    assert os.path.getsize(rv.FLOAT_NPZ) < 256 * 1024
    for geom in rv.FLOAT_GEOMETRIES:
        # the reference's own level sizes
        assert [tuple(g) for g in vec[f"geometry/{geom}"].tolist()] == rv.FLOAT_LEVELS[geom]
        for dt in rv.NAN_DTYPES:
            x = vec[f"in/{geom}/{np.dtype(dt).name}"]
            want = rv.make_float_class_inputs(geom, dt)
            ut = f"u{np.dtype(dt).itemsize}"
            assert x.dtype == np.dtype(dt) and np.array_equal(x.view(ut), want.view(ut))


@pytest.mark.parametrize("geom,dtype,method", rv.float_class_cases(),
                         ids=[f"{g}-{d}-{rv.METHOD_NAMES[m]}" for g, d, m in
                              rv.float_class_cases()])
def test_oracle_replays_reference_float_classes(oracle, geom, dtype, method):
    vec = np.load(rv.FLOAT_NPZ, allow_pickle=False)
    rv.replay(_oracle_make(oracle), rv.float_class_manifest(), vec, geom, dtype, method,
              nan_bits=True)
    # and what the reference stored shows the classes: every planted output
    # of every level holds the bits worked out above
    f = fc.Fmt(dtype)
    dims, n, _ = rv.FLOAT_GEOMETRIES[geom]
    geo = rv.float_class_pyramid(geom)
    (w, h, planes), nl = geo[0], len(geo)
    name = rv.case_name(geom, dtype, method)
    ev, out = vec[f"ev/{name}"], vec[f"out/{name}"]
    frames, off = {L: [] for L in range(1, nl)}, 0
    for _, L, has, nb in ev:
        if has:
            gw, gh, _ = geo[L]
            frames[int(L)].append(out[off:off + nb].view(f.ut).reshape(gh, gw))
            off += int(nb)
    for L in range(1, nl):
        plants = fc.planted(dtype, n, h, w, nl, method, L, planes, geometry=geo)
        assert {p.name for p in plants} == fc.claimed(dtype, [tuple(g) for g in geo], method, L)
        for p in plants:
            got = int(frames[L][p.frame][p.y, p.x])
            assert got == expected_bits(f, method, p.ops), (L, p, hex(got))
            check_defining_bits(f, method, p, got)


@pytest.mark.parametrize("dtype", FLOATS, ids=["f32", "f64"])
def test_zero_region_stack_reaches_its_tiles(oracle, dtype):
    """The stack tests/test_gpu_float_classes.py sends through the tiled
    volume call: under Mean the oracle's level-1 and level-2 planes, tiled,
    hold whole tiles of +0.0 (flag 0), whole tiles of -0.0 (flag 1) and a tile
    whose only nonzero bytes are one -0.0, and the bottom right quarter keeps
    the planted classes."""
    geo, n, _ = BATCH_GEOMETRIES["3d_fused"]
    w, h, planes = geo[0]
    edge = fc.edge_frames(dtype, n, h, w, len(geo), planes, geometry=geo)
    stack = fc.zero_region_stack(edge)
    ut = np.dtype(f"u{np.dtype(dtype).itemsize}")
    assert np.array_equal(stack[:, h // 2:, w // 2:].view(ut), edge[:, h // 2:, w // 2:].view(ut))
    lv = oracle_levels(oracle, geo, dtype, fc.MEAN, stack)
    plain = oracle_levels(oracle, geo, dtype, fc.MEAN, edge)
    tr, tc = fc.ZERO_TILE
    for L in (1, 2):
        gw, gh, _ = geo[L]
        t = [oracle.tile_frame(p, tr, tc) for p in lv[L]]
        fc.check_zero_region_tiles(dtype, L, np.stack([a for a, _ in t]),
                                   np.stack([b for _, b in t]), gh, gw)
        # outputs fed by the bottom right quarter alone are the edge stack's own
        y0, x0 = (h // 2 >> L) + 1, (w // 2 >> L) + 1
        for a, b in zip(lv[L], plain[L]):
            assert np.array_equal(a[y0:, x0:].view(ut), b[y0:, x0:].view(ut))
        kept = fc.class_map(dtype, n, h, w, len(geo), fc.MEAN, L, planes, geometry=geo)[:, y0:, x0:]
        assert (kept != None).any(), f"level {L}: no planted class left"  # noqa: E711
