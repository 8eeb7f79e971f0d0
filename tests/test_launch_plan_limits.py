"""CPU: the launch planner's refusal limits (acquire-zarr_amd/csrc/ds_plan.cpp).

The pyramid kernels keep their unit arithmetic in 32 bits (unit index, units
per frame, `items = p.zitems * n_frames; // < 2^32: checked at launch`), which
is sound only because the planner refuses what would not fit:

* 2^31 units and more for the row-major cascade and the fused volume,
* 2^30 and more for the chunk-tiled cascade,
* 2^32 zero-fill items (overhang rows x frames) and more,
* a padded tile width or height of 2^31 and more.

For each limit the largest request under it must be valid with its `units`
and `grid` the exact 64-bit values, and one frame (one plane group, one
column, one row) more must be `invalid`.  Driven as tests/test_launch_plan.py
drives it: tests/cpp/plan_probe.cpp linked with ds_plan.cpp alone, built with
the host compiler under ASan + UBSan; no buffer exists, the planner looks at
addresses and never through them.
"""
import os
import subprocess

import pytest

import launch_rule_child as child
from test_launch_plan import CSRC, ROOT, parse

U8, U16, F32 = 0, 1, 8


def build_probe(out_dir):
    """Build plan_probe under ASan + UBSan into `out_dir`; returns
    run(requests) -> one parsed launch line (None for `invalid`) per request."""
    exe = str(out_dir / "plan_probe")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "plan_probe.cpp"),
                    os.path.join(CSRC, "ds_plan.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("AQZ_")}

    def run(requests):
        r = subprocess.run([exe], input="\n".join(requests) + "\n", env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(requests)
        return [parse(l) for l in lines]
    return run


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    return build_probe(tmp_path_factory.mktemp("plan_probe_limits"))


def ceil_div(a, b):
    return -(-a // b)


def exact_grid(rec):
    """The grid the line's own 64-bit numbers give (cascade_kernel,
    cascade_band_kernel and volume_kernel index their units with it)."""
    units, waves = rec["units"], rec["block"] // 64
    if rec["family"] == "volume":
        return ceil_div(ceil_div(units, rec["UPW"]), 4)
    bands = units // rec["units_x"]
    if rec["family"] == "band":
        return bands * (ceil_div(rec["units_x"], rec["seg_tiles"]) if rec["seg_tiles"] else 1)
    if rec["family"] == "cascade":
        if rec["seg_w"]:
            return bands * ceil_div(rec["units_x"], rec["seg_w"])
        return ceil_div(ceil_div(units, rec["upw"]), waves)
    assert rec["family"] == "tiled" and not rec["seg_w"]
    return rec["zwaves"] // rec["wpb"] + ceil_div(units, rec["wpb"])


CASCADE = [
    # (dtype, method, W, H, n_out, the form the request takes)
    (U16, 1, 1024, 512, 4, {"family": "cascade", "seg_w": 0, "upw": 1}),
    (U8, 0, 512, 512, 2, {"family": "cascade", "upw": 4}),           # units looped per wave
    (U16, 1, 4096, 48, 3, {"family": "band", "seg_tiles": 3}),       # aligned band segments
    (U16, 1, 1500, 90, 3, {"family": "band", "seg_tiles": 0}),       # a band staged whole
    (F32, 1, 2600, 70, 3, {"family": "cascade", "seg_w": 6}),        # band workgroups
]


def at_the_limit(ask, request, limit, step=1):
    """`request` is a format string over the frame (plane) count.  Returns
    the record of the largest count under `limit` units; asserts the next
    count is invalid."""
    one = ask([request.format(n=step)])[0]
    assert one is not None, request
    per = one["units"]                       # units of one frame / plane group
    n_max = (limit - 1) // per * step
    assert n_max + step < 1 << 32
    last, over = ask([request.format(n=n_max), request.format(n=n_max + step)])
    assert last is not None, f"{request.format(n=n_max)}: invalid under the limit"
    assert over is None, f"{request.format(n=n_max + step)}: {per * (n_max // step + 1)} units accepted"
    assert last["units"] == per * (n_max // step) < limit <= per * (n_max // step + 1)
    assert not child.check_launch(last), (child.check_launch(last), last)
    assert last["grid"] == exact_grid(last), last
    assert last["grid"] < 1 << 31
    return last


@pytest.mark.parametrize("dtype,method,w,h,n_out,form", CASCADE)
def test_cascade_refuses_2_31_units(ask, dtype, method, w, h, n_out, form):
    last = at_the_limit(ask, f"cascade {dtype} {method} {w} {h} {n_out} {{n}}", 1 << 31)
    assert all(last[k] == v for k, v in form.items()), (form, last)


@pytest.mark.parametrize("dtype,method", [(U16, 0), (U16, 1), (F32, 1)])
def test_volume_refuses_2_31_units(ask, dtype, method):
    # 256 x 128, two fused levels: plane groups of 4
    last = at_the_limit(ask, f"volume {dtype} {method} 256 128 2 {{n}}", 1 << 31, step=4)
    assert last["family"] == "volume" and last["zfast"] == int(method == 0)


@pytest.mark.parametrize("dtype,w,h,n_out,tile", [(U16, 1000, 600, 3, "64x128"),
                                                   (U8, 512, 512, 3, "64x64")])
def test_tiled_cascade_refuses_2_30_units(ask, dtype, w, h, n_out, tile):
    # 1000 x 600 in 64 x 128 tiles has 212 overhang rows a frame, under 2^32
    # items at this count; 512^2 in 64 x 64 tiles has none
    last = at_the_limit(ask, f"tiled {dtype} 1 {w} {h} {n_out} {{n}} tile={tile} flags=1", 1 << 30)
    assert last["family"] == "tiled" and last["main_blocks"] == -(-last["units"] // last["wpb"])


def test_tiled_cascade_refuses_2_32_zero_fill_items(ask):
    """64 x 2 u8, one level (32 x 1), tiles of 4096 rows x 64 columns: one
    unit per frame, and of the padded 4096 rows the unit covers one, so a
    frame has 4095 zero-fill rows (plan_cascade_tiled: zrows = ph - cov_h
    when the columns are covered).  The largest frame count with
    4095 * n < 2^32 is valid, one more is refused; with one-row tiles (no
    overhang) that count is valid, so the refusal is the item limit's."""
    z = 4095
    n_max = ((1 << 32) - 1) // z
    assert n_max + 1 < 1 << 30      # far under the unit limit
    req = "tiled 0 1 64 2 1 {n} tile={t} flags=1"
    last, over, no_overhang = ask([req.format(n=n_max, t="4096x64"),
                                   req.format(n=n_max + 1, t="4096x64"),
                                   req.format(n=n_max + 1, t="1x64")])
    assert last is not None and last["units"] == n_max and z * n_max < 1 << 32
    assert not child.check_launch(last) and last["grid"] == exact_grid(last)
    assert last["zwaves"] > 0
    assert over is None and z * (n_max + 1) >= 1 << 32
    assert no_overhang is not None and no_overhang["units"] == n_max + 1


@pytest.mark.parametrize("tile_ok,tile_over", [("1x2147483647", "1x2147483648"),
                                               ("2147483647x1", "2147483648x1")],
                         ids=["width", "height"])
def test_tiled_cascade_refuses_padded_sides_of_2_31(ask, tile_ok, tile_over):
    """One tile per level side: the padded width (height) is the tile's."""
    req = "tiled 1 1 1024 512 1 1 tile={t} flags=1"
    ok, over = ask([req.format(t=tile_ok), req.format(t=tile_over)])
    assert ok is not None and ok["family"] == "tiled" and not child.check_launch(ok)
    assert over is None
