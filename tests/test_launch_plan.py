"""CPU: the launch planner (acquire-zarr_amd/csrc/ds_plan.cpp) against the
tables the GPU launch-rule suite owns.

What launch_cascade, launch_cascade_tiled and launch_volume launch is host
arithmetic, so it runs here: tests/cpp/plan_probe.cpp links ds_plan.cpp alone,
is built with the host compiler under ASan + UBSan, and prints the launch-log
line of every request in one run.  Requests are the first fused run of the
cases tests/launch_rule_child.py runs on the GPU: levels 1..min(4, levels - 1)
(volume: 2), dense levels, every buffer 256-byte aligned (the child's `al`
pass), frames capped at FRAMES_CAP for the cascade.  Every pin and every proof
of the three families is met by that first run; no later run is needed.

tests/test_gpu_launch_rules.py asserts the same pins and proofs on the lines
the library records on the GPU.
"""
import os
import subprocess

import numpy as np
import pytest

import launch_rule_child as child
import test_gpu_launch_rules as rules
from test_gpu_parity import BATCH_GEOMETRIES
from test_gpu_tiled import TILED_CASES, halving

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acquire-zarr_amd", "csrc")
FAMILIES = ("cascade", "tiled", "volume")
DTYPE_CODE = {"uint8": 0, "uint16": 1, "uint32": 2, "uint64": 3, "int8": 4, "int16": 5,
              "int32": 6, "int64": 7, "float32": 8, "float64": 9}
SMALL_LDS = 65536  # the cap when the device query fails, against LDS_MAX on gfx950


def base_requests():
    """{family: {case id: request without switches}}, the cases and ids of
    launch_rule_child.Runner.cascade / tiled / volume."""
    req = {f: {} for f in FAMILIES}
    for name in child.CASCADE_GEOMETRIES:
        geo, n, _ = BATCH_GEOMETRIES[name]
        w, h, _ = geo[0]
        for dt in child.DTYPES:
            for m in child.METHODS:
                req["cascade"][f"{name}/{child.dtype_name(dt)}/m{m}/al"] = (
                    f"cascade {DTYPE_CODE[child.dtype_name(dt)]} {m} {w} {h} "
                    f"{min(4, len(geo) - 1)} {min(n, child.FRAMES_CAP)}")
    for name in child.VOLUME_GEOMETRIES:
        geo, n, _ = BATCH_GEOMETRIES[name]
        w, h, _ = geo[0]
        for dt in child.DTYPES:
            for m in child.METHODS:
                req["volume"][f"{name}/{child.dtype_name(dt)}/m{m}"] = (
                    f"volume {DTYPE_CODE[child.dtype_name(dt)]} {m} {w} {h} "
                    f"{min(2, len(geo) - 1)} {n}")
    cases = [c for c in TILED_CASES if c[0] * c[1] < child.TILED_MAX_PIXELS]
    for case in cases + child.EXTRA_TILED_CASES:
        w, h, nl, dt, tr, tc, n = case
        assert len(halving(w, h, nl)) == nl
        for m in child.METHODS:
            req["tiled"][child.tiled_id(case, m)] = (
                f"tiled {DTYPE_CODE[child.dtype_name(dt)]} {m} {w} {h} {min(4, nl - 1)} {n} "
                f"tile={tr}x{tc} flags=1")
    return req


BASE = base_requests()
# the default launch, then every rule's switches
ENVS = {f: [{}] + [p.values[1] for p in rules.RULES if p.values[0] == f] for f in FAMILIES}


def with_env(request, env, extra=""):
    return " ".join([request] + [f"{k}={v}" for k, v in sorted(env.items())] + [extra]).strip()


def parse(line):
    if line == "invalid":
        return None
    rec = {}
    for kv in line.split():
        k, _, v = kv.partition("=")
        rec[k] = int(v) if v.lstrip("-").isdigit() else v
    return rec


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{request line: its launch line as a dict, or None for `invalid`}: the
    probe built with the sanitizers and run once over every request."""
    out = tmp_path_factory.mktemp("plan_probe")
    exe = str(out / "plan_probe")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "plan_probe.cpp"),
                    os.path.join(CSRC, "ds_plan.cpp"), "-o", exe], check=True)
    requests = []
    for f in FAMILIES:
        for env in ENVS[f]:
            requests += [with_env(r, env) for r in BASE[f].values()]
    for env in ENVS["cascade"]:
        requests += [with_env(r, env, f"lds={SMALL_LDS}") for r in BASE["cascade"].values()]
    requests = sorted(set(requests))
    # the probe never reads the environment; a switch set here changes nothing
    env = {k: v for k, v in os.environ.items() if not k.startswith("AQZ_")}
    r = subprocess.run([exe], input="\n".join(requests) + "\n", env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests)
    return {q: parse(l) for q, l in zip(requests, lines)}


def shows(rec, fields):
    return rec is not None and all(rec.get(k) == v for k, v in fields.items())


@pytest.mark.parametrize("family", FAMILIES)
def test_default_pins_hold_on_the_plan(plans, family):
    for fields, case_ids in rules.DEFAULT_PINS[family]:
        for cid in case_ids:
            rec = plans[with_env(BASE[family][cid], {})]
            assert shows(rec, fields), f"{cid}: {fields} not on {rec}"


@pytest.mark.parametrize("family,env,proofs",
                         [p for p in rules.RULES if p.values[0] in FAMILIES])
def test_rule_shows_on_the_plan(plans, family, env, proofs):
    for fields, case_ids in proofs:
        recs = {cid: plans[with_env(BASE[family][cid], env)] for cid in case_ids}
        assert any(shows(r, fields) for r in recs.values()), f"{fields} on none of {recs}"


@pytest.mark.parametrize("family", FAMILIES)
def test_every_plan_is_consistent_with_its_kernel(plans, family):
    """Every case the child runs (dtype sizes 1 / 2 / 4 / 8, methods 0-3),
    under the default switches and under every rule's: a valid plan whose
    grid covers its units with the kernel it names (check_launch)."""
    assert {np.dtype(d).itemsize for d in child.DTYPES} == {1, 2, 4, 8}
    n = 0
    for env in ENVS[family]:
        for cid, request in BASE[family].items():
            rec = plans[with_env(request, env)]
            assert rec is not None, f"{cid} {env}: invalid"
            assert rec["family"] in (("cascade", "band") if family == "cascade" else (family,))
            err = child.check_launch(rec)
            assert not err, f"{cid} {env}: {err}: {rec}"
            n += 1
    assert n == len(ENVS[family]) * len(BASE[family]) and n >= 16 * len(ENVS[family])


def test_band_plans_fit_a_small_lds_cap(plans):
    """With the cap the device-query fallback gives, no band asks for more,
    and the bands that fit it are still planned."""
    bands = 0
    for env in ENVS["cascade"]:
        for cid, request in BASE["cascade"].items():
            rec = plans[with_env(request, env, f"lds={SMALL_LDS}")]
            assert rec is not None and not child.check_launch(rec), f"{cid} {env}: {rec}"
            if rec["family"] == "band":
                bands += 1
                assert rec["lds"] <= SMALL_LDS, f"{cid} {env}: {rec}"
            else:
                assert rec["lds"] == 0
    assert bands > 0
