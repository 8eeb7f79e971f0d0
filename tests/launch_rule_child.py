"""Runner for tests/test_gpu_launch_rules.py (not a test module).

The launchers read their A/B switches ($AQZ_*) once per process (the
process-wide LaunchSwitches, ds_plan.hh), so every launch rule runs in a
process of its own: the test starts
this file (a new process, never exec'd) with one rule's environment plus
AQZ_LAUNCH_LOG=1.

  --family cascade|tiled|volume|volume_tiled|codec

runs that family's fixed case list against the oracle, byte for byte for
every dtype (floats and NaN payloads included: the alternative launches keep
the operation order), into output buffers filled with 0xA5 first, so that a
result never written cannot pass on stale allocator contents.  After each
case the launch log (aqz_debug_launch_log) is drained and one JSON object is
printed:

  {"case": id, "differing": bytes that differ from the oracle,
   "poison": output bytes still 0xA5 where the oracle's byte is not,
   "stray": bytes changed outside the outputs (the padding around them),
   "launches": [the launch lines, as dicts],
   "launch_errors": [what a line's own geometry contradicts]}

and at the end `TOTAL <n> differing` (differing + stray bytes).

The case lists are the smallest shapes at which each scheme triggers,
imported from the suite's own tables.  Frame 0 is gpu_util.random_frames;
float32 cases of the cascade, tiled and volume families end in
tests/float_cases.py's edge frames (plant_edge_frames).  Frames per case are capped at
FRAMES_CAP: the schemes depend on the frame shape, not on the batch length
beyond "more than one frame".
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

POISON = 0xA5
PAD = 64          # poisoned bytes kept behind every row-major output
FRAMES_CAP = 2
DTYPES = [np.uint8, np.uint16, np.float32, np.int64]
METHODS = [0, 1, 2, 3]

CASCADE_GEOMETRIES = [
    "2d", "2d_odd", "2d_narrow", "2d_narrow_odd", "2d_six", "2d_oddw_deep",
    "2d_wide_misaligned", "2d_band_staged", "2d_band8_aligned", "2d_band6_edge_rows",
    "2d_band_segments", "2d_complete_8tile", "2d_complete_short_last", "2d_mis_segments",
]
VOLUME_GEOMETRIES = [
    "3d_fused", "3d_fused_deep", "3d_fused_edge", "3d_fused_oddw", "3d_fused_oddw_even_h",
    "3d_fused_one_level", "3d_fused_many_groups", "3d_fused_many_groups_edge",
]
# beside the imported TILED_CASES: rows that split 128-B lines over more than
# one tile ($AQZ_TILED_BAND_WG needs both), and a 1-byte frame whose tiles
# overhang it by more than 2048 rows in all, the least at which the 32-rows-
# per-wave rule of 1-byte types ($AQZ_TILED_ZROWS_PER_WAVE) asks for more
# than the 64 zero-fill waves every launch has
# (w, h, levels, dtype, tile_rows, tile_cols, frames)
EXTRA_TILED_CASES = [
    (1500, 90, 4, np.uint16, 64, 128, 2),
    (2600, 70, 4, np.uint16, 64, 128, 2),
    (600, 40, 3, np.uint8, 256, 1024, 5),
]
TILED_MAX_PIXELS = 2_500_000  # leaves out TILED_CASES' three multi-megapixel frames
# beside the imported FILTER_CASES: 1-byte elements in 16-byte-aligned
# buffers, the only ones to take the vector bit shuffle with typesize 1
EXTRA_FILTER_CASES = [
    (1, 4096, 4096 * 5, 2),
]
# LDS a workgroup may use on gfx950, less the band kernel's arrival counter
# (device_lds_cap, ds_dispatch.cpp)
LDS_MAX = 160 * 1024 - 16


def dtype_name(dt):
    return np.dtype(dt).name


def tiled_id(case, method):
    w, h, _, dt, tr, tc, _ = case
    return f"{w}x{h}_{dtype_name(dt)}_{tr}x{tc}/m{method}"


def filter_id(case, shuffle):
    ts, bs, nbytes, nbuf = case
    return f"ts{ts}_bs{bs}_n{nbytes}x{nbuf}/" + {1: "shuffle", 2: "bitshuffle"}[shuffle]


def plant_edge_frames(frames, geo):
    """float32 cases end in tests/float_cases.py's edge frames of the case's
    shape, so that every launch rule runs the float result classes (the sign
    of a zero, subnormal rounding, overflow, NaN payloads, zero ties) through
    its alternative instantiation: the last frame of a 2-D batch, the last
    half of a one-stack volume (whole Z pairs of every level), the last stack
    of a longer one.  Frame 0 stays random."""
    import float_cases as fc

    dt = np.dtype(frames[0].dtype)
    n = len(frames)
    if dt != np.float32 or n < 2:
        return
    w, h, planes = geo[0]
    k = 1 if planes == 1 else min(planes, n // 2)
    edge = fc.edge_frames(dt, planes, h, w, len(geo), planes, geometry=geo)
    for i in range(1, k + 1):
        frames[-i][...] = edge[-i]


def byte_counts(got, want):
    """(differing, poison) of two equally long uint8 arrays."""
    bad = got != want
    return int(np.count_nonzero(bad)), int(np.count_nonzero(bad & (got == POISON)))


def check_launch(rec):
    """What a launch line's own numbers contradict: the grid must cover the
    units with the kernel actually instantiated, the block must stay inside
    the kernel's launch bounds, and a band's wave count, segment width and
    LDS must agree."""
    err = []
    fam = rec.get("family")
    grid, block = rec.get("grid", 0), rec.get("block", 0)
    if grid < 1 or block < 64 or block % 64:
        err.append(f"grid {grid} block {block}")
    waves = block // 64
    if fam in ("cascade", "band", "tiled"):
        units, ux = rec["units"], rec["units_x"]
        bands = units // ux
        if block > 512:
            err.append("block above __launch_bounds__(512)")
        if fam == "cascade":
            if rec["seg_w"]:
                segs = -(-ux // rec["seg_w"])
                if grid < segs * bands or waves != rec["seg_w"]:
                    err.append("band workgroups do not cover the units")
            elif grid * waves * rec["upw"] < units:
                err.append("grid * waves * upw < units")
        elif fam == "band":
            segs = -(-ux // rec["seg_tiles"]) if rec["seg_tiles"] else 1
            want_waves = rec["seg_tiles"] if rec["seg_tiles"] else ux
            if grid != segs * bands or waves != want_waves:
                err.append("band grid or wave count does not match its segments")
            if rec["lds"] > LDS_MAX or rec["band_last"] > 8:
                err.append("band lds or band_last out of range")
            if rec["seg_rowwise"] and not rec["seg_tiles"]:
                err.append("rowwise staging without segments")
        else:
            if waves != rec["wpb"] or rec["zwaves"] % rec["wpb"]:
                err.append("tiled block / zero-fill waves do not match wpb")
            if grid != rec["zwaves"] // rec["wpb"] + rec["main_blocks"]:
                err.append("tiled grid is not zero-fill blocks + cascade blocks")
            need = (-(-ux // rec["seg_w"]) * bands if rec["seg_w"]
                    else -(-units // rec["wpb"]))
            if rec["main_blocks"] < need:
                err.append("tiled cascade blocks do not cover the units")
    elif fam == "volume_tiled":
        if waves != rec["wpb"] or rec["zwaves"] % rec["wpb"]:
            err.append("tiled volume block / zero-fill waves do not match wpb")
        if grid != rec["zwaves"] // rec["wpb"] + rec["main_blocks"]:
            err.append("tiled volume grid is not zero-fill blocks + unit blocks")
        if rec["main_blocks"] * rec["wpb"] < rec["units"]:
            err.append("tiled volume blocks do not cover the units")
        if (rec["zwaves"] > 0) != (rec["zitems"] > 0):
            err.append("zero-fill waves without items, or items without waves")
    elif fam == "volume":
        if block != 256:
            err.append("volume block is not 256")
        if grid * 4 * rec["UPW"] < rec["units"]:
            err.append("grid * 4 * UPW < total_units")
    elif fam in ("shuffle", "bitshuffle", "copy"):
        if block > 256 or waves != rec["waves"]:
            err.append("filter block does not match its waves")
    elif fam in ("generic", "zpair"):
        if block != 256:
            err.append("block is not 256")
    else:
        err.append(f"unknown family {fam}")
    return err


class Runner:
    def __init__(self):
        import torch
        import aqz_pkg
        import oracle

        self.torch = torch
        self.aqz = aqz_pkg.load()
        self.oracle = oracle
        oracle.lib()
        torch.cuda.set_device(0)
        self.total = 0

    def report(self, case, differing, poison, stray=0, error=None):
        launches = self.aqz.debug_launch_log()
        res = {"case": case, "differing": differing, "poison": poison, "stray": stray,
               "launches": launches,
               "launch_errors": [f"{e}: {rec}" for rec in launches for e in check_launch(rec)]}
        if error:
            res["error"] = error
        self.total += differing + stray
        print(json.dumps(res), flush=True)

    # ---- row-major device batches (fused cascade, fused volume) -----------

    def run_batch(self, case, geo, dtype, method, d_in, in_off, offs, n, expected, kind):
        """One aqz_ds_run_device_batch into poisoned outputs; `offs[L]`
        elements before level L in its buffer, PAD bytes behind it."""
        from gpu_util import empty_device, from_device, launch_stream

        bpp = np.dtype(dtype).itemsize
        sizes = [len(expected[L]) * geo[L][0] * geo[L][1] * bpp if L else 0
                 for L in range(len(geo))]
        outs = [None]
        for L in range(1, len(geo)):
            o = empty_device(offs[L] * bpp + sizes[L] + PAD)
            o.fill_(POISON)
            outs.append(o)
        ptrs = [0] + [outs[L].data_ptr() + offs[L] * bpp for L in range(1, len(geo))]
        ds = self.aqz.Downsampler(geo, dtype, method)
        counts = ds.run_device_batch(d_in.data_ptr() + in_off * bpp, n, ptrs, launch_stream())
        self.torch.cuda.synchronize()
        got_kind = ds.last_batch_kind()
        ds.close()
        differing = poison = stray = 0
        error = None
        if got_kind != kind:
            error = f"batch kind {got_kind}, expected {kind}"
        for L in range(1, len(geo)):
            raw = from_device(outs[L], np.uint8, (-1,))
            a = offs[L] * bpp
            if counts[L] != len(expected[L]):
                error = f"level {L}: {counts[L]} frames, expected {len(expected[L])}"
                differing += sizes[L]
                continue
            want = np.stack(expected[L]).view(np.uint8).reshape(-1)
            d, p = byte_counts(raw[a:a + sizes[L]], want)
            differing += d
            poison += p
            stray += int(np.count_nonzero(raw[:a] != POISON) +
                         np.count_nonzero(raw[a + sizes[L]:] != POISON))
        self.report(case, differing + (1 if error and not differing else 0), poison, stray,
                    error)

    def cascade(self):
        from gpu_util import random_frames, to_device
        from test_gpu_parity import BATCH_GEOMETRIES, seed_of

        for name in CASCADE_GEOMETRIES:
            geo, n, kind = BATCH_GEOMETRIES[name]
            n = min(n, FRAMES_CAP)
            w, h, _ = geo[0]
            for dtype in DTYPES:
                rng = np.random.default_rng(seed_of("launch-rules", name, dtype_name(dtype)))
                frames = random_frames(rng, dtype, (n, h, w))
                plant_edge_frames(frames, geo)
                bpp = np.dtype(dtype).itemsize
                # the second pass: the input and every level at a seeded
                # element offset of 1-7, which turns aligned rows into
                # misaligned ones (as test_fuzz_device_batch does)
                offs = [int(x) for x in rng.integers(1, 8, len(geo))]
                passes = []
                for tag, off in (("al", [0] * len(geo)), ("off", offs)):
                    raw = np.zeros(off[0] * bpp + frames.nbytes, dtype=np.uint8)
                    raw[off[0] * bpp:] = frames.view(np.uint8).reshape(-1)
                    passes.append((tag, off, to_device(raw)))
                for method in METHODS:
                    per_frame = [self.oracle.cascade_2d(f, len(geo), method) for f in frames]
                    expected = {L: [pf[L - 1] for pf in per_frame] for L in range(1, len(geo))}
                    for tag, off, d_in in passes:
                        self.run_batch(f"{name}/{dtype_name(dtype)}/m{method}/{tag}", geo, dtype,
                                       method, d_in, off[0], off, n, expected, kind)

    def volume(self):
        from gpu_util import random_frames, to_device
        from test_gpu_fuzz import oracle_stream
        from test_gpu_parity import BATCH_GEOMETRIES, seed_of

        for name in VOLUME_GEOMETRIES:
            geo, n, kind = BATCH_GEOMETRIES[name]
            w, h, _ = geo[0]
            for dtype in DTYPES:
                rng = np.random.default_rng(seed_of("launch-rules", name, dtype_name(dtype)))
                frames = random_frames(rng, dtype, (n, h, w))
                plant_edge_frames(frames, geo)
                d_in = to_device(frames)
                for method in METHODS:
                    expected = oracle_stream(self.oracle, geo, dtype, method, frames)
                    self.run_batch(f"{name}/{dtype_name(dtype)}/m{method}", geo, dtype, method,
                                   d_in, 0, [0] * len(geo), n, expected, kind)

    # ---- chunk-tiled batches ------------------------------------------------

    def tiled(self):
        from gpu_util import random_frames
        from test_gpu_parity import seed_of
        from test_gpu_tiled import TILED_CASES, halving, run_tiled

        cases = [c for c in TILED_CASES if c[0] * c[1] < TILED_MAX_PIXELS] + EXTRA_TILED_CASES
        for case in cases:
            w, h, nl, dt, tr, tc, n = case
            geo = halving(w, h, nl)
            rng = np.random.default_rng(seed_of("launch-rules-tiled", w, h, dtype_name(dt)))
            frames = [random_frames(rng, dt, (h, w)) for _ in range(n)]
            frames[0][: h // 2, : w // 2] = 0  # zero tiles at every level
            plant_edge_frames(frames, geo)
            for method in METHODS:
                differing = poison = 0
                error = None
                try:
                    # run_tiled poisons tiles and flag slots and checks that
                    # every flag slot was written
                    got, _ = run_tiled(self.aqz, geo, dt, method, frames, tr, tc)
                except (AssertionError, self.aqz.AqzError) as e:
                    error = f"{type(e).__name__}: {e}"
                    differing = 1
                else:
                    for k, fr in enumerate(frames):
                        ref = self.oracle.cascade_2d(fr, nl, method)
                        for L in range(1, nl):
                            want_t, want_nz = self.oracle.tile_frame(ref[L - 1], tr, tc)
                            t, f = got[L - 1]
                            d, p = byte_counts(t[k].view(np.uint8).reshape(-1),
                                               want_t.view(np.uint8).reshape(-1))
                            differing += d + int(np.count_nonzero(f[k] != want_nz))
                            poison += p
                self.report(tiled_id(case, method), differing, poison, 0, error)

    # ---- chunk-tiled volumes ---------------------------------------------------

    def volume_tiled(self):
        """aqz_ds_run_device_volume_tiled on volume_tiled_cases.ZROWS_CASES: tiles, flags
        and the PAD bytes behind both against the oracle."""
        import volume_tiled_cases as vc
        from gpu_util import empty_device, from_device, launch_stream, to_device

        for case in vc.ZROWS_CASES:
            w, h, planes, levels, dt, _, _, _ = case
            geo = vc.volume_geo(w, h, planes, levels)
            tiles = vc.case_tiles(case)
            frames = vc.case_frames(case)
            n = len(frames)
            d_in = to_device(frames)
            for method in METHODS:
                want = vc.expected_tiled(
                    self.oracle, vc.oracle_planes(self.oracle, geo, dt, method, frames), tiles)
                outs, flags = [None], [None]
                for L in range(1, levels):
                    outs.append(empty_device(want[L][0].nbytes + PAD))
                    flags.append(empty_device(want[L][1].size + PAD))
                    outs[L].fill_(POISON)
                    flags[L].fill_(POISON)
                ds = self.aqz.Downsampler(geo, dt, method)
                differing = poison = stray = 0
                error = None
                try:
                    ds.run_device_volume_tiled(d_in.data_ptr(), n, tiles,
                                               [0] + [o.data_ptr() for o in outs[1:]],
                                               [0] + [f.data_ptr() for f in flags[1:]],
                                               launch_stream())
                    self.torch.cuda.synchronize()
                    if ds.last_batch_kind() != 5:
                        error = f"batch kind {ds.last_batch_kind()}, expected 5"
                        differing = 1
                except self.aqz.AqzError as e:
                    error = f"AqzError: {e}"
                    differing = 1
                ds.close()
                for L in range(1, levels):
                    t, nz = want[L]
                    raw = from_device(outs[L], np.uint8, (-1,))
                    d, p = byte_counts(raw[:t.nbytes], t.view(np.uint8).reshape(-1))
                    fl = from_device(flags[L], np.uint8, (-1,))
                    d2, p2 = byte_counts(fl[:nz.size], nz.reshape(-1).astype(np.uint8))
                    differing += d + d2
                    poison += p + p2
                    stray += int(np.count_nonzero(raw[t.nbytes:] != POISON) +
                                 np.count_nonzero(fl[nz.size:] != POISON))
                self.report(f"{vc.case_id(case)}/m{method}", differing, poison, stray, error)

    # ---- blosc filters --------------------------------------------------------

    def codec(self):
        from gpu_util import empty_device, from_device, launch_stream, to_device
        from test_gpu_codecs import FILTER_CASES

        for case in FILTER_CASES[:-1] + EXTRA_FILTER_CASES:  # all but the 4 MiB one
            ts, bs, nbytes, nbuf = case
            for shuffle in (1, 2):
                rng = np.random.default_rng(ts * 1000 + bs + nbytes + shuffle)
                host = rng.integers(0, 256, nbytes * nbuf, dtype=np.uint8)
                host[: nbytes // 3] = 0
                d_src = to_device(host)
                d_dst = empty_device(host.size + PAD)
                d_dst.fill_(POISON)
                self.aqz.blosc_filter_device(shuffle, ts, bs, d_src.data_ptr(), nbytes, nbuf,
                                             d_dst.data_ptr(), launch_stream())
                raw = from_device(d_dst, np.uint8, (-1,))
                want = np.concatenate([
                    self.oracle.blosc_filter(host[k * nbytes:(k + 1) * nbytes], shuffle, ts, bs)
                    for k in range(nbuf)])
                d, p = byte_counts(raw[:host.size], want)
                stray = int(np.count_nonzero(raw[host.size:] != POISON))
                self.report(filter_id(case, shuffle), d, p, stray)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", required=True, choices=["cascade", "tiled", "volume", "volume_tiled", "codec"])
    args = ap.parse_args()
    r = Runner()
    getattr(r, args.family)()
    print(f"TOTAL {r.total} differing", flush=True)


if __name__ == "__main__":
    main()
