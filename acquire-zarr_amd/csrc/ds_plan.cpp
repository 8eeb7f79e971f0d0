// ds_plan.cpp — the launch decisions of ds_plan.hh, with the measurements
// behind each rule.  Host arithmetic only: compiled once, no HIP header.
#include "ds_plan.hh"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace aqz {

LaunchSwitches
LaunchSwitches::from(const std::function<const char*(const char*)>& get)
{
    auto int_env = [&](const char* name, int dflt) {
        const char* e = get(name);
        return (e && *e) ? std::atoi(e) : dflt;
    };
    LaunchSwitches s;
    s.load_nt = int_env("AQZ_LOAD_NT", -1);
    s.store_wb = int_env("AQZ_STORE_WB", -1);
    s.split_loads = int_env("AQZ_SPLIT_LOADS", 0) != 0;
    s.xcd_remap = int_env("AQZ_XCD_REMAP", -1);
    s.cascade_narrow = int_env("AQZ_CASCADE_NARROW", -1);
    s.cascade_waves = uint32_t(std::clamp(int_env("AQZ_CASCADE_WAVES", 4), 1, 8));
    s.unit_order = uint32_t(std::clamp(int_env("AQZ_UNIT_ORDER", 0), 0, 2));
    s.units_per_wave = int_env("AQZ_UNITS_PER_WAVE", 0);
    const char* staging = get("AQZ_BAND_STAGING");
    s.band_off = staging && std::strcmp(staging, "0") == 0;
    s.band_last = int_env("AQZ_BAND_LAST", -1);
    s.band_mis_max = int_env("AQZ_BAND_MIS_MAX", -1);
    s.band_mis_seg = std::min(int_env("AQZ_BAND_MIS_SEG", -1), 8);
    s.band_force = uint32_t(int_env("AQZ_BAND_FORCE", 0));
    s.band_aligned = int_env("AQZ_BAND_ALIGNED", 1) != 0;
    s.band_segments = int_env("AQZ_BAND_SEGMENTS", 1) != 0;
    s.band_seg4 = int_env("AQZ_BAND_SEG4", -1);
    s.band_segn = int_env("AQZ_BAND_SEGN", 0);
    s.band_wg = int_env("AQZ_BAND_WG", 1) != 0;
    s.band_lds_cap = int_env("AQZ_BAND_LDS_CAP", 0);
    s.tiled_narrow = int_env("AQZ_TILED_NARROW", -1);
    s.tiled_zwaves = int_env("AQZ_TILED_ZWAVES", -1);
    s.tiled_zrows_per_wave = int_env("AQZ_TILED_ZROWS_PER_WAVE", -1);
    s.tiled_band_wg = int_env("AQZ_TILED_BAND_WG", 0) != 0;
    s.tiled_waves = int_env("AQZ_TILED_WAVES", 0);
    s.volume_nt = int_env("AQZ_VOLUME_NT", -1);
    s.volume_upw = int_env("AQZ_VOLUME_UPW", 0);
    s.volume_zfast = int_env("AQZ_VOLUME_ZFAST", -1);
    return s;
}

const LaunchSwitches&
launch_switches()
{
    static const LaunchSwitches s = LaunchSwitches::from_env();
    return s;
}

size_t
dtype_bytes(int dtype)
{
    // u8 u16 u32 u64 i8 i16 i32 i64 f32 f64
    static const uint8_t bytes[10] = {1, 2, 4, 8, 1, 2, 4, 8, 4, 8};
    return dtype >= 0 && dtype < 10 ? bytes[dtype] : 0;
}

uint32_t
grid_for(uint64_t work_items, uint32_t per_block, uint32_t cap)
{
    uint64_t blocks = (work_items + per_block - 1) / per_block;
    if (blocks < 1)
        blocks = 1;
    if (cap && blocks > cap)
        blocks = cap;
    return uint32_t(blocks);
}

namespace {

// Non-temporal loads unless the frame rows are not whole 128-B lines: there a
// line straddles two waves' row segments, and without the streaming hint the
// second wave finds it in L2 (3000^2 u16: 2.7% fewer read requests, 4%
// faster; aligned rows lose 6% without the hint; profiles/r02/loadnt_ab.log).
uint32_t
load_nt(uint32_t W, size_t bpp, const LaunchSwitches& sw)
{
    if (sw.load_nt >= 0)
        return sw.load_nt != 0;
    return (uint64_t(W) * bpp) % 128 == 0;
}

// Columns of T per lane in the fused cascade (kCascadeCols, ds_kernels.hip):
// 16 bytes for 1- and 2-byte types, 32 bytes for 4- and 8-byte types.
uint32_t
cascade_cols(size_t bpp)
{
    return uint32_t((bpp >= 4 ? 32 : 16) / bpp);
}

// LDS a band workgroup may use: the device's per-workgroup maximum (160 KiB
// on gfx950, so f32 bands of 8 waves, 85 KiB, fit; the caller's lds_cap);
// $AQZ_BAND_LDS_CAP (bytes) lowers it for A/B.
uint32_t
band_lds_cap(uint32_t lds_cap, const LaunchSwitches& sw)
{
    return sw.band_lds_cap > 0 ? std::min(lds_cap, uint32_t(sw.band_lds_cap)) : lds_cap;
}

// Bytes of LDS cascade_band_kernel needs for a band (upper bound over
// bands; 0 if no level is staged).
uint32_t
band_lds_bytes(size_t b, const LevelOut* outs, int n_out, uint32_t stage_mask,
               uint32_t seg_cols = 0, bool rowwise = false)
{
    uint64_t total = 0;
    for (int i = 0; i < n_out; ++i) {
        if ((stage_mask >> i) & 1u) {
            const uint64_t rows = uint64_t(1) << (n_out - i - 1);
            const uint64_t w = seg_cols ? std::min<uint64_t>(seg_cols >> (i + 1), outs[i].w)
                                        : outs[i].w;
            if (rowwise)
                total += rows * ((w * b + 30) & ~uint64_t(15)); // StageCtx::rowb slots
            else
                total += (15 + rows * w * b + 15) & ~uint64_t(15);
        }
    }
    return total > (1u << 30) ? (1u << 30) : uint32_t(total);
}

// Can the fused cascade run this level run with C columns per lane?
bool
cascade_fits(size_t b, const void* src, uint32_t W, uint32_t H, const LevelOut* outs, int n_out,
             uint32_t C)
{
    if (!b || C == 0 || n_out < 1 || n_out > kMaxFusedLevels || W == 0 || H == 0)
        return false;
    // Frames of any width and byte offset: loads and stores take any
    // alignment; a lane straddling a row end loads one vector (load_chunk)
    // and stores element by element (store_level).  Needs element-aligned
    // buffers and a row of at least one load (E elements); narrower frames
    // take the single-level kernels.
    const size_t lb = std::min<size_t>(16, size_t(C) * b);
    if (reinterpret_cast<uintptr_t>(src) % b != 0 || W < lb / b)
        return false;
    uint32_t w = W, h = H;
    for (int i = 0; i < n_out; ++i) {
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        if (outs[i].w != w || outs[i].h != h)
            return false;
        if (reinterpret_cast<uintptr_t>(outs[i].ptr) % b != 0)
            return false;
    }
    return true;
}

// 16-byte tiles for 4- and 8-byte types: rows whose level 1-4 rows are all
// whole 64-B bursts (cascade_pick_cols, cascade_tiled_cols)
bool
narrow_rows(size_t b, uint32_t W)
{
    return b >= 4 && (uint64_t(W) * b) % 1024 == 0;
}

template<typename... A>
std::string
line(const char* fmt, A... a)
{
    char buf[320]; // the launch log's line length
    std::snprintf(buf, sizeof(buf), fmt, a...);
    return buf;
}

} // namespace

uint32_t
cascade_pick_cols(int dtype, const void* src, uint64_t, uint32_t W, uint32_t H,
                  const LevelOut* outs, int n_out, const LaunchSwitches& sw)
{
    const size_t b = dtype_bytes(dtype);
    if (!b)
        return 0;
    // wide tiles (kCascadeCols) where a wave's 64 lanes fit in the frame;
    // half-width tiles for narrower frames (a 512-px u8 frame would leave half
    // of every wide wave idle on the edge path) and for widths only the
    // narrow tile divides
    const uint32_t cw = cascade_cols(b), cn = cw / 2;
    const bool wide = cascade_fits(b, src, W, H, outs, n_out, cw);
    const bool narrow = cascade_fits(b, src, W, H, outs, n_out, cn);
    // 4-byte types on rows of whole 128-B lines take 16-byte tiles too (4
    // columns per lane: 73 VGPRs, 6 waves per SIMD, against 138 VGPRs and 3
    // waves for 32-byte tiles) now that such rows leave through LDS-staged
    // bands: 4096^2 f32 Mean 985 -> 948 us, Max 992 -> 946, Decimate 604 ->
    // 583, 8192x2048 947 -> 903, 3072^2 1105 -> 1018 (profiles/r05/narrow/;
    // round 1, before band staging, had measured the opposite, 1083 -> 975
    // us for the wide tiles).  Rows that split lines keep the wide tiles and
    // their misaligned segments: 5472x3648 1091 against 1206 us narrow,
    // 6000x4000 1049 against 1150, 2000^2 1085 against 1123.  The same holds
    // for the other 4- and 8-byte types at 4096^2: u32 Mean 994 -> 947 us,
    // f64 Mean 1034 -> 884, f64 Max 1056 -> 889 (profiles/r05/widths/).
    // "Whole lines" must hold for the levels too, not only level 0: f32
    // 5472x3648 (21888-B rows, level 2 splits bursts) ran 1155 us narrow
    // against 1065-1091 wide (profiles/r05/shapes/), so the rule asks for
    // W * b a multiple of 1024 (levels 1-4 rows whole 64-B bursts).
    // $AQZ_CASCADE_NARROW=0/1 (A/B) forces wide / narrow for 4- and 8-byte
    // types.
    const bool prefer_narrow = sw.cascade_narrow >= 0 ? (sw.cascade_narrow != 0 && b >= 4)
                                                      : narrow_rows(b, W);
    if (prefer_narrow && narrow)
        return cn;
    if (wide && W >= 64 * cw)
        return cw;
    if (narrow)
        return cn;
    return wide ? cw : 0;
}

CascadePlan
plan_cascade(int dtype, int method, const void* src, uint64_t src_frame_elems, uint32_t W,
             uint32_t H, const LevelOut* outs, int n_out, uint32_t n_frames, uint32_t lds_cap,
             const LaunchSwitches& sw)
{
    CascadePlan p;
    const uint32_t cols = cascade_pick_cols(dtype, src, src_frame_elems, W, H, outs, n_out, sw);
    if (cols == 0 || n_frames == 0 || !method_valid(method))
        return p;
    const size_t b = dtype_bytes(dtype);
    const uint32_t CW = cascade_cols(b), CN = CW / 2;
    lds_cap = band_lds_cap(lds_cap, sw);
    p.dtype = dtype;
    p.method = method;
    p.n_out = n_out;
    p.bytes = uint32_t(b);
    p.cols = cols;
    p.units_x = (W + 64 * cols - 1) / (64 * cols);
    const uint32_t R = 1u << n_out;
    p.units_y = (H + R - 1) / R;
    const uint64_t total = uint64_t(p.units_x) * p.units_y * n_frames;
    if (total >= (1ull << 31))
        return p;
    p.total_units = uint32_t(total);
    // 4 waves per block, one tile per wave per iteration.
    const uint32_t wpb = sw.cascade_waves;
    const uint32_t order = sw.unit_order;
    // Units per wave (cascade_kernel's loop): a Decimate wave whose unit
    // reads under 4 KiB takes 2, 4 or 8 consecutive units, so that it
    // moves at least that much: 512^2 u8 Decimate (1 KiB read per unit)
    // 55.3 -> 40.7 us with 4 (8: 45.8).  Other methods keep one unit per
    // wave and, where that unit is under 4 KiB, load plain: 512^2 u8
    // Mean 61.4-62.0 -> 59.4-59.8 us, Max 61.8 -> 60.6-61.2 against two
    // units with nontemporal loads.  Round 5, with the input and output
    // in HBM (rotating buffer sets); round 4's
    // two-unit Mean/Max choice had been timed with the whole read set
    // resident in the Infinity Cache.  2048^2 u16 Decimate (4 KiB units)
    // keeps 1 (two: 76.5 -> 78.8-80.1 us).  $AQZ_UNITS_PER_WAVE=k forces k.
    uint32_t upw = 1;
    bool small_plain = false;
    if (sw.units_per_wave > 0) {
        upw = uint32_t(std::min(sw.units_per_wave, 16));
    } else {
        const uint64_t unit_bytes = (uint64_t(R) * 64u * cols * b) >>
                                    (method == kDecimate ? 1 : 0);
        if (method == kDecimate) {
            while (upw < 8 && unit_bytes * upw < 4096)
                upw *= 2;
        } else {
            small_plain = unit_bytes < 4096;
        }
    }
    p.upw = order == 0 ? upw : 1u;
    const uint32_t grid = grid_for((total + p.upw - 1) / p.upw, wpb, 0);
    p.main_blocks = grid;
    p.order = order;
    p.remap = sw.xcd_remap == 1;
    p.wb = sw.store_wb >= 0 ? uint32_t(sw.store_wb) : 0u;
    p.nt = load_nt(W, b, sw);
    // Loads keep the nontemporal hint on aligned rows, Decimate's looped
    // small units included (512^2 u8 Decimate 40.7 us against 42.1-42.5
    // plain, with the data in HBM; the round-5 plain-load rule had been
    // timed with its 128 MiB read set resident in the Infinity Cache,
    // DESIGN.md §11.11), except the small single units above.
    if (sw.load_nt < 0 && small_plain)
        p.nt = 0;
    // Band staging when some level's rows are not whole 64-byte bursts
    // and a row band is at most 4 tiles, 6 for 2-byte types
    // ($AQZ_BAND_STAGING=0: never; $AQZ_BAND_MIS_MAX: the widest such
    // band).  These bands are stored by their last wave to finish
    // (p.band_last = 1), not after a barrier: any wait for the band's
    // slowest wave cost more than staging saves (u16 3000^2 805 us with
    // a barrier, 594 / 676 us with the last two / three waves storing,
    // 546 us with the last one, against 575 us for direct stores;
    // profiles/r03/misaligned/last_wave_ab.log).  Against the barrier
    // form of <= 4 tiles and direct stores above (mis6_edges_ab.log):
    // u16 2000^2 570 -> 523 us, 2304^2 565 -> 498, 3000^2 575 -> 549,
    // 2600^2 538 -> 547; u8 3000^2 104 -> 85; f32 2000^2 unchanged.
    // One wave storing a wider band is too slow: u16 4000x3000 (8 tiles)
    // 557 -> 627 us, u8 5000x4000 (5 tiles) 91 -> 101, f32 3000^2 (6
    // tiles, 64 KiB) 1095 -> 1442, so those keep direct stores.  Aligned
    // bands keep the barrier, where all waves share the stores (4096^2
    // f32 987 us against 1026 / 1058 us).  $AQZ_BAND_LAST=K forces the
    // last K waves to store every band (0: the barrier).  Also tried and
    // dropped: waves storing the bursts inside their own tile from
    // registers and the last wave only the shared ones (5-27% slower).
    // 16-byte tiles of 4-byte types move 1 KiB per row per wave, as the
    // 2-byte tiles do, so they share the 2-byte thresholds
    const bool tile16 = b == 2 || (b == 4 && cols == CN);
    const uint32_t mis_max = sw.band_mis_max >= 0 ? uint32_t(std::min(sw.band_mis_max, 8))
                                                  : (tile16 ? 6u : 4u);
    uint32_t stage_mask = 0;
    for (int i = 0; i < n_out; ++i) {
        const bool whole = (uint64_t(outs[i].w) * b) % 64 == 0 &&
                           (outs[i].frame_elems * b) % 64 == 0 &&
                           reinterpret_cast<uintptr_t>(outs[i].ptr) % 64 == 0;
        if (!whole)
            stage_mask |= 1u << i;
    }
    // Aligned frames of 4-8 tiles per row band (the headline's 4096 u16
    // pixels, 3072, 4096 f32, config C2's 2048 u16) stage every level
    // too, in workgroups of one wave per tile, so each level's band
    // leaves as one contiguous span.  4-tile bands joined in round 5,
    // timed with the data in HBM (rotating buffer sets): C2 Mean 123.0-
    // 123.5 -> 118.1-118.4 us, Decimate 76.7-76.9 -> 72.1-72.4
    // (profiles/r05/c2knobs/ab.log).
    // On most MI355X boxes tried, row-major level rows at a >= 4 KiB
    // pitch written 512 B per wave ran 15-20% below the same kernel with
    // tile-order stores; staged bands remove that (headline 535 -> 463
    // us, 3072^2 541 -> 448 us; profiles/r02/band8_*).
    // $AQZ_BAND_ALIGNED=0 turns this off; $AQZ_BAND_FORCE (A/B) stages a
    // level mask whatever the alignment, in bands of up to 8 waves.
    // Aligned bands wider than 8 tiles go in 8-tile segments, one
    // workgroup each, every level row of a segment one contiguous piece:
    // 8192x2048 u16 517 -> 485 us, 8704x2040 532 -> 447 us, 6144x3072
    // 531 -> 516 us, 8192x2048 f32 1012 -> 962 us
    // (profiles/r02/band8/segments_ab.log); $AQZ_BAND_SEGMENTS=0: off.
    uint32_t band_waves = p.units_x;
    const uint32_t all_levels = (1u << n_out) - 1u;
    uint32_t wide_max = mis_max, seg_tiles = 0;
    const bool misaligned = stage_mask != 0;
    p.band_last = sw.band_last >= 0 ? uint32_t(std::min(sw.band_last, 8))
                                    : (misaligned ? 1u : 0u);
    if (sw.band_force) {
        stage_mask |= sw.band_force & all_levels;
        wide_max = 8;
    } else if (sw.band_aligned && stage_mask == 0 && band_waves >= 4 && band_waves <= 8 &&
               band_lds_bytes(b, outs, n_out, all_levels) <= lds_cap) {
        stage_mask = all_levels;
        wide_max = 8;
        // 8-tile bands go in segments (first measured as two of 4 tiles,
        // below): a whole 4096 f32 band
        // needs 85 KiB of LDS, one workgroup per CU, whose loads and
        // stores then never overlap; segments fit two or three.  Same
        // box, two rounds (profiles/r03/f32/band_seg4_ab.log): f32 Max
        // 1062 -> 999 us, Mean 1042 -> 991, Min 1064 -> 998, the headline
        // 478 -> 473; 6-tile bands lost (3072^2 470 -> 510), so only
        // bands of 8.  $AQZ_BAND_SEG4=0 / 1: never / always.
        // Tiles per segment: 3 (segments of 3, 3, 2) for 2-byte Mean and
        // for Decimate, 4 otherwise.  Same box, two rounds each
        // (profiles/r03/f32/segment_tiles_ab*.log): headline (u16 Mean)
        // 473-475 -> 462-463 us, 4096x2160 469-473 -> 461-462, u16
        // Decimate 297 -> 294, f32 Decimate 644-652 -> 607-608; but u16
        // Min/Max 472-474 -> 480-483 and f32 Mean/Min/Max 990-1000 ->
        // 1027-1030, which keep 4.  $AQZ_BAND_SEGN overrides (A/B).
        const uint32_t segn = sw.band_segn > 0 ? uint32_t(std::min(sw.band_segn, 8))
                              : (method == kDecimate || (method == kMean && b == 2))
                                ? 3u : 4u;
        if (sw.band_seg4 == 1 || (sw.band_seg4 < 0 && band_waves == 8)) {
            seg_tiles = segn;
            band_waves = segn;
        }
    } else if (sw.band_aligned && sw.band_segments && stage_mask == 0 && band_waves > 8 &&
               band_lds_bytes(b, outs, n_out, all_levels, 8u * 64u * cols) <= lds_cap) {
        stage_mask = all_levels;
        seg_tiles = 8;
        band_waves = 8;
        wide_max = 8;
    } else if (misaligned && band_waves > mis_max && (b == 2 || b == 4) &&
               // exactly the tiles the dispatch builds a rowwise (RW) band
               // kernel for (2-byte narrow tiles have none)
               (cols == CW || (b == 4 && cols == CN)) &&
               (sw.band_mis_seg > 0 || (sw.band_mis_seg < 0 && band_waves > 8))) {
        // Misaligned bands of more than 8 tiles (2- and 4-byte types, wide
        // tiles): balanced segments of at most 4 tiles
        // ($AQZ_BAND_MIS_SEG: any band of those types wider than one
        // wave may store, segments of that many tiles; 0: never), each staged and stored by its last wave,
        // every level row of a segment its own piece (StageCtx::rowb);
        // only the pieces' ends share bursts with the neighbouring
        // segments.  Same box, two rounds, against band workgroups with
        // direct stores (profiles/r03/misaligned/mis_segments_ab*.log):
        // f32 5472x3648 1264 -> 1092 us, 6000x4000 1167 -> 1104, 4100^2
        // 1150 -> 1077; u16 6000x4000 585 -> 557, 5472x3648 534 -> 530.
        // Narrower bands lost or tied (u16 4000x3000 557 -> 612 us, f32
        // 3000^2 1099 -> 1428), and u8 gained only at exactly 6 tiles in
        // 2-tile segments, so those keep direct stores.
        const uint32_t mis_seg = sw.band_mis_seg > 0 ? uint32_t(sw.band_mis_seg) : 4u;
        const uint32_t nseg = (p.units_x + mis_seg - 1) / mis_seg;
        seg_tiles = (p.units_x + nseg - 1) / nseg;
        band_waves = seg_tiles;
        p.seg_rowwise = 1;
        // these segments are stored by their last two waves when level
        // 1's rows split bursts: u16 6000x4000 556 -> 543 us, 5472x3648
        // 535 -> 523, 4100^2 597 -> 582, f32 6000x4000 1085 -> 1045,
        // 4100^2 1074 -> 1060; but f32 5472x3648 (level 1 whole bursts)
        // 1087 -> 1117, so it keeps one (same box, two rounds,
        // profiles/r04/misseg/).  Whole misaligned bands of <= 6 tiles
        // keep one too (3000^2 548-550 -> 600 us with two).
        if (sw.band_last < 0)
            p.band_last = (stage_mask & 1u) ? 2u : 1u;
    }
    const uint32_t lds = band_lds_bytes(b, outs, n_out, stage_mask, seg_tiles * 64u * cols,
                                        p.seg_rowwise != 0);
    p.band = stage_mask && !sw.band_off && band_waves <= wide_max && lds <= lds_cap &&
             total < (1ull << 31);
    p.valid = true;
    if (p.band) {
        const uint32_t segs = seg_tiles ? (p.units_x + seg_tiles - 1) / seg_tiles : 1u;
        p.grid = p.units_y * n_frames * segs;
        p.block = 64 * band_waves;
        p.lds = lds;
        p.stage_mask = stage_mask;
        p.seg_tiles = seg_tiles;
        // whole-line loads for 4- and 8-byte types at the wide tile
        // (cascade_unit SPLIT); misaligned segments have no such form
        p.split = !p.seg_rowwise && b >= 4 && cols == CW && sw.split_loads;
        return p;
    }
    // Direct stores of rows that split 64-B bursts, bands wider than the
    // staged form takes: one workgroup per band (or per balanced piece
    // of <= 8 tiles), so a burst shared by neighbouring waves is written
    // through one L2.  3000^2 622 -> 576 us, 2600^2 601 -> 540 us,
    // 5472x3648 571 -> 540 us against 4-wave blocks that straddle bands
    // (profiles/r03/misaligned/); $AQZ_BAND_WG=0: off.
    p.grid = grid;
    p.block = 64 * wpb;
    if (sw.band_wg && stage_mask && !sw.band_force && p.order == 0 && p.units_x > 4) {
        const uint32_t nseg = (p.units_x + 7) / 8;
        p.seg_w = (p.units_x + nseg - 1) / nseg;
        p.block = 64 * p.seg_w;
        p.grid = nseg * p.units_y * n_frames;
        p.main_blocks = p.grid;
    }
    return p;
}

// cascade and band lines list the same fields; a band runs one unit per
// wave, columns fastest, without the XCD remap, and a cascade stages nothing
std::string
format_plan(const CascadePlan& p)
{
    const uint32_t upw = p.band ? 1u : (!p.seg_w && p.order == 0) ? std::max(p.upw, 1u) : 1u;
    return line("family=%s dtype=%u method=%d n_out=%d grid=%u block=%u units=%u units_x=%u "
                "cols=%u nt=%u upw=%u order=%u remap=%u wb=%u stage_mask=%u seg_tiles=%u "
                "seg_rowwise=%u band_last=%u seg_w=%u split=%d lds=%u",
                p.band ? "band" : "cascade", p.bytes, p.method, p.n_out, p.grid, p.block,
                p.total_units, p.units_x, p.cols, p.nt, upw, p.band ? 0u : p.order,
                p.band ? 0u : p.remap, p.wb, p.stage_mask, p.seg_tiles,
                p.band ? p.seg_rowwise : 0u, p.band ? p.band_last : 0u, p.seg_w, int(p.split),
                p.lds);
}

uint32_t
cascade_tiled_cols(int dtype, uint32_t W, const LaunchSwitches& sw)
{
    // cascade_pick_cols for element-aligned buffers: wide tiles once a wave's
    // 64 lanes fit in the frame, half-width ones below
    const size_t b = dtype_bytes(dtype);
    if (!b)
        return 0;
    const uint32_t cw = cascade_cols(b);
    // $AQZ_TILED_NARROW (A/B): 1 half-width tiles wherever they fit, 0 wide;
    // unset: half-width for 4- and 8-byte types on rows whose levels are
    // whole bursts (narrow_rows), as cascade_pick_cols (the streaming path writes a run tiled in one launch
    // only when both agree): chunk-tiled 4096^2 f32 964-979 against
    // 995-1033 us wide; 5472x3648, 6000x4000 and 2000^2 keep wide tiles
    // (1113 / 990 / 1031 against 1129 / 1074 / 1055 us narrow;
    // profiles/r05/narrow/ab_shapes.log)
    const int narrow = sw.tiled_narrow;
    if ((narrow == 1 || (narrow < 0 && narrow_rows(b, W))) &&
        W >= 64 * (cw / 2))
        return cw / 2;
    return W >= 64 * cw ? cw : cw / 2;
}

namespace {

// cascade_tiled_slots for level >= 1, cascade_tiled_base_slots for level 0
uint32_t
tiled_slots_at(int dtype, uint32_t W, int n_out, int level, uint32_t tile_rows,
               uint32_t tile_cols, uint32_t* slots_x, const LaunchSwitches& sw)
{
    const uint32_t cols = cascade_tiled_cols(dtype, W, sw);
    const uint32_t cw = (64u * cols) >> level;       // level columns per wave block
    const uint32_t rh = (1u << n_out) >> level;      // level rows per wave block
    const uint32_t co = std::max(1u, cols >> level); // columns per lane store
    if (slots_x)
        *slots_x = 1;
    if (cols == 0 || level < 0 || level > n_out || tile_rows == 0 || tile_cols == 0 ||
        tile_rows % rh != 0)
        return 0;
    // blocks inside tiles: one slot per block; blocks spanning whole tiles
    // (and lane stores inside one tile): one slot per (tile, block row)
    uint32_t sx = 0;
    if (tile_cols % cw == 0)
        sx = tile_cols / cw;
    else if (cw % tile_cols == 0 && tile_cols % co == 0)
        sx = 1;
    if (sx == 0)
        return 0;
    if (slots_x)
        *slots_x = sx;
    return (tile_rows / rh) * sx;
}

} // namespace

uint32_t
cascade_tiled_slots(int dtype, uint32_t W, int n_out, int level, uint32_t tile_rows,
                    uint32_t tile_cols, uint32_t* slots_x, const LaunchSwitches& sw)
{
    if (level < 1) {
        if (slots_x)
            *slots_x = 1;
        return 0;
    }
    return tiled_slots_at(dtype, W, n_out, level, tile_rows, tile_cols, slots_x, sw);
}

uint32_t
cascade_tiled_base_slots(int dtype, uint32_t W, int n_out, uint32_t tile_rows,
                         uint32_t tile_cols, uint32_t* slots_x, const LaunchSwitches& sw)
{
    return tiled_slots_at(dtype, W, n_out, 0, tile_rows, tile_cols, slots_x, sw);
}

TiledPlan
plan_cascade_tiled(int dtype, int method, const void* src, uint64_t src_frame_elems, uint32_t W,
                   uint32_t H, const LevelOut* outs, const TiledOut* touts, int n_out,
                   uint32_t n_frames, const LaunchSwitches& sw, const TiledOut* tbase)
{
    TiledPlan p;
    // the flag layout (cascade_tiled_slots) assumes the geometry-only choice;
    // cascade_pick_cols != 0 says the buffers and level sizes fit the fused
    // cascade (its conditions do not depend on the tile width)
    const uint32_t cols = cascade_tiled_cols(dtype, W, sw);
    const size_t b = dtype_bytes(dtype);
    if (cols == 0 || n_frames == 0 || !method_valid(method) ||
        cascade_pick_cols(dtype, src, src_frame_elems, W, H, outs, n_out, sw) == 0)
        return p;
    const uint32_t R = 1u << n_out;
    p.dtype = dtype;
    p.method = method;
    p.n_out = n_out;
    p.bytes = uint32_t(b);
    p.cols = cols;
    p.n_frames = n_frames;
    // The grid's blocks cover the frame; zero-fill waves cover the rest of
    // the padded tile area.
    p.units_x = (W + 64 * cols - 1) / (64 * cols);
    p.units_y = (H + R - 1) / R;
    const uint64_t total = uint64_t(p.units_x) * p.units_y * n_frames;
    if (total >= (1ull << 30))
        return p;
    p.total_units = uint32_t(total);
    bool flag_fill = false;
    uint64_t zitems_frame = 0; // p.zitems before it is known to fit 32 bits
    // level `lvl` of the launch (0: the input itself, `tbase`), w x h
    const auto plan_level = [&](TiledLevelPlan& q, const TiledOut& t, int lvl, uint32_t w,
                                uint32_t h) {
        if (!t.ptr || t.tile_rows == 0 || t.tile_cols == 0 ||
            reinterpret_cast<uintptr_t>(t.ptr) % b != 0)
            return false;
        q.ntx = (w + t.tile_cols - 1) / t.tile_cols;
        q.nty = (h + t.tile_rows - 1) / t.tile_rows;
        const uint64_t pw = uint64_t(q.ntx) * t.tile_cols, ph = uint64_t(q.nty) * t.tile_rows;
        if (pw >= (1ull << 31) || ph >= (1ull << 31))
            return false;
        q.tframe_elems = pw * ph;
        q.tstride = t.frame_offsets ? t.tile_stride : uint64_t(t.tile_rows) * t.tile_cols;
        if (q.tstride < uint64_t(t.tile_rows) * t.tile_cols)
            return false;
        q.pw = uint32_t(pw);
        q.ph = uint32_t(ph);
        // below 2^31: units_x * 64 * cols < W + 64 * cols, units_y * R < H + R
        q.cov_w = uint32_t((uint64_t(p.units_x) * (64u * cols)) >> lvl);
        q.cov_h = uint32_t((uint64_t(p.units_y) * R) >> lvl);
        q.zrows = q.cov_w < pw ? uint32_t(ph) : (q.cov_h < ph ? uint32_t(ph) - q.cov_h : 0u);
        zitems_frame += q.zrows;
        q.slots = tiled_slots_at(dtype, W, n_out, lvl, t.tile_rows, t.tile_cols, &q.slots_x, sw);
        if (!q.slots)
            p.nested = false;
        q.flags_frame = q.ntx * q.nty * std::max<uint32_t>(1, q.slots);
        if (t.nonzero && q.slots && (q.cov_w < pw || q.cov_h < ph))
            flag_fill = true;
        q.clear_flags = t.nonzero && !q.slots;
        return true;
    };
    for (int i = 0; i < n_out; ++i)
        if (!plan_level(p.lv[i], touts[i], i + 1, outs[i].w, outs[i].h))
            return p;
    if (tbase) {
        if (!plan_level(p.base_lv, *tbase, 0, W, H))
            return p;
        p.base = true;
    }
    // zero-fill waves: a whole number of 8-block (one per XCD) groups
    // (the kernel walks the base's items and the levels' one after the other,
    // each count in 32 bits: the sum is held to that)
    const uint64_t zitems = zitems_frame * n_frames;
    if (zitems >= (1ull << 32))
        return p;
    p.zitems = uint32_t(zitems_frame) - p.base_lv.zrows; // the levels' alone
    // One zero-fill wave per 128 KiB of overhang (64..4096).  The waves run
    // first and hold their slots while the cascade blocks start; one per
    // item (up to 4096) cost 4-5% at 3000^2 and 5472x3648 against 512, and
    // putting them after the cascade blocks made them the kernel's tail
    // (profiles/r02/tiled_zero_fill_ab.log).
    uint64_t zbytes = 0;
    for (int i = p.base ? -1 : 0; i < n_out; ++i) {
        const TiledLevelPlan& q = i < 0 ? p.base_lv : p.lv[i];
        const uint64_t cw = std::min(q.cov_w, q.pw), chh = std::min(q.cov_h, q.ph);
        zbytes += (uint64_t(q.pw) * q.ph - cw * chh) * b;
    }
    zbytes *= n_frames;
    // ... and for 1-byte types at most ZI = 32 overhang rows per wave: each
    // row is a short dependent loop, and the byte rule left u8 pyramids
    // (chunk 128, rows of a few dozen bytes) with thousands of rows per
    // wave, the kernel's tail.  Same box (profiles/r04/zrows/ab.log): u8
    // 2600^2 262 -> 111 us, 2304^2 273 -> 131, 1500^2 189 -> 113, 3000^2
    // 141 -> 93, 5000x4000 100 -> 81; the same cap cost u16 2-4% (3000^2
    // 516-519 -> 528-531 us), so wider types keep the byte rule.
    // $AQZ_TILED_ZROWS_PER_WAVE: ZI for every type (0: the byte rule alone).
    const int zi = sw.tiled_zrows_per_wave >= 0 ? sw.tiled_zrows_per_wave : (b == 1 ? 32 : 0);
    uint64_t zw = (zbytes >> 17) + 1;
    if (zi > 0)
        zw = std::max<uint64_t>(zw, (zitems + zi - 1) / uint64_t(zi));
    p.zwaves = (zitems || flag_fill)
                 ? uint32_t(std::min<uint64_t>(std::max<uint64_t>(zw, 64), 4096))
                 : 0u;
    if (sw.tiled_zwaves >= 0)
        p.zwaves = uint32_t(sw.tiled_zwaves); // A/B only: 0 leaves the overhang unwritten
    p.remap = sw.xcd_remap == 1;
    // Nontemporal loads on aligned rows for every unit size: with the data
    // in HBM (rotating buffer sets) chunk-tiled 2048^2
    // u16 Decimate runs 73.8-73.9 us with them against 79.0-79.7 plain, and
    // 512^2 u8 Decimate / Mean 73.1-73.5 / 82.6-82.7 against 74.1 / 83.4-
    // 84.8.  (A round-5 plain-load rule for units of <= 4 KiB had been timed
    // with the read set resident in the Infinity Cache.)
    p.nt = load_nt(W, b, sw);
    // $AQZ_TILED_BAND_WG=1 (A/B, off by default): on rows that split 128-B
    // lines, one workgroup per row band (or balanced piece of <= 8 tiles), as
    // the row-major launcher does, so that the two waves sharing a line read
    // it through one L2.  Reads drop to 1.00-1.01x the frame (from 1.02-1.05x)
    // but every shape got slower: u16 3000^2 543 -> 615 us, 5472x3648 517 ->
    // 610, 6000x4000 503 -> 597, 2000^2 507 -> 511, f32 6000x4000 990 -> 1111
    // (same box, two rounds, profiles/r04/tiledwg/).
    if (sw.tiled_band_wg && !p.remap && (uint64_t(W) * b) % 128 != 0 && p.units_x > 1) {
        const uint32_t nseg = (p.units_x + 7) / 8;
        p.seg_w = (p.units_x + nseg - 1) / nseg;
        p.wpb = p.seg_w;
        p.main_blocks = nseg * p.units_y * n_frames;
    } else {
        // Waves per workgroup: 4 when a row band's tile count divides by 4,
        // else 2.  Same box, two rounds (profiles/r04/tiledwaves/): u16
        // 3000^2 541-549 -> 518-521 us, 2304^2 614-621 -> 576-577, 3500^2
        // 552 -> 519, 4600x3000 531 -> 510, f32 5472x3648 1191-1193 -> 1116-
        // 1118, u8 6000x4000 89-96 -> 80-85; but 2-wave blocks lose where 4
        // divide the band (u16 2000^2 505 -> 580, 6000x4000 505 -> 546-550,
        // f32 6000x4000 989 -> 1063), and 3-wave blocks lose on 6 tiles
        // (3000^2 574-576).  $AQZ_TILED_WAVES (1..8) forces a count (A/B).
        p.wpb = sw.tiled_waves > 0 ? uint32_t(std::min(sw.tiled_waves, 8))
                                   : (p.units_x % 4 == 0 ? 4u : 2u);
        p.main_blocks = grid_for(total, p.wpb, 0);
    }
    // zero-fill blocks: a whole number of 8-block (one per XCD) groups
    const uint32_t zblocks = ((p.zwaves + p.wpb - 1) / p.wpb + 7) & ~7u;
    p.zwaves = zblocks * p.wpb;
    p.grid = zblocks + p.main_blocks;
    p.block = 64 * p.wpb;
    p.valid = true;
    return p;
}

std::string
format_plan(const TiledPlan& p)
{
    const std::string s =
      line("family=tiled dtype=%u method=%d n_out=%d grid=%u block=%u units=%u "
           "units_x=%u cols=%u nt=%u remap=%u seg_w=%u wpb=%u zwaves=%u nested=%d "
           "main_blocks=%u",
           p.bytes, p.method, p.n_out, p.grid, p.block, p.total_units, p.units_x, p.cols, p.nt,
           p.remap, p.seg_w, p.wpb, p.zwaves, int(p.nested), p.main_blocks);
    if (!p.base)
        return s;
    return s + line(" base=1 base_slots=%u base_slots_x=%u base_zrows=%u", p.base_lv.slots,
                    p.base_lv.slots_x, p.base_lv.zrows);
}

bool
volume_supported(int dtype, const void* src, uint32_t W, uint32_t H, const LevelOut* outs,
                 int n_out)
{
    return n_out >= 1 && n_out <= kMaxVolumeLevels &&
           cascade_fits(dtype_bytes(dtype), src, W, H, outs, n_out,
                        cascade_cols(dtype_bytes(dtype)));
}

VolumePlan
plan_volume(int dtype, int method, const void* src, uint64_t, uint32_t W, uint32_t H,
            const LevelOut* outs, int n_out, uint32_t n_planes, const LaunchSwitches& sw)
{
    VolumePlan p;
    if (!volume_supported(dtype, src, W, H, outs, n_out) || n_planes == 0 ||
        n_planes % (1u << n_out) != 0 || !method_valid(method))
        return p;
    p.dtype = dtype;
    p.method = method;
    p.n_out = n_out;
    p.bytes = uint32_t(dtype_bytes(dtype));
    const uint32_t C = 16 / p.bytes;
    const uint32_t R = 1u << n_out;
    p.units_x = (W + 64 * C - 1) / (64 * C);
    p.units_y = (H + R - 1) / R;
    const uint64_t total = uint64_t(p.units_x) * p.units_y * (n_planes >> n_out);
    if (total >= (1ull << 31))
        return p;
    p.total_units = uint32_t(total);
    // Load policy and units per wave: with the
    // volume in HBM (rotating buffer sets) nontemporal loads beat plain
    // ones for every method, Decimate's every-other-row, every-other-
    // plane reads included (44.0-44.4 against 46.7-47.4 us); Decimate's
    // 4-KiB units go two to a wave (one ties).  The plain-load choice of
    // §11.2 had been timed with Decimate's 128 MiB read set resident in
    // the Infinity Cache.  $AQZ_VOLUME_NT=0/1 and $AQZ_VOLUME_UPW=1/2
    // (Decimate) override.
    p.ntl = sw.volume_nt >= 0 ? sw.volume_nt != 0 : true;
    // $AQZ_VOLUME_UPW=4 (A/B, Decimate): four units per wave, 16 KiB
    // of loads in flight per wave.  Only the nontemporal-load kernels
    // are built for four, so with plain loads ($AQZ_VOLUME_NT=0) the
    // request is clamped to two.  (Until round 6 the grid was sized
    // for four while the one-unit kernel ran, which left three
    // quarters of the units unwritten.)  The grid below is sized from the
    // same upw the dispatch instantiates its kernel with.
    p.upw = method == kDecimate ? (sw.volume_upw >= 4 ? (p.ntl ? 4 : 2)
                                   : sw.volume_upw > 0 ? std::min(sw.volume_upw, 2) : 2)
                                : 1;
    // Decimate launches of 128 or more plane groups (two or more
    // config-V volumes) take the plane groups fastest in the unit
    // order, so the units in flight spread over many planes: four
    // 1024^2 x 256 volumes 172.1-172.3 -> 148.1-149.0 us, data in HBM
    // (profiles/r05/vzfast/ab.log); one volume (64 groups) loses
    // 1-2% that way and keeps columns fastest.  Its reads never set
    // the address bits of odd rows and odd planes.
    // $AQZ_VOLUME_ZFAST=0 / 1: never / always (nontemporal loads, two or
    // four units per wave: the kernels built with that order).
    const bool zfast = sw.volume_zfast >= 0 ? sw.volume_zfast != 0 : (n_planes >> n_out) >= 128;
    p.zfast = zfast && method == kDecimate && p.ntl && p.upw >= 2;
    p.grid = grid_for((total + p.upw - 1) / p.upw, 4, 0);
    p.valid = true;
    return p;
}

std::string
format_plan(const VolumePlan& p)
{
    return line("family=volume dtype=%u method=%d n_out=%d grid=%u block=%u units=%u "
                "units_x=%u upw=%d ntl=%d zfast=%d UPW=%d",
                p.bytes, p.method, p.n_out, p.grid, p.block, p.total_units, p.units_x, p.upw,
                int(p.ntl), int(p.zfast), p.upw);
}

VolumeTiledPlan
plan_volume_tiled(int dtype, int method, const void* src, uint64_t, uint32_t W, uint32_t H,
                  const LevelOut* outs, const TiledOut* touts, int n_out, uint32_t n_planes,
                  const LaunchSwitches& sw)
{
    VolumeTiledPlan p;
    if (!volume_supported(dtype, src, W, H, outs, n_out) || n_planes == 0 ||
        n_planes % (1u << n_out) != 0 || !method_valid(method) || !touts)
        return p;
    const size_t b = dtype_bytes(dtype);
    p.dtype = dtype;
    p.method = method;
    p.n_out = n_out;
    p.bytes = uint32_t(b);
    p.n_planes = n_planes;
    // plan_volume's units, one per wave, columns first
    const uint32_t C = 16 / p.bytes;
    const uint32_t R = 1u << n_out;
    const uint32_t groups = n_planes >> n_out;
    p.units_x = (W + 64 * C - 1) / (64 * C);
    p.units_y = (H + R - 1) / R;
    const uint64_t total = uint64_t(p.units_x) * p.units_y * groups;
    if (total >= (1ull << 31))
        return p;
    p.total_units = uint32_t(total);
    uint64_t zitems = 0, zbytes = 0;
    for (int i = 0; i < n_out; ++i) {
        const TiledOut& t = touts[i];
        if (!t.ptr || t.tile_rows == 0 || t.tile_cols == 0 ||
            reinterpret_cast<uintptr_t>(t.ptr) % b != 0)
            return p;
        TiledLevelPlan& q = p.lv[i];
        q.ntx = (outs[i].w + t.tile_cols - 1) / t.tile_cols;
        q.nty = (outs[i].h + t.tile_rows - 1) / t.tile_rows;
        const uint64_t pw = uint64_t(q.ntx) * t.tile_cols, ph = uint64_t(q.nty) * t.tile_rows;
        if (pw >= (1ull << 31) || ph >= (1ull << 31))
            return p;
        q.tframe_elems = pw * ph;
        q.tstride = t.frame_offsets ? t.tile_stride : uint64_t(t.tile_rows) * t.tile_cols;
        if (q.tstride < uint64_t(t.tile_rows) * t.tile_cols)
            return p;
        q.pw = uint32_t(pw);
        q.ph = uint32_t(ph);
        // what the units reach at this level, as in plan_cascade_tiled; the
        // zero-fill waves take the rest of the padded area: columns past
        // cov_w of every padded row, else the rows past cov_h
        q.cov_w = p.units_x * ((64u * C) >> (i + 1));
        q.cov_h = p.units_y * (R >> (i + 1));
        q.zrows = q.cov_w < pw ? uint32_t(ph) : (q.cov_h < ph ? uint32_t(ph) - q.cov_h : 0u);
        // one flag byte per tile, cleared ahead of the kernel (no nested slots)
        q.slots = 0;
        q.slots_x = 1;
        q.flags_frame = q.ntx * q.nty;
        q.clear_flags = t.nonzero != nullptr;
        const uint32_t per_group = 1u << (n_out - 1 - i); // the level's planes per group
        zitems += uint64_t(q.zrows) * per_group;
        const uint64_t cw = std::min(q.cov_w, q.pw), chh = std::min(q.cov_h, q.ph);
        zbytes += (uint64_t(q.pw) * q.ph - cw * chh) * b * per_group;
    }
    if (zitems * groups >= (1ull << 32))
        return p;
    p.zitems = uint32_t(zitems);
    // zero-fill waves by plan_cascade_tiled's rule: one per 128 KiB of
    // overhang, at most 32 overhang rows per wave for 1-byte types, 64..4096
    zbytes *= groups;
    const int zi = sw.tiled_zrows_per_wave >= 0 ? sw.tiled_zrows_per_wave : (b == 1 ? 32 : 0);
    uint64_t zw = (zbytes >> 17) + 1;
    if (zi > 0)
        zw = std::max<uint64_t>(zw, (zitems * groups + zi - 1) / uint64_t(zi));
    p.zwaves = zitems ? uint32_t(std::min<uint64_t>(std::max<uint64_t>(zw, 64), 4096)) : 0u;
    p.wpb = 4;
    p.block = 64 * p.wpb;
    p.main_blocks = grid_for(total, p.wpb, 0);
    // zero-fill blocks: a whole number of 8-block (one per XCD) groups
    const uint32_t zblocks = ((p.zwaves + p.wpb - 1) / p.wpb + 7) & ~7u;
    p.zwaves = zblocks * p.wpb;
    p.grid = zblocks + p.main_blocks;
    p.valid = true;
    return p;
}

std::string
format_plan(const VolumeTiledPlan& p)
{
    std::string s = line("family=volume_tiled dtype=%u method=%d n_out=%d grid=%u block=%u "
                         "units=%u units_x=%u units_y=%u wpb=%u zwaves=%u zitems=%u "
                         "main_blocks=%u",
                         p.bytes, p.method, p.n_out, p.grid, p.block, p.total_units, p.units_x,
                         p.units_y, p.wpb, p.zwaves, p.zitems, p.main_blocks);
    for (int i = 0; i < p.n_out; ++i) {
        const TiledLevelPlan& q = p.lv[i];
        s += line(" ntx%d=%u nty%d=%u pw%d=%u ph%d=%u cov_w%d=%u cov_h%d=%u zrows%d=%u", i + 1,
                  q.ntx, i + 1, q.nty, i + 1, q.pw, i + 1, q.ph, i + 1, q.cov_w, i + 1, q.cov_h,
                  i + 1, q.zrows);
    }
    return s.substr(0, 319); // the launch log's line length
}

ZRunPlan
plan_zrun(int dtype, int method, const void* src, uint64_t src_frame_elems, uint64_t elems,
          const LevelOut* outs, int n_out, uint32_t planes)
{
    ZRunPlan p;
    const size_t b = dtype_bytes(dtype);
    if (!b || !method_valid(method) || n_out < 1 || n_out > kMaxZLevels || planes == 0 ||
        planes % (1u << n_out) != 0 || elems == 0 || elems > (~0ull >> 4) || !src || !outs ||
        src_frame_elems < elems || reinterpret_cast<uintptr_t>(src) % b != 0)
        return p;
    for (int i = 0; i < n_out; ++i)
        if (!outs[i].ptr || outs[i].frame_elems < elems ||
            reinterpret_cast<uintptr_t>(outs[i].ptr) % b != 0)
            return p;
    p.dtype = dtype;
    p.method = method;
    p.n_out = n_out;
    p.bytes = uint32_t(b);
    p.planes = planes;
    p.elems = elems;
    p.groups = planes >> n_out;
    // a plane's bytes in spans; the last one may hold no whole vector at all
    // (the 1..15 bytes behind the last vector go from it element by element)
    const uint64_t spans = (elems * b + kZRunSpanBytes - 1) / kZRunSpanBytes;
    if (spans >= (1ull << 31) || spans * p.groups >= (1ull << 31))
        return p;
    p.spans = uint32_t(spans);
    p.grid = grid_for(spans * p.groups, 4, 0);
    p.valid = true;
    return p;
}

std::string
format_plan(const ZRunPlan& p)
{
    return line("family=zrun dtype=%u method=%d n_out=%d planes=%u groups=%u spans=%u "
                "elems=%llu grid=%u block=%u",
                p.bytes, p.method, p.n_out, p.planes, p.groups, p.spans,
                static_cast<unsigned long long>(p.elems), p.grid, p.block);
}

ZRunTiledPlan
plan_zrun_tiled(int dtype, int method, const void* src, uint64_t src_frame_elems, uint32_t W,
                uint32_t H, const LevelOut* outs, const TiledOut* touts, int n_out,
                uint32_t planes)
{
    ZRunTiledPlan p;
    const size_t b = dtype_bytes(dtype);
    if (!b || W == 0 || H == 0 || !outs || !touts || n_out < 1 || n_out > kMaxZLevels)
        return p;
    const uint64_t elems = uint64_t(W) * H;
    // plan_zrun's rules, with a level's row-major copy optional
    LevelOut rm[kMaxZLevels];
    for (int i = 0; i < n_out; ++i) {
        rm[i] = outs[i];
        if (!rm[i].ptr) {
            rm[i].ptr = const_cast<void*>(src);
            rm[i].frame_elems = elems;
        }
    }
    const ZRunPlan z = plan_zrun(dtype, method, src, src_frame_elems, elems, rm, n_out, planes);
    if (!z.valid)
        return p;
    p.dtype = dtype;
    p.method = method;
    p.n_out = n_out;
    p.bytes = z.bytes;
    p.W = W;
    p.H = H;
    p.planes = planes;
    p.groups = z.groups;
    p.spans = z.spans;
    p.elems = elems;
    uint64_t zitems = 0, zbytes = 0;
    for (int i = 0; i < n_out; ++i) {
        const TiledOut& t = touts[i];
        if (!t.ptr || t.tile_rows == 0 || t.tile_cols == 0 ||
            reinterpret_cast<uintptr_t>(t.ptr) % b != 0)
            return p;
        TiledLevelPlan& q = p.lv[i];
        const uint64_t ntx = (uint64_t(W) + t.tile_cols - 1) / t.tile_cols;
        const uint64_t nty = (uint64_t(H) + t.tile_rows - 1) / t.tile_rows;
        const uint64_t pw = ntx * t.tile_cols, ph = nty * t.tile_rows;
        if (pw >= (1ull << 31) || ph >= (1ull << 31))
            return p;
        q.ntx = uint32_t(ntx);
        q.nty = uint32_t(nty);
        q.tframe_elems = pw * ph;
        q.tstride = t.frame_offsets ? t.tile_stride : uint64_t(t.tile_rows) * t.tile_cols;
        if (q.tstride < uint64_t(t.tile_rows) * t.tile_cols)
            return p;
        q.pw = uint32_t(pw);
        q.ph = uint32_t(ph);
        // the units store the frame and nothing else; the zero-fill waves take
        // the rest of the padded area: columns past W of every padded row,
        // else the rows past H
        q.cov_w = W;
        q.cov_h = H;
        q.zrows = W < pw ? uint32_t(ph) : (H < ph ? uint32_t(ph) - H : 0u);
        q.slots = 0;
        q.slots_x = 1;
        q.flags_frame = q.ntx * q.nty;
        q.clear_flags = t.nonzero != nullptr;
        const uint32_t per_group = 1u << (n_out - 1 - i); // the level's planes per group
        zitems += uint64_t(q.zrows) * per_group;
        zbytes += (pw * ph - elems) * b * per_group;
    }
    if (zitems * p.groups >= (1ull << 32))
        return p;
    p.zitems = uint32_t(zitems);
    // zero-fill waves by plan_volume_tiled's rule: one per 128 KiB of
    // overhang, at most 32 overhang rows per wave for 1-byte types, 64..4096
    zbytes *= p.groups;
    uint64_t zw = (zbytes >> 17) + 1;
    if (b == 1)
        zw = std::max<uint64_t>(zw, (zitems * p.groups + 31) / 32);
    p.zwaves = zitems ? uint32_t(std::min<uint64_t>(std::max<uint64_t>(zw, 64), 4096)) : 0u;
    p.main_blocks = z.grid;
    // zero-fill blocks: a whole number of 8-block (one per XCD) groups
    const uint32_t zblocks = ((p.zwaves + p.wpb - 1) / p.wpb + 7) & ~7u;
    p.zwaves = zblocks * p.wpb;
    p.grid = zblocks + p.main_blocks;
    p.valid = true;
    return p;
}

std::string
format_plan(const ZRunTiledPlan& p)
{
    return line("family=zrun_tiled dtype=%u method=%d n_out=%d planes=%u groups=%u spans=%u "
                "zitems=%u zwaves=%u grid=%u block=%u",
                p.bytes, p.method, p.n_out, p.planes, p.groups, p.spans, p.zitems, p.zwaves,
                p.grid, p.block);
}

int
level_class(const PyramidLevel& in, const PyramidLevel& out)
{
    const bool xy = out.w < in.w || out.h < in.h;
    const bool zh = out.planes < in.planes;
    return xy ? (zh ? kClassXYZ : kClassXY) : (zh ? kClassZ : kClassNone);
}

PyramidRuns
plan_pyramid_runs(const PyramidLevel* lv, uint32_t n_levels, uint32_t n_frames)
{
    PyramidRuns r;
    const auto refuse = [&](const std::string& why) {
        r.reason = why;
        r.runs.clear();
        return r;
    };
    if (!lv || n_levels < 2)
        return refuse("fewer than two levels");
    std::vector<int> cls(n_levels, kClassNone);
    uint32_t zcount = 0;
    for (uint32_t l = 1; l < n_levels; ++l) {
        cls[l] = level_class(lv[l - 1], lv[l]);
        if (cls[l] == kClassNone)
            return refuse("level " + std::to_string(l) + " halves neither XY nor Z");
        if (cls[l] == kClassXY)
            continue;
        if (lv[l - 1].planes % 2 != 0)
            return refuse("level " + std::to_string(l) + " pairs an odd plane count");
        if (lv[l].holds_plane)
            return refuse("level " + std::to_string(l) + " holds an earlier plane");
        if (++zcount >= 32)
            return refuse("32 or more Z-halving levels");
    }
    if (n_frames == 0 || n_frames % (1u << zcount) != 0)
        return refuse("frame count is no nonzero multiple of " + std::to_string(1u << zcount));
    uint32_t frames = n_frames;
    for (uint32_t l = 1; l < n_levels;) {
        uint32_t end = l + 1;
        while (end < n_levels && cls[end] == cls[l])
            ++end;
        const uint32_t depth = uint32_t(cls[l] == kClassXYZ  ? kMaxVolumeLevels
                                        : cls[l] == kClassXY ? kMaxFusedLevels
                                                             : kMaxZLevels);
        for (; l < end; l += std::min(depth, end - l)) {
            const uint32_t k = std::min(depth, end - l);
            r.runs.push_back({ cls[l], l, k, frames });
            if (cls[l] != kClassXY)
                frames >>= k;
        }
    }
    r.ok = true;
    return r;
}

uint32_t
tile_slices(uint32_t tile_rows, uint32_t tile_cols)
{
    // ~8 K elements per block, at most 64 blocks per tile
    const uint64_t tile_elems = uint64_t(tile_rows) * tile_cols;
    return uint32_t(std::min<uint64_t>(64, std::max<uint64_t>(1, tile_elems / 8192)));
}

} // namespace aqz
