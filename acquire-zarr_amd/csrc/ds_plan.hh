// ds_plan.hh — what launch_cascade, launch_cascade_tiled, launch_volume,
// launch_volume_tiled and launch_zrun launch, and how a mixed pyramid is cut
// into runs of them (plan_pyramid_runs): host-only integer arithmetic over the dtype size, method, geometry,
// buffer alignment and the $AQZ_* A/B switches.  No HIP type appears here
// (ds_plan.cpp builds with a plain C++ compiler; tests/cpp/plan_probe.cpp
// runs it on the CPU).  ds_dispatch.cpp builds a plan per launch, logs
// format_plan() of it and hands it to the dtype's kernel shard
// (ds_kernels.hip), which maps the selector fields to template arguments and
// takes grid, block and LDS from the plan as they stand.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

namespace aqz {

constexpr int kMaxFusedLevels = 4;
constexpr int kMaxVolumeLevels = 2;
constexpr int kMaxZLevels = 3;
// zrun_kernel's unit: 64 lanes x kZRunVecs 16-byte vectors of every plane of
// one plane group.
constexpr uint32_t kZRunVecs = 2;
constexpr uint32_t kZRunSpanBytes = 64 * kZRunVecs * 16;

enum
{
    kDecimate = 0,
    kMean = 1,
    kMin = 2,
    kMax = 3
};

// One output level of a cascade launch.  `frame_elems` is the element stride
// between consecutive frames of that level (w*h for densely packed batches).
struct LevelOut
{
    void* ptr;
    uint64_t frame_elems;
    uint32_t w, h;
};

// Chunk-tiled output of one cascade level: frame k of
// the level at ptr + k * n_tiles * tile_rows * tile_cols elements, tile
// t = ty * n_tiles_x + tx holding tile_rows x tile_cols elements row-major,
// zero where it overhangs the level — the layout Array::write_frame_to_chunks_
// fills (array.cpp:507-622, chunk.cpp:17-58).  `nonzero` (optional, device)
// receives the chunk zero scan as flag bytes (cascade_tiled_slots).
// Chunk lattice instead (frame_offsets non-null, device): frame k's tile t at
// ptr + frame_offsets[k] + t * tile_stride elements — every tile straight
// into its chunk buffer at the frame's place in it.
struct TiledOut
{
    void* ptr;
    uint32_t tile_rows, tile_cols;
    uint8_t* nonzero;
    const uint64_t* frame_offsets = nullptr; // elements, n_frames entries
    uint64_t tile_stride = 0;                // elements (with frame_offsets)
};

// The A/B switches of the three launchers, one field per $AQZ_* name, each
// at its "unset" value.  Rationale and measurements stand where a switch is
// used (ds_plan.cpp).
struct LaunchSwitches
{
    // $AQZ_LOAD_NT: 1 / 0 forces the fused cascade's loads with / without the
    // non-temporal hint (A/B only); unset (-1): the planner decides.
    int load_nt = -1;
    // $AQZ_STORE_WB: a level bit mask (bit J-1 = level J) of row-major stores
    // issued write-back instead of non-temporal (A/B).
    int store_wb = -1;
    // $AQZ_SPLIT_LOADS: 1 / 0 = band kernels of 4- and 8-byte types load each
    // row's 2 KiB wave segment as two contiguous halves (cascade_unit SPLIT)
    // or as 32 bytes per lane.
    bool split_loads = false;
    // $AQZ_XCD_REMAP: unset = the default (off), 0 = off, 1 = on (A/B only).
    int xcd_remap = -1;
    // $AQZ_CASCADE_NARROW=0/1: wide / narrow tiles for 4- and 8-byte types.
    int cascade_narrow = -1;
    // $AQZ_CASCADE_WAVES (waves per workgroup, 4 = default, 1..8) and
    // $AQZ_UNIT_ORDER (0 columns fastest = default, 1 frames fastest, 2 row
    // bands fastest): the row-major cascade's unit-to-wave mapping.
    uint32_t cascade_waves = 4;
    uint32_t unit_order = 0;
    // $AQZ_UNITS_PER_WAVE=k forces k (up to 16) units per cascade wave.
    int units_per_wave = 0;
    // $AQZ_BAND_STAGING=0: never stage a band in LDS.
    bool band_off = false;
    // $AQZ_BAND_LAST=K forces the last K (up to 8) waves to store every band
    // (0: the barrier).
    int band_last = -1;
    // $AQZ_BAND_MIS_MAX: the widest misaligned band staged whole (up to 8).
    int band_mis_max = -1;
    // $AQZ_BAND_MIS_SEG: misaligned bands wider than one wave may store go in
    // rowwise segments of that many tiles (up to 8); 0: never.
    int band_mis_seg = -1;
    // $AQZ_BAND_FORCE stages a level mask whatever the alignment, in bands of
    // up to 8 waves.
    uint32_t band_force = 0;
    // $AQZ_BAND_ALIGNED=0: aligned frames keep direct stores.
    bool band_aligned = true;
    // $AQZ_BAND_SEGMENTS=0: no 8-tile segments of aligned bands wider than 8.
    bool band_segments = true;
    // $AQZ_BAND_SEG4=0 / 1: aligned bands never / always go in segments.
    int band_seg4 = -1;
    // $AQZ_BAND_SEGN: tiles per such segment (up to 8).
    int band_segn = 0;
    // $AQZ_BAND_WG=0: no band workgroups for direct stores of split bursts.
    bool band_wg = true;
    // $AQZ_BAND_LDS_CAP (bytes) lowers the device's LDS cap.
    int band_lds_cap = 0;
    // $AQZ_TILED_NARROW: 1 half-width tiles wherever they fit, 0 wide
    // (cascade_tiled_cols).
    int tiled_narrow = -1;
    // $AQZ_TILED_ZWAVES: unset = the planner's count of zero-fill waves, else
    // that count (0 skips the zero fill and leaves the overhang unwritten).
    int tiled_zwaves = -1;
    // $AQZ_TILED_ZROWS_PER_WAVE: overhang rows per zero-fill wave for every
    // type (0: the byte rule alone).
    int tiled_zrows_per_wave = -1;
    // $AQZ_TILED_BAND_WG=1: one workgroup per row band on rows that split
    // 128-B lines (off by default).
    bool tiled_band_wg = false;
    // $AQZ_TILED_WAVES (1..8) forces the waves per workgroup.
    int tiled_waves = 0;
    // $AQZ_VOLUME_NT=0/1, $AQZ_VOLUME_UPW=1/2/4 (Decimate) and
    // $AQZ_VOLUME_ZFAST=0 / 1 (never / always, nontemporal loads).
    int volume_nt = -1;
    int volume_upw = 0;
    int volume_zfast = -1;

    // `get(name)`: the switch's text, or null when unset.
    static LaunchSwitches from(const std::function<const char*(const char*)>& get);
    static LaunchSwitches from_env()
    {
        return from([](const char* name) -> const char* { return std::getenv(name); });
    }
};

// The process-wide instance the library plans with: read from the
// environment on first use, once per process.
const LaunchSwitches& launch_switches();

size_t dtype_bytes(int dtype);
inline bool dtype_valid(int dtype) { return dtype_bytes(dtype) != 0; }
inline bool method_valid(int method) { return method >= kDecimate && method <= kMax; }

uint32_t grid_for(uint64_t work_items, uint32_t per_block, uint32_t cap);

// Columns per lane the fused cascade would use for this run of levels (0:
// unsupported).  Any width and byte offset works as long as the buffers are
// element-aligned, a row holds at least one 16-byte (narrow tiles: 8-byte)
// load, and each output level is exactly ceil(in/2) of the one before.
uint32_t cascade_pick_cols(int dtype, const void* src, uint64_t src_frame_elems, uint32_t W,
                           uint32_t H, const LevelOut* outs, int n_out,
                           const LaunchSwitches& sw = launch_switches());
inline bool
cascade_supported(int dtype, const void* src, uint64_t src_frame_elems, uint32_t W, uint32_t H,
                  const LevelOut* outs, int n_out)
{
    return cascade_pick_cols(dtype, src, src_frame_elems, W, H, outs, n_out) != 0;
}

// Columns per lane launch_cascade_tiled uses for W-wide frames of `dtype`
// (cascade_pick_cols for element-aligned buffers).
uint32_t cascade_tiled_cols(int dtype, uint32_t W, const LaunchSwitches& sw = launch_switches());

// Zero-scan flag bytes per tile that launch_cascade_tiled writes for level
// `level` (1-based within a launch of n_out levels over W-wide frames): when
// the kernel's wave blocks tile the chunk tiles exactly, `slots` bytes per
// tile (*slots_x across), each written once by the wave owning that block —
// the tile is nonzero iff any of its slots is; returns 0 otherwise (one byte
// per tile, cleared before the launch).
uint32_t cascade_tiled_slots(int dtype, uint32_t W, int n_out, int level, uint32_t tile_rows,
                             uint32_t tile_cols, uint32_t* slots_x,
                             const LaunchSwitches& sw = launch_switches());
// The same rule for the launch's input level written as tiles too
// (plan_cascade_tiled with a base): wave blocks of 2^n_out rows x 64 * cols
// columns, `cols` columns per lane store.
uint32_t cascade_tiled_base_slots(int dtype, uint32_t W, int n_out, uint32_t tile_rows,
                                  uint32_t tile_cols, uint32_t* slots_x,
                                  const LaunchSwitches& sw = launch_switches());

bool volume_supported(int dtype, const void* src, uint32_t W, uint32_t H, const LevelOut* outs,
                      int n_out);

// Slices per tile of launch_tile_frame_sliced.
uint32_t tile_slices(uint32_t tile_rows, uint32_t tile_cols);

// ---- plans ------------------------------------------------------------------
// A plan is a pure function of its arguments.  `valid` is false for exactly
// the inputs the launcher answers with hipErrorInvalidValue.  Selector fields
// choose the kernel instantiation; grid / block / lds are the launch shape;
// the rest are the scalars of CascadeParams / VolumeParams.

struct CascadePlan
{
    bool valid = false;
    int dtype = 0, method = 0, n_out = 0;
    uint32_t bytes = 0; // dtype size
    // selectors: cascade_kernel<T, M, n_out, cols, nt>, or with `band`
    // cascade_band_kernel<T, M, n_out, cols, nt, seg_rowwise, split>
    uint32_t cols = 0, nt = 0;
    bool band = false, split = false;
    uint32_t grid = 0, block = 0, lds = 0;
    uint32_t units_x = 0, units_y = 0, total_units = 0;
    uint32_t upw = 1, main_blocks = 0, order = 0, remap = 0, wb = 0;
    uint32_t seg_w = 0, band_last = 0, seg_rowwise = 0;
    uint32_t stage_mask = 0, seg_tiles = 0; // band kernel arguments
};

struct TiledLevelPlan
{
    uint32_t ntx = 0, nty = 0, pw = 0, ph = 0;
    uint64_t tframe_elems = 0, tstride = 0;
    uint32_t cov_w = 0, cov_h = 0, zrows = 0;
    uint32_t slots = 0, slots_x = 1, flags_frame = 0;
    // one flag per tile, OR-ed by plain stores of 1: the launcher clears
    // n_frames * ntx * nty flag bytes first
    bool clear_flags = false;
};

struct TiledPlan
{
    bool valid = false;
    int dtype = 0, method = 0, n_out = 0;
    uint32_t bytes = 0;
    // selectors: cascade_kernel<T, M, n_out, cols, nt, nested ? 1 : 2>
    uint32_t cols = 0, nt = 0;
    bool nested = true; // every level's wave blocks and tiles nest
    uint32_t grid = 0, block = 0, wpb = 0;
    uint32_t n_frames = 0;
    uint32_t units_x = 0, units_y = 0, total_units = 0;
    uint32_t zitems = 0, zwaves = 0, main_blocks = 0, remap = 0, seg_w = 0;
    TiledLevelPlan lv[kMaxFusedLevels];
    // The launch's input level written as tiles too (selector: TILED 3 / 4
    // for nested / not): its units cover cov_w = units_x * 64 * cols by
    // cov_h = units_y * 2^n_out, never less than the frame, so its zero-fill
    // items (base_lv.zrows a frame, beside zitems for the levels) are the
    // padded area past them alone.  zwaves, nested and the limits count it.
    bool base = false;
    TiledLevelPlan base_lv;
};

struct VolumePlan
{
    bool valid = false;
    int dtype = 0, method = 0, n_out = 0;
    uint32_t bytes = 0;
    // selectors: volume_kernel<T, M, n_out, ntl, upw, 16 / bytes, zfast>
    bool ntl = true, zfast = false;
    int upw = 1;
    uint32_t grid = 0, block = 256;
    uint32_t units_x = 0, units_y = 0, total_units = 0;
};

// launch_volume_tiled: VolumePlan's unit geometry (one unit per wave, columns
// first, nontemporal loads) with one TiledLevelPlan per level of the run.
// Level i + 1 emits n_planes >> (i + 1) planes; lv[i].zrows counts the
// zero-fill items of one such plane, zitems those of one plane group (every
// level's zrows times its 2^(n_out-1-i) planes per group).  Flags are one
// cleared byte per tile (clear_flags where the level has a flag buffer).
struct VolumeTiledPlan
{
    bool valid = false;
    int dtype = 0, method = 0, n_out = 0;
    uint32_t bytes = 0;
    // selectors: volume_kernel<T, M, n_out, true, 1, 16 / bytes, false, true>
    uint32_t grid = 0, block = 256, wpb = 4;
    uint32_t n_planes = 0;
    uint32_t units_x = 0, units_y = 0, total_units = 0;
    uint32_t zitems = 0, zwaves = 0, main_blocks = 0;
    TiledLevelPlan lv[kMaxVolumeLevels];
};

// launch_zrun: `planes` consecutive frames of `elems` elements paired down
// n_out times in Z alone.  One unit (a wave) is one plane group — 2^n_out
// input planes — by one span of kZRunSpanBytes of the plane; `spans` is the
// plane's bytes over that, rounded up, so the span that ends the plane also
// carries the bytes behind its last whole 16-byte vector.  Units go spans
// fastest, then groups, four to a workgroup.
struct ZRunPlan
{
    bool valid = false;
    int dtype = 0, method = 0, n_out = 0;
    uint32_t bytes = 0;
    // selectors: zrun_kernel<T, M, n_out>
    uint32_t planes = 0, groups = 0, spans = 0;
    uint64_t elems = 0;
    uint32_t grid = 0, block = 256;
};

// launch_zrun_tiled: ZRunPlan's unit geometry over planes of W x H elements
// (elems = W * H) with one TiledLevelPlan per level of the run.  Level i + 1
// emits planes >> (i + 1) planes, each W x H, in its own tile shape.  The
// units' stores cover exactly the frame (cov_w = W, cov_h = H); lv[i].zrows
// counts the zero-fill items of one emitted plane, zitems those of one plane
// group (every level's zrows times its 2^(n_out-1-i) planes per group).  Flags
// are one cleared byte per tile (clear_flags where the level has a flag
// buffer).  The grid's first zwaves waves (a whole number of workgroups)
// zero-fill; main_blocks workgroups of four units follow.
struct ZRunTiledPlan
{
    bool valid = false;
    int dtype = 0, method = 0, n_out = 0;
    uint32_t bytes = 0;
    // selectors: zrun_tiled_kernel<T, M, n_out>
    uint32_t W = 0, H = 0;
    uint32_t planes = 0, groups = 0, spans = 0;
    uint64_t elems = 0;
    uint32_t grid = 0, block = 256, wpb = 4;
    uint32_t zitems = 0, zwaves = 0, main_blocks = 0;
    TiledLevelPlan lv[kMaxZLevels];
};

// `lds_cap`: the device's LDS per workgroup, less the band kernel's static
// arrival counter (ds_dispatch.cpp asks the device once).
CascadePlan plan_cascade(int dtype, int method, const void* src, uint64_t src_frame_elems,
                         uint32_t W, uint32_t H, const LevelOut* outs, int n_out,
                         uint32_t n_frames, uint32_t lds_cap, const LaunchSwitches& sw);
TiledPlan plan_cascade_tiled(int dtype, int method, const void* src, uint64_t src_frame_elems,
                             uint32_t W, uint32_t H, const LevelOut* outs, const TiledOut* touts,
                             int n_out, uint32_t n_frames, const LaunchSwitches& sw,
                             const TiledOut* tbase = nullptr);
VolumePlan plan_volume(int dtype, int method, const void* src, uint64_t src_frame_elems,
                       uint32_t W, uint32_t H, const LevelOut* outs, int n_out,
                       uint32_t n_planes, const LaunchSwitches& sw);
// touts[i].frame_offsets, when set, holds n_planes >> (i + 1) entries.
// Invalid on top of plan_volume's rules: a null, misaligned or zero-shaped
// tile output, a tile stride below one tile, a padded side or the unit count
// at 2^31 or more, zero-fill items at 2^32 or more.
VolumeTiledPlan plan_volume_tiled(int dtype, int method, const void* src,
                                  uint64_t src_frame_elems, uint32_t W, uint32_t H,
                                  const LevelOut* outs, const TiledOut* touts, int n_out,
                                  uint32_t n_planes, const LaunchSwitches& sw);

// Only outs[i].ptr and outs[i].frame_elems are read (a Z level keeps w x h).
// Invalid: n_out outside 1..kMaxZLevels, `planes` zero or no multiple of
// 2^n_out, elems zero, a frame stride (source or level) below elems, a null
// or not element-aligned pointer, groups * spans at 2^31 or more.
ZRunPlan plan_zrun(int dtype, int method, const void* src, uint64_t src_frame_elems,
                   uint64_t elems, const LevelOut* outs, int n_out, uint32_t planes);

// plan_zrun over planes of W x H elements, every level also (outs[i].ptr
// null: only) written as chunk tiles.  outs[i].ptr may be null; where it is
// set, plan_zrun's rules hold for it.  touts[i].frame_offsets, when set, holds
// planes >> (i + 1) entries.  Invalid on top of plan_zrun's rules: W or H
// zero, a null, misaligned or zero-shaped tile output, a tile stride below one
// tile, a padded side or the unit count at 2^31 or more, zero-fill items at
// 2^32 or more (plan_volume_tiled's limits).  A Z level has no width rule.
ZRunTiledPlan plan_zrun_tiled(int dtype, int method, const void* src, uint64_t src_frame_elems,
                              uint32_t W, uint32_t H, const LevelOut* outs,
                              const TiledOut* touts, int n_out, uint32_t planes);

// The launch log's line (launch_log.hh) for a valid plan: family=cascade or
// family=band, family=tiled, family=volume, family=volume_tiled, family=zrun,
// family=zrun_tiled.
std::string format_plan(const CascadePlan& p);
std::string format_plan(const TiledPlan& p);
std::string format_plan(const VolumePlan& p);
std::string format_plan(const VolumeTiledPlan& p);
std::string format_plan(const ZRunPlan& p);
std::string format_plan(const ZRunTiledPlan& p);

// ---- pyramids as runs ---------------------------------------------------------
// What a level (l >= 1) does to the one before it: halve XY and Z, XY alone,
// Z alone, or neither (kClassNone: no batched launch takes it) — the
// streaming handle's rule: XY when w or h shrinks, Z when the plane count
// does.  Whether a run's exact extents fit its kernel is the launch plans'.
enum
{
    kClassNone = 0,
    kClassXYZ = 1,
    kClassXY = 2,
    kClassZ = 3
};

struct PyramidLevel
{
    uint32_t w = 0, h = 0, planes = 0;
    bool holds_plane = false; // the level has stored the earlier plane of a pair
};

struct PyramidRun
{
    int cls = kClassNone;
    uint32_t first = 0;     // the run's first level (>= 1)
    uint32_t levels = 0;    // how many: <= kMaxVolumeLevels / kMaxFusedLevels / kMaxZLevels
    uint32_t frames_in = 0; // frames of level first - 1 the run reads
};

struct PyramidRuns
{
    bool ok = false;
    std::string reason; // why not, when !ok
    std::vector<PyramidRun> runs;
};

int level_class(const PyramidLevel& in, const PyramidLevel& out);

// Cuts levels 1..n_levels-1 into maximal stretches of one class, each in
// pieces of that class's launch depth.  Level l emits n_frames >> zcount(l)
// frames, zcount(l) the Z-halving levels among 1..l.  Refused: fewer than two
// levels, 32 or more Z-halving ones, a level without a class, an odd plane count in
// front of a Z-halving level, a Z-halving level that holds a plane, n_frames
// zero or no multiple of 2^zcount(last).
PyramidRuns plan_pyramid_runs(const PyramidLevel* lv, uint32_t n_levels, uint32_t n_frames);

} // namespace aqz
