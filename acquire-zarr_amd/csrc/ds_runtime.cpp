// ds_runtime.cpp — implementation of the C ABI in include/aqz_downsampler.h.
//
// Host orchestration of the per-frame pyramid on one MI355X:
//   * the level planner (restates downsampler.cpp:8-37, 493-597);
//   * the add_frame state machine (restates downsampler.cpp:306-401): level
//     cascade, Z pairing against the stored earlier plane, odd-plane
//     pass-through, emit-without-overwrite (:599-605);
//   * take_frame (:403-414): the cached level frame is copied from HBM
//     straight into the caller's buffer.
// Runs of consecutive levels that only halve XY are fused into one cascade
// launch (up to 4 levels per launch), so the frame is read from HBM once.
//
// Level buffers: every level L >= 1 owns two device slots.  A frame emitted
// while the level's cache is empty becomes the cached frame (its slot is
// then left alone until take_frame); new results always go to the other
// slot, so an untaken frame is never overwritten — the reference's
// unordered_map::emplace rule.
#include "aqz_downsampler.h"
#include "abi_guard.hh"
#include "ds_kernels.hh"
#include "hip_raii.hh"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <array>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace {

thread_local std::string g_last_error;

// Pyramids up to this many level bytes are read back eagerly (aqz_ds::eager).
// (A host memcpy of a larger pyramid would cost more than the round trips
// it saves)
constexpr size_t kEagerBytes = size_t(1) << 20;

void
set_global_error(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

uint32_t
bit_width(uint32_t x)
{
    uint32_t n = 0;
    for (; x; x >>= 1)
        ++n;
    return n;
}

// Number of 2x divisions a dimension supports before it fits one chunk
// (downsampler.cpp:507-520): bit_width(ceil(size/chunk) - 1).
uint32_t
divisions(const aqz_dimension& d)
{
    const uint32_t n = (d.array_size_px + d.chunk_size_px - 1) / d.chunk_size_px;
    return n > 1 ? bit_width(n - 1) : 0;
}

// downsample_dimension, downsampler.cpp:8-37.
aqz_dimension
halve(const aqz_dimension& d)
{
    aqz_dimension o = d;
    o.array_size_px = (d.array_size_px + d.array_size_px % 2) / 2;
    const uint32_t n = (o.array_size_px + d.chunk_size_px - 1) / d.chunk_size_px;
    o.shard_size_chunks = std::min(n, d.shard_size_chunks);
    o.scale = d.scale * 2.0;
    return o;
}

bool
env_flag(const char* name)
{
    const char* v = std::getenv(name);
    return v && *v && std::strcmp(v, "0") != 0;
}

} // namespace

struct aqz_ds
{
    // One pyramid level's streaming state (level 0 uses the descriptor,
    // `bytes` and `count` only).
    struct Level
    {
        aqz_level_desc desc{};
        size_t bytes = 0;     // bytes of one frame
        bool xy = false;      // halves XY (L >= 1)
        bool zh = false;      // halves Z (L >= 1)
        uint32_t count = 0;   // level_frame_count_
        bool has_partial = false;
        // aqz_ds_add_frame_async_take with AQZ_TAKE_HOLD: the caller still
        // holds an untaken frame of the level, so new ones are dropped (the
        // emplace rule, downsampler.cpp:599-605) as if it were cached here
        bool held = false;

        aqz::DeviceBuf slot[2];    // two result slots
        aqz::DeviceBuf d_partial;  // stored earlier plane (Z levels)
        aqz::PinnedBuf h_level;    // eager readback: pinned copy of the frame
        bool no_eager = false;     // level taken tiled: that copy would be wasted

        // aqz_ds_set_level_tiling: the tile shape (0,0: off) and two tiled
        // slots paired with `slot`.  `flags` is pinned and kernel-written;
        // its capacity is what the half can hold, `slices` the flag bytes per
        // tile of the frame tiled there (tile_slices for the tile kernel,
        // cascade_tiled_slots for the one-pass tiled cascade).
        uint32_t tile_rows = 0, tile_cols = 0;
        struct Tiled
        {
            aqz::DeviceBuf tiles;
            aqz::PinnedBuf flags;
            uint32_t slices = 1;
        } tiled[2];
        aqz::PinnedBuf h_tiles; // eager readback: pinned copy of the tiles

        uint64_t elems() const { return uint64_t(desc.width) * desc.height; }

        // What has been done to the untaken frame.  cached_ is the slot that
        // holds it (-1: none).  The other three name the slot whose frame
        // tiled[k] (tiled_for_), h_level (host_for_) and h_tiles (htile_for_)
        // hold.  Invariant: each of the three is -1 or equal to cached_, so
        // nothing derived from a frame outlives it.  Only the members below
        // write them.
        int cached() const { return cached_; }
        bool is_tiled() const { return cached_ >= 0 && tiled_for_ == cached_; }
        bool on_host() const { return cached_ >= 0 && host_for_ == cached_; }
        bool tiles_on_host() const { return cached_ >= 0 && htile_for_ == cached_; }
        // where a new frame is written: never the cached slot
        int free_slot() const { return cached_ == 0 ? 1 : 0; }
        void cache(int k) { cached_ = k; }
        void mark_tiled() { tiled_for_ = cached_; }
        void mark_on_host() { host_for_ = cached_; }
        void mark_tiles_on_host() { htile_for_ = cached_; }
        void drop_tiled() { tiled_for_ = htile_for_ = -1; } // the tiling changed
        void drop_cached() { cached_ = tiled_for_ = host_for_ = htile_for_ = -1; }

      private:
        int cached_ = -1, tiled_for_ = -1, host_for_ = -1, htile_for_ = -1;
    };

    // Member order is destruction order reversed.  The streams come first, so
    // every buffer and event below is destroyed before the stream it was used
    // on; inside Pipe likewise.  release() synchronises `stream`, both
    // lattice_done events and chain_done before it deletes the handle, so
    // nothing is freed under queued work.
    aqz::Stream own_stream;
    hipStream_t stream = nullptr; // own_stream, or a batch caller's (StreamSwap)

    // aqz_ds_run_host_batch pipeline, allocated on first use
    struct Pipe
    {
        aqz::Stream s_in, s_work, s_out;
        uint32_t group = 0;                  // frames per group the buffers hold
        aqz::DeviceBuf d_in[2];
        std::vector<aqz::DeviceBuf> d_out[2]; // per level, group-sized
        aqz::Event in_done[2], work_done[2], out_done[2];
    } pipe;

    int device = 0;
    int dtype = 0;
    int method = 0;
    size_t bpp = 0;
    uint32_t n = 0;
    std::vector<Level> lv;

    aqz::DeviceBuf d_in; // level-0 frame on device
    aqz::Event h2d_done;
    // orders a caller's stream against `stream` around a batch run on it
    aqz::Event join;
    // optional pinned staging of host frames ($AQZ_PINNED_STAGING=1)
    bool staged = false;
    aqz::PinnedBuf h_stage;
    size_t device_bytes = 0;
    int last_batch_kind = -1;
    // aqz_debug_ds_force_per_frame_batch: aqz_ds_run_device_batch takes the
    // per-frame state machine (kind 0) whatever the pyramid
    bool force_per_frame = false;

    // Small pyramids (all levels together <= kEagerBytes): every newly cached
    // level frame is copied to pinned host memory (Level::h_level) right
    // behind the kernels, so the take_frame calls that follow cost one event
    // wait and a memcpy each instead of a device round trip each
    // ($AQZ_EAGER_READBACK=0: off).  With level tiling the tiles are copied
    // instead (Level::h_tiles), queued right behind their tile kernel.
    bool eager = false;
    aqz::Event levels_d2h;

    // aqz_ds_take_frame_tiled: on-demand scratch (tiles, and pinned slice flags)
    aqz::DeviceBuf d_tiles;
    aqz::PinnedBuf h_flags;
    // aqz_ds_run_device_batch_tiled: row-major copy of the last level of a
    // fused run that feeds the next run (pyramids deeper than 4 XY levels)
    aqz::DeviceBuf d_chain;
    // recorded after every tiled batch: the next one (on any stream) waits on
    // it before it rewrites d_chain
    aqz::Event chain_done;
    // aqz_ds_run_device_batch_chunked: per-level frame offsets (elements),
    // staged in pinned memory and copied to the device on the batch's
    // stream; two halves used by alternate calls, each guarded by the event
    // recorded after the batch that read it
    aqz::DeviceBuf d_lattice;
    aqz::PinnedBuf h_lattice;
    uint32_t lattice_calls = 0;
    aqz::Event lattice_done[2];
    // $AQZ_STREAM_TILE_PASS=1: eager tiling as a tile pass behind the
    // row-major cascade (the round-2 path), for A/B
    bool tile_pass = false;
    uint64_t stream_tiled_runs = 0; // runs the streaming path tiled in one launch

    // aqz_ds_set_input_transpose: input frames arrive in acquisition order
    // (rows = level-0 width) and are transposed into d_tin on the device
    bool transpose = false;
    aqz::DeviceBuf d_tin;
    // the last level-0 frame added (storage order), for aqz_ds_take_input_frame;
    // null once taken or after a batch
    const void* last_input = nullptr;

    // aqz_ds_add_frame_async: one worker thread (started on first use) runs
    // at most one pending add_frame; every other entry point settles it first
    struct Async
    {
        std::thread worker;
        std::mutex m;
        std::condition_variable cv;
        const void* frame = nullptr; // the pending job's frame, null when idle
        // the pending job's frame while the job may still read it (until its
        // upload is done); null once the caller may reuse it
        const void* input = nullptr;
        aqz_level_take* takes = nullptr; // aqz_ds_add_frame_async_take's takes
        bool stop = false;
        int rc = 0;                  // status of the last finished job
    } async;

    std::string err;

    int fail(hipError_t e, const char* what)
    {
        err = std::string(what) + ": " + hipGetErrorString(e);
        return AQZ_INTERNAL_ERROR;
    }
    int fail_arg(const std::string& what)
    {
        err = what;
        return AQZ_INVALID_ARGUMENT;
    }
};

namespace aqz {

inline std::string*
abi_err_slot(aqz_ds* ds)
{
    return ds ? &ds->err : nullptr;
}

} // namespace aqz

namespace {

#define HIP_TRY(ds, expr, what)                                                \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess)                                                  \
            return (ds)->fail(e_, what);                                       \
    } while (0)

// Where the frames a level emits go.
struct Sink
{
    // false: streaming add_frame — the frame may become the cached one
    bool batch = false;
    // batch mode: frame k of level L goes to out[L] + k*bytes[L]
    void* const* out = nullptr;
    std::vector<uint32_t>* emitted = nullptr;
};

using Level = aqz_ds::Level;

// Tiled layout of a level at (tr, tc): tile bytes and slice-flag bytes.
struct TileGeom
{
    size_t n_tiles, tile_bytes, flag_bytes;
};

TileGeom
tile_geom(const aqz_ds* ds, const Level& lv, uint32_t tr, uint32_t tc)
{
    const size_t ntx = (lv.desc.width + tc - 1) / tc, nty = (lv.desc.height + tr - 1) / tr;
    const size_t nt = ntx * nty;
    return { nt, nt * tr * tc * ds->bpp, nt * aqz::tile_slices(tr, tc) };
}

// LevelOut[] of the run of levels L..L+k-1, level l written at ptr_of(l).
template<class PtrOf>
void
fill_outs(const aqz_ds* ds, uint32_t L, uint32_t k, PtrOf ptr_of, aqz::LevelOut* outs)
{
    for (uint32_t j = 0; j < k; ++j) {
        const Level& lv = ds->lv[L + j];
        outs[j] = { ptr_of(L + j), lv.elems(), lv.desc.width, lv.desc.height };
    }
}

// XY-reduce `n_frames` frames at `src` (level L-1) into the run `outs`: the
// fused cascade where the planner takes the run (*fused), else one generic
// launch per level.
hipError_t
launch_xy_run(const aqz_ds* ds, const void* src, uint32_t L, uint32_t k,
              const aqz::LevelOut* outs, uint32_t n_frames, hipStream_t stream, bool* fused)
{
    const Level& a = ds->lv[L - 1];
    *fused = aqz::cascade_supported(ds->dtype, src, a.elems(), a.desc.width, a.desc.height, outs,
                                    int(k));
    if (*fused)
        return aqz::launch_cascade(ds->dtype, ds->method, src, a.elems(), a.desc.width,
                                   a.desc.height, outs, int(k), n_frames, stream);
    hipError_t e = hipSuccess;
    for (uint32_t j = 0; j < k && e == hipSuccess; ++j) {
        const Level& in = ds->lv[L + j - 1];
        e = aqz::launch_xy_generic(ds->dtype, ds->method, src, in.elems(), in.desc.width,
                                   in.desc.height, outs[j], n_frames, stream);
        src = outs[j].ptr;
    }
    return e;
}

// One flag per tile: the OR of its `slices` flag bytes (pinned,
// kernel-written, tile-major).
void
reduce_slice_flags(const TileGeom& g, size_t slices, const uint8_t* flags,
                   uint8_t* tile_nonzero)
{
    for (size_t t = 0; t < g.n_tiles; ++t) {
        // most tiles hold data: stop at the first set flag
        const uint8_t* f = flags + t * slices;
        tile_nonzero[t] = std::any_of(f, f + slices, [](uint8_t b) { return b != 0; }) ? 1 : 0;
    }
}

// D2H of tiles already laid out on the device, then one flag per tile from
// its slice flags (pinned, written by the tile kernel).
int
tiles_to_host(aqz_ds* ds, const TileGeom& g, size_t slices, const void* d_tiles,
              const uint8_t* flags, void* dst, uint8_t* tile_nonzero)
{
    HIP_TRY(ds,
            hipMemcpyAsync(dst, d_tiles, g.tile_bytes, hipMemcpyDeviceToHost, ds->stream),
            "hipMemcpyAsync D2H");
    HIP_TRY(ds, hipStreamSynchronize(ds->stream), "hipStreamSynchronize");
    if (tile_nonzero)
        reduce_slice_flags(g, slices, flags, tile_nonzero);
    return AQZ_OK;
}

// Tile a device frame into the on-demand scratch buffers and copy it out.
int
tile_to_host(aqz_ds* ds, const void* d_frame, const aqz_level_desc& lv, uint32_t tile_rows,
             uint32_t tile_cols, const TileGeom& g, void* dst, uint8_t* tile_nonzero)
{
    // every earlier use of the scratch was waited for (tiles_to_host)
    HIP_TRY(ds, ds->d_tiles.reserve(g.tile_bytes), "hipMalloc tiles");
    HIP_TRY(ds, ds->h_flags.reserve(g.flag_bytes), "hipHostMalloc flags");
    HIP_TRY(ds,
            aqz::launch_tile_frame_sliced(ds->dtype, d_frame, lv.width, lv.height, tile_rows,
                                          tile_cols, ds->d_tiles.get(), ds->h_flags.bytes(),
                                          ds->stream),
            "tile kernel");
    return tiles_to_host(ds, g, g.flag_bytes / g.n_tiles, ds->d_tiles.get(),
                         ds->h_flags.bytes(), dst, tile_nonzero);
}

// Working buffer for a level-L result: the caller's batch slot when the
// sink is a batch, else the level's free device slot.
void*
level_target(aqz_ds* ds, uint32_t L, const Sink& sink)
{
    const Level& lv = ds->lv[L];
    if (sink.batch)
        return static_cast<uint8_t*>(sink.out[L]) + (*sink.emitted)[L] * lv.bytes;
    return lv.slot[lv.free_slot()].get();
}

// emplace_downsampled_frame_ (downsampler.cpp:599-605).  `pretiled`: the
// one-pass tiled cascade has already written this frame's tiles and flags
// into the tiled slot paired with its slot.
int
emit(aqz_ds* ds, uint32_t level, const void* d_frame, const Sink& sink, bool pretiled = false)
{
    Level& lv = ds->lv[level];
    ++lv.count;
    void* want = level_target(ds, level, sink);
    if (want != d_frame) {
        HIP_TRY(ds,
                hipMemcpyAsync(want, d_frame, lv.bytes, hipMemcpyDeviceToDevice, ds->stream),
                "hipMemcpyAsync D2D");
    }
    if (sink.batch) {
        ++(*sink.emitted)[level];
        return AQZ_OK;
    }
    // unordered_map::emplace keeps an untaken frame; the new one is dropped
    // (it stays in the free slot only as the next level's input).
    if (lv.cached() < 0 && !lv.held) {
        const int k = lv.free_slot(); // `want` is that slot
        lv.cache(k);
        const uint32_t tr = lv.tile_rows, tc = lv.tile_cols;
        if (tr && pretiled) {
            lv.mark_tiled();
        } else if (tr) {
            // queue the chunk tiling right behind the pyramid (§8(f) row 2)
            Level::Tiled& t = lv.tiled[k];
            HIP_TRY(ds,
                    aqz::launch_tile_frame_sliced(ds->dtype, want, lv.desc.width, lv.desc.height,
                                                  tr, tc, t.tiles.get(), t.flags.bytes(),
                                                  ds->stream),
                    "tile kernel");
            lv.mark_tiled();
            t.slices = aqz::tile_slices(tr, tc);
        }
    }
    return AQZ_OK;
}

// One run of k pure-XY levels from L, every one of them tiled: the tiled
// cascade writes each level row-major into its free slot (the next run's
// input and take_frame's copy) and chunk-tiled, zero scan included, into the
// tiled slot paired with it — one launch instead of the cascade plus a tile
// pass per level.  *launched is false when the geometry needs the separate
// tile pass (nothing was queued but, at most, a flag clear).
int
launch_run_tiled(aqz_ds* ds, uint32_t L, uint32_t k, const void* cur,
                 const aqz::LevelOut* outs, bool* launched)
{
    *launched = false;
    if (ds->tile_pass)
        return AQZ_OK;
    const Level& a = ds->lv[L - 1];
    if (aqz::cascade_tiled_cols(ds->dtype, a.desc.width) !=
        aqz::cascade_pick_cols(ds->dtype, cur, a.elems(), a.desc.width, a.desc.height, outs,
                               int(k)))
        return AQZ_OK;
    aqz::TiledOut t[aqz::kMaxFusedLevels];
    uint32_t slices[aqz::kMaxFusedLevels];
    for (uint32_t j = 0; j < k; ++j) {
        Level& lv = ds->lv[L + j];
        const uint32_t tr = lv.tile_rows, tc = lv.tile_cols;
        if (!tr)
            return AQZ_OK;
        slices[j] = aqz::cascade_tiled_slots(ds->dtype, a.desc.width, int(k), int(j + 1), tr, tc,
                                             nullptr);
        if (!slices[j])
            return AQZ_OK; // one OR-ed flag per tile would need a clear of pinned memory
        // outs[j] is the level's free slot: its tiled half is free too
        Level::Tiled& half = lv.tiled[lv.free_slot()];
        const size_t need = tile_geom(ds, lv, tr, tc).n_tiles * slices[j];
        if (half.flags.capacity() < need) {
            // earlier kernels may still write the half
            HIP_TRY(ds, hipStreamSynchronize(ds->stream), "hipStreamSynchronize");
            HIP_TRY(ds, half.flags.reserve(need), "hipHostMalloc flags");
        }
        t[j] = { half.tiles.get(), tr, tc, half.flags.bytes() };
    }
    const hipError_t e = aqz::launch_cascade_tiled(ds->dtype, ds->method, cur, a.elems(),
                                                   a.desc.width, a.desc.height, outs, t, int(k),
                                                   1, ds->stream);
    if (e == hipErrorInvalidValue)
        return AQZ_OK;
    HIP_TRY(ds, e, "tiled cascade kernel");
    for (uint32_t j = 0; j < k; ++j)
        ds->lv[L + j].tiled[ds->lv[L + j].free_slot()].slices = slices[j];
    ++ds->stream_tiled_runs;
    *launched = true;
    return AQZ_OK;
}

// XY-reduce `src` (level L-1 geometry) into `dst` (level L geometry).
int
reduce_xy(aqz_ds* ds, uint32_t L, const void* src, void* dst)
{
    aqz::LevelOut o;
    fill_outs(ds, L, 1, [&](uint32_t) { return dst; }, &o);
    bool fused;
    HIP_TRY(ds, launch_xy_run(ds, src, L, 1, &o, 1, ds->stream, &fused), "xy level kernel");
    return AQZ_OK;
}

// One frame through the level cascade: Downsampler::add_frame
// (downsampler.cpp:306-401) with device buffers.
int
process_frame(aqz_ds* ds, const void* d_frame, const Sink& sink)
{
    ++ds->lv[0].count;
    const void* cur = d_frame;
    uint32_t L = 1;
    while (L < ds->n) {
        Level& lv = ds->lv[L];
        if (lv.xy && !lv.zh) {
            // Run of pure-XY levels: they always emit, fuse up to 4.
            uint32_t k = 1;
            while (L + k < ds->n && k < aqz::kMaxFusedLevels && ds->lv[L + k].xy &&
                   !ds->lv[L + k].zh)
                ++k;
            aqz::LevelOut outs[aqz::kMaxFusedLevels];
            fill_outs(ds, L, k, [&](uint32_t l) { return level_target(ds, l, sink); }, outs);
            bool pretiled = false;
            if (!sink.batch)
                if (int rc = launch_run_tiled(ds, L, k, cur, outs, &pretiled))
                    return rc;
            // pretiled: levels and their tiles written by the tiled cascade
            if (!pretiled) {
                bool fused;
                const hipError_t e = launch_xy_run(ds, cur, L, k, outs, 1, ds->stream, &fused);
                HIP_TRY(ds, e, fused ? "cascade kernel" : "xy level kernel");
            }
            for (uint32_t j = 0; j < k; ++j) {
                int rc = emit(ds, L + j, outs[j].ptr, sink, pretiled);
                if (rc)
                    return rc;
            }
            cur = outs[k - 1].ptr;
            L += k;
            continue;
        }

        // General level: optional XY reduce, then optional Z pairing.
        const uint32_t prev_planes = ds->lv[L - 1].desc.planes;
        bool average = lv.zh;
        if (prev_planes % 2 != 0 && ds->lv[L - 1].count % prev_planes == 0)
            average = false; // last plane of an odd stack passes through

        if (average && !lv.has_partial) {
            // store this plane as the earlier half of the pair, then stop
            if (lv.xy) {
                int rc = reduce_xy(ds, L, cur, lv.d_partial.get());
                if (rc)
                    return rc;
            } else {
                HIP_TRY(ds,
                        hipMemcpyAsync(lv.d_partial.get(), cur, lv.bytes,
                                       hipMemcpyDeviceToDevice, ds->stream),
                        "hipMemcpyAsync D2D");
            }
            lv.has_partial = true;
            break;
        }

        void* target = level_target(ds, L, sink);
        const void* next = cur;
        if (lv.xy) {
            int rc = reduce_xy(ds, L, cur, target);
            if (rc)
                return rc;
            next = target;
        }
        if (average) {
            // average_two_frames(dst = earlier, src = current)
            HIP_TRY(ds,
                    aqz::launch_zpair(ds->dtype, ds->method, target, lv.d_partial.get(), next,
                                      lv.elems(), ds->stream),
                    "zpair kernel");
            lv.has_partial = false;
            next = target;
        }
        int rc = emit(ds, L, next, sink);
        if (rc)
            return rc;
        cur = target; // emit() left the level's frame in `target`
        ++L;
    }
    return AQZ_OK;
}

int
bind_device(aqz_ds* ds)
{
    HIP_TRY(ds, hipSetDevice(ds->device), "hipSetDevice");
    return AQZ_OK;
}

int
check_host_frame(aqz_ds* ds, const void* host_frame, size_t nbytes, const char* who)
{
    if (!host_frame || nbytes != ds->lv[0].bytes)
        return ds->fail_arg(std::string(who) + ": expected " +
                            std::to_string(ds->lv[0].bytes) + " bytes, got " +
                            std::to_string(nbytes));
    return AQZ_OK;
}

// The pyramid of one level-0 frame already on the device.  With input
// transposition the frame is first transposed into storage order
// (transpose_frame, array.cpp:517-530), which is what the reference's
// downsampler receives.
int
process_input(aqz_ds* ds, const void* d_frame)
{
    if (ds->transpose) {
        // acquisition rows = storage width (array.dimensions.cpp:578-599)
        HIP_TRY(ds,
                aqz::launch_transpose(ds->dtype, d_frame, ds->lv[0].desc.width,
                                      ds->lv[0].desc.height, ds->d_tin.get(), ds->stream),
                "transpose kernel");
        d_frame = ds->d_tin.get();
    }
    ds->last_input = d_frame;
    return process_frame(ds, d_frame, Sink{});
}

// Downsampler::add_frame for a host frame: upload it, queue the pyramid, and
// return once the upload has completed (the caller may then reuse its frame;
// the kernels are still queued).
// Queue the D2H of every newly cached level frame into its pinned copy,
// right behind the kernels that made it (aqz_ds::eager).
int
eager_readback(aqz_ds* ds)
{
    if (!ds->eager)
        return AQZ_OK;
    bool any = false;
    for (uint32_t L = 1; L < ds->n; ++L) {
        Level& lv = ds->lv[L];
        const int k = lv.cached();
        if (k < 0)
            continue;
        if (lv.no_eager) {
            // taken tiled: copy the tiles out instead, so the D2H overlaps
            // whatever the caller does before take_frame_tiled
            if (lv.h_tiles && lv.is_tiled() && !lv.tiles_on_host()) {
                const TileGeom g = tile_geom(ds, lv, lv.tile_rows, lv.tile_cols);
                HIP_TRY(ds,
                        hipMemcpyAsync(lv.h_tiles.get(), lv.tiled[k].tiles.get(), g.tile_bytes,
                                       hipMemcpyDeviceToHost, ds->stream),
                        "hipMemcpyAsync D2H (eager tiles)");
                lv.mark_tiles_on_host();
                any = true;
            }
            continue;
        }
        if (lv.on_host())
            continue;
        HIP_TRY(ds,
                hipMemcpyAsync(lv.h_level.get(), lv.slot[k].get(), lv.bytes,
                               hipMemcpyDeviceToHost, ds->stream),
                "hipMemcpyAsync D2H (eager)");
        lv.mark_on_host();
        any = true;
    }
    if (any)
        HIP_TRY(ds, hipEventRecord(ds->levels_d2h, ds->stream), "hipEventRecord");
    return AQZ_OK;
}

int
add_host_frame(aqz_ds* ds, const void* host_frame)
{
    if (int rc = bind_device(ds))
        return rc;
    const size_t nbytes = ds->lv[0].bytes;
    const void* src = host_frame;
    if (ds->staged) {
        // previous upload must be done before the staging buffer is reused
        HIP_TRY(ds, hipEventSynchronize(ds->h2d_done), "hipEventSynchronize");
        std::memcpy(ds->h_stage.get(), host_frame, nbytes);
        src = ds->h_stage.get();
    }
    // Straight from the caller's (pageable) frame: the copy engine reads it
    // at full PCIe rate, no host staging memcpy (tools/e2e_probe.cpp).
    HIP_TRY(ds,
            hipMemcpyAsync(ds->d_in.get(), src, nbytes, hipMemcpyHostToDevice, ds->stream),
            "hipMemcpyAsync H2D");
    // From here on the copy may still read the caller's frame: every way out
    // waits for it first, so that a failed add, too, releases the frame only
    // once nothing reads it (aqz_ds_wait_input's contract).
    if (const hipError_t e = hipEventRecord(ds->h2d_done, ds->stream); e != hipSuccess) {
        (void)hipStreamSynchronize(ds->stream);
        return ds->fail(e, "hipEventRecord");
    }
    int rc = process_input(ds, ds->d_in.get());
    if (rc == AQZ_OK)
        rc = eager_readback(ds);
    if (rc != AQZ_OK) {
        if (!ds->staged)
            (void)hipEventSynchronize(ds->h2d_done);
        return rc;
    }
    if (!ds->staged) {
        // the caller may reuse its frame as soon as we return
        HIP_TRY(ds, hipEventSynchronize(ds->h2d_done), "hipEventSynchronize");
    }
    return AQZ_OK;
}

// aqz_ds_take_frame's body (its caller has settled any pending add).
int
take_plain(aqz_ds* ds, uint32_t level, void* dst, size_t cap, size_t* nbytes, int* has_frame)
{
    *has_frame = 0;
    if (level == 0 || level >= ds->n)
        return AQZ_OK; // the reference's map lookup simply misses
    Level& lv = ds->lv[level];
    if (lv.cached() < 0)
        return AQZ_OK;
    *has_frame = 1;
    if (nbytes)
        *nbytes = lv.bytes;
    if (!dst)
        return AQZ_OK;
    if (cap < lv.bytes)
        return ds->fail_arg("take_frame: buffer too small");
    if (int rc = bind_device(ds))
        return rc;
    if (ds->eager && lv.on_host()) {
        // already on its way to pinned memory (eager_readback)
        HIP_TRY(ds, hipEventSynchronize(ds->levels_d2h), "hipEventSynchronize");
        std::memcpy(dst, lv.h_level.get(), lv.bytes);
    } else {
        // HBM -> caller memory directly (stream-ordered after the kernels)
        HIP_TRY(ds,
                hipMemcpyAsync(dst, lv.slot[lv.cached()].get(), lv.bytes, hipMemcpyDeviceToHost,
                               ds->stream),
                "hipMemcpyAsync D2H");
        HIP_TRY(ds, hipStreamSynchronize(ds->stream), "hipStreamSynchronize");
    }
    lv.drop_cached();
    return AQZ_OK;
}

// aqz_ds_take_frame_tiled's body (its caller has settled any pending add).
int
take_tiled(aqz_ds* ds,
           uint32_t level,
           uint32_t tile_rows,
           uint32_t tile_cols,
           void* dst,
           size_t cap,
           uint8_t* tile_nonzero,
           size_t* nbytes,
           int* has_frame)
{
    *has_frame = 0;
    if (tile_rows == 0 || tile_cols == 0)
        return ds->fail_arg("take_frame_tiled: empty tile");
    if (level == 0 || level >= ds->n || ds->lv[level].cached() < 0)
        return AQZ_OK;
    Level& lv = ds->lv[level];
    const TileGeom g = tile_geom(ds, lv, tile_rows, tile_cols);
    *has_frame = 1;
    if (nbytes)
        *nbytes = g.tile_bytes;
    if (!dst)
        return AQZ_OK;
    if (cap < g.tile_bytes)
        return ds->fail_arg("take_frame_tiled: buffer too small");
    if (int rc = bind_device(ds))
        return rc;
    const Level::Tiled& t = lv.tiled[lv.cached()];
    const bool pretiled = lv.tile_rows == tile_rows && lv.tile_cols == tile_cols && lv.is_tiled();
    if (pretiled && lv.tiles_on_host()) {
        // tiled and copied out when the frame was emitted (eager readback)
        HIP_TRY(ds, hipEventSynchronize(ds->levels_d2h), "hipEventSynchronize");
        std::memcpy(dst, lv.h_tiles.get(), g.tile_bytes);
        if (tile_nonzero)
            reduce_slice_flags(g, t.slices, t.flags.bytes(), tile_nonzero);
    } else if (pretiled) {
        // tiled when the frame was emitted (aqz_ds_set_level_tiling)
        if (int rc = tiles_to_host(ds, g, t.slices, t.tiles.get(), t.flags.bytes(), dst,
                                   tile_nonzero))
            return rc;
    } else if (int rc = tile_to_host(ds, lv.slot[lv.cached()].get(), lv.desc, tile_rows,
                                     tile_cols, g, dst, tile_nonzero)) {
        return rc;
    }
    lv.drop_cached();
    lv.no_eager = true; // this caller takes the level tiled
    return AQZ_OK;
}

// The takes of aqz_ds_add_frame_async_take, in the job right behind its add:
// each level's device-to-host copy then overlaps the caller's work too.
int
run_takes(aqz_ds* ds, aqz_level_take* takes)
{
    for (uint32_t L = 1; L < ds->n; ++L) {
        aqz_level_take& t = takes[L];
        t.has_frame = 0;
        t.nbytes = 0;
        if (t.mode != AQZ_TAKE_INTO)
            continue;
        const int rc = (t.tile_rows || t.tile_cols)
                         ? take_tiled(ds, L, t.tile_rows, t.tile_cols, t.dst, t.cap,
                                      t.tile_nonzero, &t.nbytes, &t.has_frame)
                         : take_plain(ds, L, t.dst, t.cap, &t.nbytes, &t.has_frame);
        if (rc)
            return rc;
    }
    return AQZ_OK;
}

void
async_worker(aqz_ds* ds)
{
    auto& a = ds->async;
    std::unique_lock<std::mutex> lk(a.m);
    for (;;) {
        a.cv.wait(lk, [&] { return a.stop || a.frame != nullptr; });
        if (!a.frame)
            return; // stop requested and nothing pending
        const void* frame = a.frame;
        aqz_level_take* takes = a.takes;
        lk.unlock();
        int rc;
        try {
            rc = add_host_frame(ds, frame);
            // add_host_frame returns once the upload no longer reads the
            // caller's frame (or on failure): release it before the takes
            {
                std::lock_guard<std::mutex> in(a.m);
                a.input = nullptr;
            }
            a.cv.notify_all();
            if (rc == AQZ_OK && takes)
                rc = run_takes(ds, takes);
        } catch (...) {
            rc = ABI_GUARD_FAIL(ds); // reported by the next settle()
        }
        lk.lock();
        a.rc = rc;
        a.frame = nullptr;
        a.input = nullptr;
        a.takes = nullptr;
        a.cv.notify_all();
    }
}

// A plain add: the caller holds no untaken frame (Level::held).
void
release_holds(aqz_ds* ds)
{
    for (Level& lv : ds->lv)
        lv.held = false;
}

// Wait for a pending aqz_ds_add_frame_async; returns (and clears) its status.
int
settle(aqz_ds* ds)
{
    auto& a = ds->async;
    if (!a.worker.joinable())
        return AQZ_OK;
    std::unique_lock<std::mutex> lk(a.m);
    a.cv.wait(lk, [&] { return a.frame == nullptr; });
    const int rc = a.rc;
    a.rc = AQZ_OK;
    return rc;
}

void
release(aqz_ds* ds)
{
    if (!ds)
        return;
    if (ds->async.worker.joinable()) {
        (void)settle(ds);
        {
            std::lock_guard<std::mutex> lk(ds->async.m);
            ds->async.stop = true;
        }
        ds->async.cv.notify_all();
        ds->async.worker.join();
    }
    // Best-effort teardown: errors here have nowhere to go.  Everything the
    // handle owns frees itself (see the member order in aqz_ds) once the
    // work that may still use it is done.
    (void)hipSetDevice(ds->device);
    if (ds->stream)
        (void)hipStreamSynchronize(ds->stream);
    for (hipEvent_t e : { ds->lattice_done[0].get(), ds->lattice_done[1].get(),
                          ds->chain_done.get() })
        if (e)
            (void)hipEventSynchronize(e);
    delete ds;
}

} // namespace

extern "C" {

// array.dimensions.cpp:168-178 (bytes_per_chunk_, number_of_chunks_in_memory_)
// and :232-314 (chunk_lattice_index, tile_group_offset, chunk_internal_offset).
int
aqz_chunk_frame_offsets(const aqz_dimension* dims,
                        uint32_t ndims,
                        uint32_t bytes_per_px,
                        uint64_t first_frame,
                        uint32_t n_frames,
                        uint64_t* frame_offset_bytes,
                        uint64_t* chunk_bytes,
                        uint64_t* layer_bytes)
{
    try {
        if (!dims || ndims < 3 || bytes_per_px == 0 || (n_frames && !frame_offset_bytes)) {
            aqz::set_last_error("chunk_frame_offsets: invalid argument");
            return AQZ_INVALID_ARGUMENT;
        }
        for (uint32_t i = 0; i < ndims; ++i)
            if (dims[i].chunk_size_px == 0 || (i > 0 && dims[i].array_size_px == 0)) {
                aqz::set_last_error("chunk_frame_offsets: zero chunk size, or a zero-size "
                                    "dimension other than the append dimension");
                return AQZ_INVALID_ARGUMENT;
            }
        const int nd = int(ndims);
        uint64_t per_chunk = bytes_per_px, chunks_in_layer = 1;
        for (int i = 0; i < nd; ++i) {
            per_chunk *= dims[i].chunk_size_px;
            if (i > 0)
                chunks_in_layer *= (uint64_t(dims[i].array_size_px) + dims[i].chunk_size_px - 1) /
                                   dims[i].chunk_size_px;
        }
        // lattice strides of every dim (chunks), frames per chunk layer
        std::vector<uint64_t> strides(nd, 1);
        for (int i = nd - 1; i > 0; --i)
            strides[i - 1] =
              strides[i] * ((uint64_t(dims[i].array_size_px) + dims[i].chunk_size_px - 1) /
                            dims[i].chunk_size_px);
        uint64_t layer_frames = dims[0].chunk_size_px;
        for (int i = 1; i + 2 < nd; ++i)
            layer_frames *= dims[i].array_size_px;
        const uint64_t tile_bytes =
          uint64_t(bytes_per_px) * dims[nd - 1].chunk_size_px * dims[nd - 2].chunk_size_px;
        auto lattice_index = [&](uint64_t fid, int d) -> uint64_t {
            uint64_t mod = 1, div = 1;
            for (int i = d; i < nd - 2; ++i) {
                mod *= dims[i].array_size_px;
                div *= (i == d ? dims[i].chunk_size_px : dims[i].array_size_px);
            }
            return (fid % mod) / div;
        };
        auto internal = [&](uint64_t fid) -> uint64_t {
            std::vector<uint64_t> astr(nd - 2, 1), cstr(nd - 2, 1);
            uint64_t off = 0;
            for (int i = nd - 3; i > 0; --i) {
                const uint64_t idx =
                  (fid / astr[i]) % dims[i].array_size_px % dims[i].chunk_size_px;
                astr[i - 1] = astr[i] * dims[i].array_size_px;
                cstr[i - 1] = cstr[i] * dims[i].chunk_size_px;
                off += idx * cstr[i];
            }
            off += ((fid / astr[0]) % dims[0].chunk_size_px) * cstr[0];
            return off * tile_bytes;
        };
        const uint64_t layer0 = first_frame / layer_frames;
        for (uint32_t k = 0; k < n_frames; ++k) {
            const uint64_t fid = first_frame + k;
            uint64_t group = 0;
            for (int i = nd - 3; i > 0; --i)
                group += lattice_index(fid, i) * strides[i];
            frame_offset_bytes[k] = (fid / layer_frames - layer0) * chunks_in_layer * per_chunk +
                                    group * per_chunk + internal(fid);
        }
        if (chunk_bytes)
            *chunk_bytes = per_chunk;
        if (layer_bytes)
            *layer_bytes = chunks_in_layer * per_chunk;
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_plan_levels(const aqz_dimension* dims,
                uint32_t ndims,
                uint32_t max_levels,
                aqz_dimension* out,
                uint32_t out_cap_levels,
                uint32_t* n_levels)
{
    try {
        if (!dims || !n_levels || ndims < 3 || ndims > AQZ_MAX_DIMS) {
            set_global_error("plan_levels: need 3..%d dimensions", AQZ_MAX_DIMS);
            return AQZ_INVALID_ARGUMENT;
        }
        for (uint32_t i = 0; i < ndims; ++i) {
            if (dims[i].chunk_size_px == 0) {
                set_global_error("plan_levels: dimension %u has chunk size 0", i);
                return AQZ_INVALID_ARGUMENT;
            }
        }
        const aqz_dimension& x = dims[ndims - 1];
        const aqz_dimension& y = dims[ndims - 2];
        const aqz_dimension& z = dims[ndims - 3];
        uint32_t levels = std::min(divisions(x), divisions(y));
        if (z.type == AQZ_DIM_SPACE)
            levels = std::max(levels, divisions(z));
        if (max_levels > 0)
            levels = std::min(levels, max_levels);
        *n_levels = levels + 1;
        if (!out)
            return AQZ_OK;
        if (out_cap_levels < levels + 1) {
            set_global_error("plan_levels: room for %u levels, need %u",
                             out_cap_levels, levels + 1);
            return AQZ_OVERFLOW;
        }
        std::copy(dims, dims + ndims, out);
        for (uint32_t l = 1; l <= levels; ++l) {
            const aqz_dimension* p = out + size_t(l - 1) * ndims;
            aqz_dimension* c = out + size_t(l) * ndims;
            std::copy(p, p + ndims - 3, c);
            const aqz_dimension& pz = p[ndims - 3];
            c[ndims - 3] = (pz.type == AQZ_DIM_SPACE && pz.array_size_px > pz.chunk_size_px)
                             ? halve(pz)
                             : pz;
            const aqz_dimension& py = p[ndims - 2];
            const aqz_dimension& px = p[ndims - 1];
            const bool shrink_xy = std::min(py.array_size_px, px.array_size_px) >
                                   std::max(py.chunk_size_px, px.chunk_size_px);
            c[ndims - 2] = shrink_xy ? halve(py) : py;
            c[ndims - 1] = shrink_xy ? halve(px) : px;
        }
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_ds_create(const aqz_level_desc* levels,
              uint32_t n_levels,
              int dtype,
              int method,
              int device,
              aqz_ds** out)
{
    try {
        if (!out) {
            set_global_error("create: null output handle");
            return AQZ_INVALID_ARGUMENT;
        }
        *out = nullptr;
        if (!levels || n_levels == 0 || n_levels > AQZ_MAX_LEVELS) {
            set_global_error("create: need 1..%d levels", AQZ_MAX_LEVELS);
            return AQZ_INVALID_ARGUMENT;
        }
        if (!aqz::dtype_valid(dtype)) {
            set_global_error("Invalid data type: %d", dtype);
            return AQZ_INVALID_ARGUMENT;
        }
        if (!aqz::method_valid(method)) {
            set_global_error("Invalid downsampling method: %d", method);
            return AQZ_INVALID_ARGUMENT;
        }
        for (uint32_t l = 0; l < n_levels; ++l) {
            if (levels[l].width == 0 || levels[l].height == 0) {
                set_global_error("create: level %u has an empty frame", l);
                return AQZ_INVALID_ARGUMENT;
            }
            if (l > 0) {
                const aqz_level_desc& a = levels[l - 1];
                const aqz_level_desc& b = levels[l];
                const bool same = b.width == a.width && b.height == a.height;
                const bool half = b.width == (a.width + 1) / 2 &&
                                  b.height == (a.height + 1) / 2;
                // scale_image always halves both; anything else fails the
                // reference's dimension EXPECTs (downsampler.cpp:348-356).
                if (!same && !half) {
                    set_global_error("create: level %u is neither a copy nor a 2x "
                                     "reduction of level %u", l, l - 1);
                    return AQZ_INVALID_ARGUMENT;
                }
            }
        }

        int n_devices = 0;
        if (hipGetDeviceCount(&n_devices) != hipSuccess)
            n_devices = 0;
        if (device < 0) {
            const char* env = std::getenv("AQZ_GPU_DEVICE");
            if (env && std::strcmp(env, "spread") == 0) {
                // each new handle on the next GPU: the arrays of a stream (or
                // several streams in one process) spread their pyramids over
                // the node; their frames are independent, so no collective
                static std::atomic<uint32_t> next{ 0 };
                device = n_devices > 0 ? int(next++ % uint32_t(n_devices)) : 0;
            } else if (env && *env) {
                device = std::atoi(env);
            } else if (hipGetDevice(&device) != hipSuccess) {
                device = 0;
            }
        }
        if (n_devices > 0 && (device < 0 || device >= n_devices)) {
            set_global_error("create: no HIP device %d (%d visible)", device, n_devices);
            return AQZ_INVALID_ARGUMENT;
        }

        auto* ds = new aqz_ds();
        ds->device = device;
        ds->dtype = dtype;
        ds->method = method;
        ds->bpp = aqz::dtype_bytes(dtype);
        ds->n = n_levels;
        ds->lv = std::vector<Level>(n_levels);
        ds->staged = env_flag("AQZ_PINNED_STAGING");
        ds->tile_pass = env_flag("AQZ_STREAM_TILE_PASS");
        size_t level_total = 0;
        for (uint32_t l = 0; l < n_levels; ++l) {
            Level& lv = ds->lv[l];
            lv.desc = levels[l];
            lv.bytes = size_t(levels[l].width) * levels[l].height * ds->bpp;
            if (l > 0) {
                lv.xy = levels[l].width < levels[l - 1].width ||
                        levels[l].height < levels[l - 1].height;
                lv.zh = levels[l].planes < levels[l - 1].planes;
                level_total += lv.bytes;
            }
        }
        const char* eager_env = std::getenv("AQZ_EAGER_READBACK");
        ds->eager = n_levels > 1 && level_total <= kEagerBytes &&
                    !(eager_env && std::strcmp(eager_env, "0") == 0);

        auto fail = [&](hipError_t e, const char* what) {
            const int code = e == hipErrorOutOfMemory ? AQZ_OUT_OF_MEMORY
                                                      : AQZ_INTERNAL_ERROR;
            set_global_error("%s: %s", what, hipGetErrorString(e));
            release(ds);
            return code;
        };
    #define CREATE_TRY(expr, what)                                                 \
        do {                                                                       \
            if (const hipError_t e_ = (expr); e_ != hipSuccess)                    \
                return fail(e_, what);                                             \
        } while (0)
        CREATE_TRY(hipSetDevice(device), "hipSetDevice");
        CREATE_TRY(ds->own_stream.create(), "hipStreamCreate");
        ds->stream = ds->own_stream;
        CREATE_TRY(ds->h2d_done.create(), "hipEventCreate");
        CREATE_TRY(ds->join.create(), "hipEventCreate");
        CREATE_TRY(ds->d_in.reserve(ds->lv[0].bytes), "hipMalloc level 0");
        if (ds->eager) {
            CREATE_TRY(ds->levels_d2h.create(), "hipEventCreate");
            for (uint32_t l = 1; l < n_levels; ++l)
                CREATE_TRY(ds->lv[l].h_level.reserve(ds->lv[l].bytes),
                           "hipHostMalloc level copy");
        }
        if (ds->staged)
            CREATE_TRY(ds->h_stage.reserve(ds->lv[0].bytes), "hipHostMalloc staging");
        ds->device_bytes = ds->lv[0].bytes;
        for (uint32_t l = 1; l < n_levels; ++l) {
            Level& lv = ds->lv[l];
            CREATE_TRY(lv.slot[0].reserve(lv.bytes), "hipMalloc level");
            CREATE_TRY(lv.slot[1].reserve(lv.bytes), "hipMalloc level");
            ds->device_bytes += 2 * lv.bytes;
            if (lv.zh) {
                CREATE_TRY(lv.d_partial.reserve(lv.bytes), "hipMalloc partial");
                ds->device_bytes += lv.bytes;
            }
        }
    #undef CREATE_TRY
        *out = ds;
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

void
aqz_ds_destroy(aqz_ds* ds)
{
    try {
        release(ds);
    } catch (...) {
        (void)ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_ds_add_frame(aqz_ds* ds, const void* host_frame, size_t nbytes)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (int rc = settle(ds))
            return rc;
        if (int rc = check_host_frame(ds, host_frame, nbytes, "add_frame"))
            return rc;
        release_holds(ds);
        return add_host_frame(ds, host_frame);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_add_frame_async(aqz_ds* ds, const void* host_frame, size_t nbytes)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (int rc = settle(ds))
            return rc;
        if (int rc = check_host_frame(ds, host_frame, nbytes, "add_frame_async"))
            return rc;
        release_holds(ds);
        auto& a = ds->async;
        if (!a.worker.joinable())
            a.worker = std::thread(async_worker, ds);
        {
            std::lock_guard<std::mutex> lk(a.m);
            a.frame = host_frame;
            a.input = host_frame;
        }
        a.cv.notify_all();
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_add_frame_async_take(aqz_ds* ds,
                            const void* host_frame,
                            size_t nbytes,
                            aqz_level_take* takes)
{
    try {
        if (!ds || !takes)
            return AQZ_INVALID_ARGUMENT;
        if (int rc = settle(ds))
            return rc;
        if (int rc = check_host_frame(ds, host_frame, nbytes, "add_frame_async_take"))
            return rc;
        for (uint32_t L = 1; L < ds->n; ++L) {
            const aqz_level_take& t = takes[L];
            if (t.mode < AQZ_TAKE_NONE || t.mode > AQZ_TAKE_HOLD ||
                ((t.tile_rows == 0) != (t.tile_cols == 0)))
                return ds->fail_arg("add_frame_async_take: level " + std::to_string(L) +
                                    ": bad mode or tile shape");
            if (t.mode == AQZ_TAKE_HOLD && ds->lv[L].cached() >= 0)
                return ds->fail_arg("add_frame_async_take: level " + std::to_string(L) +
                                    " is held by the caller but also cached here");
            // every take buffer is checked before the job is queued, so the
            // background takes cannot fail half way and leave a level taken
            // (uncached here) that the caller never learns about
            if (t.mode == AQZ_TAKE_INTO) {
                const Level& lv = ds->lv[L];
                const size_t need =
                  t.tile_rows ? tile_geom(ds, lv, t.tile_rows, t.tile_cols).tile_bytes : lv.bytes;
                if (!t.dst || t.cap < need)
                    return ds->fail_arg("add_frame_async_take: level " + std::to_string(L) +
                                        ": take buffer missing or smaller than " +
                                        std::to_string(need) + " bytes");
            }
        }
        for (uint32_t L = 1; L < ds->n; ++L)
            ds->lv[L].held = takes[L].mode == AQZ_TAKE_HOLD;
        auto& a = ds->async;
        if (!a.worker.joinable())
            a.worker = std::thread(async_worker, ds);
        {
            std::lock_guard<std::mutex> lk(a.m);
            a.frame = host_frame;
            a.input = host_frame;
            a.takes = takes;
        }
        a.cv.notify_all();
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_wait(aqz_ds* ds)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        return settle(ds);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_wait_input(aqz_ds* ds)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        auto& a = ds->async;
        if (!a.worker.joinable())
            return AQZ_OK;
        std::unique_lock<std::mutex> lk(a.m);
        a.cv.wait(lk, [&] { return a.input == nullptr; });
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_input_pending(aqz_ds* ds, int* pending)
{
    try {
        if (!ds || !pending)
            return AQZ_INVALID_ARGUMENT;
        *pending = 0;
        auto& a = ds->async;
        if (a.worker.joinable()) {
            std::lock_guard<std::mutex> lk(a.m);
            *pending = a.input != nullptr;
        }
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_poll(aqz_ds* ds, int* done)
{
    try {
        if (!ds || !done)
            return AQZ_INVALID_ARGUMENT;
        *done = 1;
        auto& a = ds->async;
        if (a.worker.joinable()) {
            std::lock_guard<std::mutex> lk(a.m);
            *done = a.frame == nullptr;
        }
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_add_device_frame(aqz_ds* ds, const void* device_frame, size_t nbytes)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (int rc = settle(ds))
            return rc;
        if (!device_frame || nbytes != ds->lv[0].bytes)
            return ds->fail_arg("add_device_frame: expected " +
                                std::to_string(ds->lv[0].bytes) + " bytes, got " +
                                std::to_string(nbytes));
        release_holds(ds);
        if (int rc = bind_device(ds))
            return rc;
        if (int rc = process_input(ds, device_frame))
            return rc;
        return eager_readback(ds);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_take_frame(aqz_ds* ds,
                  uint32_t level,
                  void* dst,
                  size_t cap,
                  size_t* nbytes,
                  int* has_frame)
{
    try {
        if (!ds || !has_frame)
            return AQZ_INVALID_ARGUMENT;
        *has_frame = 0;
        if (int rc = settle(ds))
            return rc;
        return take_plain(ds, level, dst, cap, nbytes, has_frame);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_set_level_tiling(aqz_ds* ds, uint32_t level, uint32_t tile_rows, uint32_t tile_cols)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (int rc = settle(ds))
            return rc;
        if (level == 0 || level >= ds->n)
            return ds->fail_arg("set_level_tiling: bad level " + std::to_string(level));
        if ((tile_rows == 0) != (tile_cols == 0))
            return ds->fail_arg("set_level_tiling: tile rows/cols must both be 0 or >0");
        if (int rc = bind_device(ds))
            return rc;
        HIP_TRY(ds, hipStreamSynchronize(ds->stream), "hipStreamSynchronize");
        Level& lv = ds->lv[level];
        for (Level::Tiled& t : lv.tiled) {
            t.tiles.reset();
            t.flags.reset();
        }
        lv.h_tiles.reset();
        lv.tile_rows = lv.tile_cols = 0;
        lv.drop_tiled();
        lv.no_eager = tile_rows != 0;
        if (tile_rows == 0)
            return AQZ_OK;
        const TileGeom g = tile_geom(ds, lv, tile_rows, tile_cols);
        for (Level::Tiled& t : lv.tiled)
            HIP_TRY(ds, t.tiles.reserve(g.tile_bytes), "hipMalloc tiles");
        // slice flags live in pinned host memory the kernel writes directly, so
        // take_frame_tiled needs no separate flag copy
        for (Level::Tiled& t : lv.tiled)
            HIP_TRY(ds, t.flags.reserve(g.flag_bytes), "hipHostMalloc flags");
        if (ds->eager)
            HIP_TRY(ds, lv.h_tiles.reserve(g.tile_bytes), "hipHostMalloc tile copy");
        lv.tile_rows = tile_rows;
        lv.tile_cols = tile_cols;
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_take_frame_tiled(aqz_ds* ds,
                        uint32_t level,
                        uint32_t tile_rows,
                        uint32_t tile_cols,
                        void* dst,
                        size_t cap,
                        uint8_t* tile_nonzero,
                        size_t* nbytes,
                        int* has_frame)
{
    try {
        if (!ds || !has_frame)
            return AQZ_INVALID_ARGUMENT;
        *has_frame = 0;
        if (int rc = settle(ds))
            return rc;
        return take_tiled(ds, level, tile_rows, tile_cols, dst, cap, tile_nonzero, nbytes,
                          has_frame);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_set_input_transpose(aqz_ds* ds, int transpose)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (int rc = settle(ds))
            return rc;
        if (int rc = bind_device(ds))
            return rc;
        if (transpose && !ds->d_tin) {
            HIP_TRY(ds, hipStreamSynchronize(ds->stream), "hipStreamSynchronize");
            HIP_TRY(ds, ds->d_tin.reserve(ds->lv[0].bytes), "hipMalloc transposed input");
            ds->device_bytes += ds->lv[0].bytes;
        }
        ds->transpose = transpose != 0;
        ds->last_input = nullptr;
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_take_input_frame(aqz_ds* ds,
                        uint32_t tile_rows,
                        uint32_t tile_cols,
                        void* dst,
                        size_t cap,
                        uint8_t* tile_nonzero,
                        size_t* nbytes,
                        int* has_frame)
{
    try {
        if (!ds || !has_frame)
            return AQZ_INVALID_ARGUMENT;
        *has_frame = 0;
        if (int rc = settle(ds))
            return rc;
        if ((tile_rows == 0) != (tile_cols == 0))
            return ds->fail_arg("take_input_frame: tile_rows and tile_cols must both be 0 "
                                "or both be nonzero");
        if (!ds->last_input)
            return AQZ_OK;
        const bool tiled = tile_rows != 0;
        const TileGeom g = tiled ? tile_geom(ds, ds->lv[0], tile_rows, tile_cols)
                                 : TileGeom{ 1, ds->lv[0].bytes, 0 };
        *has_frame = 1;
        if (nbytes)
            *nbytes = g.tile_bytes;
        if (!dst)
            return AQZ_OK;
        if (cap < g.tile_bytes)
            return ds->fail_arg("take_input_frame: buffer too small");
        if (int rc = bind_device(ds))
            return rc;
        if (tiled) {
            if (int rc = tile_to_host(ds, ds->last_input, ds->lv[0].desc, tile_rows, tile_cols, g,
                                      dst, tile_nonzero))
                return rc;
        } else {
            HIP_TRY(ds,
                    hipMemcpyAsync(dst, ds->last_input, g.tile_bytes, hipMemcpyDeviceToHost,
                                   ds->stream),
                    "hipMemcpyAsync D2H");
            HIP_TRY(ds, hipStreamSynchronize(ds->stream), "hipStreamSynchronize");
        }
        ds->last_input = nullptr;
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_transpose_frame_device(int dtype,
                           const void* device_src,
                           uint32_t rows,
                           uint32_t cols,
                           void* device_dst,
                           void* hip_stream)
{
    try {
        if (!aqz::dtype_valid(dtype) || !device_src || !device_dst || rows == 0 || cols == 0) {
            set_global_error("transpose_frame_device: invalid argument");
            return AQZ_INVALID_ARGUMENT;
        }
        const hipError_t e = aqz::launch_transpose(dtype, device_src, rows, cols, device_dst,
                                                   static_cast<hipStream_t>(hip_stream));
        if (e != hipSuccess) {
            set_global_error("transpose_frame_device: %s", hipGetErrorString(e));
            return e == hipErrorInvalidValue ? AQZ_INVALID_ARGUMENT : AQZ_INTERNAL_ERROR;
        }
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_tile_frame_device(int dtype,
                      const void* device_frame,
                      uint32_t width,
                      uint32_t height,
                      uint32_t tile_rows,
                      uint32_t tile_cols,
                      void* device_tiles,
                      uint32_t* device_nonzero,
                      void* hip_stream)
{
    try {
        if (!aqz::dtype_valid(dtype) || !device_frame || !device_tiles ||
            !device_nonzero) {
            set_global_error("tile_frame_device: invalid argument");
            return AQZ_INVALID_ARGUMENT;
        }
        const hipError_t e = aqz::launch_tile_frame(
          dtype, device_frame, width, height, tile_rows, tile_cols, device_tiles,
          device_nonzero, static_cast<hipStream_t>(hip_stream));
        if (e != hipSuccess) {
            set_global_error("tile_frame_device: %s", hipGetErrorString(e));
            return e == hipErrorInvalidValue ? AQZ_INVALID_ARGUMENT : AQZ_INTERNAL_ERROR;
        }
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

uint32_t
aqz_tile_slices(uint32_t tile_rows, uint32_t tile_cols)
{
    return aqz::tile_slices(tile_rows, tile_cols);
}

int
aqz_tile_frame_device_sliced(int dtype,
                             const void* device_frame,
                             uint32_t width,
                             uint32_t height,
                             uint32_t tile_rows,
                             uint32_t tile_cols,
                             void* device_tiles,
                             uint8_t* device_slice_flags,
                             void* hip_stream)
{
    try {
        if (!aqz::dtype_valid(dtype) || !device_frame || !device_tiles || !device_slice_flags) {
            set_global_error("tile_frame_device_sliced: invalid argument");
            return AQZ_INVALID_ARGUMENT;
        }
        const hipError_t e = aqz::launch_tile_frame_sliced(
          dtype, device_frame, width, height, tile_rows, tile_cols, device_tiles,
          device_slice_flags, static_cast<hipStream_t>(hip_stream));
        if (e != hipSuccess) {
            set_global_error("tile_frame_device_sliced: %s", hipGetErrorString(e));
            return e == hipErrorInvalidValue ? AQZ_INVALID_ARGUMENT : AQZ_INTERNAL_ERROR;
        }
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_ds_run_device_batch(aqz_ds* ds,
                        const void* device_frames,
                        uint32_t n_frames,
                        void* const* device_out_levels,
                        uint32_t* out_counts,
                        void* hip_stream)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (int rc = settle(ds))
            return rc;
        if (ds->transpose)
            return ds->fail_arg("ds_run_device_batch: input transposition applies to the per-frame path "
                                "(add_frame / add_device_frame) only");
        ds->last_input = nullptr;
        if (!device_frames || !device_out_levels)
            return ds->fail_arg("run_device_batch: null buffer");
        for (uint32_t l = 1; l < ds->n; ++l)
            if (!device_out_levels[l])
                return ds->fail_arg("run_device_batch: null output for level " +
                                    std::to_string(l));
        if (int rc = bind_device(ds))
            return rc;
        // The batch runs on the caller's stream.  The fused paths touch only
        // the caller's buffers; the per-frame fallback reads and writes the
        // handle's device state (the stored Z plane, level slots) that earlier
        // add_frame calls left queued on ds->stream, and later add_frame calls
        // must see what it wrote.  So the fallback joins the two streams both
        // ways (joining on every batch put a cross-stream wait in front of
        // each fused launch), and the guard restores ds->stream on
        // every exit, exceptions included.
        struct StreamSwap
        {
            aqz_ds* ds;
            hipStream_t saved, user;
            bool joined = false;
            void enter() { ds->stream = user ? user : saved; }
            hipError_t join()
            {
                if (!user || user == saved)
                    return hipSuccess;
                hipError_t e = hipEventRecord(ds->join, saved);
                if (e == hipSuccess)
                    e = hipStreamWaitEvent(user, ds->join, 0);
                joined = e == hipSuccess;
                return e;
            }
            ~StreamSwap()
            {
                if (joined && hipEventRecord(ds->join, ds->stream) == hipSuccess)
                    (void)hipStreamWaitEvent(saved, ds->join, 0);
                ds->stream = saved;
            }
        } swap{ ds, ds->stream, static_cast<hipStream_t>(hip_stream) };
        swap.enter();

        std::vector<uint32_t> emitted(ds->n, 0);
        int rc = AQZ_OK;

        bool pure_xy = ds->n > 1;
        bool pure_xyz = ds->n > 1;
        for (uint32_t l = 1; l < ds->n; ++l) {
            const Level& lv = ds->lv[l];
            pure_xy = pure_xy && lv.xy && !lv.zh;
            // every level halves XY and Z, no odd stack (no pass-through plane)
            // and no stored earlier plane: planes pair up consecutively
            pure_xyz = pure_xyz && lv.xy && lv.zh && ds->lv[l - 1].desc.planes % 2 == 0 &&
                       !lv.has_partial;
        }
        pure_xyz = pure_xyz && n_frames > 0 && (n_frames % (1u << (ds->n - 1))) == 0;

        // Runs of up to `maxk` levels per launch, each level into the caller's
        // buffer.  A 2-D batch always stays batched: a run the fused cascade
        // cannot take (width or alignment) runs as one batched single-level
        // generic launch per level (launch_xy_run).  A volume batch is
        // all-or-nothing (its fallback is the per-frame state machine).
        const auto out_of = [&](uint32_t l) { return device_out_levels[l]; };
        const auto volume_takes_every_run = [&] {
            const void* src = device_frames;
            for (uint32_t L = 1, k; L < ds->n; L += k) {
                k = std::min<uint32_t>(ds->n - L, aqz::kMaxVolumeLevels);
                aqz::LevelOut o[aqz::kMaxFusedLevels];
                fill_outs(ds, L, k, out_of, o);
                const aqz_level_desc& a = ds->lv[L - 1].desc;
                if (!aqz::volume_supported(ds->dtype, src, a.width, a.height, o, int(k)))
                    return false;
                src = o[k - 1].ptr;
            }
            return true;
        };
        const bool batched_2d = !ds->force_per_frame && pure_xy && n_frames > 0;
        const bool volume =
          !ds->force_per_frame && !batched_2d && pure_xyz && volume_takes_every_run();

        // Mixed pyramids (kind 7), only where both routes above pass: XYZ
        // levels followed by an XY-only or a Z-only tail, or any other order
        // of the three classes, cut into runs (plan_pyramid_runs) that chain
        // through the caller's level buffers — launch_volume, launch_xy_run,
        // launch_zrun — on the caller's stream.  Every run is planned before
        // the first is queued; one the launchers would refuse leaves the
        // whole call to the per-frame state machine, as a volume batch does.
        aqz::PyramidRuns mixed;
        const auto run_src = [&](const aqz::PyramidRun& r) -> const void* {
            return r.first == 1 ? device_frames : device_out_levels[r.first - 1];
        };
        const auto mixed_takes_every_run = [&] {
            std::vector<aqz::PyramidLevel> pl(ds->n);
            for (uint32_t l = 0; l < ds->n; ++l) {
                const Level& lv = ds->lv[l];
                pl[l] = { lv.desc.width, lv.desc.height, lv.desc.planes, l > 0 && lv.has_partial };
            }
            mixed = aqz::plan_pyramid_runs(pl.data(), ds->n, n_frames);
            if (!mixed.ok)
                return false;
            for (const aqz::PyramidRun& r : mixed.runs) {
                aqz::LevelOut o[aqz::kMaxFusedLevels];
                fill_outs(ds, r.first, r.levels, out_of, o);
                const Level& a = ds->lv[r.first - 1];
                const void* src = run_src(r);
                bool ok = true;
                if (r.cls == aqz::kClassXYZ) {
                    ok = aqz::plan_volume(ds->dtype, ds->method, src, a.elems(), a.desc.width,
                                          a.desc.height, o, int(r.levels), r.frames_in,
                                          aqz::launch_switches())
                           .valid;
                } else if (r.cls == aqz::kClassXY) {
                    // the fused cascade, or launch_xy_generic's rule level by level
                    if (!aqz::cascade_supported(ds->dtype, src, a.elems(), a.desc.width,
                                                a.desc.height, o, int(r.levels)))
                        for (uint32_t j = 0; j < r.levels; ++j) {
                            const aqz_level_desc& in = ds->lv[r.first + j - 1].desc;
                            ok = ok && in.width && in.height && o[j].w == (in.width + 1) / 2 &&
                                 o[j].h == (in.height + 1) / 2;
                        }
                } else {
                    for (uint32_t j = 0; j < r.levels; ++j)
                        ok = ok && o[j].w == a.desc.width && o[j].h == a.desc.height;
                    ok = ok && aqz::plan_zrun(ds->dtype, ds->method, src, a.elems(), a.elems(), o,
                                              int(r.levels), r.frames_in)
                                 .valid;
                }
                if (!ok)
                    return false;
            }
            return true;
        };
        const bool mixed_runs =
          !ds->force_per_frame && !batched_2d && !volume && mixed_takes_every_run();

        if (mixed_runs) {
            for (const aqz::PyramidRun& r : mixed.runs) {
                aqz::LevelOut o[aqz::kMaxFusedLevels];
                fill_outs(ds, r.first, r.levels, out_of, o);
                const Level& a = ds->lv[r.first - 1];
                const void* src = run_src(r);
                hipError_t e;
                bool fused;
                if (r.cls == aqz::kClassXYZ)
                    e = aqz::launch_volume(ds->dtype, ds->method, src, a.elems(), a.desc.width,
                                           a.desc.height, o, int(r.levels), r.frames_in,
                                           ds->stream);
                else if (r.cls == aqz::kClassXY)
                    e = launch_xy_run(ds, src, r.first, r.levels, o, r.frames_in, ds->stream,
                                      &fused);
                else
                    e = aqz::launch_zrun(ds->dtype, ds->method, src, a.elems(), a.elems(), o,
                                         int(r.levels), r.frames_in, ds->stream);
                if (e != hipSuccess) {
                    rc = ds->fail(e, "batch mixed runs");
                    break;
                }
            }
            // as below: a failed launch leaves the counts where they were
            if (rc == AQZ_OK) {
                uint32_t frames = n_frames;
                for (uint32_t l = 0; l < ds->n; ++l) {
                    if (l > 0 && ds->lv[l].zh)
                        frames >>= 1;
                    emitted[l] = frames;
                    ds->lv[l].count += frames;
                }
            }
            ds->last_batch_kind = 7;
        } else if (batched_2d || volume) {
            // Whole batch in batched launches; every frame / plane group independent.
            const uint32_t maxk = volume ? aqz::kMaxVolumeLevels : aqz::kMaxFusedLevels;
            const void* src = device_frames;
            uint32_t planes = n_frames;
            bool all_fused = true;
            for (uint32_t L = 1, k; L < ds->n; L += k) {
                k = std::min<uint32_t>(ds->n - L, maxk);
                aqz::LevelOut o[aqz::kMaxFusedLevels];
                fill_outs(ds, L, k, out_of, o);
                hipError_t e;
                if (volume) {
                    const Level& a = ds->lv[L - 1];
                    e = aqz::launch_volume(ds->dtype, ds->method, src, a.elems(), a.desc.width,
                                           a.desc.height, o, int(k), planes, ds->stream);
                    planes >>= k;
                } else {
                    bool fused;
                    e = launch_xy_run(ds, src, L, k, o, n_frames, ds->stream, &fused);
                    all_fused = all_fused && fused;
                }
                if (e != hipSuccess) {
                    rc = ds->fail(e, volume ? "batch volume" : "batch cascade");
                    break;
                }
                src = o[k - 1].ptr;
            }
            // a failed launch leaves the counts (and the odd-stack state they
            // carry) where they were
            if (rc == AQZ_OK) {
                for (uint32_t l = 0; l < ds->n; ++l) {
                    emitted[l] = volume ? (n_frames >> l) : n_frames;
                    ds->lv[l].count += emitted[l];
                }
            }
            ds->last_batch_kind = volume ? 2 : (all_fused ? 1 : 3);
        } else {
            ds->last_batch_kind = 0;
            if (hipError_t e = swap.join(); e != hipSuccess)
                return ds->fail(e, "run_device_batch: stream join");
            Sink sink;
            sink.batch = true;
            sink.out = device_out_levels;
            sink.emitted = &emitted;
            const uint8_t* base = static_cast<const uint8_t*>(device_frames);
            for (uint32_t i = 0; i < n_frames && rc == AQZ_OK; ++i)
                rc = process_frame(ds, base + size_t(i) * ds->lv[0].bytes, sink);
            emitted[0] = n_frames;
        }
        if (out_counts)
            std::copy(emitted.begin(), emitted.end(), out_counts);
        return rc;
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

} // extern "C"

namespace {

// Per-level frame offsets of a chunk-lattice batch into the device (elements),
// through one half of the pinned staging; returns the device pointers.
// `counts`, when set: level l carries counts[l] <= n_frames offsets (a volume
// or mixed batch, whose Z-halving levels emit fewer frames), not n_frames.
int
stage_lattice(aqz_ds* ds, const aqz_chunk_lattice* lat, uint32_t n_frames, hipStream_t stream,
              std::vector<const uint64_t*>* dev, int* half_out, const uint32_t* counts = nullptr,
              bool base = false)
{
    // `base`: slot 0 (level 0's offsets) is staged too
    const uint32_t l0 = base ? 0 : 1;
    const size_t need = size_t(ds->n) * n_frames;
    if (ds->d_lattice.capacity() < 2 * need * 8 || ds->h_lattice.capacity() < 2 * need * 8) {
        for (const aqz::Event& e : ds->lattice_done)
            if (e)
                HIP_TRY(ds, hipEventSynchronize(e), "hipEventSynchronize lattice");
        // both go, so the two always have one size (a half is capacity / 2)
        ds->d_lattice.reset();
        ds->h_lattice.reset();
        HIP_TRY(ds, ds->d_lattice.reserve(2 * need * 8), "hipMalloc lattice");
        HIP_TRY(ds, ds->h_lattice.reserve(2 * need * 8), "hipHostMalloc lattice");
        for (aqz::Event& e : ds->lattice_done)
            HIP_TRY(ds, e.create(), "event");
    }
    const int half = int(ds->lattice_calls++ & 1);
    // the batch two calls back read this half: it must have finished
    HIP_TRY(ds, hipEventSynchronize(ds->lattice_done[half]), "hipEventSynchronize lattice");
    const size_t lattice_half = ds->d_lattice.capacity() / 16; // entries per half
    uint64_t* h = static_cast<uint64_t*>(ds->h_lattice.get()) + size_t(half) * lattice_half;
    uint64_t* d = static_cast<uint64_t*>(ds->d_lattice.get()) + size_t(half) * lattice_half;
    dev->assign(ds->n, nullptr);
    for (uint32_t l = l0; l < ds->n; ++l)
        for (uint32_t k = 0, nk = counts ? counts[l] : n_frames; k < nk; ++k)
            h[size_t(l) * n_frames + k] = lat[l].frame_offset_bytes[k] / ds->bpp;
    HIP_TRY(ds, hipMemcpyAsync(d, h, need * 8, hipMemcpyHostToDevice, stream), "lattice upload");
    for (uint32_t l = l0; l < ds->n; ++l)
        (*dev)[l] = d + size_t(l) * n_frames;
    *half_out = half;
    return AQZ_OK;
}

// aqz_ds_run_device_batch_tiled (lat == nullptr: tiles of a frame back to
// back, frames back to back) and aqz_ds_run_device_batch_chunked (every tile
// into its chunk of the lattice).  `base` (the _base forms): index 0 of the
// per-level arguments is level 0's, written as tiles by the first run.
int
run_tiled(aqz_ds* ds,
          const char* who,
          const void* device_frames,
          uint32_t n_frames,
          const uint32_t* tile_rows,
          const uint32_t* tile_cols,
          void* const* device_out_levels,
          const aqz_chunk_lattice* lat,
          uint8_t* const* device_tile_nonzero,
          uint32_t* out_counts,
          void* hip_stream,
          bool base = false)
{
    const std::string w(who);
    if (int rc = settle(ds))
        return rc;
    if (ds->transpose)
        return ds->fail_arg(w + ": input transposition applies to the per-frame path only" +
                            (base ? " (level 0 is tiled as it arrives)" : ""));
    ds->last_input = nullptr;
    if (!device_frames || (!lat && (!device_out_levels || !tile_rows || !tile_cols)))
        return ds->fail_arg(w + ": null argument");
    if (ds->n < 2)
        return ds->fail_arg(w + ": the pyramid has no level to tile" +
                            (base ? ": level 0 is tiled by the kernel that reduces it" : ""));
    // levels 1 .. n-1 in order, then (`base`) level 0
    for (uint32_t i = 1; i < ds->n + (base ? 1u : 0u); ++i) {
        const uint32_t l = i < ds->n ? i : 0;
        if (l && (!ds->lv[l].xy || ds->lv[l].zh))
            return ds->fail_arg(w + ": pure-XY (2-D) pyramids only; level " + std::to_string(l) +
                                " does not halve XY alone" +
                                (base ? ", so level 0 cannot be tiled by this call either" : ""));
        const uint32_t tr = lat ? lat[l].tile_rows : tile_rows[l];
        const uint32_t tc = lat ? lat[l].tile_cols : tile_cols[l];
        const void* out = lat ? lat[l].device_base : device_out_levels[l];
        if (!out || !tr || !tc)
            return ds->fail_arg(w + ": level " + std::to_string(l) +
                                " needs an output and a nonzero tile shape");
        if (lat) {
            // every tile of every frame inside the lattice buffer: a bad
            // offset must be an argument error here, not a device fault
            const aqz_chunk_lattice& c = lat[l];
            const uint64_t ntiles = uint64_t((ds->lv[l].desc.width + tc - 1) / tc) *
                                    ((ds->lv[l].desc.height + tr - 1) / tr);
            const uint64_t tile_bytes = uint64_t(tr) * tc * ds->bpp;
            if (!c.frame_offset_bytes || c.chunk_stride_bytes % ds->bpp ||
                c.chunk_stride_bytes < tile_bytes)
                return ds->fail_arg(w + ": level " + std::to_string(l) +
                                    ": chunk stride must hold a tile and be a multiple of the "
                                    "pixel size, and frame offsets are required");
            const uint64_t extent = (ntiles - 1) * c.chunk_stride_bytes + tile_bytes;
            for (uint32_t k = 0; k < n_frames; ++k) {
                const uint64_t off = c.frame_offset_bytes[k];
                if (off % ds->bpp || off > c.capacity_bytes || c.capacity_bytes - off < extent)
                    return ds->fail_arg(w + ": level " + std::to_string(l) + " frame " +
                                        std::to_string(k) + ": offset " + std::to_string(off) +
                                        " puts its tiles outside the lattice buffer");
            }
        }
    }
    const auto tiled_out = [&](uint32_t l,
                               const std::vector<const uint64_t*>& off) -> aqz::TiledOut {
        uint8_t* nz = device_tile_nonzero ? device_tile_nonzero[l] : nullptr;
        if (lat)
            return { lat[l].device_base, lat[l].tile_rows, lat[l].tile_cols, nz, off[l],
                     lat[l].chunk_stride_bytes / ds->bpp };
        return { device_out_levels[l], tile_rows[l], tile_cols[l], nz };
    };
    // one run's outputs: row-major nowhere (the loop below fills in the chain),
    // level l's tiles by the caller's arguments and the staged offsets `off`
    const auto run_outs = [&](uint32_t L, uint32_t k, const std::vector<const uint64_t*>& off,
                              aqz::LevelOut* o, aqz::TiledOut* t) {
        fill_outs(ds, L, k, [](uint32_t) { return nullptr; }, o);
        for (uint32_t j = 0; j < k; ++j)
            t[j] = tiled_out(L + j, off);
    };
    if (base) {
        // every run's plan, the first with the base in it, before anything is
        // queued: a later run refused after the first had run would leave
        // level 0 written by a call that fails.  (The offsets' host copy
        // stands in for the staged one, and an aligned address for the chain
        // scratch later runs read: a plan reads neither.)
        std::vector<const uint64_t*> host_off(ds->n, nullptr);
        if (lat)
            for (uint32_t l = 0; l < ds->n; ++l)
                host_off[l] = lat[l].frame_offset_bytes;
        const aqz::TiledOut t0 = tiled_out(0, host_off);
        for (uint32_t L = 1; L < ds->n;) {
            const uint32_t k = std::min<uint32_t>(ds->n - L, aqz::kMaxFusedLevels);
            aqz::LevelOut o[aqz::kMaxFusedLevels];
            aqz::TiledOut t[aqz::kMaxFusedLevels];
            run_outs(L, k, host_off, o, t);
            const void* from = L == 1 ? device_frames : reinterpret_cast<const void*>(uintptr_t(256));
            const aqz_level_desc& a = ds->lv[L - 1].desc;
            const std::string also = L == 1 ? "" : ", so level 0 is not written either";
            if (!aqz::cascade_supported(ds->dtype, from, ds->lv[L - 1].elems(), a.width, a.height,
                                        o, int(k)))
                return ds->fail_arg(w + ": level " + std::to_string(L - 1) +
                                    " is narrower than one vector load (" +
                                    std::to_string(a.width) + " px) or misaligned" + also);
            if (!aqz::plan_cascade_tiled(ds->dtype, ds->method, from, ds->lv[L - 1].elems(),
                                         a.width, a.height, o, t, int(k), n_frames,
                                         aqz::launch_switches(), L == 1 ? &t0 : nullptr)
                   .valid)
                return ds->fail_arg(w + ": level " + std::to_string(L - 1) +
                                    ": unsupported geometry (a misaligned output, a padded side "
                                    "of 2^31 or more, 2^30 or more units or 2^32 or more "
                                    "zero-fill rows, or no frames)" + also);
            L += k;
        }
    }
    if (int rc = bind_device(ds))
        return rc;
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ds->stream;
    std::vector<const uint64_t*> d_off;
    int half = -1;
    if (lat)
        if (int rc = stage_lattice(ds, lat, n_frames, stream, &d_off, &half, nullptr, base))
            return rc;
    // From here on the staged half's upload is queued on `stream`: whatever
    // the exit, record the event that guards the pinned half, so a later call
    // never rewrites it while that copy may still read it.
    struct LatticeGuard
    {
        aqz_ds* ds;
        int half;
        hipStream_t stream;
        ~LatticeGuard()
        {
            if (half >= 0)
                (void)hipEventRecord(ds->lattice_done[half], stream);
        }
    } lattice_guard{ ds, half, stream };
    // Runs of up to kMaxFusedLevels levels; a run that feeds another also
    // writes its last level row-major into one half of d_chain (the runs
    // alternate halves, so a run never reads the half it writes).  The
    // first chained level is the largest: 1/256 of the base after 4 levels.
    const uint32_t first_feed = aqz::kMaxFusedLevels;
    const bool chained = first_feed + 1 < ds->n;
    // A previous batch may still be reading or writing d_chain on another
    // stream: order this one behind it.  Only pyramids deeper than one fused
    // run touch d_chain, so only they wait and record.  Once the wait is
    // queued, chain_done is recorded on every way out (ChainGuard), so a
    // failure after some runs were queued still fences them.
    if (chained) {
        if (ds->chain_done)
            HIP_TRY(ds, hipStreamWaitEvent(stream, ds->chain_done, 0), "hipStreamWaitEvent chain");
        else
            HIP_TRY(ds, ds->chain_done.create(), "event");
    }
    struct ChainGuard
    {
        aqz_ds* ds;
        hipStream_t stream;
        bool on;
        ~ChainGuard()
        {
            if (on)
                (void)hipEventRecord(ds->chain_done, stream);
        }
    } chain_guard{ ds, stream, chained };
    if (chained) {
        const size_t chain_half = size_t(n_frames) * ds->lv[first_feed].bytes;
        if (ds->d_chain.capacity() < 2 * chain_half) {
            HIP_TRY(ds, hipStreamSynchronize(stream), "hipStreamSynchronize");
            HIP_TRY(ds, ds->d_chain.reserve(2 * chain_half), "hipMalloc chain");
        }
    }
    const void* src = device_frames;
    for (uint32_t L = 1, run = 0; L < ds->n; ++run) {
        const uint32_t k = std::min<uint32_t>(ds->n - L, aqz::kMaxFusedLevels);
        const bool feeds = L + k < ds->n;
        aqz::LevelOut o[aqz::kMaxFusedLevels];
        aqz::TiledOut t[aqz::kMaxFusedLevels];
        // row-major only where the run feeds the next one (below)
        run_outs(L, k, d_off, o, t);
        // the base leaves with the run that reads it; later runs read chain
        // scratch and know nothing of level 0
        const bool with_base = base && run == 0;
        const aqz::TiledOut t0 = with_base ? tiled_out(0, d_off) : aqz::TiledOut{};
        void* chain = ds->d_chain.bytes() + (run & 1) * (ds->d_chain.capacity() / 2);
        if (feeds)
            o[k - 1].ptr = chain;
        const aqz_level_desc& a = ds->lv[L - 1].desc;
        const uint64_t a_elems = ds->lv[L - 1].elems();
        if (!aqz::cascade_supported(ds->dtype, src, a_elems, a.width, a.height, o, int(k)))
            return ds->fail_arg(w + ": level " + std::to_string(L - 1) +
                                " is narrower than one vector load (" + std::to_string(a.width) +
                                " px)");
        const hipError_t e =
          aqz::launch_cascade_tiled(ds->dtype, ds->method, src, a_elems, a.width, a.height, o, t,
                                    int(k), n_frames, stream, with_base ? &t0 : nullptr);
        if (e != hipSuccess)
            return e == hipErrorInvalidValue ? ds->fail_arg(w + ": unsupported geometry")
                                             : ds->fail(e, "batch tiled cascade");
        src = chain;
        L += k;
    }
    for (uint32_t l = 0; l < ds->n; ++l) {
        ds->lv[l].count += n_frames;
        if (out_counts)
            out_counts[l] = n_frames;
    }
    ds->last_batch_kind = base ? 6 : 4;
    return AQZ_OK;
}

// aqz_ds_run_device_volume_tiled (lat == nullptr) and
// aqz_ds_run_device_volume_chunked: run_tiled's two forms for pyramids whose
// levels halve XY and Z, through the fused volume kernel.  Level l emits
// n_frames >> l planes.  All or nothing: the per-frame state machine has no
// tiled batch form to fall back to.
int
run_volume_tiled(aqz_ds* ds,
                 const char* who,
                 const void* device_frames,
                 uint32_t n_frames,
                 const uint32_t* tile_rows,
                 const uint32_t* tile_cols,
                 void* const* device_out_levels,
                 const aqz_chunk_lattice* lat,
                 uint8_t* const* device_tile_nonzero,
                 uint32_t* out_counts,
                 void* hip_stream)
{
    const std::string w(who);
    if (int rc = settle(ds))
        return rc;
    if (ds->transpose)
        return ds->fail_arg(w + ": input transposition applies to the per-frame path only");
    ds->last_input = nullptr;
    if (!device_frames || (!lat && (!device_out_levels || !tile_rows || !tile_cols)))
        return ds->fail_arg(w + ": null argument");
    if (ds->n < 2)
        return ds->fail_arg(w + ": the pyramid has no level to tile");
    // aqz_ds_run_device_batch's pure_xyz condition, level by level
    for (uint32_t l = 1; l < ds->n; ++l) {
        const Level& lv = ds->lv[l];
        if (!lv.xy || !lv.zh)
            return ds->fail_arg(w + ": volume pyramids only; level " + std::to_string(l) +
                                " does not halve XY and Z");
        if (ds->lv[l - 1].desc.planes % 2 != 0)
            return ds->fail_arg(w + ": level " + std::to_string(l - 1) +
                                " has an odd plane count (level " + std::to_string(l) +
                                " would pass a plane through)");
        if (lv.has_partial)
            return ds->fail_arg(w + ": level " + std::to_string(l) +
                                " holds an earlier plane of the per-frame path");
    }
    if (n_frames == 0 || n_frames % (1u << (ds->n - 1)) != 0)
        return ds->fail_arg(w + ": " + std::to_string(n_frames) +
                            " planes is not a nonzero multiple of " +
                            std::to_string(1u << (ds->n - 1)) + ", what level " +
                            std::to_string(ds->n - 1) + " pairs up");
    for (uint32_t l = 1; l < ds->n; ++l) {
        const uint32_t tr = lat ? lat[l].tile_rows : tile_rows[l];
        const uint32_t tc = lat ? lat[l].tile_cols : tile_cols[l];
        const void* out = lat ? lat[l].device_base : device_out_levels[l];
        if (!out || !tr || !tc)
            return ds->fail_arg(w + ": level " + std::to_string(l) +
                                " needs an output and a nonzero tile shape");
        if (lat) {
            // run_tiled's lattice checks over the level's n_frames >> l planes
            const aqz_chunk_lattice& c = lat[l];
            const uint64_t ntiles = uint64_t((ds->lv[l].desc.width + tc - 1) / tc) *
                                    ((ds->lv[l].desc.height + tr - 1) / tr);
            const uint64_t tile_bytes = uint64_t(tr) * tc * ds->bpp;
            if (!c.frame_offset_bytes || c.chunk_stride_bytes % ds->bpp ||
                c.chunk_stride_bytes < tile_bytes)
                return ds->fail_arg(w + ": level " + std::to_string(l) +
                                    ": chunk stride must hold a tile and be a multiple of the "
                                    "pixel size, and frame offsets are required");
            const uint64_t extent = (ntiles - 1) * c.chunk_stride_bytes + tile_bytes;
            for (uint32_t k = 0; k < (n_frames >> l); ++k) {
                const uint64_t off = c.frame_offset_bytes[k];
                if (off % ds->bpp || off > c.capacity_bytes || c.capacity_bytes - off < extent)
                    return ds->fail_arg(w + ": level " + std::to_string(l) + " plane " +
                                        std::to_string(k) + ": offset " + std::to_string(off) +
                                        " puts its tiles outside the lattice buffer");
            }
        }
    }
    // Runs of up to kMaxVolumeLevels levels.  Every run must fit the fused
    // volume kernel and the tiled plan's limits before anything is queued:
    // the plans look at addresses and sizes only, so a stand-in for the chain
    // scratch (aligned, like the allocation) serves here.
    const uint32_t maxk = aqz::kMaxVolumeLevels;
    const bool chained = 1 + maxk < ds->n;
    const auto tiled_outs = [&](uint32_t L, uint32_t k, const std::vector<const uint64_t*>& off,
                                aqz::TiledOut* t) {
        for (uint32_t j = 0; j < k; ++j) {
            const uint32_t l = L + j;
            uint8_t* nz = device_tile_nonzero ? device_tile_nonzero[l] : nullptr;
            if (lat)
                t[j] = { lat[l].device_base, lat[l].tile_rows, lat[l].tile_cols, nz,
                         off.empty() ? nullptr : off[l], lat[l].chunk_stride_bytes / ds->bpp };
            else
                t[j] = { device_out_levels[l], tile_rows[l], tile_cols[l], nz };
        }
    };
    {
        const void* src = device_frames;
        void* const stand_in = reinterpret_cast<void*>(uintptr_t(256));
        const std::vector<const uint64_t*> none;
        for (uint32_t L = 1, k, planes = n_frames; L < ds->n; L += k, planes >>= k) {
            k = std::min<uint32_t>(ds->n - L, maxk);
            aqz::LevelOut o[aqz::kMaxFusedLevels];
            aqz::TiledOut t[aqz::kMaxFusedLevels];
            fill_outs(ds, L, k, [](uint32_t) { return nullptr; }, o);
            tiled_outs(L, k, none, t);
            if (L + k < ds->n)
                o[k - 1].ptr = stand_in;
            const Level& a = ds->lv[L - 1];
            if (!aqz::volume_supported(ds->dtype, src, a.desc.width, a.desc.height, o, int(k)))
                return ds->fail_arg(w + ": level " + std::to_string(L - 1) +
                                    " does not fit the fused volume kernel (" +
                                    std::to_string(a.desc.width) +
                                    " px wide: narrower than one vector load, or a misaligned "
                                    "buffer)");
            if (!aqz::plan_volume_tiled(ds->dtype, ds->method, src, a.elems(), a.desc.width,
                                        a.desc.height, o, t, int(k), planes,
                                        aqz::launch_switches())
                   .valid)
                return ds->fail_arg(w + ": levels " + std::to_string(L) + ".." +
                                    std::to_string(L + k - 1) +
                                    ": misaligned output, or units, padded sides or zero-fill "
                                    "items past the launch limits");
            src = stand_in;
        }
    }
    if (int rc = bind_device(ds))
        return rc;
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ds->stream;
    std::vector<const uint64_t*> d_off;
    int half = -1;
    if (lat) {
        std::vector<uint32_t> per_level(ds->n);
        for (uint32_t l = 0; l < ds->n; ++l)
            per_level[l] = n_frames >> l;
        if (int rc = stage_lattice(ds, lat, n_frames, stream, &d_off, &half, per_level.data()))
            return rc;
    }
    // as in run_tiled: the staged half's event on every way out
    struct LatticeGuard
    {
        aqz_ds* ds;
        int half;
        hipStream_t stream;
        ~LatticeGuard()
        {
            if (half >= 0)
                (void)hipEventRecord(ds->lattice_done[half], stream);
        }
    } lattice_guard{ ds, half, stream };
    // A run that feeds another also writes its last level row-major into one
    // half of d_chain (alternating), ordered behind the handle's previous deep
    // batch by chain_done — run_tiled's scheme.  The first chained level is
    // the largest.
    if (chained) {
        if (ds->chain_done)
            HIP_TRY(ds, hipStreamWaitEvent(stream, ds->chain_done, 0), "hipStreamWaitEvent chain");
        else
            HIP_TRY(ds, ds->chain_done.create(), "event");
    }
    struct ChainGuard
    {
        aqz_ds* ds;
        hipStream_t stream;
        bool on;
        ~ChainGuard()
        {
            if (on)
                (void)hipEventRecord(ds->chain_done, stream);
        }
    } chain_guard{ ds, stream, chained };
    if (chained) {
        const size_t chain_half = size_t(n_frames >> maxk) * ds->lv[maxk].bytes;
        if (ds->d_chain.capacity() < 2 * chain_half) {
            HIP_TRY(ds, hipStreamSynchronize(stream), "hipStreamSynchronize");
            HIP_TRY(ds, ds->d_chain.reserve(2 * chain_half), "hipMalloc chain");
        }
    }
    const void* src = device_frames;
    uint32_t planes = n_frames;
    for (uint32_t L = 1, run = 0; L < ds->n; ++run) {
        const uint32_t k = std::min<uint32_t>(ds->n - L, maxk);
        const bool feeds = L + k < ds->n;
        aqz::LevelOut o[aqz::kMaxFusedLevels];
        aqz::TiledOut t[aqz::kMaxFusedLevels];
        fill_outs(ds, L, k, [](uint32_t) { return nullptr; }, o);
        tiled_outs(L, k, d_off, t);
        void* chain = ds->d_chain.bytes() + (run & 1) * (ds->d_chain.capacity() / 2);
        if (feeds)
            o[k - 1].ptr = chain;
        const Level& a = ds->lv[L - 1];
        const hipError_t e =
          aqz::launch_volume_tiled(ds->dtype, ds->method, src, a.elems(), a.desc.width,
                                   a.desc.height, o, t, int(k), planes, stream);
        if (e != hipSuccess)
            return e == hipErrorInvalidValue ? ds->fail_arg(w + ": unsupported geometry")
                                             : ds->fail(e, "batch tiled volume");
        src = chain;
        planes >>= k;
        L += k;
    }
    for (uint32_t l = 0; l < ds->n; ++l) {
        ds->lv[l].count += n_frames >> l;
        if (out_counts)
            out_counts[l] = n_frames >> l;
    }
    ds->last_batch_kind = 5;
    return AQZ_OK;
}

// The handle's pyramid as plan_pyramid_runs reads it.
std::vector<aqz::PyramidLevel>
pyramid_levels(const aqz_ds* ds)
{
    std::vector<aqz::PyramidLevel> pl(ds->n);
    for (uint32_t l = 0; l < ds->n; ++l) {
        const Level& lv = ds->lv[l];
        pl[l] = { lv.desc.width, lv.desc.height, lv.desc.planes, l > 0 && lv.has_partial };
    }
    return pl;
}

// aqz_ds_run_device_mixed_tiled (lat == nullptr) and
// aqz_ds_run_device_mixed_chunked: run_tiled's two forms for the pyramids
// aqz_ds_run_device_batch runs as kind 7 — plan_pyramid_runs' runs, each
// through its tiled launcher (launch_volume_tiled, launch_cascade_tiled,
// launch_zrun_tiled), chained through d_chain.  Level l emits
// n_frames >> zcount(l) frames.  All or nothing: every run is planned before
// anything is queued, and there is no per-frame form to fall back to.
int
run_mixed_tiled(aqz_ds* ds,
                const char* who,
                const void* device_frames,
                uint32_t n_frames,
                const uint32_t* tile_rows,
                const uint32_t* tile_cols,
                void* const* device_out_levels,
                const aqz_chunk_lattice* lat,
                uint8_t* const* device_tile_nonzero,
                uint32_t* out_counts,
                void* hip_stream)
{
    const std::string w(who);
    if (int rc = settle(ds))
        return rc;
    if (ds->transpose)
        return ds->fail_arg(w + ": input transposition applies to the per-frame path only");
    ds->last_input = nullptr;
    if (!device_frames || (!lat && (!device_out_levels || !tile_rows || !tile_cols)))
        return ds->fail_arg(w + ": null argument");
    if (ds->n < 2)
        return ds->fail_arg(w + ": the pyramid has no level to tile");
    const std::vector<aqz::PyramidLevel> pl = pyramid_levels(ds);
    const aqz::PyramidRuns mixed = aqz::plan_pyramid_runs(pl.data(), ds->n, n_frames);
    if (!mixed.ok)
        return ds->fail_arg(w + ": " + mixed.reason);
    // frames each level emits: n_frames >> zcount(l)
    std::vector<uint32_t> emits(ds->n);
    for (uint32_t l = 0, frames = n_frames; l < ds->n; ++l) {
        if (l > 0 && pl[l].planes < pl[l - 1].planes)
            frames >>= 1;
        emits[l] = frames;
    }
    for (uint32_t l = 1; l < ds->n; ++l) {
        const uint32_t tr = lat ? lat[l].tile_rows : tile_rows[l];
        const uint32_t tc = lat ? lat[l].tile_cols : tile_cols[l];
        const void* out = lat ? lat[l].device_base : device_out_levels[l];
        if (!out || !tr || !tc)
            return ds->fail_arg(w + ": level " + std::to_string(l) +
                                " needs an output and a nonzero tile shape");
        if (lat) {
            // run_tiled's lattice checks over the level's own frame count
            const aqz_chunk_lattice& c = lat[l];
            const uint64_t ntiles = uint64_t((ds->lv[l].desc.width + tc - 1) / tc) *
                                    ((ds->lv[l].desc.height + tr - 1) / tr);
            const uint64_t tile_bytes = uint64_t(tr) * tc * ds->bpp;
            if (!c.frame_offset_bytes || c.chunk_stride_bytes % ds->bpp ||
                c.chunk_stride_bytes < tile_bytes)
                return ds->fail_arg(w + ": level " + std::to_string(l) +
                                    ": chunk stride must hold a tile and be a multiple of the "
                                    "pixel size, and frame offsets are required");
            const uint64_t extent = (ntiles - 1) * c.chunk_stride_bytes + tile_bytes;
            for (uint32_t k = 0; k < emits[l]; ++k) {
                const uint64_t off = c.frame_offset_bytes[k];
                if (off % ds->bpp || off > c.capacity_bytes || c.capacity_bytes - off < extent)
                    return ds->fail_arg(w + ": level " + std::to_string(l) + " frame " +
                                        std::to_string(k) + ": offset " + std::to_string(off) +
                                        " puts its tiles outside the lattice buffer");
            }
        }
    }
    const auto tiled_outs = [&](uint32_t L, uint32_t k, const std::vector<const uint64_t*>& off,
                                aqz::TiledOut* t) {
        for (uint32_t j = 0; j < k; ++j) {
            const uint32_t l = L + j;
            uint8_t* nz = device_tile_nonzero ? device_tile_nonzero[l] : nullptr;
            if (lat)
                t[j] = { lat[l].device_base, lat[l].tile_rows, lat[l].tile_cols, nz,
                         off.empty() ? lat[l].frame_offset_bytes : off[l],
                         lat[l].chunk_stride_bytes / ds->bpp };
            else
                t[j] = { device_out_levels[l], tile_rows[l], tile_cols[l], nz };
        }
    };
    // One run through its tiled launcher, or (`queue` false) its plan alone.
    // The plans look at addresses and sizes only, so a stand-in for the chain
    // scratch (aligned, like the allocation) and the offsets' host copy serve
    // there.
    const size_t n_runs = mixed.runs.size();
    const auto do_run = [&](size_t i, const void* src, void* feed,
                            const std::vector<const uint64_t*>& off, bool queue,
                            hipStream_t stream, std::string* why) -> hipError_t {
        const aqz::PyramidRun& r = mixed.runs[i];
        const int k = int(r.levels);
        aqz::LevelOut o[aqz::kMaxFusedLevels];
        aqz::TiledOut t[aqz::kMaxFusedLevels];
        fill_outs(ds, r.first, r.levels, [](uint32_t) { return nullptr; }, o);
        tiled_outs(r.first, r.levels, off, t);
        if (i + 1 < n_runs)
            o[k - 1].ptr = feed;
        const Level& a = ds->lv[r.first - 1];
        const uint32_t W = a.desc.width, H = a.desc.height;
        const std::string levels = "levels " + std::to_string(r.first) + ".." +
                                   std::to_string(r.first + r.levels - 1);
        const char* limits = ": misaligned output, or units, padded sides or zero-fill items "
                             "past the launch limits";
        if (r.cls == aqz::kClassXYZ) {
            if (queue)
                return aqz::launch_volume_tiled(ds->dtype, ds->method, src, a.elems(), W, H, o, t,
                                                k, r.frames_in, stream);
            if (!aqz::volume_supported(ds->dtype, src, W, H, o, k))
                *why = "level " + std::to_string(r.first - 1) +
                       " does not fit the fused volume kernel (" + std::to_string(W) +
                       " px wide: narrower than one vector load, or a misaligned buffer)";
            else if (!aqz::plan_volume_tiled(ds->dtype, ds->method, src, a.elems(), W, H, o, t, k,
                                             r.frames_in, aqz::launch_switches())
                        .valid)
                *why = levels + limits;
        } else if (r.cls == aqz::kClassXY) {
            if (queue)
                return aqz::launch_cascade_tiled(ds->dtype, ds->method, src, a.elems(), W, H, o, t,
                                                 k, r.frames_in, stream);
            if (!aqz::cascade_supported(ds->dtype, src, a.elems(), W, H, o, k))
                *why = "level " + std::to_string(r.first - 1) +
                       " is narrower than one vector load (" + std::to_string(W) +
                       " px) or misaligned";
            else if (!aqz::plan_cascade_tiled(ds->dtype, ds->method, src, a.elems(), W, H, o, t, k,
                                              r.frames_in, aqz::launch_switches())
                        .valid)
                *why = levels + limits;
        } else {
            if (queue)
                return aqz::launch_zrun_tiled(ds->dtype, ds->method, src, a.elems(), W, H, o, t, k,
                                              r.frames_in, stream);
            bool same = true;
            for (int j = 0; j < k; ++j)
                same = same && o[j].w == W && o[j].h == H;
            if (!same)
                *why = levels + " do not keep level " + std::to_string(r.first - 1) + "'s size";
            else if (!aqz::plan_zrun_tiled(ds->dtype, ds->method, src, a.elems(), W, H, o, t, k,
                                           r.frames_in)
                        .valid)
                *why = levels + limits;
        }
        return hipSuccess;
    };
    {
        void* const stand_in = reinterpret_cast<void*>(uintptr_t(256));
        const std::vector<const uint64_t*> none;
        for (size_t i = 0; i < n_runs; ++i) {
            std::string why;
            (void)do_run(i, i == 0 ? device_frames : stand_in, stand_in, none, false, nullptr,
                         &why);
            if (!why.empty())
                return ds->fail_arg(w + ": " + why);
        }
    }
    if (int rc = bind_device(ds))
        return rc;
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ds->stream;
    std::vector<const uint64_t*> d_off;
    int half = -1;
    if (lat)
        if (int rc = stage_lattice(ds, lat, n_frames, stream, &d_off, &half, emits.data()))
            return rc;
    // as in run_tiled: the staged half's event on every way out
    struct LatticeGuard
    {
        aqz_ds* ds;
        int half;
        hipStream_t stream;
        ~LatticeGuard()
        {
            if (half >= 0)
                (void)hipEventRecord(ds->lattice_done[half], stream);
        }
    } lattice_guard{ ds, half, stream };
    // A run that feeds another also writes its last level row-major into one
    // half of d_chain (alternating by run parity), ordered behind the handle's
    // previous deep batch by chain_done — run_tiled's scheme.  A half holds
    // the largest level a run feeds.
    const bool chained = n_runs > 1;
    if (chained) {
        if (ds->chain_done)
            HIP_TRY(ds, hipStreamWaitEvent(stream, ds->chain_done, 0), "hipStreamWaitEvent chain");
        else
            HIP_TRY(ds, ds->chain_done.create(), "event");
    }
    struct ChainGuard
    {
        aqz_ds* ds;
        hipStream_t stream;
        bool on;
        ~ChainGuard()
        {
            if (on)
                (void)hipEventRecord(ds->chain_done, stream);
        }
    } chain_guard{ ds, stream, chained };
    if (chained) {
        size_t chain_half = 0;
        for (size_t i = 0; i + 1 < n_runs; ++i) {
            const uint32_t last = mixed.runs[i].first + mixed.runs[i].levels - 1;
            chain_half = std::max(chain_half, size_t(emits[last]) * ds->lv[last].bytes);
        }
        chain_half = (chain_half + 255) & ~size_t(255);
        if (ds->d_chain.capacity() < 2 * chain_half) {
            HIP_TRY(ds, hipStreamSynchronize(stream), "hipStreamSynchronize");
            HIP_TRY(ds, ds->d_chain.reserve(2 * chain_half), "hipMalloc chain");
        }
    }
    const void* src = device_frames;
    for (size_t i = 0; i < n_runs; ++i) {
        void* chain = ds->d_chain.bytes() + (i & 1) * (ds->d_chain.capacity() / 2);
        const hipError_t e = do_run(i, src, chain, d_off, true, stream, nullptr);
        if (e != hipSuccess)
            return e == hipErrorInvalidValue ? ds->fail_arg(w + ": unsupported geometry")
                                             : ds->fail(e, "batch tiled mixed runs");
        src = chain;
    }
    for (uint32_t l = 0; l < ds->n; ++l) {
        ds->lv[l].count += emits[l];
        if (out_counts)
            out_counts[l] = emits[l];
    }
    ds->last_batch_kind = 8;
    return AQZ_OK;
}

} // namespace

extern "C" {

int
aqz_ds_run_device_batch_tiled(aqz_ds* ds,
                              const void* device_frames,
                              uint32_t n_frames,
                              const uint32_t* tile_rows,
                              const uint32_t* tile_cols,
                              void* const* device_out_levels,
                              uint8_t* const* device_tile_nonzero,
                              uint32_t* out_counts,
                              void* hip_stream)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        return run_tiled(ds, "run_device_batch_tiled", device_frames, n_frames, tile_rows,
                         tile_cols, device_out_levels, nullptr, device_tile_nonzero, out_counts,
                         hip_stream);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_run_device_batch_chunked(aqz_ds* ds,
                                const void* device_frames,
                                uint32_t n_frames,
                                const aqz_chunk_lattice* lattices,
                                uint8_t* const* device_tile_nonzero,
                                uint32_t* out_counts,
                                void* hip_stream)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (!lattices)
            return ds->fail_arg("run_device_batch_chunked: null lattices");
        return run_tiled(ds, "run_device_batch_chunked", device_frames, n_frames, nullptr,
                         nullptr, nullptr, lattices, device_tile_nonzero, out_counts, hip_stream);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_run_device_batch_tiled_base(aqz_ds* ds,
                                   const void* device_frames,
                                   uint32_t n_frames,
                                   const uint32_t* tile_rows,
                                   const uint32_t* tile_cols,
                                   void* const* device_out_levels,
                                   uint8_t* const* device_tile_nonzero,
                                   uint32_t* out_counts,
                                   void* hip_stream)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        return run_tiled(ds, "run_device_batch_tiled_base", device_frames, n_frames, tile_rows,
                         tile_cols, device_out_levels, nullptr, device_tile_nonzero, out_counts,
                         hip_stream, true);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_run_device_batch_chunked_base(aqz_ds* ds,
                                     const void* device_frames,
                                     uint32_t n_frames,
                                     const aqz_chunk_lattice* lattices,
                                     uint8_t* const* device_tile_nonzero,
                                     uint32_t* out_counts,
                                     void* hip_stream)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (!lattices)
            return ds->fail_arg("run_device_batch_chunked_base: null lattices");
        return run_tiled(ds, "run_device_batch_chunked_base", device_frames, n_frames, nullptr,
                         nullptr, nullptr, lattices, device_tile_nonzero, out_counts, hip_stream,
                         true);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

uint32_t
aqz_ds_tiled_base_flag_slots(const aqz_ds* ds, uint32_t tile_rows, uint32_t tile_cols)
{
    if (!ds || ds->n < 2 || tile_rows == 0 || tile_cols == 0)
        return 0;
    // level 0 leaves with the first fused run: levels 1 .. min(n - 1, 4)
    const uint32_t k = std::min<uint32_t>(ds->n - 1, aqz::kMaxFusedLevels);
    const uint32_t s = aqz::cascade_tiled_base_slots(ds->dtype, ds->lv[0].desc.width, int(k),
                                                     tile_rows, tile_cols, nullptr);
    return s ? s : 1;
}

int
aqz_ds_run_device_volume_tiled(aqz_ds* ds,
                               const void* device_frames,
                               uint32_t n_frames,
                               const uint32_t* tile_rows,
                               const uint32_t* tile_cols,
                               void* const* device_out_levels,
                               uint8_t* const* device_tile_nonzero,
                               uint32_t* out_counts,
                               void* hip_stream)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        return run_volume_tiled(ds, "run_device_volume_tiled", device_frames, n_frames, tile_rows,
                                tile_cols, device_out_levels, nullptr, device_tile_nonzero,
                                out_counts, hip_stream);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_run_device_volume_chunked(aqz_ds* ds,
                                 const void* device_frames,
                                 uint32_t n_frames,
                                 const aqz_chunk_lattice* lattices,
                                 uint8_t* const* device_tile_nonzero,
                                 uint32_t* out_counts,
                                 void* hip_stream)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (!lattices)
            return ds->fail_arg("run_device_volume_chunked: null lattices");
        return run_volume_tiled(ds, "run_device_volume_chunked", device_frames, n_frames, nullptr,
                                nullptr, nullptr, lattices, device_tile_nonzero, out_counts,
                                hip_stream);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

uint32_t
aqz_ds_tiled_flag_slots(const aqz_ds* ds, uint32_t level, uint32_t tile_rows, uint32_t tile_cols)
{
    if (!ds || level == 0 || level >= ds->n || tile_rows == 0 || tile_cols == 0)
        return 0;
    // the fused run holding `level`: levels 1-4, 5-8, ... (kMaxFusedLevels)
    const uint32_t start = 1 + ((level - 1) / aqz::kMaxFusedLevels) * aqz::kMaxFusedLevels;
    const uint32_t k = std::min<uint32_t>(ds->n - start, aqz::kMaxFusedLevels);
    const uint32_t s = aqz::cascade_tiled_slots(ds->dtype, ds->lv[start - 1].desc.width, int(k),
                                                int(level - start + 1), tile_rows, tile_cols,
                                                nullptr);
    return s ? s : 1;
}

int
aqz_ds_run_device_mixed_tiled(aqz_ds* ds,
                              const void* device_frames,
                              uint32_t n_frames,
                              const uint32_t* tile_rows,
                              const uint32_t* tile_cols,
                              void* const* device_out_levels,
                              uint8_t* const* device_tile_nonzero,
                              uint32_t* out_counts,
                              void* hip_stream)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        return run_mixed_tiled(ds, "run_device_mixed_tiled", device_frames, n_frames, tile_rows,
                               tile_cols, device_out_levels, nullptr, device_tile_nonzero,
                               out_counts, hip_stream);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_run_device_mixed_chunked(aqz_ds* ds,
                                const void* device_frames,
                                uint32_t n_frames,
                                const aqz_chunk_lattice* lattices,
                                uint8_t* const* device_tile_nonzero,
                                uint32_t* out_counts,
                                void* hip_stream)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (!lattices)
            return ds->fail_arg("run_device_mixed_chunked: null lattices");
        return run_mixed_tiled(ds, "run_device_mixed_chunked", device_frames, n_frames, nullptr,
                               nullptr, nullptr, lattices, device_tile_nonzero, out_counts,
                               hip_stream);
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

uint32_t
aqz_ds_mixed_flag_slots(const aqz_ds* ds, uint32_t level, uint32_t tile_rows, uint32_t tile_cols)
{
    try {
        if (!ds || level == 0 || level >= ds->n || tile_rows == 0 || tile_cols == 0)
            return 0;
        // the run cut does not depend on the batch: any accepted frame count
        // gives it, and a plane some level holds now is the call's to refuse
        std::vector<aqz::PyramidLevel> pl = pyramid_levels(ds);
        uint32_t zcount = 0;
        for (uint32_t l = 1; l < ds->n; ++l) {
            pl[l].holds_plane = false;
            zcount += pl[l].planes < pl[l - 1].planes ? 1 : 0;
        }
        if (zcount >= 32)
            return 0;
        const aqz::PyramidRuns mixed = aqz::plan_pyramid_runs(pl.data(), ds->n, 1u << zcount);
        if (!mixed.ok)
            return 0;
        for (const aqz::PyramidRun& r : mixed.runs) {
            if (level < r.first || level >= r.first + r.levels)
                continue;
            if (r.cls != aqz::kClassXY)
                return 1;
            const uint32_t s =
              aqz::cascade_tiled_slots(ds->dtype, ds->lv[r.first - 1].desc.width, int(r.levels),
                                       int(level - r.first + 1), tile_rows, tile_cols, nullptr);
            return s ? s : 1;
        }
        return 0;
    } catch (...) {
        return 0;
    }
}

namespace {

// Frames per pipeline group: about 64 MiB of input per group, and a whole
// number of plane groups when the pyramid pairs planes (so fused volume
// launches see aligned groups).
uint32_t
pipe_group(const aqz_ds* ds, uint32_t n_frames)
{
    uint32_t g = uint32_t(std::max<size_t>(1, (size_t(64) << 20) / ds->lv[0].bytes));
    uint32_t align = 1;
    for (uint32_t l = 1; l < ds->n; ++l)
        if (ds->lv[l].zh)
            align <<= 1;
    g = std::max(align, (g / align) * align);
    return std::min(g, std::max(align, n_frames));
}

int
ensure_pipe(aqz_ds* ds, uint32_t group)
{
    auto& p = ds->pipe;
    if (p.group >= group)
        return AQZ_OK;
    // the buffers hold `group` frames only once every one of them is there:
    // a failed growth is followed by a fresh attempt
    p.group = 0;
    for (int b = 0; b < 2; ++b) {
        // all of the old buffers go before any new one is made
        p.d_in[b].reset();
        p.d_out[b].clear();
        p.d_out[b].resize(ds->n);
    }
    if (!p.s_in) {
        HIP_TRY(ds, p.s_in.create(), "stream");
        HIP_TRY(ds, p.s_work.create(), "stream");
        HIP_TRY(ds, p.s_out.create(), "stream");
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(ds, p.in_done[b].create(), "event");
            HIP_TRY(ds, p.work_done[b].create(), "event");
            HIP_TRY(ds, p.out_done[b].create(), "event");
            // start "done" so the first waits pass
            HIP_TRY(ds, hipEventRecord(p.work_done[b], p.s_work), "event");
            HIP_TRY(ds, hipEventRecord(p.out_done[b], p.s_out), "event");
        }
    }
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(ds, p.d_in[b].reserve(size_t(group) * ds->lv[0].bytes), "hipMalloc pipe");
        for (uint32_t l = 1; l < ds->n; ++l)
            HIP_TRY(ds, p.d_out[b][l].reserve(size_t(group) * ds->lv[l].bytes),
                    "hipMalloc pipe");
    }
    p.group = group;
    return AQZ_OK;
}

} // namespace

int
aqz_ds_run_host_batch(aqz_ds* ds,
                      const void* host_frames,
                      uint32_t n_frames,
                      void* const* host_out_levels,
                      uint32_t* out_counts)
{
    try {
        if (!ds)
            return AQZ_INVALID_ARGUMENT;
        if (int rc = settle(ds))
            return rc;
        if (ds->transpose)
            return ds->fail_arg("ds_run_host_batch: input transposition applies to the per-frame path "
                                "(add_frame / add_device_frame) only");
        ds->last_input = nullptr;
        if (!host_frames || !host_out_levels)
            return ds->fail_arg("run_host_batch: null buffer");
        for (uint32_t l = 1; l < ds->n; ++l)
            if (!host_out_levels[l])
                return ds->fail_arg("run_host_batch: null output for level " +
                                    std::to_string(l));
        if (int rc = bind_device(ds))
            return rc;
        const uint32_t group = pipe_group(ds, n_frames);
        if (int rc = ensure_pipe(ds, group))
            return rc;
        auto& p = ds->pipe;
        std::vector<uint32_t> total(ds->n, 0);
        const uint8_t* src = static_cast<const uint8_t*>(host_frames);
        int rc = AQZ_OK;
        uint32_t k = 0;
        // Any failure below still drains all three streams before returning, so
        // no copy is left reading or writing the caller's buffers.
        auto drain = [&](int code) {
            (void)hipStreamSynchronize(p.s_in);
            (void)hipStreamSynchronize(p.s_work);
            (void)hipStreamSynchronize(p.s_out);
            return code;
        };
    #define HIP_TRY_DRAIN(ds, expr, what)                                          \
        do {                                                                       \
            hipError_t e_ = (expr);                                                \
            if (e_ != hipSuccess)                                                  \
                return drain((ds)->fail(e_, what));                                \
        } while (0)
        for (uint32_t f0 = 0; f0 < n_frames && rc == AQZ_OK; f0 += group, ++k) {
            const int b = int(k & 1);
            const uint32_t g = std::min(group, n_frames - f0);
            // upload: buffer b is free once group k-2's kernels are done with it
            HIP_TRY_DRAIN(ds, hipStreamWaitEvent(p.s_in, p.work_done[b], 0), "wait");
            HIP_TRY_DRAIN(ds,
                    hipMemcpyAsync(p.d_in[b].get(), src + size_t(f0) * ds->lv[0].bytes,
                                   size_t(g) * ds->lv[0].bytes, hipMemcpyHostToDevice,
                                   p.s_in),
                    "hipMemcpyAsync H2D");
            HIP_TRY_DRAIN(ds, hipEventRecord(p.in_done[b], p.s_in), "event");
            // kernels: after the upload, and after group k-2's download of d_out[b]
            HIP_TRY_DRAIN(ds, hipStreamWaitEvent(p.s_work, p.in_done[b], 0), "wait");
            HIP_TRY_DRAIN(ds, hipStreamWaitEvent(p.s_work, p.out_done[b], 0), "wait");
            std::vector<uint32_t> counts(ds->n, 0);
            std::vector<void*> d_out(ds->n);
            for (uint32_t l = 1; l < ds->n; ++l)
                d_out[l] = p.d_out[b][l].get();
            rc = aqz_ds_run_device_batch(ds, p.d_in[b].get(), g, d_out.data(), counts.data(),
                                         p.s_work);
            if (rc)
                return drain(rc);
            HIP_TRY_DRAIN(ds, hipEventRecord(p.work_done[b], p.s_work), "event");
            // download every frame this group emitted, appended per level
            HIP_TRY_DRAIN(ds, hipStreamWaitEvent(p.s_out, p.work_done[b], 0), "wait");
            for (uint32_t l = 1; l < ds->n; ++l) {
                if (!counts[l])
                    continue;
                uint8_t* dst = static_cast<uint8_t*>(host_out_levels[l]) +
                               size_t(total[l]) * ds->lv[l].bytes;
                HIP_TRY_DRAIN(ds,
                        hipMemcpyAsync(dst, d_out[l], size_t(counts[l]) * ds->lv[l].bytes,
                                       hipMemcpyDeviceToHost, p.s_out),
                        "hipMemcpyAsync D2H");
                total[l] += counts[l];
            }
            HIP_TRY_DRAIN(ds, hipEventRecord(p.out_done[b], p.s_out), "event");
        }
        drain(AQZ_OK);
        total[0] = n_frames;
        if (out_counts)
            std::copy(total.begin(), total.end(), out_counts);
        return rc;
    #undef HIP_TRY_DRAIN
    } catch (...) {
        return ABI_GUARD_FAIL(ds);
    }
}

int
aqz_ds_last_batch_kind(const aqz_ds* ds)
{
    return ds ? ds->last_batch_kind : -1;
}

int
aqz_debug_ds_force_per_frame_batch(aqz_ds* ds, int on)
{
    if (!ds)
        return AQZ_INVALID_ARGUMENT;
    ds->force_per_frame = on != 0;
    return AQZ_OK;
}

uint64_t
aqz_ds_stream_tiled_runs(const aqz_ds* ds)
{
    return ds ? ds->stream_tiled_runs : 0;
}

size_t
aqz_ds_level_bytes(const aqz_ds* ds, uint32_t level)
{
    return (ds && level < ds->n) ? ds->lv[level].bytes : 0;
}

uint32_t
aqz_ds_level_count(const aqz_ds* ds)
{
    return ds ? ds->n : 0;
}

int
aqz_ds_device(const aqz_ds* ds)
{
    return ds ? ds->device : -1;
}

size_t
aqz_ds_device_memory_usage(const aqz_ds* ds)
{
    return ds ? ds->device_bytes : 0;
}

const char*
aqz_ds_last_error(const aqz_ds* ds)
{
    return ds ? ds->err.c_str() : "null handle";
}

const char*
aqz_last_error(void)
{
    return g_last_error.c_str();
}

const char*
aqz_method_name(int method)
{
    // Downsampler::downsampling_method, downsampler.cpp:422-437
    switch (method) {
        case AQZ_METHOD_DECIMATE:
            return "decimate";
        case AQZ_METHOD_MEAN:
            return "local_mean";
        case AQZ_METHOD_MIN:
            return "local_min";
        case AQZ_METHOD_MAX:
            return "local_max";
        default:
            return nullptr;
    }
}

const char*
aqz_method_metadata_json(int method)
{
    // Downsampler::get_metadata, downsampler.cpp:440-485: the OME
    // `multiscales[0].metadata` object (nlohmann::json serialises keys in
    // sorted order).
    switch (method) {
        case AQZ_METHOD_MEAN:
            return "{\"description\":\"The fields in the metadata describe how "
                   "to reproduce this multiscaling in scikit-image. The method "
                   "and its parameters are given here.\",\"kwargs\":{\"cval\":"
                   "\"0\",\"factors\":\"(2, 2)\"},\"method\":\"skimage."
                   "transform.downscale_local_mean\",\"version\":\"0.25.2\"}";
        case AQZ_METHOD_DECIMATE:
            return "{\"args\":[\"(slice(0, None, 2), slice(0, None, 2))\"],"
                   "\"description\":\"Subsampling by taking every 2nd "
                   "pixel/voxel (top-left corner of each 2x2 block). "
                   "Equivalent to numpy array slicing with stride 2.\","
                   "\"method\":\"np.ndarray.__getitem__\",\"version\":"
                   "\"2.2.6\"}";
        case AQZ_METHOD_MIN:
            return "{\"description\":\"Minimum pooling over 2x2 blocks. "
                   "Equivalent to reshaping into blocks and taking numpy.min "
                   "along block dimensions.\",\"kwargs\":{\"func\":\"np.min\"},"
                   "\"method\":\"skimage.measure.block_reduce\",\"version\":"
                   "\"0.25.2\"}";
        case AQZ_METHOD_MAX:
            return "{\"description\":\"Maximum pooling over 2x2 blocks. "
                   "Equivalent to reshaping into blocks and taking numpy.max "
                   "along block dimensions.\",\"kwargs\":{\"func\":\"np.max\"},"
                   "\"method\":\"skimage.measure.block_reduce\",\"version\":"
                   "\"0.25.2\"}";
        default:
            return nullptr;
    }
}

const char*
aqz_version(void)
{
    // AQZ_BUILD_ID: the source revision and time the Makefile built this
    // library from, so a bench line names the binary it ran
#ifndef AQZ_BUILD_ID
#define AQZ_BUILD_ID "unknown build"
#endif
    return "aqz-mi355x 0.2.0 (gfx950; " AQZ_BUILD_ID ")";
}

} // extern "C"

namespace aqz {

// aqz_last_error() text for the other C-ABI translation units
// (codec_runtime.cpp)
void
set_last_error(const std::string& msg)
{
    g_last_error = msg;
}

} // namespace aqz
