// ds_dispatch.cpp — the host entry of every launcher of ds_kernels.hh.
//
// launch_cascade, launch_cascade_tiled, launch_volume and launch_volume_tiled
// plan here
// (ds_plan.hh: the process-wide switches, the device's LDS cap), record the
// plan's line in the launch log and hand the plan to run_cascade,
// run_cascade_tiled, run_volume or run_volume_tiled of the dtype's kernel
// shard; the other launchers are routed as they are.
//
// ds_kernels.hip is compiled AQZ_SHARDS times (acquire-zarr_amd/Makefile);
// shard k holds the kernels of the dtypes whose code % AQZ_SHARDS == k and
// names its launchers <launcher>_shard<k>.  This file is compiled once.  A
// tools/ probe includes it after ds_kernels.hip, unsharded: the planned
// launchers then call the one set of run_* functions.
#include "ds_kernels.hh"

#ifndef AQZ_SHARDS
#error "ds_dispatch.cpp is built with -DAQZ_SHARDS=<n> (acquire-zarr_amd/Makefile)"
#endif
#if AQZ_SHARDS != 8 && AQZ_SHARDS != 1
#error "ds_dispatch.cpp routes to exactly 8 shards"
#endif
#if AQZ_SHARDS > 1
#include "launch_log.hh"
#endif

namespace aqz {

#if AQZ_SHARDS > 1
#define AQZ_SHARD_FNS(name)                                                    \
    name##_shard0, name##_shard1, name##_shard2, name##_shard3, name##_shard4, \
      name##_shard5, name##_shard6, name##_shard7

#define AQZ_DECLARE_SHARDS(name, params)                                       \
    using name##_fn = hipError_t params;                                       \
    name##_fn AQZ_SHARD_FNS(name);

#define AQZ_ROUTE(name, dtype, args)                                           \
    do {                                                                       \
        static constexpr decltype(&name##_shard0) shard[] = { AQZ_SHARD_FNS(name) }; \
        if (!dtype_valid(dtype))                                               \
            return hipErrorInvalidValue;                                       \
        return shard[(dtype) % AQZ_SHARDS] args;                               \
    } while (0)

AQZ_DECLARE_SHARDS(run_cascade,
                   (const CascadePlan&, const void*, uint64_t, uint32_t, uint32_t,
                    const LevelOut*, hipStream_t))
AQZ_DECLARE_SHARDS(run_cascade_tiled,
                   (const TiledPlan&, const void*, uint64_t, uint32_t, uint32_t, const LevelOut*,
                    const TiledOut*, const TiledOut*, hipStream_t))
AQZ_DECLARE_SHARDS(run_volume,
                   (const VolumePlan&, const void*, uint64_t, uint32_t, uint32_t,
                    const LevelOut*, hipStream_t))
AQZ_DECLARE_SHARDS(run_volume_tiled,
                   (const VolumeTiledPlan&, const void*, uint64_t, uint32_t, uint32_t,
                    const LevelOut*, const TiledOut*, hipStream_t))
#else
#define AQZ_ROUTE(name, dtype, args) return name args
#endif

namespace {

// LDS a band workgroup may use: the device's per-workgroup maximum (160 KiB
// on gfx950), 64 KiB if the query fails, less the band kernel's static
// arrival counter.  Asked once per process.
uint32_t
device_lds_cap()
{
    static const uint32_t cap = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) ==
              hipSuccess &&
            v > 16)
            return uint32_t(v) - 16u;
        return 65536u;
    }();
    return cap;
}

} // namespace

hipError_t
launch_cascade(int dtype, int method, const void* src, uint64_t src_frame_elems, uint32_t W,
               uint32_t H, const LevelOut* outs, int n_out, uint32_t n_frames, hipStream_t stream)
{
    const CascadePlan pl = plan_cascade(dtype, method, src, src_frame_elems, W, H, outs, n_out,
                                        n_frames, device_lds_cap(), launch_switches());
    if (!pl.valid)
        return hipErrorInvalidValue;
    if (launch_log_on())
        launch_log_record("%s", format_plan(pl).c_str());
    AQZ_ROUTE(run_cascade, dtype, (pl, src, src_frame_elems, W, H, outs, stream));
}

hipError_t
launch_cascade_tiled(int dtype, int method, const void* src, uint64_t src_frame_elems,
                     uint32_t W, uint32_t H, const LevelOut* outs, const TiledOut* touts,
                     int n_out, uint32_t n_frames, hipStream_t stream, const TiledOut* tbase)
{
    const TiledPlan pl = plan_cascade_tiled(dtype, method, src, src_frame_elems, W, H, outs,
                                            touts, n_out, n_frames, launch_switches(), tbase);
    if (!pl.valid)
        return hipErrorInvalidValue;
    if (launch_log_on())
        launch_log_record("%s", format_plan(pl).c_str());
    AQZ_ROUTE(run_cascade_tiled, dtype,
              (pl, src, src_frame_elems, W, H, outs, touts, tbase, stream));
}

hipError_t
launch_volume(int dtype, int method, const void* src, uint64_t src_frame_elems, uint32_t W,
              uint32_t H, const LevelOut* outs, int n_out, uint32_t n_planes, hipStream_t stream)
{
    const VolumePlan pl = plan_volume(dtype, method, src, src_frame_elems, W, H, outs, n_out,
                                      n_planes, launch_switches());
    if (!pl.valid)
        return hipErrorInvalidValue;
    if (launch_log_on())
        launch_log_record("%s", format_plan(pl).c_str());
    AQZ_ROUTE(run_volume, dtype, (pl, src, src_frame_elems, W, H, outs, stream));
}

hipError_t
launch_volume_tiled(int dtype, int method, const void* src, uint64_t src_frame_elems, uint32_t W,
                    uint32_t H, const LevelOut* outs, const TiledOut* touts, int n_out,
                    uint32_t n_planes, hipStream_t stream)
{
    const VolumeTiledPlan pl = plan_volume_tiled(dtype, method, src, src_frame_elems, W, H, outs,
                                                 touts, n_out, n_planes, launch_switches());
    if (!pl.valid)
        return hipErrorInvalidValue;
    if (launch_log_on())
        launch_log_record("%s", format_plan(pl).c_str());
    AQZ_ROUTE(run_volume_tiled, dtype, (pl, src, src_frame_elems, W, H, outs, touts, stream));
}

#if AQZ_SHARDS > 1
// The launchers that only route: each shard's has the launcher's own type.
#define AQZ_FORWARD(name, params, args)                                        \
    decltype(name) AQZ_SHARD_FNS(name);                                        \
    hipError_t name params { AQZ_ROUTE(name, dtype, args); }

AQZ_FORWARD(launch_xy_generic,
            (int dtype, int method, const void* src, uint64_t src_frame_elems, uint32_t w,
             uint32_t h, const LevelOut& out, uint32_t n_frames, hipStream_t stream),
            (dtype, method, src, src_frame_elems, w, h, out, n_frames, stream))
AQZ_FORWARD(launch_zpair,
            (int dtype, int method, void* out, const void* earlier, const void* current,
             uint64_t n, hipStream_t stream),
            (dtype, method, out, earlier, current, n, stream))
AQZ_FORWARD(launch_zrun,
            (int dtype, int method, const void* src, uint64_t src_frame_elems, uint64_t elems,
             const LevelOut* outs, int n_out, uint32_t planes, hipStream_t stream),
            (dtype, method, src, src_frame_elems, elems, outs, n_out, planes, stream))
AQZ_FORWARD(launch_zrun_tiled,
            (int dtype, int method, const void* src, uint64_t src_frame_elems, uint32_t W,
             uint32_t H, const LevelOut* outs, const TiledOut* touts, int n_out, uint32_t planes,
             hipStream_t stream),
            (dtype, method, src, src_frame_elems, W, H, outs, touts, n_out, planes, stream))
AQZ_FORWARD(launch_transpose,
            (int dtype, const void* src, uint32_t rows, uint32_t cols, void* dst,
             hipStream_t stream),
            (dtype, src, rows, cols, dst, stream))
AQZ_FORWARD(launch_tile_frame,
            (int dtype, const void* src, uint32_t W, uint32_t H, uint32_t tile_rows,
             uint32_t tile_cols, void* dst, uint32_t* nonzero, hipStream_t stream),
            (dtype, src, W, H, tile_rows, tile_cols, dst, nonzero, stream))
AQZ_FORWARD(launch_tile_frame_sliced,
            (int dtype, const void* src, uint32_t W, uint32_t H, uint32_t tile_rows,
             uint32_t tile_cols, void* dst, uint8_t* slice_flags, hipStream_t stream),
            (dtype, src, W, H, tile_rows, tile_cols, dst, slice_flags, stream))
#endif // AQZ_SHARDS > 1

} // namespace aqz
