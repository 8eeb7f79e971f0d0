// gather_kernels.hh — launcher of the chunk -> frame gather (gather_kernels.hip;
// C ABI in include/aqz_shard.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace aqz {

// frames of one gather launch: their chunk bases and internal offsets are
// kernel arguments (768 bytes), like kShardFlagFrames' bases
constexpr uint32_t kGatherFrames = 64;
// destination bytes one workgroup of the vector form owns, rounded up to whole
// frame rows: two rounds of 8 vectors a lane
constexpr uint32_t kGatherBandBytes = 64u << 10;

struct GatherArgs
{
    const uint8_t* chunks;
    uint64_t chunk_stride;
    const uint32_t* slot; // or null: chunk c lies in slot c
    uint32_t n_slots;
    uint32_t bpp_log2;
    uint32_t W, H, tile_rows, tile_cols, n_tiles_x;
    uint8_t* frames;
    uint64_t frame_stride;
    uint32_t* bad_slot; // or null
};

// 0: the element form, 1: the 16-byte vector form (a tile row holds at least
// one vector and a frame row is shorter than 2^31 bytes)
int gather_form(uint32_t width, uint32_t tile_cols, uint32_t bpp_log2);

// Frame k of n_frames from chunks host_base[k] + t at host_internal[k].  The
// caller has checked every extent and table entry; hipErrorInvalidValue when a
// launch's grid reaches 2^31 workgroups, before anything is queued.
hipError_t launch_chunk_gather(const GatherArgs& a, const uint32_t* host_base,
                               const uint64_t* host_internal, uint32_t n_frames,
                               hipStream_t stream);

} // namespace aqz
