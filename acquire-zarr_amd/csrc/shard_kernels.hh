// shard_kernels.hh — launchers of the Zarr v3 shard assembly kernels
// (shard_kernels.hip; C ABI in include/aqz_shard.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace aqz {

// The piece of a frame one pack workgroup copies, and the cache policy of its
// loads and stores: chosen by the A/B of tools/zarr_shard_bench.py
// (profiles/zarr_shard/bench.jsonl; ms per batch of >= 1 GiB
// read, median of 15, spread within 0.012 ms):
//   64 uncompressed 2 MiB chunks: 16 KiB nt 0.354, 64 KiB nt 0.370,
//     64 KiB plain 0.388, 256 KiB nt 0.388 (hipMemcpyDtoDAsync 0.397,
//     pack_frames_kernel 2.00);
//   256 LZ4 frames, compressible: 16 KiB nt 0.607, 64 KiB nt 0.579,
//     256 KiB nt 0.592 (plain 0.696 / 0.605 / 0.649; pack_frames_kernel 0.916).
// 16 KiB is the fastest on the large chunks but 0.028 ms slower than 64 KiB on
// the compressible frames, more than the spread: there about four in ten of a
// frame's 16 KiB workgroups find it ended and exit (the supposed cause; not
// profiled).  64 KiB is the best there and within 4 % on the large chunks.  Nontemporal is faster or equal at 16 and 64 KiB on
// every workload.
constexpr uint32_t kShardPackPiece = 64u << 10;
constexpr bool kShardPackNontemporal = true;
// frames of one has_data launch (their chunk bases are kernel arguments)
constexpr uint32_t kShardFlagFrames = 64;

struct ShardGeometry
{
    uint32_t n_shards;
    uint32_t slots_per_layer; // chunks_per_shard / layers_per_shard
    uint32_t chunks_per_shard;
    uint32_t chunks_per_layer;
};

// What a layer's kernels read and write; every pointer is device memory.
struct ShardLayerArgs
{
    const uint8_t* frames;
    uint64_t stride;
    const uint32_t* sizes;    // or null: every frame `stride` bytes
    const uint8_t* has_data;  // or null: every chunk present
    const int32_t* slot_chunk; // [n_shards * slots_per_layer] chunk of the slot, or -1
    const uint32_t* chunk_shard; // [chunks_per_layer]
    uint64_t* chunk_rel;      // [chunks_per_layer] bytes before the chunk in its segment
    uint64_t* file_off;       // [n_shards] running file offsets
    uint64_t* pairs;          // [n_shards * chunks_per_shard * 2]
    uint64_t* segments;       // [3 * n_shards + 1]
    uint8_t* out;
};

// The two scans of a layer: per shard over its slots (table pairs, segment
// bytes and file offset, new running offset, each chunk's place in its
// segment), then over the shards (segment starts, total).
hipError_t launch_shard_scan(const ShardLayerArgs& a, const ShardGeometry& g, uint32_t layer,
                             hipStream_t stream);

// Workgroup (c, p) copies piece p of frame c to its place.  hipErrorInvalidValue
// when the grid chunks_per_layer * ceil(stride / piece) reaches 2^31.
hipError_t launch_shard_pack(const ShardLayerArgs& a, const ShardGeometry& g, uint32_t piece,
                             bool nontemporal, hipStream_t stream);

// pairs + crcs[s] -> table bytes, running offsets -> table_offsets
hipError_t launch_shard_tables(const uint64_t* pairs, const uint32_t* crcs,
                               const uint64_t* file_off, uint8_t* tables, uint64_t* table_offsets,
                               const ShardGeometry& g, hipStream_t stream);

// has_data[base[k] + t] = 1 where tile t of frame k has a nonzero flag byte
hipError_t launch_shard_chunk_flags(const uint8_t* tile_nonzero, uint32_t n_frames,
                                    uint32_t n_tiles, uint32_t flag_slots,
                                    const uint32_t* host_base, uint8_t* has_data,
                                    hipStream_t stream);

} // namespace aqz
