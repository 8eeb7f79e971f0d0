// shard_layout.cpp — host-only Zarr v3 shard geometry (include/aqz_shard.h).
// Plain C++, no HIP header: it compiles and runs stand-alone
// (tests/cpp/shard_layout_sweep.cpp, under the host sanitizers).
//
// Restates ArrayDimensions' constructor counts (array.dimensions.cpp:168-178)
// and shard_index_for_chunk_ / shard_internal_index_ (:461-548) for the chunks
// of one layer.
#include "aqz_shard.h"

#include <cstdint>
#include <vector>

namespace {

constexpr uint64_t kLimit = 1ull << 31;

uint64_t
ceil_div(uint64_t a, uint64_t b)
{
    return (a + b - 1) / b;
}

} // namespace

extern "C" int
aqz_zarr_shard_layout(const aqz_dimension* dims, uint32_t ndims, uint32_t layer_in_shard,
                      aqz_zarr_shard_geometry* geo, uint32_t* shard_of, uint32_t* internal_of)
{
    if (!dims || !geo || ndims < 3 || ndims > AQZ_MAX_DIMS)
        return AQZ_INVALID_ARGUMENT;
    uint64_t chunks[AQZ_MAX_DIMS]; // chunks_along_dimension (zarr.common.cpp:88-92)
    uint64_t shards[AQZ_MAX_DIMS]; // shards_along_dimension (:94-104)
    for (uint32_t i = 0; i < ndims; ++i) {
        if (dims[i].chunk_size_px == 0 || dims[i].shard_size_chunks == 0 ||
            (i > 0 && dims[i].array_size_px == 0))
            return AQZ_INVALID_ARGUMENT;
        chunks[i] = ceil_div(dims[i].array_size_px, dims[i].chunk_size_px);
        shards[i] = ceil_div(chunks[i], dims[i].shard_size_chunks);
    }
    // array.dimensions.cpp:169-178: dimension 0 counts for chunks_per_shard_
    // only; every product is checked before it can wrap
    uint64_t per_layer = 1, per_shard = 1, n_shards = 1;
    for (uint32_t i = 0; i < ndims; ++i) {
        per_shard *= dims[i].shard_size_chunks;
        if (per_shard >= kLimit)
            return AQZ_OVERFLOW;
        if (i > 0) {
            per_layer *= chunks[i];
            n_shards *= shards[i];
            if (per_layer >= kLimit || n_shards >= kLimit)
                return AQZ_OVERFLOW;
        }
    }
    const uint32_t layers = dims[0].shard_size_chunks;
    if (layer_in_shard >= layers)
        return AQZ_INVALID_ARGUMENT;
    geo->n_shards = uint32_t(n_shards);
    geo->chunks_per_shard = uint32_t(per_shard);
    geo->chunks_per_layer = uint32_t(per_layer);
    geo->layers_per_shard = layers;
    if (!shard_of && !internal_of)
        return AQZ_OK;

    // strides of the shard lattice (:483-488) and of a chunk inside its shard
    // (:533-538); index 0 is the layer's own stride
    uint64_t shard_stride[AQZ_MAX_DIMS], internal_stride[AQZ_MAX_DIMS];
    shard_stride[ndims - 1] = internal_stride[ndims - 1] = 1;
    for (uint32_t i = ndims - 1; i > 0; --i) {
        shard_stride[i - 1] = shard_stride[i] * shards[i];
        internal_stride[i - 1] = internal_stride[i] * dims[i].shard_size_chunks;
    }
    // walk the layer's chunk lattice in order: lattice[i] is :477-480's
    // chunk_index % chunk_strides[i - 1] / chunk_strides[i], i >= 1
    uint32_t lattice[AQZ_MAX_DIMS] = { 0 };
    for (uint64_t c = 0; c < per_layer; ++c) {
        uint64_t shard = 0;                                         // lattice[0] stays 0 (:476-480)
        uint64_t internal = uint64_t(layer_in_shard) * internal_stride[0]; // :524, :543
        for (uint32_t i = 1; i < ndims; ++i) {
            shard += uint64_t(lattice[i] / dims[i].shard_size_chunks) * shard_stride[i];
            internal += uint64_t(lattice[i] % dims[i].shard_size_chunks) * internal_stride[i];
        }
        if (shard_of)
            shard_of[c] = uint32_t(shard);
        if (internal_of)
            internal_of[c] = uint32_t(internal);
        for (uint32_t i = ndims - 1; i > 0; --i) {
            if (++lattice[i] < chunks[i])
                break;
            lattice[i] = 0;
        }
    }
    return AQZ_OK;
}

// array.dimensions.cpp:232-314 (chunk_lattice_index, tile_group_offset,
// chunk_internal_offset) with the sum of aqz_chunk_frame_offsets kept in its
// parts: offsets[k] == base[k] * chunk_bytes + internal[k].
extern "C" int
aqz_chunk_frame_places(const aqz_dimension* dims, uint32_t ndims, uint32_t bytes_per_px,
                       uint64_t first_frame, uint32_t n_frames, uint32_t* frame_chunk_base,
                       uint64_t* frame_internal_offset_bytes, uint64_t* chunk_bytes,
                       uint32_t* chunks_per_layer)
{
    if (!dims || ndims < 3 || bytes_per_px == 0 ||
        (n_frames && (!frame_chunk_base || !frame_internal_offset_bytes)))
        return AQZ_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < ndims; ++i)
        if (dims[i].chunk_size_px == 0 || (i > 0 && dims[i].array_size_px == 0))
            return AQZ_INVALID_ARGUMENT;
    const uint32_t nd = ndims;
    // chunk-lattice strides of every dimension; strides[0] is a layer's chunks
    std::vector<uint64_t> strides(nd, 1);
    for (uint32_t i = nd - 1; i > 0; --i)
        strides[i - 1] = strides[i] * ceil_div(dims[i].array_size_px, dims[i].chunk_size_px);
    const uint64_t per_layer = strides[0];
    const uint64_t n_tiles = strides[nd - 3]; // tiles of one frame
    uint64_t per_chunk = bytes_per_px;
    for (uint32_t i = 0; i < nd; ++i)
        per_chunk *= dims[i].chunk_size_px;
    const uint64_t tile_bytes =
      uint64_t(bytes_per_px) * dims[nd - 1].chunk_size_px * dims[nd - 2].chunk_size_px;
    uint64_t layer_frames = dims[0].chunk_size_px;
    for (uint32_t i = 1; i + 2 < nd; ++i)
        layer_frames *= dims[i].array_size_px;
    const uint64_t layer0 = first_frame / layer_frames;
    for (uint32_t k = 0; k < n_frames; ++k) {
        const uint64_t fid = first_frame + k;
        // walk the frame dimensions from the innermost: `rest` is the frame id
        // in units of dimension i, `inner` the frames of one chunk below it
        uint64_t rest = fid, group = 0, internal = 0, inner = 1;
        for (uint32_t i = nd - 3; i > 0; --i) {
            const uint64_t idx = rest % dims[i].array_size_px;
            rest /= dims[i].array_size_px;
            group += idx / dims[i].chunk_size_px * strides[i];
            internal += idx % dims[i].chunk_size_px * inner;
            inner *= dims[i].chunk_size_px;
        }
        internal += rest % dims[0].chunk_size_px * inner;
        const uint64_t base = (fid / layer_frames - layer0) * per_layer + group;
        if (base + n_tiles >= UINT32_MAX) // UINT32_MAX is AQZ_CHUNK_SLOT_ABSENT
            return AQZ_OVERFLOW;
        frame_chunk_base[k] = uint32_t(base);
        frame_internal_offset_bytes[k] = internal * tile_bytes;
    }
    if (chunk_bytes)
        *chunk_bytes = per_chunk;
    if (chunks_per_layer) {
        if (per_layer >= UINT32_MAX)
            return AQZ_OVERFLOW;
        *chunks_per_layer = uint32_t(per_layer);
    }
    return AQZ_OK;
}
