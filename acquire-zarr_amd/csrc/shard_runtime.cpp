// shard_runtime.cpp — the aqz_zarr_shard_set of include/aqz_shard.h over
// shard_kernels.hip: device state of one array's shards, the layer append,
// the index tables and the host delivery.
#include "aqz_shard.h"
#include "abi_guard.hh"
#include "codec_kernels.hh"
#include "ds_plan.hh"
#include "gather_kernels.hh"
#include "shard_kernels.hh"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

struct aqz_zarr_shard_set
{
    int device = 0;
    aqz_zarr_shard_geometry geo{};
    aqz::ShardGeometry kg{};
    uint32_t layer = 0; // next layer of the open shards
    // device state
    uint64_t* d_file_off = nullptr;
    uint64_t* d_pairs = nullptr;
    int32_t* d_slot_chunk = nullptr;
    uint32_t* d_chunk_shard = nullptr;
    uint64_t* d_chunk_rel = nullptr;
    uint32_t* d_crcs = nullptr;
    // host delivery
    uint64_t* d_segments = nullptr;
    uint64_t* h_segments = nullptr; // pinned
    void* d_out = nullptr;
    size_t out_cap = 0;
    void* d_tables = nullptr; // tables, then their offsets
    uint64_t d2h_bytes = 0;
};

namespace {

int
hip_status(hipError_t e, const char* who)
{
    if (e == hipSuccess)
        return AQZ_OK;
    aqz::set_last_error(std::string("zarr_shard ") + who + ": " + hipGetErrorString(e));
    if (e == hipErrorOutOfMemory)
        return AQZ_OUT_OF_MEMORY;
    return e == hipErrorInvalidValue ? AQZ_INVALID_ARGUMENT : AQZ_INTERNAL_ERROR;
}

#define SHARD_HIP(call, who)                                                                       \
    do {                                                                                           \
        const int rc_ = hip_status((call), who);                                                   \
        if (rc_ != AQZ_OK)                                                                         \
            return rc_;                                                                            \
    } while (0)

int
invalid(const char* what)
{
    aqz::set_last_error(std::string("zarr_shard: ") + what);
    return AQZ_INVALID_ARGUMENT;
}

struct DeviceScope
{
    int prev = 0;
    explicit DeviceScope(int d)
    {
        (void)hipGetDevice(&prev);
        ok = hipSetDevice(d);
    }
    ~DeviceScope() { (void)hipSetDevice(prev); }
    hipError_t ok;
};

size_t
table_bytes(const aqz_zarr_shard_set* s)
{
    return 16 * size_t(s->geo.chunks_per_shard) + 4;
}

void
release(aqz_zarr_shard_set* s)
{
    (void)hipFree(s->d_file_off);
    (void)hipFree(s->d_pairs);
    (void)hipFree(s->d_slot_chunk);
    (void)hipFree(s->d_chunk_shard);
    (void)hipFree(s->d_chunk_rel);
    (void)hipFree(s->d_crcs);
    (void)hipFree(s->d_segments);
    (void)hipFree(s->d_out);
    (void)hipFree(s->d_tables);
    if (s->h_segments)
        (void)hipHostFree(s->h_segments);
    delete s;
}

int
reset(aqz_zarr_shard_set* s, hipStream_t stream)
{
    // kUnwrittenSentinel is all ones: a byte fill
    SHARD_HIP(hipMemsetAsync(s->d_pairs, 0xFF,
                             16 * size_t(s->geo.chunks_per_shard) * s->geo.n_shards, stream),
              "reset pairs");
    SHARD_HIP(hipMemsetAsync(s->d_file_off, 0, sizeof(uint64_t) * s->geo.n_shards, stream),
              "reset offsets");
    s->layer = 0;
    return AQZ_OK;
}

// The shared argument check and queueing of the two append forms.
int
queue_layer(aqz_zarr_shard_set* s, const void* frames, size_t stride, const uint32_t* sizes,
            const uint8_t* has_data, void* out, size_t capacity, uint64_t* segments,
            hipStream_t stream)
{
    if (!frames || !out || !segments)
        return invalid("append_layer: null pointer");
    if (stride == 0)
        return invalid("append_layer: frame_stride 0");
    if (sizes && stride >= (1ull << 32))
        return invalid("append_layer: frame_stride >= 2^32 with a size table");
    // chunks_per_layer < 2^31 and stride < 2^64: compare by division
    if (capacity / stride < s->geo.chunks_per_layer)
        return invalid("append_layer: capacity below chunks_per_layer * frame_stride");
    const uint64_t pieces = (uint64_t(stride) + aqz::kShardPackPiece - 1) / aqz::kShardPackPiece;
    if (pieces >= (1ull << 31) || pieces * s->geo.chunks_per_layer >= (1ull << 31))
        return invalid("append_layer: pack grid past the launch limit");
    if (s->layer >= s->geo.layers_per_shard)
        return invalid("append_layer: shards are full, call aqz_zarr_shard_set_begin");
    aqz::ShardLayerArgs a{};
    a.frames = static_cast<const uint8_t*>(frames);
    a.stride = stride;
    a.sizes = sizes;
    a.has_data = has_data;
    a.slot_chunk = s->d_slot_chunk;
    a.chunk_shard = s->d_chunk_shard;
    a.chunk_rel = s->d_chunk_rel;
    a.file_off = s->d_file_off;
    a.pairs = s->d_pairs;
    a.segments = segments;
    a.out = static_cast<uint8_t*>(out);
    SHARD_HIP(aqz::launch_shard_scan(a, s->kg, s->layer, stream), "scan");
    ++s->layer; // the scan is queued: the tables now hold this layer
    SHARD_HIP(aqz::launch_shard_pack(a, s->kg, aqz::kShardPackPiece, aqz::kShardPackNontemporal,
                                     stream),
              "pack");
    return AQZ_OK;
}

int
queue_tables(aqz_zarr_shard_set* s, void* tables, uint64_t* offsets, hipStream_t stream)
{
    if (!tables || !offsets)
        return invalid("tables: null pointer");
    const size_t pair_bytes = 16 * size_t(s->geo.chunks_per_shard);
    SHARD_HIP(aqz::launch_crc32c(s->d_pairs, pair_bytes, pair_bytes, s->geo.n_shards, s->d_crcs,
                                 stream),
              "table crc");
    SHARD_HIP(aqz::launch_shard_tables(s->d_pairs, s->d_crcs, s->d_file_off,
                                       static_cast<uint8_t*>(tables), offsets, s->kg, stream),
              "tables");
    return AQZ_OK;
}

} // namespace

extern "C" {

int
aqz_zarr_shard_set_create(const aqz_dimension* dims, uint32_t ndims, int device,
                          aqz_zarr_shard_set** out)
{
    try {
        if (!out)
            return invalid("set_create: null out");
        *out = nullptr;
        aqz_zarr_shard_geometry geo{};
        if (const int rc = aqz_zarr_shard_layout(dims, ndims, 0, &geo, nullptr, nullptr);
            rc != AQZ_OK) {
            aqz::set_last_error("zarr_shard_set_create: bad dimensions");
            return rc;
        }
        // launch_crc32c takes tables below 2^16 workgroups of 16 KiB
        if (16ull * geo.chunks_per_shard >= (1ull << 30)) {
            aqz::set_last_error("zarr_shard_set_create: index table of 1 GiB or more");
            return AQZ_OVERFLOW;
        }
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
            return invalid("set_create: no such device");
        std::vector<uint32_t> shard_of(geo.chunks_per_layer), internal_of(geo.chunks_per_layer);
        if (const int rc = aqz_zarr_shard_layout(dims, ndims, 0, &geo, shard_of.data(),
                                                 internal_of.data());
            rc != AQZ_OK)
            return rc;
        // layer 0's internal indices are the slot numbers
        const uint32_t spl = geo.chunks_per_shard / geo.layers_per_shard;
        std::vector<int32_t> slot_chunk(size_t(geo.n_shards) * spl, -1);
        for (uint32_t c = 0; c < geo.chunks_per_layer; ++c)
            slot_chunk[size_t(shard_of[c]) * spl + internal_of[c]] = int32_t(c);

        DeviceScope scope(device);
        if (scope.ok != hipSuccess)
            return hip_status(scope.ok, "set device");
        auto* s = new aqz_zarr_shard_set;
        s->device = device;
        s->geo = geo;
        s->kg = aqz::ShardGeometry{ geo.n_shards, spl, geo.chunks_per_shard, geo.chunks_per_layer };
        const size_t n = geo.n_shards;
        auto fail = [&](int rc) {
            release(s);
            return rc;
        };
#define SHARD_ALLOC(ptr, bytes)                                                                    \
    if (const int rc_ = hip_status(hipMalloc(reinterpret_cast<void**>(&(ptr)), (bytes)), "alloc"); \
        rc_ != AQZ_OK)                                                                             \
        return fail(rc_)
        SHARD_ALLOC(s->d_file_off, sizeof(uint64_t) * n);
        SHARD_ALLOC(s->d_pairs, 16 * size_t(geo.chunks_per_shard) * n);
        SHARD_ALLOC(s->d_slot_chunk, sizeof(int32_t) * slot_chunk.size());
        SHARD_ALLOC(s->d_chunk_shard, sizeof(uint32_t) * geo.chunks_per_layer);
        SHARD_ALLOC(s->d_chunk_rel, sizeof(uint64_t) * geo.chunks_per_layer);
        SHARD_ALLOC(s->d_crcs, sizeof(uint32_t) * n);
        SHARD_ALLOC(s->d_segments, sizeof(uint64_t) * (3 * n + 1));
#undef SHARD_ALLOC
        if (const int rc = hip_status(hipHostMalloc(reinterpret_cast<void**>(&s->h_segments),
                                                    sizeof(uint64_t) * (3 * n + 1)),
                                      "pinned segments");
            rc != AQZ_OK)
            return fail(rc);
        // blocking copies: the maps are in place when create returns
        if (const int rc = hip_status(hipMemcpy(s->d_slot_chunk, slot_chunk.data(),
                                                sizeof(int32_t) * slot_chunk.size(),
                                                hipMemcpyHostToDevice),
                                      "slot map");
            rc != AQZ_OK)
            return fail(rc);
        if (const int rc = hip_status(hipMemcpy(s->d_chunk_shard, shard_of.data(),
                                                sizeof(uint32_t) * shard_of.size(),
                                                hipMemcpyHostToDevice),
                                      "shard map");
            rc != AQZ_OK)
            return fail(rc);
        if (const int rc = hip_status(hipMemset(s->d_chunk_rel, 0,
                                                sizeof(uint64_t) * geo.chunks_per_layer),
                                      "clear");
            rc != AQZ_OK)
            return fail(rc);
        if (const int rc = reset(s, nullptr); rc != AQZ_OK)
            return fail(rc);
        if (const int rc = hip_status(hipStreamSynchronize(nullptr), "sync"); rc != AQZ_OK)
            return fail(rc);
        *out = s;
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

void
aqz_zarr_shard_set_destroy(aqz_zarr_shard_set* set)
{
    if (!set)
        return;
    DeviceScope scope(set->device);
    (void)hipDeviceSynchronize();
    release(set);
}

int
aqz_zarr_shard_set_geometry(const aqz_zarr_shard_set* set, aqz_zarr_shard_geometry* geo)
{
    if (!set || !geo)
        return invalid("set_geometry: null pointer");
    *geo = set->geo;
    return AQZ_OK;
}

int
aqz_zarr_shard_set_begin(aqz_zarr_shard_set* set, void* hip_stream)
{
    try {
        if (!set)
            return invalid("set_begin: null set");
        DeviceScope scope(set->device);
        SHARD_HIP(scope.ok, "set device");
        return reset(set, static_cast<hipStream_t>(hip_stream));
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_zarr_shard_set_append_layer_device(aqz_zarr_shard_set* set, const void* device_frames,
                                       size_t frame_stride, const uint32_t* device_frame_bytes,
                                       const uint8_t* device_has_data, void* device_out,
                                       size_t out_capacity, uint64_t* device_segments,
                                       void* hip_stream)
{
    try {
        if (!set)
            return invalid("append_layer_device: null set");
        DeviceScope scope(set->device);
        SHARD_HIP(scope.ok, "set device");
        return queue_layer(set, device_frames, frame_stride, device_frame_bytes, device_has_data,
                           device_out, out_capacity, device_segments,
                           static_cast<hipStream_t>(hip_stream));
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_zarr_shard_set_tables_device(aqz_zarr_shard_set* set, void* device_tables,
                                 uint64_t* device_table_offsets, void* hip_stream)
{
    try {
        if (!set)
            return invalid("tables_device: null set");
        DeviceScope scope(set->device);
        SHARD_HIP(scope.ok, "set device");
        return queue_tables(set, device_tables, device_table_offsets,
                            static_cast<hipStream_t>(hip_stream));
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_zarr_shard_set_append_layer(aqz_zarr_shard_set* set, const void* device_frames,
                                size_t frame_stride, const uint32_t* device_frame_bytes,
                                const uint8_t* device_has_data, void* host_out,
                                size_t host_capacity, uint64_t* host_segments, void* hip_stream)
{
    try {
        if (!set || !host_out || !host_segments)
            return invalid("append_layer: null pointer");
        if (frame_stride == 0 || host_capacity / frame_stride < set->geo.chunks_per_layer)
            return invalid("append_layer: host_capacity below chunks_per_layer * frame_stride");
        DeviceScope scope(set->device);
        SHARD_HIP(scope.ok, "set device");
        auto stream = static_cast<hipStream_t>(hip_stream);
        const size_t want = size_t(set->geo.chunks_per_layer) * frame_stride;
        if (set->out_cap < want) {
            SHARD_HIP(hipFree(set->d_out), "free");
            set->d_out = nullptr;
            set->out_cap = 0;
            SHARD_HIP(hipMalloc(&set->d_out, want), "layer scratch");
            set->out_cap = want;
        }
        // every exit drains `stream`: nothing of this call stays queued on
        // the set's scratch
        struct Drain
        {
            hipStream_t s;
            ~Drain() { (void)hipStreamSynchronize(s); }
        } drain{ stream };
        if (const int rc = queue_layer(set, device_frames, frame_stride, device_frame_bytes,
                                       device_has_data, set->d_out, set->out_cap, set->d_segments,
                                       stream);
            rc != AQZ_OK)
            return rc;
        // the segment table crosses first; then the segments in one copy
        const size_t seg_bytes = sizeof(uint64_t) * (3 * size_t(set->geo.n_shards) + 1);
        SHARD_HIP(hipMemcpyAsync(set->h_segments, set->d_segments, seg_bytes,
                                 hipMemcpyDeviceToHost, stream),
                  "segment table");
        SHARD_HIP(hipStreamSynchronize(stream), "sync");
        const uint64_t total = set->h_segments[3 * size_t(set->geo.n_shards)];
        if (total > want) {
            aqz::set_last_error("zarr_shard append_layer: total out of range");
            return AQZ_INTERNAL_ERROR;
        }
        if (total) {
            SHARD_HIP(hipMemcpyAsync(host_out, set->d_out, total, hipMemcpyDeviceToHost, stream),
                      "segments");
            SHARD_HIP(hipStreamSynchronize(stream), "sync");
        }
        set->d2h_bytes = seg_bytes + total;
        std::memcpy(host_segments, set->h_segments, seg_bytes);
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_zarr_shard_set_tables(aqz_zarr_shard_set* set, void* host_tables,
                          uint64_t* host_table_offsets, void* hip_stream)
{
    try {
        if (!set || !host_tables || !host_table_offsets)
            return invalid("tables: null pointer");
        DeviceScope scope(set->device);
        SHARD_HIP(scope.ok, "set device");
        auto stream = static_cast<hipStream_t>(hip_stream);
        const size_t n = set->geo.n_shards;
        const size_t tb = (table_bytes(set) * n + 7) / 8 * 8; // the uint64 offsets after the tables
        if (!set->d_tables)
            SHARD_HIP(hipMalloc(&set->d_tables, tb + sizeof(uint64_t) * n), "table scratch");
        auto* d_tab = static_cast<uint8_t*>(set->d_tables);
        auto* d_off = reinterpret_cast<uint64_t*>(d_tab + tb);
        struct Drain
        {
            hipStream_t s;
            ~Drain() { (void)hipStreamSynchronize(s); }
        } drain{ stream };
        if (const int rc = queue_tables(set, d_tab, d_off, stream); rc != AQZ_OK)
            return rc;
        SHARD_HIP(hipMemcpyAsync(host_tables, d_tab, table_bytes(set) * n, hipMemcpyDeviceToHost,
                                 stream),
                  "tables");
        SHARD_HIP(hipMemcpyAsync(host_table_offsets, d_off, sizeof(uint64_t) * n,
                                 hipMemcpyDeviceToHost, stream),
                  "table offsets");
        SHARD_HIP(hipStreamSynchronize(stream), "sync");
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_zarr_shard_chunk_has_data_device(const uint8_t* device_tile_nonzero, uint32_t n_frames,
                                     uint32_t n_tiles, uint32_t flag_slots,
                                     const uint32_t* host_frame_chunk_base,
                                     uint8_t* device_has_data, void* hip_stream)
{
    try {
        if (!device_tile_nonzero || !host_frame_chunk_base || !device_has_data || n_frames == 0 ||
            n_tiles == 0 || flag_slots == 0 || n_tiles >= (1u << 31))
            return invalid("chunk_has_data_device: invalid argument");
        return hip_status(aqz::launch_shard_chunk_flags(device_tile_nonzero, n_frames, n_tiles,
                                                        flag_slots, host_frame_chunk_base,
                                                        device_has_data,
                                                        static_cast<hipStream_t>(hip_stream)),
                          "chunk flags");
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

// Every refusal of the gather, then the launcher: shared by the batch call and
// the single-frame inverse.
static int
gather_frames(const char* who, int dtype, uint32_t width, uint32_t height, uint32_t tile_rows,
              uint32_t tile_cols, const void* device_chunks, size_t chunk_stride_bytes,
              uint32_t n_slots, const uint32_t* device_chunk_slot, uint32_t n_chunks,
              const uint32_t* host_base, const uint64_t* host_internal, uint32_t n_frames,
              void* device_frames, size_t frame_stride_bytes, uint32_t* device_bad_slot,
              void* hip_stream)
{
    auto refuse = [who](const char* what) { return invalid((std::string(who) + ": " + what).c_str()); };
    if (!device_chunks || !host_base || !host_internal || !device_frames)
        return refuse("null pointer");
    if (!aqz::dtype_valid(dtype))
        return refuse("bad dtype");
    if (width == 0 || height == 0 || tile_rows == 0 || tile_cols == 0 || n_slots == 0 ||
        n_chunks == 0 || n_frames == 0 || chunk_stride_bytes == 0 || frame_stride_bytes == 0)
        return refuse("a zero extent, tile side, count or stride");
    const uint64_t bpp = aqz::dtype_bytes(dtype);
    uint32_t lg = 0;
    while ((1u << lg) < bpp)
        ++lg;
    const uint64_t tile_elems = uint64_t(tile_rows) * tile_cols;
    const uint64_t ntx = (uint64_t(width) + tile_cols - 1) / tile_cols;
    const uint64_t n_tiles = ntx * ((uint64_t(height) + tile_rows - 1) / tile_rows);
    if (tile_elems >= (1ull << 31) || n_tiles >= (1ull << 31))
        return refuse("a tile of 2^31 elements or more, or 2^31 tiles or more");
    if (chunk_stride_bytes % bpp || frame_stride_bytes % bpp)
        return refuse("a stride that is not a multiple of the pixel size");
    if (reinterpret_cast<uintptr_t>(device_chunks) % bpp ||
        reinterpret_cast<uintptr_t>(device_frames) % bpp)
        return refuse("a buffer that is not aligned to the pixel size");
    const uint64_t n_px = uint64_t(width) * height;
    if (n_px > UINT64_MAX / bpp || frame_stride_bytes < n_px * bpp)
        return refuse("frame_stride_bytes below width * height * pixel size");
    if (!device_chunk_slot && n_chunks != n_slots)
        return refuse("no slot table, and n_chunks differs from n_slots");
    const uint64_t tile_bytes = tile_elems * bpp;
    for (uint32_t k = 0; k < n_frames; ++k) {
        if (host_internal[k] % bpp)
            return refuse("an internal offset that is not a multiple of the pixel size");
        if (host_internal[k] > chunk_stride_bytes ||
            tile_bytes > chunk_stride_bytes - host_internal[k])
            return refuse("an internal offset whose tile ends past chunk_stride_bytes");
        if (uint64_t(host_base[k]) + n_tiles > n_chunks)
            return refuse("a frame's chunks end past n_chunks");
    }
    aqz::GatherArgs a{};
    a.chunks = static_cast<const uint8_t*>(device_chunks);
    a.chunk_stride = chunk_stride_bytes;
    a.slot = device_chunk_slot;
    a.n_slots = n_slots;
    a.bpp_log2 = lg;
    a.W = width;
    a.H = height;
    a.tile_rows = tile_rows;
    a.tile_cols = tile_cols;
    a.n_tiles_x = uint32_t(ntx);
    a.frames = static_cast<uint8_t*>(device_frames);
    a.frame_stride = frame_stride_bytes;
    a.bad_slot = device_bad_slot;
    const hipError_t e = aqz::launch_chunk_gather(a, host_base, host_internal, n_frames,
                                                  static_cast<hipStream_t>(hip_stream));
    if (e == hipErrorInvalidValue)
        return refuse("a launch grid of 2^31 workgroups or more");
    return hip_status(e, who);
}

int
aqz_chunk_gather_frames_device(int dtype, uint32_t width, uint32_t height, uint32_t tile_rows,
                               uint32_t tile_cols, const void* device_chunks,
                               size_t chunk_stride_bytes, uint32_t n_slots,
                               const uint32_t* device_chunk_slot, uint32_t n_chunks,
                               const uint32_t* host_frame_chunk_base,
                               const uint64_t* host_frame_internal_offset_bytes,
                               uint32_t n_frames, void* device_frames, size_t frame_stride_bytes,
                               uint32_t* device_bad_slot, void* hip_stream)
{
    try {
        return gather_frames("chunk_gather_frames_device", dtype, width, height, tile_rows,
                             tile_cols, device_chunks, chunk_stride_bytes, n_slots,
                             device_chunk_slot, n_chunks, host_frame_chunk_base,
                             host_frame_internal_offset_bytes, n_frames, device_frames,
                             frame_stride_bytes, device_bad_slot, hip_stream);
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_untile_frame_device(int dtype, const void* device_tiles, uint32_t width, uint32_t height,
                        uint32_t tile_rows, uint32_t tile_cols, void* device_frame,
                        void* hip_stream)
{
    try {
        const char* who = "untile_frame_device";
        if (!aqz::dtype_valid(dtype) || width == 0 || height == 0 || tile_rows == 0 ||
            tile_cols == 0)
            return invalid("untile_frame_device: bad dtype or a zero extent or tile side");
        const uint64_t bpp = aqz::dtype_bytes(dtype);
        const uint64_t tile_elems = uint64_t(tile_rows) * tile_cols;
        const uint64_t n_tiles = ((uint64_t(width) + tile_cols - 1) / tile_cols) *
                                 ((uint64_t(height) + tile_rows - 1) / tile_rows);
        const uint64_t n_px = uint64_t(width) * height;
        if (tile_elems >= (1ull << 31) || n_tiles >= (1ull << 31) || n_px > UINT64_MAX / bpp)
            return invalid("untile_frame_device: a tile of 2^31 elements or more, 2^31 tiles or "
                           "more, or a frame past the address space");
        // one frame, tiles back to back: slot t is tile t
        const uint32_t base = 0;
        const uint64_t internal = 0;
        return gather_frames(who, dtype, width, height, tile_rows, tile_cols, device_tiles,
                             size_t(tile_elems * bpp), uint32_t(n_tiles), nullptr,
                             uint32_t(n_tiles), &base, &internal, 1, device_frame,
                             size_t(n_px * bpp), nullptr, hip_stream);
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

uint64_t
aqz_debug_zarr_shard_d2h_bytes(const aqz_zarr_shard_set* set)
{
    return set ? set->d2h_bytes : 0;
}

int
aqz_debug_zarr_shard_set_file_offsets(aqz_zarr_shard_set* set, const uint64_t* host_offsets,
                                      void* hip_stream)
{
    try {
        if (!set || !host_offsets)
            return invalid("set_file_offsets: null pointer");
        DeviceScope scope(set->device);
        SHARD_HIP(scope.ok, "set device");
        auto stream = static_cast<hipStream_t>(hip_stream);
        SHARD_HIP(hipMemcpyAsync(set->d_file_off, host_offsets,
                                 sizeof(uint64_t) * set->geo.n_shards, hipMemcpyHostToDevice,
                                 stream),
                  "file offsets");
        SHARD_HIP(hipStreamSynchronize(stream), "sync");
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

int
aqz_debug_zarr_shard_pack_device(aqz_zarr_shard_set* set, const void* device_frames,
                                 size_t frame_stride, const uint32_t* device_frame_bytes,
                                 const uint8_t* device_has_data, void* device_out,
                                 const uint64_t* device_segments, uint32_t piece_bytes, int policy,
                                 const uint64_t* device_offsets, void* hip_stream)
{
    try {
        if (!set || !device_frames || !device_out || frame_stride == 0)
            return invalid("debug_pack_device: invalid argument");
        DeviceScope scope(set->device);
        SHARD_HIP(scope.ok, "set device");
        auto stream = static_cast<hipStream_t>(hip_stream);
        if (piece_bytes == 0) {
            if (!device_frame_bytes || !device_offsets)
                return invalid("debug_pack_device: sizes and offsets needed");
            SHARD_HIP(aqz::launch_pack_frames(device_frames, frame_stride, device_frame_bytes,
                                              device_offsets, device_out,
                                              set->geo.chunks_per_layer, stream),
                      "pack_frames");
            return AQZ_OK;
        }
        if (!device_segments || piece_bytes % 16 || policy < 0 || policy > 1 ||
            (device_frame_bytes && frame_stride >= (1ull << 32)))
            return invalid("debug_pack_device: invalid argument");
        aqz::ShardLayerArgs a{};
        a.frames = static_cast<const uint8_t*>(device_frames);
        a.stride = frame_stride;
        a.sizes = device_frame_bytes;
        a.has_data = device_has_data;
        a.chunk_shard = set->d_chunk_shard;
        a.chunk_rel = set->d_chunk_rel;
        a.segments = const_cast<uint64_t*>(device_segments); // read only by the pack kernel
        a.out = static_cast<uint8_t*>(device_out);
        SHARD_HIP(aqz::launch_shard_pack(a, set->kg, piece_bytes, policy == 1, stream), "pack");
        return AQZ_OK;
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}

} // extern "C"
