/*
 * aqz_shard.h — Zarr v3 shards assembled on the device from chunk frames
 * that were made on the device.  Same library
 * (libaqz_downsampler.so) and status codes as aqz_downsampler.h.
 *
 * Naming: the prefix here is aqz_zarr_shard_.  aqz_shard_unit
 * (aqz_downsampler.h) is something else: the slab of frames a node deals to
 * one GPU.  A "shard" in this header is always the Zarr v3 sharding codec's
 * file: chunk bytes end to end, then the index table.
 *
 * What is restated: Shard::write_chunk / skip_chunk / write_table_
 * (shard.cpp:53-165) as driven by Array::compress_and_flush_data_
 * (array.cpp:762-811), with the chunk -> (shard, internal index) map of
 * ArrayDimensions::shard_index_for_chunk_ / shard_internal_index_
 * (array.dimensions.cpp:461-548).  Nothing here writes a file: a caller gets
 * each shard's next bytes ("segment") with the file offset at which they
 * belong, and each shard's index table with its offset.
 */
#ifndef AQZ_SHARD_H
#define AQZ_SHARD_H

#include "aqz_blosc.h"
#include "aqz_downsampler.h"

#ifdef __cplusplus
extern "C"
{
#endif

/* kUnwrittenSentinel (shard.hh): offset and extent of a chunk that was
 * skipped, is ragged padding, or has not been appended yet. */
#define AQZ_ZARR_SHARD_SENTINEL UINT64_MAX

typedef struct
{
    uint32_t n_shards;         /* number_of_shards_ (array.dimensions.cpp:176) */
    uint32_t chunks_per_shard; /* chunks_per_shard_ (:172) */
    uint32_t chunks_per_layer; /* number_of_chunks_in_memory_ (:175) */
    uint32_t layers_per_shard; /* dims[0].shard_size_chunks (:388-391) */
} aqz_zarr_shard_geometry;

/*
 * Host only, no GPU involved (csrc/shard_layout.cpp compiles without HIP).
 *
 * `dims` are an array's dimensions in storage order (ndims 3..AQZ_MAX_DIMS,
 * a 2-D array with the phantom singleton dimension already prepended, as for
 * aqz_plan_levels).  For chunk c of a layer, c = 0 .. chunks_per_layer - 1 in
 * lattice order (the order of aqz_chunk_lattice and of
 * aqz_blosc_lz4_frames_device's frames), with `layer_in_shard` the layer's
 * place in its shards (0 .. layers_per_shard - 1), the chunk index is
 * layer_in_shard * chunks_per_layer + c and
 *   shard_of[c]    = shard_index_for_chunk_(chunk index)   (:461-502)
 *   internal_of[c] = shard_internal_index_(chunk index)    (:504-548)
 * Lattice index 0 takes no part in the shard index, as there (:477-480 leaves
 * chunk_lattice_indices[0] at 0).  `shard_of` and `internal_of` hold
 * chunks_per_layer entries each; both may be NULL for a geometry query.
 *
 * A shard-layer's internal indices are layer_in_shard * S .. + S - 1 with
 * S = chunks_per_shard / layers_per_shard.  Those no chunk of the layer takes
 * are the reference's skipped_internal_indices_for_shard_layer (:424-453):
 * the padding of ragged shards.
 *
 * AQZ_INVALID_ARGUMENT: a null dims or geo, ndims outside 3..AQZ_MAX_DIMS, a
 * zero chunk_size_px or shard_size_chunks, a zero array_size_px in any
 * dimension but the first, layer_in_shard >= layers_per_shard.
 * AQZ_OVERFLOW: chunks_per_layer, chunks_per_shard or n_shards >= 2^31.
 */
int aqz_zarr_shard_layout(const aqz_dimension* dims,
                          uint32_t ndims,
                          uint32_t layer_in_shard,
                          aqz_zarr_shard_geometry* geo,
                          uint32_t* shard_of,
                          uint32_t* internal_of);

/*
 * The shards of one array on one device.  Device state: per shard the
 * running file offset (Shard::file_offset_) and the chunks_per_shard
 * (offset, extent) uint64 pairs (offsets_ / extents_), and the slot map
 * (shard, slot j) -> chunk c of a layer or none, uploaded once: a layer only
 * adds layer_in_shard * S to the slot number to get the internal index.
 * A set serves one call at a time.  It orders nothing itself: begin, the
 * layers and the tables queued on one stream follow each other by stream
 * order; a caller that moves to another stream while earlier calls may still
 * run must order the two itself (an event recorded behind the earlier calls
 * and waited for by the new stream).
 * Refused with AQZ_OVERFLOW at create: what aqz_zarr_shard_layout refuses,
 * and an index table of 1 GiB or more (aqz_crc32c_device's limit).
 */
typedef struct aqz_zarr_shard_set aqz_zarr_shard_set;

int aqz_zarr_shard_set_create(const aqz_dimension* dims,
                              uint32_t ndims,
                              int device,
                              aqz_zarr_shard_set** out);
void aqz_zarr_shard_set_destroy(aqz_zarr_shard_set* set);
int aqz_zarr_shard_set_geometry(const aqz_zarr_shard_set* set, aqz_zarr_shard_geometry* geo);

/*
 * Fresh shards (the append-dimension rollover, array.cpp:804-808, and
 * Shard's constructor): every pair the sentinel, every file offset 0, next
 * layer 0.  Queued on `hip_stream`, no synchronisation.  A new set has begun.
 */
int aqz_zarr_shard_set_begin(aqz_zarr_shard_set* set, void* hip_stream);

/*
 * One chunk layer into its shards (compress_and_flush_data_'s loop,
 * array.cpp:783-802, with write_chunk / skip_chunk, shard.cpp:53-133).
 *
 * Frame c (c < chunks_per_layer, lattice order) lies at
 * device_frames + c * frame_stride.  Its size is device_frame_bytes[c], the
 * uint32 table aqz_blosc_lz4_frames_device writes (a size above frame_stride
 * counts as frame_stride); NULL: every frame is frame_stride bytes (an
 * uncompressed array's chunk buffers).  device_has_data[c] == 0 is
 * skip_chunk (Chunk::has_data, array.cpp:713-716); NULL: every chunk is
 * present.  A present frame of size 0 is a written chunk of extent 0.
 *
 * Per shard the present frames go end to end in ascending internal index —
 * the order the reference takes with one thread (array.cpp:786-801, jobs run
 * inline); under its thread pool the order is arbitrary, so every order is a
 * valid shard and this one is deterministic.  The shards' segments are packed
 * end to end, in shard order, into device_out.  device_segments receives
 * 3 * n_shards + 1 uint64: per shard s
 *   [3s]     where the segment starts in device_out,
 *   [3s + 1] its bytes,
 *   [3s + 2] the file offset at which it belongs (the shard's running offset
 *            before this layer),
 * and last the total bytes.  The table entries of this layer's slots become
 * (file offset, extent), or the sentinel for skipped chunks and ragged
 * padding; the running offsets advance.
 *
 * Everything is queued on `hip_stream`; the call never synchronises and
 * nothing crosses to the host.  Only bytes [start, start + bytes) of each
 * segment are written; no frame is read past its size.
 *
 * AQZ_INVALID_ARGUMENT before anything is queued: a null set, device_frames,
 * device_out or device_segments; frame_stride 0; out_capacity <
 * chunks_per_layer * frame_stride; frame_stride >= 2^32 with
 * device_frame_bytes given; a launch grid of 2^31 workgroups or more
 * (chunks_per_layer * ceil(frame_stride / piece)); a layer past
 * layers_per_shard without aqz_zarr_shard_set_begin.
 */
int aqz_zarr_shard_set_append_layer_device(aqz_zarr_shard_set* set,
                                           const void* device_frames,
                                           size_t frame_stride,
                                           const uint32_t* device_frame_bytes,
                                           const uint8_t* device_has_data,
                                           void* device_out,
                                           size_t out_capacity,
                                           uint64_t* device_segments,
                                           void* hip_stream);

/*
 * Shard::write_table_ (shard.cpp:145-165) for every shard: table s, the
 * 16 * chunks_per_shard + 4 bytes (pairs, then the CRC-32C of the pairs), at
 * device_tables + s * (16 * chunks_per_shard + 4), and the file offset at
 * which it goes (the shard's running offset) in device_table_offsets[s].
 * Callable at any time: a partial trailing shard has the sentinel for the
 * layers never appended, as Shard::finalize gives (shard.cpp:167-196).
 * Queued on `hip_stream`, no synchronisation.  Null pointers are
 * AQZ_INVALID_ARGUMENT.
 */
int aqz_zarr_shard_set_tables_device(aqz_zarr_shard_set* set,
                                     void* device_tables,
                                     uint64_t* device_table_offsets,
                                     void* hip_stream);

/*
 * Host delivery.  The layer is assembled in device memory the set owns; the
 * 24 * n_shards + 8 byte segment table crosses first, then exactly `total`
 * bytes cross in one copy into host_out; the call returns when they are
 * there.  host_segments as device_segments (starts are offsets into
 * host_out).  host_capacity < chunks_per_layer * frame_stride is
 * AQZ_INVALID_ARGUMENT, like out_capacity.
 */
int aqz_zarr_shard_set_append_layer(aqz_zarr_shard_set* set,
                                    const void* device_frames,
                                    size_t frame_stride,
                                    const uint32_t* device_frame_bytes,
                                    const uint8_t* device_has_data,
                                    void* host_out,
                                    size_t host_capacity,
                                    uint64_t* host_segments,
                                    void* hip_stream);

/* aqz_zarr_shard_set_tables_device into host memory; returns when the
 * n_shards tables and offsets are there. */
int aqz_zarr_shard_set_tables(aqz_zarr_shard_set* set,
                              void* host_tables,
                              uint64_t* host_table_offsets,
                              void* hip_stream);

/*
 * Per-chunk has_data from the tiled batch's per-frame zero scan, without a
 * host pass.  device_tile_nonzero is one level's flag array of
 * aqz_ds_run_device_batch_tiled / _chunked: n_frames frames of n_tiles tiles
 * of flag_slots bytes (aqz_ds_tiled_flag_slots).  Tile t of frame k belongs
 * to chunk host_frame_chunk_base[k] + t, the base being tile_group_offset(k)
 * (array.dimensions.cpp:264-282; array.cpp:563-617 writes chunks_[t + base]);
 * device_has_data[that chunk] is set to 1 when any of the tile's flag bytes
 * is nonzero and left alone otherwise.  So it accumulates over the batches
 * of a layer; the caller clears device_has_data at the layer's start, and it
 * must hold max(base) + n_tiles bytes.  The bases travel as kernel
 * arguments: `host_frame_chunk_base` may be freed on return.  Queued on
 * `hip_stream`, no synchronisation.  AQZ_INVALID_ARGUMENT: null pointers,
 * n_frames, n_tiles or flag_slots 0, n_tiles >= 2^31.
 */
int aqz_zarr_shard_chunk_has_data_device(const uint8_t* device_tile_nonzero,
                                         uint32_t n_frames,
                                         uint32_t n_tiles,
                                         uint32_t flag_slots,
                                         const uint32_t* host_frame_chunk_base,
                                         uint8_t* device_has_data,
                                         void* hip_stream);

/*
 * A shard's chunks back out of its bytes, on the device: the read side of
 * append_layer_device + tables_device for blosc LZ4 chunks
 * (aqz_blosc_lz4_decompress_device with the frames found through an index
 * table; statuses AQZ_BLOSC_FRAME_* of aqz_blosc.h).
 *
 * `device_table` is one shard's index table exactly as
 * aqz_zarr_shard_set_tables_device writes it: n_chunks (offset, extent)
 * uint64 pairs at any byte alignment (tables lie 16 * n + 4 bytes apart); the
 * CRC behind them is not read (aqz_crc32c_device checks
 * it).  The offsets are file offsets; device_shard_bytes holds the
 * shard_bytes bytes of the file from base_file_offset on, so chunk i's frame
 * lies at device_shard_bytes + offset - base_file_offset, at any byte
 * alignment.  Chunk i is written to device_dst + i * dst_stride and its
 * status to device_status[i]:
 *   - the sentinel pair: ABSENT, the chunk zero-filled (the fill value of the
 *     arrays written here);
 *   - a pair that leaves [0, shard_bytes): CORRUPT;
 *   - else what the frame's header and bytes give.
 * Not the tool for an uncompressed array's shards, whose extents are nbytes
 * and whose chunks carry no blosc header: those are BAD_HEADER here; copy
 * them with the table instead.
 *
 * Queued on `hip_stream`, never synchronises; ctx scratch as for
 * aqz_blosc_lz4_decompress_device.  AQZ_INVALID_ARGUMENT before anything is
 * queued: a null ctx or pointer, typesize, nbytes or n_chunks 0, dst_stride <
 * nbytes, nbytes above BLOSC_MAX_BUFFERSIZE.
 */
int aqz_zarr_shard_decompress_device(aqz_blosc_ctx* ctx,
                                     uint32_t typesize,
                                     size_t nbytes,
                                     const void* device_shard_bytes,
                                     size_t shard_bytes,
                                     uint64_t base_file_offset,
                                     const uint64_t* device_table,
                                     uint32_t n_chunks,
                                     void* device_dst,
                                     size_t dst_stride,
                                     uint32_t* device_status,
                                     void* hip_stream);

/*
 * The next step of a read: the decoded chunks are still tiles.
 * aqz_chunk_frame_places says where each frame's tiles lie among them and
 * aqz_chunk_gather_frames_device writes the frames out row-major
 * (DESIGN.md §12.14).
 *
 * Host only, no GPU involved (csrc/shard_layout.cpp).  aqz_chunk_frame_offsets
 * with its sum kept in parts, for the same arguments and with the same
 * refusals: for frame k = 0 .. n_frames - 1 of a batch that starts at frame
 * `first_frame` of the array,
 *   frame_chunk_base[k]            = (layer(k) - layer(first_frame))
 *                                    * chunks_per_layer + tile_group_offset(k)
 *   frame_internal_offset_bytes[k] = chunk_internal_offset(k)
 * so tile t of frame k lies in chunk frame_chunk_base[k] + t of the batch's
 * layers, at that offset, and
 *   offsets[k] == frame_chunk_base[k] * chunk_bytes + frame_internal_offset_bytes[k]
 * with aqz_chunk_frame_offsets' offsets.  chunk_bytes and chunks_per_layer may
 * be NULL.  AQZ_OVERFLOW: a base plus the frame's tile count would reach
 * UINT32_MAX (AQZ_CHUNK_SLOT_ABSENT), or chunks_per_layer would.
 */
int aqz_chunk_frame_places(const aqz_dimension* dims,
                           uint32_t ndims,
                           uint32_t bytes_per_px,
                           uint64_t first_frame,
                           uint32_t n_frames,
                           uint32_t* frame_chunk_base,
                           uint64_t* frame_internal_offset_bytes,
                           uint64_t* chunk_bytes,
                           uint32_t* chunks_per_layer);

/* A chunk no buffer holds: it reads as zeros, the fill value, as
 * AQZ_BLOSC_FRAME_ABSENT does. */
#define AQZ_CHUNK_SLOT_ABSENT UINT32_MAX

/*
 * Chunk buffers back into row-major frames, on the device: the inverse of the
 * chunk tiling.  Frame k (width x height pixels of `dtype`) is written at
 * device_frames + k * frame_stride_bytes.  With n_tiles_x = ceil(width /
 * tile_cols), its pixel (y, x) comes from chunk
 *   c = host_frame_chunk_base[k] + (y / tile_rows) * n_tiles_x + x / tile_cols
 * at byte
 *   device_chunks + slot(c) * chunk_stride_bytes
 *     + host_frame_internal_offset_bytes[k]
 *     + ((y % tile_rows) * tile_cols + x % tile_cols) * pixel size
 * where slot(c) = device_chunk_slot[c] (n_chunks entries, device memory), or
 * c itself when the table is NULL (then n_chunks must equal n_slots).  The
 * identity form reads a lattice as aqz_ds_run_device_batch_chunked[_base] and
 * aqz_ds_run_device_volume_chunked write it.  The table form reads what
 * aqz_zarr_shard_decompress_device wrote: with shard s decoded to
 * dst + s * chunks_per_shard * dst_stride, slot(c) = shard_of[c] *
 * chunks_per_shard + internal_of[c] (aqz_zarr_shard_layout).
 *
 * A slot AQZ_CHUNK_SLOT_ABSENT reads as zeros.  Any other slot >= n_slots
 * reads as zeros too, nothing is loaded for it, and *device_bad_slot (if
 * given; the caller clears it) is set to 1.
 *
 * Only pixels inside the frame are read: never a tile's overhang, never
 * another frame's bytes of a chunk.  Nothing outside [k * stride, k * stride
 * + width * height * pixel size) is written.  Everything is queued on
 * `hip_stream`; the call never synchronises and owns no scratch.  The
 * per-frame tables travel as kernel arguments, 64 frames a launch, so the
 * host arrays may be freed on return.
 *
 * AQZ_INVALID_ARGUMENT before anything is queued: a null pointer (the slot
 * table and device_bad_slot may be NULL); a zero extent, tile side, count or
 * stride; a bad dtype; a tile of 2^31 elements or more, or 2^31 tiles or
 * more; chunk_stride_bytes, an internal offset or frame_stride_bytes that is
 * no multiple of the pixel size, or device_chunks or device_frames not
 * aligned to it; internal[k] + tile_rows * tile_cols * pixel size >
 * chunk_stride_bytes; base[k] + n_tiles > n_chunks; frame_stride_bytes <
 * width * height * pixel size; a NULL table with n_chunks != n_slots; a
 * launch grid of 2^31 workgroups or more.
 */
int aqz_chunk_gather_frames_device(int dtype,
                                   uint32_t width,
                                   uint32_t height,
                                   uint32_t tile_rows,
                                   uint32_t tile_cols,
                                   const void* device_chunks,
                                   size_t chunk_stride_bytes,
                                   uint32_t n_slots,
                                   const uint32_t* device_chunk_slot,
                                   uint32_t n_chunks,
                                   const uint32_t* host_frame_chunk_base,
                                   const uint64_t* host_frame_internal_offset_bytes,
                                   uint32_t n_frames,
                                   void* device_frames,
                                   size_t frame_stride_bytes,
                                   uint32_t* device_bad_slot,
                                   void* hip_stream);

/*
 * The inverse of aqz_tile_frame_device and of aqz_ds_take_frame_tiled's
 * layout: one frame from its tiles back to back (tile t at device_tiles +
 * t * tile_rows * tile_cols * pixel size).  The same launcher and kernels as
 * aqz_chunk_gather_frames_device with one frame, base 0, offset 0, a stride
 * of one tile and identity slots; its refusals apply.
 */
int aqz_untile_frame_device(int dtype,
                            const void* device_tiles,
                            uint32_t width,
                            uint32_t height,
                            uint32_t tile_rows,
                            uint32_t tile_cols,
                            void* device_frame,
                            void* hip_stream);

/* Test seams.  Bytes the last aqz_zarr_shard_set_append_layer on `set`
 * copied from device to host (segment table + segments). */
uint64_t aqz_debug_zarr_shard_d2h_bytes(const aqz_zarr_shard_set* set);

/* Seeds the running file offsets from host_offsets[n_shards] (queued on
 * `hip_stream`; returns when they are on the device), so that a test can
 * cross 2^32 without appending 4 GiB. */
int aqz_debug_zarr_shard_set_file_offsets(aqz_zarr_shard_set* set,
                                          const uint64_t* host_offsets,
                                          void* hip_stream);

/*
 * The pack step alone, for A/B timing (tools/zarr_shard_bench.py): copies
 * the frames to where the set's LAST append_layer_device placed them, so
 * sizes, has_data and stride must be that call's.  piece_bytes > 0: the
 * product's pack kernel with that piece (a multiple of 16) and cache policy
 * `policy` (0 plain, 1 nontemporal loads and stores).  piece_bytes == 0: the
 * one-workgroup-per-frame kernel of aqz_blosc_lz4_compress_device on the
 * caller's device_offsets[c] (bytes from device_out; device_frame_bytes
 * required, has_data ignored).
 */
int aqz_debug_zarr_shard_pack_device(aqz_zarr_shard_set* set,
                                     const void* device_frames,
                                     size_t frame_stride,
                                     const uint32_t* device_frame_bytes,
                                     const uint8_t* device_has_data,
                                     void* device_out,
                                     const uint64_t* device_segments,
                                     uint32_t piece_bytes,
                                     int policy,
                                     const uint64_t* device_offsets,
                                     void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif
