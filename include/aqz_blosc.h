/*
 * aqz_blosc.h — c-blosc 1.x chunk frames around the GPU byte/bit shuffle
 * (widened to the whole call it feeds).  Same library
 * (libaqz_downsampler.so) and status codes as aqz_downsampler.h.
 *
 * The reference compresses every chunk buffer with
 *   blosc_compress_ctx(clevel, shuffle, typesize = bytes_of_type, nbytes,
 *                      src, dest, destsize = nbytes + BLOSC_MAX_OVERHEAD,
 *                      cname = "lz4" | "zstd", blocksize = 0, nthreads = 1)
 * in compress_in_place (zarr.common.cpp:106-137), called per chunk from
 * Chunk::compress_and_take_buffer (chunk.cpp:78-105); the codec names come
 * from blosc.compression.params.cpp:5-13 and zarr.stream.cpp:115-118.
 *
 * Here the filter stage (the HBM-bound part) runs on the GPU
 * (aqz_blosc_filter_device) and the entropy coder stays on the host: LZ4
 * (LZ4_compress_fast) or zstd (ZSTD_compress), from the same shared
 * libraries c-blosc links (see aqz_blosc_codec_info).  The frames are
 * byte-identical to c-blosc 1.21's: header, block starts, per-split
 * compressed sizes, raw splits for incompressible ones, and the whole-buffer
 * memcpy fallback.  tests/test_blosc_frames.py checks that against the
 * image's libblosc 1.21.0 itself.
 */
#ifndef AQZ_BLOSC_H
#define AQZ_BLOSC_H

#include "aqz_codec.h"

#ifdef __cplusplus
extern "C"
{
#endif

/* BLOSC_MAX_OVERHEAD: the frame header; a destination of nbytes + this
 * always fits (the memcpy fallback). */
#define AQZ_BLOSC_MAX_OVERHEAD 16

/*
 * The block size blosc_compress_ctx picks for (clevel, typesize, nbytes,
 * cname) with blocksize = 0 — c-blosc's compute_blocksize, the value
 * aqz_blosc_filter_device needs.  typesize > 255 counts as 1, as in c-blosc.
 * AQZ_INVALID_ARGUMENT for clevel outside 0..9, typesize 0, an unknown
 * cname (only "lz4" and "zstd", the reference's two) or a null pointer.
 */
int aqz_blosc_blocksize(int clevel,
                        uint32_t typesize,
                        size_t nbytes,
                        const char* cname,
                        uint32_t* blocksize);

/*
 * Host frame writer.  `filtered` holds the `nbytes` chunk already filtered
 * block by block (aqz_blosc_filter_device with aqz_blosc_blocksize's block
 * size, copied to host).  Writes the c-blosc frame blosc_compress_ctx would
 * write for the unfiltered chunk into dest[0, destsize) and sets
 * *frame_bytes (0: it does not fit, c-blosc's return value 0).
 * When c-blosc would store the chunk unfiltered (clevel 0, nbytes < 128, or
 * incompressible as a whole) the frame is the 16-byte header plus the raw
 * chunk: `src` (host, may be NULL) supplies it; with `src` NULL only the
 * header is written, *raw_needed is set to 1 and the caller copies the
 * nbytes raw bytes to dest + 16 itself (e.g. straight from the device).
 * `raw_needed` may be NULL when `src` is given.
 */
int aqz_blosc_frame_from_filtered(int clevel,
                                  int shuffle,
                                  uint32_t typesize,
                                  const char* cname,
                                  const void* filtered,
                                  const void* src,
                                  size_t nbytes,
                                  void* dest,
                                  size_t destsize,
                                  size_t* frame_bytes,
                                  int* raw_needed);

/* Device scratch, pinned staging and host worker threads for
 * aqz_blosc_compress_device.  n_threads 0: min(16, hardware threads).
 * A ctx serves one call at a time: its scratch is shared by every call on
 * it, so two threads must not use one ctx concurrently (one ctx per thread,
 * as the reference's compression jobs would hold one each).  The ctx orders
 * nothing itself: calls queued on one stream follow each other by stream
 * order, and a caller that queues aqz_blosc_lz4_frames_device on a second
 * stream while a call on the first may still run must order the two itself
 * (an event recorded behind the first call and waited for by the second
 * stream). */
typedef struct aqz_blosc_ctx aqz_blosc_ctx;

int aqz_blosc_ctx_create(int device, uint32_t n_threads, aqz_blosc_ctx** out);
void aqz_blosc_ctx_destroy(aqz_blosc_ctx* ctx);

/*
 * compress_in_place for `n_buffers` device chunk buffers of `nbytes` each,
 * back to back at `device_src` (e.g. the tiles aqz_ds_run_device_batch_tiled
 * or aqz_ds_take_frame_tiled lay out).  The filter runs on `hip_stream`, the
 * filtered chunks cross PCIe in groups, and host threads compress each group
 * while the next one is in flight.  Frame k is written at
 * host_dst + k * dst_stride (dst_stride >= nbytes + AQZ_BLOSC_MAX_OVERHEAD,
 * so every frame fits, as compress_in_place sizes it) and its size to
 * frame_bytes[k].  Chunks c-blosc would store unfiltered are copied raw from
 * the device.  Returns when every frame is written.
 */
int aqz_blosc_compress_device(aqz_blosc_ctx* ctx,
                              int clevel,
                              int shuffle,
                              uint32_t typesize,
                              const char* cname,
                              const void* device_src,
                              size_t nbytes,
                              uint32_t n_buffers,
                              void* host_dst,
                              size_t dst_stride,
                              size_t* frame_bytes,
                              void* hip_stream);

/*
 * The same lz4 frames with the entropy coder on the device as well: after the
 * filter, one wave per blosc split runs LZ4's fast block encoder
 * (LZ4_compress_fast on a fresh state, acceleration 10 - clevel, restated in
 * csrc/lz4_block.hh) into a slot of the split's own size, and one workgroup
 * per chunk lays out the frame c-blosc would write, raw splits and the
 * whole-chunk memcpy fallback included.  Only "lz4"; zstd stays on the host
 * (aqz_blosc_compress_device).  The frames are byte-identical to that call's.
 *
 * flags: AQZ_LZ4_PROBE_SERIAL makes a search probe the hash table one
 * position at a time; by default (0) the 64 lanes of a wave take the next 64
 * probe positions at once.  Both give the same bytes; any other bit is
 * AQZ_INVALID_ARGUMENT.
 */
#define AQZ_LZ4_PROBE_SERIAL 1u

/* filter + LZ4 + frame, all on hip_stream, no synchronisation: frame k at
 * device_dst + k * dst_stride (dst_stride >= nbytes + 16), its size in
 * device_frame_bytes[k]. lz4 only. Scratch grows inside ctx: only a call
 * that needs more of it than any before (the first, or one of more bytes)
 * frees and reallocates, which waits for the device. */
int aqz_blosc_lz4_frames_device(aqz_blosc_ctx* ctx,
                                int clevel,
                                int shuffle,
                                uint32_t typesize,
                                const void* device_src,
                                size_t nbytes,
                                uint32_t n_buffers,
                                void* device_dst,
                                size_t dst_stride,
                                uint32_t* device_frame_bytes,
                                void* hip_stream,
                                uint32_t flags);

/* same frames delivered like aqz_blosc_compress_device (host_dst, dst_stride,
 * frame_bytes), but only frame bytes and the size table cross PCIe: the
 * frames are packed end to end on the device and copied once.  Returns when
 * every frame is written. */
int aqz_blosc_lz4_compress_device(aqz_blosc_ctx* ctx,
                                  int clevel,
                                  int shuffle,
                                  uint32_t typesize,
                                  const void* device_src,
                                  size_t nbytes,
                                  uint32_t n_buffers,
                                  void* host_dst,
                                  size_t dst_stride,
                                  size_t* frame_bytes,
                                  void* hip_stream,
                                  uint32_t flags);

/* Test seams.  Bytes the last aqz_blosc_lz4_compress_device on `ctx` copied
 * from device to host (size table + packed frames). */
uint64_t aqz_debug_blosc_d2h_bytes(const aqz_blosc_ctx* ctx);

/* The serial encoder of csrc/lz4_block.hh on host memory, no GPU involved:
 * LZ4_compress_fast(src, dst, n, cap, accel) on a fresh state.  Returns the
 * compressed size, 0 when it does not fit into cap, -1 for a bad argument.
 * *need (may be NULL): the capacity the bytes written asked for; the result
 * is non-zero exactly when *need <= cap. */
int aqz_debug_lz4_block_host(const void* src,
                             size_t n,
                             void* dst,
                             size_t cap,
                             int accel,
                             uint32_t* need);

/* The device encoder on raw splits, without filter or frame: `n_splits`
 * splits of `split_bytes` each, back to back at `device_src`, one wave per
 * split on `hip_stream`, no synchronisation.  Split k is encoded into its own
 * range [k * split_bytes, (k + 1) * split_bytes) of `device_comp` (capacity
 * split_bytes, as in a frame) and its row (csize, need) goes to
 * device_rows[2k], device_rows[2k + 1]: csize 0 when need passed split_bytes.
 * `ctx` names the device only; none of its scratch is used.  flags as for
 * aqz_blosc_lz4_frames_device. */
int aqz_debug_lz4_splits_device(aqz_blosc_ctx* ctx,
                                const void* device_src,
                                size_t split_bytes,
                                uint32_t n_splits,
                                int accel,
                                void* device_comp,
                                uint32_t* device_rows,
                                void* hip_stream,
                                uint32_t flags);

/*
 * Reading the frames back on the device: blosc_d for LZ4
 * frames, c-blosc's or the ones above.  csrc/blosc_decode.hh states the
 * frame walk, the LZ4 block decoder and the unfilter serially for host and
 * device; one wave decodes one split.
 *
 * Every frame gets a status, the first of these that applies:
 */
#define AQZ_BLOSC_FRAME_OK 0u          /* decoded */
#define AQZ_BLOSC_FRAME_ABSENT 1u      /* a shard table's sentinel pair: the chunk reads as zeros */
#define AQZ_BLOSC_FRAME_BAD_HEADER 2u  /* fewer than 16 bytes; version not 2; typesize or nbytes  \
                                          not the caller's; blocksize 0, above nbytes, or not a   \
                                          typesize multiple in a split frame; cbytes not the      \
                                          frame's extent (nbytes + 16 for a memcpy frame) */
#define AQZ_BLOSC_FRAME_UNSUPPORTED 3u /* not a memcpy frame, and its codec is not LZ4 (version 1) */
#define AQZ_BLOSC_FRAME_CORRUPT 4u     /* block starts, split sizes or an LZ4 stream out of       \
                                          bounds; a split that decodes to another length; a shard \
                                          table pair outside the shard's bytes */
/* A frame that is neither OK nor ABSENT leaves its chunk's bytes unspecified;
 * nothing outside the chunk's nbytes is written, nothing outside the frame's
 * extent is read. */

/* The 16 header bytes of a frame and what they say about it. */
typedef struct
{
    uint32_t status; /* AQZ_BLOSC_FRAME_*, as far as the header and the block starts decide it */
    uint8_t version, versionlz, flags, typesize;
    uint32_t nbytes, blocksize, cbytes;
    uint32_t memcpyed; /* flags & 0x2: the chunk itself follows the header */
    uint32_t shuffle;  /* AQZ_BLOSC_NOSHUFFLE / SHUFFLE / BITSHUFFLE the blocks went through */
    uint32_t nsplits;  /* streams of a full block: typesize or 1 */
    uint32_t nblocks;
} aqz_blosc_frame_header;

/* Host only, no GPU involved: parses frame[0, extent) against the caller's
 * typesize and nbytes (0: whatever the header says).  AQZ_INVALID_ARGUMENT
 * for a null pointer; a bad frame is reported in out->status, not as an
 * error. */
int aqz_blosc_frame_info(const void* frame,
                         size_t extent,
                         uint32_t typesize,
                         size_t nbytes,
                         aqz_blosc_frame_header* out);

/*
 * blosc_d's unfilter step, the inverse of aqz_blosc_filter_device with the
 * same block rules: `n_buffers` buffers of `nbytes` each (at most 2^31 - 1),
 * back to back, every `blocksize` block byte-unshuffled (shuffle 1, typesize >
 * 1), bit-unshuffled (2, a whole element and a multiple of 8 of them) or
 * copied, the blocksize % typesize tail copied.  Not in place.  Asynchronous
 * on `hip_stream`.
 */
int aqz_blosc_unfilter_device(int shuffle,
                              uint32_t typesize,
                              uint32_t blocksize,
                              const void* device_src,
                              size_t nbytes,
                              uint32_t n_buffers,
                              void* device_dst,
                              void* hip_stream);

/*
 * `n_frames` LZ4 frames back into chunks of `nbytes` (typesize > 255 counts
 * as 1, as for the writers).  Frame k lies at device_frames + k * frame_stride
 * and is device_frame_bytes[k] long, the uint32 table
 * aqz_blosc_lz4_frames_device writes (a size above frame_stride counts as
 * frame_stride); NULL: the size is the header's cbytes, which must fit into
 * frame_stride.  Chunk k goes to device_dst + k * dst_stride, its status to
 * device_status[k].
 *
 * Header fields are read on the device only; the launch geometry follows
 * from typesize, nbytes and n_frames.  Everything is queued on `hip_stream`;
 * the call never synchronises.  The filtered chunks pass through scratch
 * inside ctx: only a call that needs more of it than any before frees and
 * reallocates, which waits for the device.  Frames without a filter and
 * memcpy frames are written straight to device_dst.
 *
 * AQZ_INVALID_ARGUMENT before anything is queued: a null ctx or pointer
 * (device_frame_bytes may be NULL), typesize, nbytes or n_frames 0,
 * dst_stride < nbytes, nbytes above BLOSC_MAX_BUFFERSIZE (2^31 - 17).
 */
int aqz_blosc_lz4_decompress_device(aqz_blosc_ctx* ctx,
                                    uint32_t typesize,
                                    size_t nbytes,
                                    const void* device_frames,
                                    size_t frame_stride,
                                    const uint32_t* device_frame_bytes,
                                    uint32_t n_frames,
                                    void* device_dst,
                                    size_t dst_stride,
                                    uint32_t* device_status,
                                    void* hip_stream);

/* Test seams, host only.  lz4::decode_block of csrc/blosc_decode.hh:
 * LZ4_decompress_safe(src, dst, n, cap), the decoded size or a negative
 * error (-1 empty input, -2 truncated, -3 / -4 literals past the input / the
 * output, -5 offset 0, -6 offset before the output, -7 match past the output,
 * -8 the block ends in a match; -100 for a bad argument). */
int aqz_debug_lz4_decode_host(const void* src, size_t n, void* dst, size_t cap);

/* A whole frame through the walker, the serial decoder and a host unfilter:
 * frame[0, extent) into dst[0, nbytes), *status as the device call gives it. */
int aqz_debug_blosc_decode_host(const void* frame,
                                size_t extent,
                                uint32_t typesize,
                                size_t nbytes,
                                void* dst,
                                uint32_t* status);

/* The device decoder on bare LZ4 blocks, without frame or unfilter: block k
 * is device_comp[comp_offsets[k], + csize[k]), one wave decodes it into
 * device_out + out_offsets[k] with capacity device_cap[k], results[k] is the decoded
 * size or the error aqz_debug_lz4_decode_host names.  All arrays are device
 * memory; queued on `hip_stream`, no synchronisation; `ctx` names the device
 * only. */
int aqz_debug_lz4_decode_blocks_device(aqz_blosc_ctx* ctx,
                                       const void* device_comp,
                                       const uint64_t* device_comp_offsets,
                                       const uint32_t* device_csize,
                                       void* device_out,
                                       const uint64_t* device_out_offsets,
                                       const uint32_t* device_cap,
                                       int32_t* device_results,
                                       uint32_t n_blocks,
                                       void* hip_stream);

/* Which LZ4 and zstd libraries the frame writer loaded, with versions
 * ("" entries for a codec that failed to load).  $AQZ_LZ4_LIB and
 * $AQZ_ZSTD_LIB name them explicitly. */
const char* aqz_blosc_codec_info(void);

#ifdef __cplusplus
}
#endif

#endif
