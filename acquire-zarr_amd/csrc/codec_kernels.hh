// codec_kernels.hh — launchers for the blosc filter and crc32c kernels
// (codec_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace aqz {

// blosc_c's filter step on `n_buffers` buffers of `nbytes` each, back to
// back: every `blocksize` block (the last one shorter) byte-shuffled
// (shuffle 1, typesize > 1), bit-shuffled (2, block >= typesize) or copied.
hipError_t launch_blosc_filter(int shuffle,
                               uint32_t typesize,
                               uint32_t blocksize,
                               const void* src,
                               uint64_t nbytes,
                               uint32_t n_buffers,
                               void* dst,
                               hipStream_t stream);

// CRC-32C of `n_buffers` buffers of `nbytes`, buffer k at k * stride.
hipError_t launch_crc32c(const void* data,
                         uint64_t nbytes,
                         uint64_t stride,
                         uint32_t n_buffers,
                         uint32_t* crcs,
                         hipStream_t stream);

// ---- blosc+LZ4 frames on the device (aqz_blosc_lz4_frames_device) ----------

// Rows (csize, need) a chunk has: `nsplits` per full block, one for the
// short leftover block.
uint32_t lz4_rows_per_chunk(uint64_t nbytes, uint32_t blocksize, uint32_t nsplits);

// LZ4_compress_fast(split, slot, len, len, accel) for every split of
// `n_buffers` filtered chunks (lz4_block.hh states the encoder): one wave per
// split, its slot the split's own bytes of `comp` (laid out like `filtered`),
// its row (uint32 csize, uint32 need) in `rows`; csize 0 when need > len.
// `serial_probe`: one table probe at a time instead of 64 (A/B form).
hipError_t launch_lz4_splits(const void* filtered,
                             void* comp,
                             void* rows,
                             uint64_t nbytes,
                             uint32_t n_buffers,
                             uint32_t blocksize,
                             uint32_t nsplits,
                             int accel,
                             bool serial_probe,
                             hipStream_t stream);

struct BloscFrameLayout
{
    uint64_t nbytes;
    uint64_t dst_stride; // >= nbytes + 16
    uint32_t blocksize;  // compute_blocksize
    uint32_t nsplits;    // splits of a full block: typesize or 1
    uint32_t rows_per;   // lz4_rows_per_chunk
    uint8_t flags;       // header_flags, without the memcpy bit
    uint8_t typesize;
    bool memcpy_only;    // clevel 0 or nbytes < 128: no rows are read
};

// The c-blosc frame of every chunk from its rows, slots and filtered bytes
// (blocks_frame's walk), or the memcpy frame from `src` where c-blosc falls
// back to it: frame k at dst + k * dst_stride, its size in sizes[k].
hipError_t launch_blosc_frames(const void* src,
                               const void* filtered,
                               const void* comp,
                               const void* rows,
                               void* dst,
                               uint32_t* sizes,
                               uint32_t n_buffers,
                               const BloscFrameLayout& layout,
                               hipStream_t stream);

// Frame k (sizes[k] bytes) from frames + k * stride to packed + offsets[k].
hipError_t launch_pack_frames(const void* frames,
                              uint64_t stride,
                              const uint32_t* sizes,
                              const uint64_t* offsets,
                              void* packed,
                              uint32_t n_buffers,
                              hipStream_t stream);

// ---- reading the frames back (aqz_blosc_lz4_decompress_device) --------------

// blosc_d's unfilter step, the inverse of launch_blosc_filter with the same
// block rules: buffer k from src + k * src_stride to dst + k * dst_stride.
// `meta` null: every buffer has `shuffle` and `blocksize`.  Else buffer k
// takes them from the pair meta[2k] (1 byte shuffle, 2 bit shuffle, 0: the
// buffer is left alone) and meta[2k + 1], as launch_blosc_decode writes them.
hipError_t launch_blosc_unfilter(int shuffle,
                                 uint32_t typesize,
                                 uint32_t blocksize,
                                 const void* src,
                                 uint64_t src_stride,
                                 uint32_t nbytes,
                                 uint32_t n_buffers,
                                 void* dst,
                                 uint64_t dst_stride,
                                 const uint32_t* meta,
                                 hipStream_t stream);

// LZ4_decompress_safe(split k, out k, csize[k], cap[k]) for `n_splits` blocks,
// one wave each (blosc_decode.hh states the decoder): block k is
// comp[comp_offsets[k], + csize[k]), its output goes to out + out_offsets[k],
// results[k] is the decoded size or the lz4::DecodeError.
hipError_t launch_lz4_decode_blocks(const void* comp,
                                    const uint64_t* comp_offsets,
                                    const uint32_t* csize,
                                    void* out,
                                    const uint64_t* out_offsets,
                                    const uint32_t* cap,
                                    int32_t* results,
                                    uint32_t n_splits,
                                    hipStream_t stream);

struct BloscDecodeCall
{
    // strided form: frame k at frames + k * frame_stride, its size in
    // frame_bytes[k] (null: from the header)
    const uint8_t* frames;
    uint64_t frame_stride;
    const uint32_t* frame_bytes;
    // shard form (table non-null): (offset, extent) pair k; frames = the
    // shard's bytes, frame_stride = their count, base = their file offset
    const uint8_t* table;
    uint64_t base;
    uint8_t* dst; // chunk k at dst + k * dst_stride
    uint64_t dst_stride;
    uint8_t* scratch; // n_frames * nbytes: the filtered chunks
    uint32_t* meta;   // n_frames pairs for launch_blosc_unfilter
    uint32_t* status; // blosc::Status per frame
    uint32_t typesize;
    uint32_t nbytes;
};

// Header parse, split decode, raw-split and memcpy copies (one kernel, a
// fixed number of waves per frame walking its splits), then the per-frame
// unfilter.  Nothing is read back: the geometry follows from typesize, nbytes
// and n_frames.
hipError_t launch_blosc_decode(const BloscDecodeCall& call, uint32_t n_frames,
                               hipStream_t stream);

} // namespace aqz
