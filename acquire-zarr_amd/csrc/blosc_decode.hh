// blosc_decode.hh — reading c-blosc 1.x LZ4 chunk frames back, stated once for
// host and device (include/aqz_blosc.h: aqz_blosc_lz4_decompress_device,
// include/aqz_shard.h: aqz_zarr_shard_decompress_device).
//
// Three serial pieces, each safe on any input:
//  * lz4::decode_block: the LZ4 block format's decoder;
//  * blosc::parse_header / blosc::locate_split: the frame walker, the mirror
//    of blocks_frame / write_frame in blosc_frame.cpp (and of blosc_d in
//    c-blosc 1.21): header, block starts, the split rule, per-split sizes;
//  * blosc::unfilter_serial: the inverse of the byte / bit shuffle, block by
//    block, with the forward filter's block rules (codec_kernels.hip).
// The wave-cooperative decoder and the unfilter kernels in codec_kernels.hip
// share the walker and the sequence parser below and must give these bytes and
// these statuses.
#pragma once

#include "lz4_block.hh"

#include <cstdint>

namespace aqz {
namespace lz4 {

// What decode_block returns instead of a size.
enum DecodeError : int32_t
{
    kDecEmpty = -1,          // n == 0 (LZ4_decompress_safe: -1)
    kDecTruncated = -2,      // the input ends inside a length or before an offset's two bytes
    kDecLiteralsInput = -3,  // a literal run past src + n
    kDecLiteralsOutput = -4, // a literal run past dst + cap
    kDecOffsetZero = -5,
    kDecOffsetBefore = -6,   // an offset past the output so far
    kDecMatchOutput = -7,    // a match past dst + cap
    kDecEndsInMatch = -8,    // the input ends right after a match: no last literals
};

// A run length: the token's nibble, and after a nibble of 15 bytes that add
// up until one is not 255.  `rd(i)` reads input byte i < n.
template<class R>
AQZ_LZ4_HD inline int32_t
read_run(R& rd, uint32_t& ip, uint32_t n, uint32_t nibble, uint64_t& len)
{
    len = nibble;
    if (nibble == 15) {
        for (;;) {
            if (ip >= n)
                return kDecTruncated;
            const uint32_t x = rd(ip++);
            len += x;
            if (x != 255)
                break;
        }
    }
    return 0;
}

// Any LZ4 block with offsets 1..65,535 (not only what encode_block emits)
// from src[0, n) into dst[0, cap): the decoded size, or a DecodeError.  Reads
// nothing outside [src, src + n), writes nothing outside [dst, dst + cap),
// reads no match source before dst.
//
// Acceptance follows LZ4_decompress_safe (liblz4 1.9.3) on every block an
// encoder may write.  Where the library's answer depends on something other
// than the block, the choices here are:
//  * the library turns down a block whose last match ends less than 5 bytes,
//    or whose last-but-one literal run ends less than 12 bytes, before
//    dst + cap — a test against the capacity, not the block, which passes
//    with a roomier destination.  Those are the encoder's end-of-block rules
//    (kLastLiterals, kMfLimit); the format does not need them to decode, so
//    such blocks are accepted here at every capacity;
//  * offset 0 is an error here; the library copies unwritten bytes;
//  * the match nibble of the last token (literals only) is ignored, as there;
//  * n == 0 is an error, as there; the one-byte block {0x00} decodes to
//    nothing at every capacity (the library wants cap == 0 for it).
AQZ_LZ4_HD inline int32_t
decode_block(const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t cap)
{
    if (n == 0)
        return kDecEmpty;
    if (cap > 0x7FFFFFFFu)
        cap = 0x7FFFFFFFu;
    auto rd = [src](uint32_t i) { return uint32_t(src[i]); };
    uint32_t ip = 0, op = 0;
    for (;;) {
        const uint32_t token = src[ip++];
        uint64_t lit;
        if (const int32_t e = read_run(rd, ip, n, token >> 4, lit))
            return e;
        if (lit > n - ip)
            return kDecLiteralsInput;
        if (lit > cap - op)
            return kDecLiteralsOutput;
        for (uint32_t i = 0; i < uint32_t(lit); ++i)
            dst[op + i] = src[ip + i];
        ip += uint32_t(lit);
        op += uint32_t(lit);
        if (ip == n)
            return int32_t(op); // the last sequence is literals only
        if (n - ip < 2)
            return kDecTruncated;
        const uint32_t off = uint32_t(src[ip]) | (uint32_t(src[ip + 1]) << 8);
        ip += 2;
        uint64_t ml;
        if (const int32_t e = read_run(rd, ip, n, token & 15, ml))
            return e;
        ml += 4;
        if (off == 0)
            return kDecOffsetZero;
        if (off > op)
            return kDecOffsetBefore;
        if (ml > cap - op)
            return kDecMatchOutput;
        // byte by byte, front to back: an overlapping match (off < ml) reads
        // what it has just written
        for (uint32_t i = 0; i < uint32_t(ml); ++i)
            dst[op + i] = dst[op - off + i];
        op += uint32_t(ml);
        if (ip >= n)
            return kDecEndsInMatch;
    }
}

} // namespace lz4

namespace blosc {

// Per-frame status of the decompress calls (AQZ_BLOSC_FRAME_* in
// include/aqz_blosc.h), in the order of detection.
enum Status : uint32_t
{
    kOk = 0,
    kAbsent = 1,
    kBadHeader = 2,
    kUnsupported = 3,
    kCorrupt = 4,
};

constexpr uint32_t kHeaderBytes = 16;   // BLOSC_MAX_OVERHEAD
constexpr uint32_t kMaxSplits = 16;     // MAX_SPLITS
constexpr uint32_t kMinSplitElems = 128; // MIN_BUFFERSIZE
constexpr uint32_t kLz4Format = 1;      // BLOSC_LZ4_FORMAT
constexpr uint32_t kMaxBuffer = 0x7FFFFFFFu - kHeaderBytes; // BLOSC_MAX_BUFFERSIZE
constexpr uint64_t kSentinel = ~0ull;   // AQZ_ZARR_SHARD_SENTINEL

enum Filter : uint32_t
{
    kNoFilter = 0,
    kByteShuffle = 1,
    kBitShuffle = 2,
};

struct FrameInfo
{
    // the 16 header bytes
    uint8_t version, versionlz, flags, typesize;
    uint32_t nbytes, blocksize, cbytes;
    // what follows from them; meaningful when parse_header gave kOk
    bool memcpyed;        // flags & 0x2: the chunk itself after the header
    uint32_t filter;      // Filter: what the stored blocks went through
    uint32_t nsplits;     // splits of a full block: typesize or 1
    uint32_t full_blocks; // nbytes / blocksize
    uint32_t leftover;    // nbytes % blocksize, one more block of one split
    uint32_t nblocks;
    uint32_t total_splits;
};

// Where chunk k's frame lies.  Strided form: frames + k * stride with its
// size from the table (a size above the stride counts as the stride), or,
// without a table, from the header's cbytes bounded by the stride.
struct FrameSpan
{
    uint64_t offset; // from the base pointer
    uint64_t extent;
};

AQZ_LZ4_HD inline Status
span_strided(const uint8_t* frames, uint64_t stride, const uint32_t* sizes, uint32_t k,
             FrameSpan* out)
{
    out->offset = uint64_t(k) * stride;
    if (sizes) {
        out->extent = sizes[k] < stride ? sizes[k] : stride;
        return kOk;
    }
    out->extent = 0;
    if (stride < kHeaderBytes)
        return kBadHeader;
    const uint32_t cbytes = lz4::read32(frames + out->offset + 12);
    if (cbytes < kHeaderBytes || cbytes > stride)
        return kBadHeader;
    out->extent = cbytes;
    return kOk;
}

// Shard form: the (offset, extent) pair i of an index table; offsets are file
// offsets, the shard's bytes start at file offset `base`.
AQZ_LZ4_HD inline Status
span_shard(const uint8_t* table, uint32_t i, uint64_t shard_bytes, uint64_t base, FrameSpan* out)
{
    // tables lie 16 * chunks_per_shard + 4 bytes apart: any alignment
    const uint64_t off = lz4::read64(table + 16 * uint64_t(i));
    const uint64_t ext = lz4::read64(table + 16 * uint64_t(i) + 8);
    out->offset = out->extent = 0;
    if (off == kSentinel && ext == kSentinel)
        return kAbsent;
    if (off < base || off - base > shard_bytes || ext > shard_bytes - (off - base))
        return kCorrupt;
    out->offset = off - base;
    out->extent = ext;
    return kOk;
}

// The header of the frame f[0, extent) against the caller's typesize and
// nbytes (typesize 0 / nbytes 0: whatever the header says).  Every field is
// checked against `extent` before anything uses it; *fi is filled as far as
// the extent allows.
AQZ_LZ4_HD inline Status
parse_header(const uint8_t* f, uint64_t extent, uint32_t typesize, uint32_t nbytes, FrameInfo* fi)
{
    *fi = FrameInfo{};
    if (extent < kHeaderBytes)
        return kBadHeader; // truncated header
    fi->version = f[0];
    fi->versionlz = f[1];
    fi->flags = f[2];
    fi->typesize = f[3];
    fi->nbytes = lz4::read32(f + 4);
    fi->blocksize = lz4::read32(f + 8);
    fi->cbytes = lz4::read32(f + 12);
    if (typesize > 255)
        typesize = 1; // as c-blosc writes it
    if (fi->version != 2 || fi->typesize == 0 || (typesize && fi->typesize != typesize) ||
        (nbytes && fi->nbytes != nbytes) || fi->nbytes == 0 || fi->nbytes > kMaxBuffer ||
        fi->cbytes != extent || fi->blocksize == 0 || fi->blocksize > fi->nbytes)
        return kBadHeader;
    const uint32_t ts = fi->typesize, bs = fi->blocksize;
    fi->memcpyed = (fi->flags & 0x2) != 0;
    fi->filter = ((fi->flags & 0x1) && ts > 1) ? kByteShuffle
                 : (fi->flags & 0x4)           ? kBitShuffle
                                               : kNoFilter;
    // blosc_d's split rule: 0x10 clear, typesize <= 16, at least 128 elements
    // a block; never the leftover block
    const bool split = !(fi->flags & 0x10) && ts <= kMaxSplits && bs / ts >= kMinSplitElems;
    fi->nsplits = split ? ts : 1;
    fi->full_blocks = fi->nbytes / bs;
    fi->leftover = fi->nbytes % bs;
    fi->nblocks = fi->full_blocks + (fi->leftover ? 1 : 0);
    fi->total_splits = fi->full_blocks * fi->nsplits + (fi->leftover ? 1 : 0);
    if (fi->memcpyed) // takes precedence over the codec bits
        return fi->cbytes == uint64_t(fi->nbytes) + kHeaderBytes ? kOk : kBadHeader;
    if (split && bs % ts)
        return kBadHeader; // a split block's streams would not cover it
    if ((fi->flags >> 5) != kLz4Format || fi->versionlz != 1)
        return kUnsupported;
    if (kHeaderBytes + 4 * uint64_t(fi->nblocks) > extent)
        return kCorrupt; // the block starts leave the frame
    return kOk;
}

// Split s (0 .. total_splits - 1, block after block) of a frame parse_header
// accepted: where its payload lies in the frame, its stored size, the size
// it decodes to and where that goes in the (filtered) chunk.  csize == neb: the
// payload is the split itself, stored raw.  Walks the block's sizes up to
// the split and checks each against the block and the frame.
struct SplitRef
{
    uint64_t src;
    uint32_t csize;
    uint32_t neb;
    uint64_t dst;
};

AQZ_LZ4_HD inline Status
locate_split(const FrameInfo& fi, const uint8_t* f, uint64_t extent, uint32_t s, SplitRef* out)
{
    uint32_t b, j, bsize, nsp;
    if (s < fi.full_blocks * fi.nsplits) {
        b = s / fi.nsplits;
        j = s % fi.nsplits;
        bsize = fi.blocksize;
        nsp = fi.nsplits;
    } else {
        b = fi.full_blocks;
        j = 0;
        bsize = fi.leftover;
        nsp = 1;
    }
    const uint32_t neb = bsize / nsp;
    const uint64_t table_end = kHeaderBytes + 4 * uint64_t(fi.nblocks);
    const uint32_t bstart = lz4::read32(f + kHeaderBytes + 4 * uint64_t(b));
    if (bstart > 0x7FFFFFFFu || bstart < table_end || bstart > extent)
        return kCorrupt;
    uint64_t p = bstart;
    for (uint32_t i = 0;; ++i) {
        if (extent - p < 4)
            return kCorrupt;
        const uint32_t c = lz4::read32(f + p);
        p += 4;
        if (c == 0 || c > 0x7FFFFFFFu || c > neb || c > extent - p)
            return kCorrupt;
        if (i == j) {
            out->src = p;
            out->csize = c;
            out->neb = neb;
            out->dst = uint64_t(b) * fi.blocksize + uint64_t(j) * neb;
            return kOk;
        }
        p += c;
    }
}

// How one block of `bsize` bytes was filtered: the forward rules.  A byte
// shuffle needs typesize > 1; a bit shuffle needs a whole element and an
// element count that is a multiple of 8; everything else was copied.
AQZ_LZ4_HD inline uint32_t
block_filter(uint32_t filter, uint32_t ts, uint32_t bsize)
{
    if (filter == kByteShuffle)
        return ts > 1 ? kByteShuffle : kNoFilter;
    if (filter == kBitShuffle)
        return (bsize >= ts && (bsize / ts) % 8 == 0) ? kBitShuffle : kNoFilter;
    return kNoFilter;
}

// One block back: elements from their byte planes or bit rows, the
// blocksize % typesize tail copied.
AQZ_LZ4_HD inline void
unfilter_block_serial(uint32_t filter, uint32_t ts, uint32_t bsize, const uint8_t* src,
                      uint8_t* dst)
{
    const uint32_t kind = block_filter(filter, ts, bsize);
    const uint32_t ne = kind == kNoFilter ? 0 : bsize / ts;
    if (kind == kByteShuffle) {
        for (uint32_t i = 0; i < ne; ++i)
            for (uint32_t j = 0; j < ts; ++j)
                dst[uint64_t(i) * ts + j] = src[uint64_t(j) * ne + i];
    } else if (kind == kBitShuffle) {
        const uint32_t row = ne / 8;
        for (uint32_t i = 0; i < ne; ++i)
            for (uint32_t j = 0; j < ts; ++j) {
                uint32_t v = 0;
                for (uint32_t b = 0; b < 8; ++b)
                    v |= ((uint32_t(src[uint64_t(j * 8 + b) * row + i / 8]) >> (i % 8)) & 1u) << b;
                dst[uint64_t(i) * ts + j] = uint8_t(v);
            }
    }
    for (uint64_t o = uint64_t(ne) * ts; o < bsize; ++o)
        dst[o] = src[o];
}

AQZ_LZ4_HD inline void
unfilter_serial(uint32_t filter, uint32_t ts, uint32_t blocksize, const uint8_t* src,
                uint64_t nbytes, uint8_t* dst)
{
    for (uint64_t off = 0; off < nbytes; off += blocksize) {
        const uint32_t bs = uint32_t(nbytes - off < blocksize ? nbytes - off : blocksize);
        unfilter_block_serial(filter, ts, bs, src + off, dst + off);
    }
}

// A whole frame f[0, extent) into dst[0, nbytes): walker, serial decoder and
// unfilter.  `scratch` holds nbytes (the filtered chunk; unused for frames
// without a filter).  A frame that is not kOk leaves dst unspecified.
AQZ_LZ4_HD inline Status
decode_frame_serial(const uint8_t* f, uint64_t extent, uint32_t typesize, uint32_t nbytes,
                    uint8_t* dst, uint8_t* scratch, FrameInfo* fi)
{
    const Status st = parse_header(f, extent, typesize, nbytes, fi);
    if (st != kOk)
        return st;
    if (fi->memcpyed) {
        for (uint32_t i = 0; i < fi->nbytes; ++i)
            dst[i] = f[kHeaderBytes + i];
        return kOk;
    }
    uint8_t* out = fi->filter == kNoFilter ? dst : scratch;
    for (uint32_t s = 0; s < fi->total_splits; ++s) {
        SplitRef r;
        if (locate_split(*fi, f, extent, s, &r) != kOk)
            return kCorrupt;
        if (r.csize == r.neb) {
            for (uint32_t i = 0; i < r.neb; ++i)
                out[r.dst + i] = f[r.src + i];
        } else if (lz4::decode_block(f + r.src, r.csize, out + r.dst, r.neb) != int32_t(r.neb)) {
            return kCorrupt;
        }
    }
    if (fi->filter != kNoFilter)
        unfilter_serial(fi->filter, fi->typesize, fi->blocksize, scratch, fi->nbytes, dst);
    return kOk;
}

} // namespace blosc
} // namespace aqz
