// lz4_block.hh — the LZ4 block format's fast encoder, restated serially for
// host and device (include/aqz_blosc.h: aqz_blosc_lz4_frames_device).
//
// c-blosc hands every split of a chunk to LZ4_compress_fast(src, dst, n, cap,
// 10 - clevel) (the reference reaches it through blosc_compress_ctx,
// zarr.common.cpp:106-137, chunk.cpp:78-105).  This file states what that call
// writes on a fresh state, without a dictionary, on a 64-bit little-endian
// machine, from the published block format and the observable behaviour of
// liblz4 1.9.3 (tests/test_lz4_block.py sweeps it against the library byte
// for byte).  The wave-cooperative kernel in codec_kernels.hip must produce
// these bytes; it shares the constants and hashes below.
//
//  * table: 16 KiB, all zero at the start (an empty entry is position 0, a
//    legitimate candidate).  n < 65547: u16 positions under a 13-bit hash of
//    four bytes; else u32 positions under a 12-bit hash of five bytes, and a
//    candidate further than 65535 behind is skipped.
//  * search: probe p, then p + step, with step = nb++ >> 6 and nb starting at
//    accel << 6 (the first step is 1); every probe stores its position.  The
//    search ends once the next probe would pass end - 11.
//  * after a match: extend backwards to the anchor, emit literals, offset,
//    match length (counted up to end - 5); store ip - 2, then test ip itself
//    before searching again from ip + 1.
//  * limited output: the encoder gives up before a write that could pass
//    dst + cap at three points; the parse never depends on cap, so it records
//    `need`, the largest such bound met, and succeeds exactly for cap >= need.
//    It stops at the first bound above cap.
//
// Unlike the library the encoder copies exact lengths: it reads nothing past
// src + n and writes nothing past dst + cap.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AQZ_LZ4_HD __host__ __device__
#else
#define AQZ_LZ4_HD
#endif

namespace aqz {
namespace lz4 {

constexpr uint32_t kTableBytes = 16 * 1024;
constexpr uint32_t kU16Limit = 65547;   // n below this: u16 table
constexpr uint32_t kMinInput = 13;      // shorter inputs are literals only
constexpr uint32_t kMfLimit = 11;       // no probe whose successor passes end - 11
constexpr uint32_t kLastLiterals = 5;   // matches stop at end - 5
constexpr uint32_t kMaxDistance = 65535;
constexpr uint32_t kSkipTrigger = 6;
constexpr int kAccelMax = 65537;

AQZ_LZ4_HD inline uint32_t
read32(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

AQZ_LZ4_HD inline uint64_t
read64(const uint8_t* p)
{
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

AQZ_LZ4_HD inline uint32_t
hash4(uint32_t v)
{
    return (v * 2654435761u) >> 19; // 13 bits
}

AQZ_LZ4_HD inline uint32_t
hash5(uint64_t v)
{
    return uint32_t(((v << 24) * 889523592379ull) >> 52); // 12 bits
}

AQZ_LZ4_HD inline int
clamp_accel(int accel)
{
    return accel < 1 ? 1 : (accel > kAccelMax ? kAccelMax : accel);
}

// Bytes a literal run of `lit` may need before its match is known, the
// bytes after an offset for a match of 4 + `count`, and the bytes of the last
// run: the three limited-output bounds, each added to the output position
// they are taken at.
AQZ_LZ4_HD inline uint64_t
bound_literals(uint64_t lit)
{
    return 1 + lit + 8 + lit / 255;
}

AQZ_LZ4_HD inline uint64_t
bound_match(uint64_t count)
{
    return 6 + (count + 240) / 255;
}

AQZ_LZ4_HD inline uint64_t
bound_last(uint64_t last)
{
    return last + 1 + (last + 240) / 255;
}

// The table under either form; `T` is uint16_t or uint32_t.
template<typename T>
struct Table
{
    T* slot; // kTableBytes / sizeof(T) entries

    AQZ_LZ4_HD uint32_t hash(const uint8_t* p) const
    {
        if constexpr (sizeof(T) == 2)
            return hash4(read32(p));
        else
            return hash5(read64(p));
    }
    // whether a candidate may be used from position p
    AQZ_LZ4_HD static bool near(uint32_t cand, uint32_t p)
    {
        if constexpr (sizeof(T) == 2)
            return true;
        else
            return cand + kMaxDistance >= p;
    }
};

// Run-length bytes after a token nibble of 15: (len - 15) as 255s and a rest.
AQZ_LZ4_HD inline uint32_t
put_length(uint8_t* op, uint32_t len)
{
    uint32_t k = 0;
    for (len -= 15; len >= 255; len -= 255)
        op[k++] = 255;
    op[k++] = uint8_t(len);
    return k;
}

// One block.  Returns the compressed size, or 0 when it needs more than
// `cap`; *need (may be null) is the capacity the bytes written so far asked
// for: the whole block's when the result is non-zero, else the first bound
// above cap.  `table` is kTableBytes of scratch, cleared here.
template<typename T>
AQZ_LZ4_HD inline uint32_t
encode_block_with(const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t cap, int accel,
                  T* table_mem, uint32_t* need_out)
{
    Table<T> tab{ table_mem };
    for (uint32_t i = 0; i < kTableBytes / sizeof(T); ++i)
        tab.slot[i] = 0;
    accel = clamp_accel(accel);
    uint64_t need = 0;
    uint32_t op = 0, anchor = 0, ip = 0;
    auto over = [&](uint64_t x) {
        if (x > need)
            need = x;
        return x > cap;
    };
    auto fail = [&]() -> uint32_t {
        if (need_out)
            *need_out = need > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(need);
        return 0;
    };
    if (n >= kMinInput) {
        const uint32_t mflimit1 = n - kMfLimit;
        const uint32_t matchlimit = n - kLastLiterals;
        tab.slot[tab.hash(src)] = 0;
        ip = 1;
        for (;;) {
            // search
            uint32_t p, cand;
            {
                uint32_t next = ip, step = 1, nb = uint32_t(accel) << kSkipTrigger;
                bool found = false;
                for (;;) {
                    p = next;
                    next += step;
                    step = nb++ >> kSkipTrigger;
                    if (next > mflimit1)
                        break;
                    const uint32_t h = tab.hash(src + p);
                    cand = tab.slot[h];
                    tab.slot[h] = T(p);
                    if (Table<T>::near(cand, p) && read32(src + cand) == read32(src + p)) {
                        found = true;
                        break;
                    }
                }
                if (!found)
                    break;
            }
            while (p > anchor && cand > 0 && src[p - 1] == src[cand - 1]) {
                --p;
                --cand;
            }
            const uint32_t lit = p - anchor;
            if (over(op + bound_literals(lit)))
                return fail();
            uint32_t token = op++;
            if (lit >= 15) {
                dst[token] = 0xF0;
                op += put_length(dst + op, lit);
            } else {
                dst[token] = uint8_t(lit << 4);
            }
            for (uint32_t i = 0; i < lit; ++i)
                dst[op + i] = src[anchor + i];
            op += lit;
            for (;;) {
                // offset, match length
                const uint32_t off = p - cand;
                dst[op++] = uint8_t(off);
                dst[op++] = uint8_t(off >> 8);
                uint32_t count = 0;
                while (p + 4 + count < matchlimit && src[p + 4 + count] == src[cand + 4 + count])
                    ++count;
                if (over(op + bound_match(count)))
                    return fail();
                if (count >= 15) {
                    dst[token] |= 15;
                    op += put_length(dst + op, count);
                } else {
                    dst[token] |= uint8_t(count);
                }
                anchor = ip = p + 4 + count;
                if (ip >= mflimit1)
                    break;
                tab.slot[tab.hash(src + ip - 2)] = T(ip - 2);
                const uint32_t h = tab.hash(src + ip);
                cand = tab.slot[h];
                tab.slot[h] = T(ip);
                if (!(Table<T>::near(cand, ip) && read32(src + cand) == read32(src + ip)))
                    break;
                p = ip;
                token = op++;
                dst[token] = 0;
            }
            if (ip >= mflimit1)
                break;
            ++ip;
        }
    }
    const uint32_t last = n - anchor;
    if (over(op + bound_last(last)))
        return fail();
    if (last >= 15) {
        dst[op++] = 0xF0;
        op += put_length(dst + op, last);
    } else {
        dst[op++] = uint8_t(last << 4);
    }
    for (uint32_t i = 0; i < last; ++i)
        dst[op + i] = src[anchor + i];
    op += last;
    if (need_out)
        *need_out = uint32_t(need);
    return op;
}

// LZ4_compress_fast(src, dst, n, cap, accel) on a fresh state; `table` is
// kTableBytes of 4-byte aligned scratch.
AQZ_LZ4_HD inline uint32_t
encode_block(const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t cap, int accel, void* table,
             uint32_t* need_out)
{
    if (n < kU16Limit)
        return encode_block_with<uint16_t>(src, n, dst, cap, accel,
                                           static_cast<uint16_t*>(table), need_out);
    return encode_block_with<uint32_t>(src, n, dst, cap, accel, static_cast<uint32_t*>(table),
                                       need_out);
}

} // namespace lz4
} // namespace aqz
