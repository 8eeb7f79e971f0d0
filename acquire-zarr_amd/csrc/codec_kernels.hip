// codec_kernels.hip — byte-level codec stages beside the pyramid on gfx950
// (SURVEY §8(f) rows 3-4), behind include/aqz_codec.h.
//
//  * blosc filters: the bytes c-blosc hands its codec for every block of a
//    chunk buffer (blosc_c's shuffle step; the reference calls
//    blosc_compress_ctx from compress_in_place, zarr.common.cpp:106-137, on
//    each chunk, chunk.cpp:78-105).  Byte shuffle gathers byte j of every
//    element into plane j; bit shuffle (bitshuffle's bshuf_trans_bit_elem)
//    writes bit row j*8+b = bit b of byte j of every element, LSB first.
//    Both are pure permutations: HBM-bound, nbytes read + nbytes written.
//  * crc32c: the Castagnoli CRC of a shard index table (shard.cpp:145-166),
//    batched over many buffers: 16 KiB of a buffer per workgroup, or several
//    small buffers packed into one workgroup.
//
// Restated from the published algorithms (c-blosc 1.21 shuffle-generic.c /
// bitshuffle-generic.c; RFC 3720 CRC-32C); the CPU restatement the tests
// compare against is oracle/codec_oracle.c.
#include "codec_kernels.hh"
#include "blosc_decode.hh"
#include "launch_log.hh"
#include "lz4_block.hh"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

namespace aqz {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1))); // any byte alignment (gfx950 global loads)

// A run of equally sized blocks: block g of the run starts at
// (g / per) * stride + first + (g % per) * bs.  A launch covers blocks
// g0 .. g0 + n_blocks - 1 and fewer than 2^31 threads, so thread ids and
// in-launch divisions stay 32-bit.
struct BlockRun
{
    uint64_t stride; // bytes between buffers
    uint64_t first;  // offset of the run's first block within a buffer
    uint32_t per;    // blocks of the run per buffer
    uint32_t bs;     // block size in bytes
    uint32_t g0;     // first block of this launch
};

__device__ __forceinline__ uint64_t
block_base(const BlockRun& r, uint32_t g)
{
    g += r.g0;
    return uint64_t(g / r.per) * r.stride + r.first + uint64_t(g % r.per) * r.bs;
}

// 8x8 bit-matrix transpose (bitshuffle's TRANS_BIT_8X8): bit 8r+c -> 8c+r
__device__ __forceinline__ uint64_t
trans_bit_8x8(uint64_t x)
{
    uint64_t t;
    t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;
    x = x ^ t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull;
    x = x ^ t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull;
    x = x ^ t ^ (t << 28);
    return x;
}

// ---- byte shuffle -----------------------------------------------------------

// Vector form, TS in {2, 4, 8, 16}: one thread = 8 elements (8*TS bytes in,
// TS 8-byte stores out, lanes contiguous per plane).  Needs every block of
// the run to hold a multiple of 8 elements and 16-B aligned block bases.
template<int TS>
__global__ __launch_bounds__(256) void
shuffle_vec_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, BlockRun run,
                   uint32_t n_blocks)
{
    const uint32_t groups = run.bs / (8 * TS); // 8-element groups per block
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= groups * n_blocks)
        return;
    const uint32_t g = gid / groups;
    const uint32_t q = gid % groups;
    const uint64_t base = block_base(run, g);
    const uint32_t ne = run.bs / TS;
    constexpr int NV = (8 * TS) / 16; // 16-B loads per thread
    u32x4 v[NV];
    const auto* s = reinterpret_cast<const u32x4*>(src + base + uint64_t(q) * 8 * TS);
#pragma unroll
    for (int k = 0; k < NV; ++k)
        v[k] = __builtin_nontemporal_load(s + k);
    uint8_t e[8 * TS];
    __builtin_memcpy(e, v, sizeof(e));
#pragma unroll
    for (int j = 0; j < TS; ++j) {
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            w |= uint64_t(e[k * TS + j]) << (8 * k);
        __builtin_nontemporal_store(
          w, reinterpret_cast<uint64_t*>(dst + base + uint64_t(j) * ne + uint64_t(q) * 8));
    }
}

// Any typesize and block size: one thread per output byte (shuffle_generic).
__global__ __launch_bounds__(256) void
shuffle_generic_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, BlockRun run,
                       uint32_t n_blocks, uint32_t ts)
{
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= run.bs * n_blocks)
        return;
    const uint32_t g = gid / run.bs;
    const uint32_t o = gid % run.bs;
    const uint64_t base = block_base(run, g);
    const uint32_t ne = run.bs / ts;
    uint8_t v;
    if (o < ne * ts) {
        const uint32_t j = o / ne, i = o % ne;
        v = src[base + uint64_t(i) * ts + j];
    } else {
        v = src[base + o]; // blocksize % typesize tail
    }
    dst[base + o] = v;
}

// ---- bit shuffle ------------------------------------------------------------

// Vector form, TS in {1, 2, 4, 8}: one thread = G groups of 8 elements
// (128 contiguous input bytes); for each of the 8*TS bit rows it writes G
// bytes.  Needs (elements/8) % G == 0 per block, so row stores stay aligned.
template<int TS>
constexpr int kBitGroups = 16 / TS;

// 32x32 bit-matrix transpose in registers, LSB first: afterwards bit e of
// a[r] is what bit r of a[e] was.  Five block-swap stages of 16 word pairs.
__device__ __forceinline__ void
transpose_bits_32(uint32_t (&a)[32])
{
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int s = 16 >> st;
        const uint32_t m = st == 0   ? 0x0000FFFFu
                           : st == 1 ? 0x00FF00FFu
                           : st == 2 ? 0x0F0F0F0Fu
                           : st == 3 ? 0x33333333u
                                     : 0x55555555u;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            if (i & s)
                continue;
            const uint32_t t = ((a[i] >> s) ^ a[i + s]) & m;
            a[i + s] ^= t;
            a[i] ^= t << s;
        }
    }
}

template<int TS, int WAVES = 4, bool WORDS = true>
__global__ __launch_bounds__(64 * WAVES) void
bitshuffle_vec_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, BlockRun run,
                      uint32_t n_blocks)
{
    constexpr int G = kBitGroups<TS>;
    // Per wave: 64 threads x 128 input bytes, one 16-B pad per thread row so
    // the per-thread reads below are bank-conflict free.
    __shared__ u32x4 stage[WAVES][64][9];
    const uint32_t ne = run.bs / TS;
    const uint32_t row = ne / 8;          // bytes per bit row
    const uint32_t per_thread = row / G;  // threads per block
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = gid < per_thread * n_blocks;
    const uint32_t g = active ? gid / per_thread : 0;
    const uint32_t t = active ? gid % per_thread : 0;
    const uint64_t base = block_base(run, g);
    // Coalesced staging: load k of lane l fetches 16 B (l % 8) of thread
    // 8k + l/8's 128 input bytes, so each load instruction reads 8 whole
    // 128-B segments (1 KiB contiguous when the threads' segments are) instead
    // of 64 scattered 16-B pieces.  Measured on MI355X: 18.7 -> see DESIGN.
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const uint64_t sp = active ? reinterpret_cast<uint64_t>(src + base + uint64_t(t) * 128) : 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int owner = k * 8 + (lane >> 3);
        const uint64_t osp = __shfl(static_cast<unsigned long long>(sp), owner);
        u32x4 q = { 0u, 0u, 0u, 0u };
        if (osp)
            q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(osp) + (lane & 7));
        stage[w][owner][lane & 7] = q;
    }
    __syncthreads();
    if (!active)
        return;
    u32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        v[k] = stage[w][lane][k];
    if constexpr (WORDS && TS >= 2) {
        // The thread's 128 B as one 32x32 bit matrix whose transpose holds
        // every bit row (bit r of element e is bit e of bit row r, LSB first):
        //  TS = 4: 32 elements, a[e] = element e, row r = a[r];
        //  TS = 8: 16 elements, a[e] / a[16 + e] = low / high word of element
        //          e, rows r and 32 + r = low / high half of a[r];
        //  TS = 2: 64 elements, a[e] = element e | element 32 + e << 16,
        //          row r = a[r] | a[16 + r] << 32.
        // About a third of the per-byte gather, transpose and scatter work.
        uint32_t wd[32];
        __builtin_memcpy(wd, v, sizeof(wd));
        uint32_t a[32];
#pragma unroll
        for (int e = 0; e < 32; ++e) {
            if constexpr (TS == 4)
                a[e] = wd[e];
            else if constexpr (TS == 8)
                a[e] = e < 16 ? wd[2 * e] : wd[2 * (e - 16) + 1];
            else
                a[e] = (e & 1) ? (wd[e / 2] >> 16) | (wd[16 + e / 2] & 0xFFFF0000u)
                               : (wd[e / 2] & 0xFFFFu) | (wd[16 + e / 2] << 16);
        }
        transpose_bits_32(a);
        uint8_t* d = dst + base + uint64_t(t) * G;
        if constexpr (TS == 4) {
#pragma unroll
            for (int r = 0; r < 32; ++r)
                __builtin_nontemporal_store(a[r], reinterpret_cast<uint32_t*>(d + uint64_t(r) * row));
        } else if constexpr (TS == 8) {
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                __builtin_nontemporal_store(uint16_t(a[r]),
                                            reinterpret_cast<uint16_t*>(d + uint64_t(r) * row));
                __builtin_nontemporal_store(
                  uint16_t(a[r] >> 16), reinterpret_cast<uint16_t*>(d + uint64_t(32 + r) * row));
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                __builtin_nontemporal_store(uint64_t(a[r]) | (uint64_t(a[16 + r]) << 32),
                                            reinterpret_cast<uint64_t*>(d + uint64_t(r) * row));
        }
        return;
    }
    uint8_t e[128];
    __builtin_memcpy(e, v, sizeof(e));
    // out[r] collects G bytes of bit row r (byte gi = group gi of this thread)
    uint64_t out[8 * TS][(G + 7) / 8];
#pragma unroll
    for (int r = 0; r < 8 * TS; ++r)
#pragma unroll
        for (int w = 0; w < (G + 7) / 8; ++w)
            out[r][w] = 0;
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
#pragma unroll
        for (int j = 0; j < TS; ++j) {
            uint64_t x = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                x |= uint64_t(e[(gi * 8 + k) * TS + j]) << (8 * k);
            x = trans_bit_8x8(x);
#pragma unroll
            for (int b = 0; b < 8; ++b)
                out[j * 8 + b][gi / 8] |= ((x >> (8 * b)) & 0xFFull) << (8 * (gi % 8));
        }
    }
#pragma unroll
    for (int r = 0; r < 8 * TS; ++r) {
        uint8_t* d = dst + base + uint64_t(r) * row + uint64_t(t) * G;
        if constexpr (G == 16) {
            u32x4 q;
            __builtin_memcpy(&q, out[r], 16);
            __builtin_nontemporal_store(q, reinterpret_cast<u32x4*>(d));
        } else if constexpr (G == 8) {
            __builtin_nontemporal_store(out[r][0], reinterpret_cast<uint64_t*>(d));
        } else if constexpr (G == 4) {
            __builtin_nontemporal_store(uint32_t(out[r][0]), reinterpret_cast<uint32_t*>(d));
        } else {
            __builtin_nontemporal_store(uint16_t(out[r][0]), reinterpret_cast<uint16_t*>(d));
        }
    }
}

// Any typesize: one thread per output byte.  Blocks whose element count is
// not a multiple of 8 are copied (c-blosc 1.x bitshuffle()).
__global__ __launch_bounds__(256) void
bitshuffle_generic_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, BlockRun run,
                          uint32_t n_blocks, uint32_t ts)
{
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= run.bs * n_blocks)
        return;
    const uint32_t g = gid / run.bs;
    const uint32_t o = gid % run.bs;
    const uint64_t base = block_base(run, g);
    const uint32_t ne = run.bs / ts;
    uint8_t v;
    if (ne % 8 != 0 || o >= ne * ts) {
        v = src[base + o];
    } else {
        const uint32_t row = ne / 8;
        const uint32_t r = o / row, m = o % row;
        const uint32_t j = r / 8, b = r % 8;
        uint32_t acc = 0;
        for (uint32_t k = 0; k < 8; ++k)
            acc |= ((uint32_t(src[base + uint64_t(8 * m + k) * ts + j]) >> b) & 1u) << k;
        v = uint8_t(acc);
    }
    dst[base + o] = v;
}

__global__ __launch_bounds__(256) void
copy_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, BlockRun run,
            uint32_t n_blocks)
{
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= run.bs * n_blocks)
        return;
    const uint32_t g = gid / run.bs;
    const uint32_t o = gid % run.bs;
    const uint64_t base = block_base(run, g);
    dst[base + o] = src[base + o];
}

// Launch one kernel over blocks [g0, g0 + n) of a run; `threads_per_block`
// threads per data block.
template<typename L>
hipError_t
split_launch(BlockRun run, uint32_t n_blocks, uint64_t threads_per_block, L&& launch)
{
    if (threads_per_block == 0)
        return hipSuccess;
    const uint64_t cap = (1ull << 31) / threads_per_block; // blocks per launch
    if (cap == 0)
        return hipErrorInvalidValue;
    for (uint64_t g = 0; g < n_blocks; g += cap) {
        const uint32_t n = uint32_t(n_blocks - g < cap ? n_blocks - g : cap);
        run.g0 = uint32_t(g);
        launch(run, n, uint32_t((threads_per_block * n + 255) / 256));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// One run of equal blocks through the right kernel for `shuffle`.
hipError_t
filter_run(int shuffle, uint32_t ts, const uint8_t* src, uint8_t* dst, const BlockRun& run,
           uint32_t n_blocks, bool aligned, hipStream_t stream)
{
    if (n_blocks == 0 || run.bs == 0)
        return hipSuccess;
    const uint32_t ne = run.bs / ts;
    const bool doshuffle = shuffle == 1 && ts > 1;
    const bool dobit = shuffle == 2 && run.bs >= ts;
    // launch log (launch_log.hh): the kernel form this run takes
    auto note = [&](const char* family, const char* form, uint32_t grid, uint32_t block,
                    uint32_t n) {
        if (launch_log_on())
            launch_log_record("family=%s dtype=%u method=%d n_out=1 grid=%u block=%u form=%s "
                              "waves=%u blocks=%u bs=%u",
                              family, ts, shuffle, grid, block, form, block / 64, n, run.bs);
    };
    auto generic = [&](auto kernel) {
        return split_launch(run, n_blocks, run.bs, [&](BlockRun r, uint32_t n, uint32_t grid) {
            note(doshuffle ? "shuffle" : "bitshuffle", "generic", grid, 256, n);
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, src, dst, r, n, ts);
        });
    };
    if (doshuffle) {
        const bool vec = aligned && run.bs % 16 == 0 && run.bs % ts == 0 && ne % 8 == 0 &&
                         (ts == 2 || ts == 4 || ts == 8 || ts == 16);
        if (!vec)
            return generic(shuffle_generic_kernel);
        return split_launch(run, n_blocks, run.bs / (8 * ts),
                            [&](BlockRun r, uint32_t n, uint32_t grid) {
            note("shuffle", "vec", grid, 256, n);
            switch (ts) {
                case 2:
                    hipLaunchKernelGGL(shuffle_vec_kernel<2>, dim3(grid), dim3(256), 0, stream,
                                       src, dst, r, n);
                    break;
                case 4:
                    hipLaunchKernelGGL(shuffle_vec_kernel<4>, dim3(grid), dim3(256), 0, stream,
                                       src, dst, r, n);
                    break;
                case 8:
                    hipLaunchKernelGGL(shuffle_vec_kernel<8>, dim3(grid), dim3(256), 0, stream,
                                       src, dst, r, n);
                    break;
                default:
                    hipLaunchKernelGGL(shuffle_vec_kernel<16>, dim3(grid), dim3(256), 0, stream,
                                       src, dst, r, n);
                    break;
            }
        });
    }
    if (dobit) {
        const int G = (ts == 1 || ts == 2 || ts == 4 || ts == 8) ? int(16 / ts) : 0;
        const bool vec = aligned && G > 0 && run.bs % ts == 0 && ne % 8 == 0 &&
                         (ne / 8) % uint32_t(G) == 0 && run.bs % 16 == 0;
        if (!vec)
            return generic(bitshuffle_generic_kernel);
        // One-wave workgroups for 1-byte types (the staging barrier then
        // spans one wave), four for the word-transpose types: with the
        // transpose, u16 runs at 104-106% of a same-size copy with 4 waves
        // against 94% with one (profiles/r02/bitshuffle_waves_word_transpose.log).
        // $AQZ_BITSHUFFLE_WAVES = 1, 2 or 4 overrides (A/B only).
        static const int waves_env = [] {
            const char* e = std::getenv("AQZ_BITSHUFFLE_WAVES");
            const int v = e ? std::atoi(e) : 0;
            return (v == 1 || v == 2 || v == 4) ? v : 0;
        }();
        const int waves = waves_env ? waves_env : (ts == 1 ? 1 : 4);
        // $AQZ_BITSHUFFLE_BYTES=1: the per-byte gather form the word transpose
        // replaced (A/B only)
        static const bool bytes_env = [] {
            const char* e = std::getenv("AQZ_BITSHUFFLE_BYTES");
            return e && *e == '1';
        }();
        if (bytes_env && ts >= 2) {
            const uint32_t per = ne / 8 / G;
            const uint32_t wv = ts <= 2 ? 1 : 4;
            return split_launch(run, n_blocks, per, [&](BlockRun r, uint32_t n, uint32_t) {
                const uint32_t grid = uint32_t((uint64_t(per) * n + 64 * wv - 1) / (64 * wv));
                note("bitshuffle", "bytes", grid, 64 * wv, n);
                if (ts == 2)
                    hipLaunchKernelGGL((bitshuffle_vec_kernel<2, 1, false>), dim3(grid), dim3(64),
                                       0, stream, src, dst, r, n);
                else if (ts == 4)
                    hipLaunchKernelGGL((bitshuffle_vec_kernel<4, 4, false>), dim3(grid), dim3(256),
                                       0, stream, src, dst, r, n);
                else
                    hipLaunchKernelGGL((bitshuffle_vec_kernel<8, 4, false>), dim3(grid), dim3(256),
                                       0, stream, src, dst, r, n);
            });
        }
        if (waves != 4) {
            const uint32_t per = ne / 8 / G;
            return split_launch(run, n_blocks, per, [&](BlockRun r, uint32_t n, uint32_t) {
                const uint32_t grid = uint32_t((uint64_t(per) * n + 64 * waves - 1) / (64 * waves));
                note("bitshuffle", "vec", grid, uint32_t(64 * waves), n);
                auto go = [&](auto kern) {
                    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * waves), 0, stream, src, dst, r, n);
                };
                if (waves == 1) {
                    if (ts == 1) go(bitshuffle_vec_kernel<1, 1>);
                    else if (ts == 2) go(bitshuffle_vec_kernel<2, 1>);
                    else if (ts == 4) go(bitshuffle_vec_kernel<4, 1>);
                    else go(bitshuffle_vec_kernel<8, 1>);
                } else {
                    if (ts == 1) go(bitshuffle_vec_kernel<1, 2>);
                    else if (ts == 2) go(bitshuffle_vec_kernel<2, 2>);
                    else if (ts == 4) go(bitshuffle_vec_kernel<4, 2>);
                    else go(bitshuffle_vec_kernel<8, 2>);
                }
            });
        }
        return split_launch(run, n_blocks, ne / 8 / G,
                            [&](BlockRun r, uint32_t n, uint32_t grid) {
            note("bitshuffle", "vec", grid, 256, n);
            switch (ts) {
                case 1:
                    hipLaunchKernelGGL(bitshuffle_vec_kernel<1>, dim3(grid), dim3(256), 0,
                                       stream, src, dst, r, n);
                    break;
                case 2:
                    hipLaunchKernelGGL(bitshuffle_vec_kernel<2>, dim3(grid), dim3(256), 0,
                                       stream, src, dst, r, n);
                    break;
                case 4:
                    hipLaunchKernelGGL(bitshuffle_vec_kernel<4>, dim3(grid), dim3(256), 0,
                                       stream, src, dst, r, n);
                    break;
                default:
                    hipLaunchKernelGGL(bitshuffle_vec_kernel<8>, dim3(grid), dim3(256), 0,
                                       stream, src, dst, r, n);
                    break;
            }
        });
    }
    return split_launch(run, n_blocks, run.bs, [&](BlockRun r, uint32_t n, uint32_t grid) {
        note("copy", "generic", grid, 256, n);
        hipLaunchKernelGGL(copy_kernel, dim3(grid), dim3(256), 0, stream, src, dst, r, n);
    });
}

// ---- crc32c -----------------------------------------------------------------

constexpr uint32_t kCrc32cPoly = 0x82F63B78u; // reflected Castagnoli

// a * b mod P over GF(2), reflected bit order (zlib's multmodp), branch-free
__host__ __device__ inline uint32_t
multmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 31; k >= 0; --k) {
        p ^= b & (0u - ((a >> k) & 1u));
        b = (b >> 1) ^ (kCrc32cPoly & (0u - (b & 1u)));
    }
    return p;
}

// x^(8n) mod P (host side, once per launch)
uint32_t
x8nmodp(uint64_t n)
{
    uint32_t sq = 1u << 30;   // x^1, squared up to x^(2^k)
    for (int k = 0; k < 3; ++k)
        sq = multmodp(sq, sq); // x^8
    uint32_t p = 1u << 31;    // x^0
    while (n) {
        if (n & 1)
            p = multmodp(sq, p);
        sq = multmodp(sq, sq);
        n >>= 1;
    }
    return p;
}

// Shift tables for crc32c_kernel, passed by value as a kernel argument.
constexpr int kCrcThreadsPerWg = 256;
constexpr uint32_t kCrcSeg = 64;                                  // bytes per thread
constexpr uint32_t kCrcWgBytes = kCrcThreadsPerWg * kCrcSeg;      // 16 KiB per workgroup
constexpr int kCrcWgLevels = 16;                                  // up to 2^16 workgroups a buffer

struct CrcPow
{
    uint32_t seg[kCrcThreadsPerWg]; // x^(8 * 64 * t) mod P
    uint32_t wg[kCrcWgLevels];      // x^(8 * 16 KiB * 2^l) mod P
};

// CRC-32C of many equal-length buffers, 16 KiB of a buffer per workgroup.
// The buffer is cut into 64-byte segments aligned to its END; segment j
// (counted from the end) belongs to thread j % 256 of workgroup j / 256.
// By linearity of the CRC register update over GF(2):
//   CRC(M) = R0(M) ^ R_init(0^n) ^ ~0,   R0(M) = XOR_j R0(seg_j) * x^(8*64*j)
// where R0 is the register after a zero-initialised run (zlib's
// crc32_combine identity).  Each thread shifts its segment's R0 by its
// place in the workgroup (one table multiply), the workgroup XOR-reduces
// them, shifts the result by the workgroup's place (binary powers), and
// XORs it into crcs[b] atomically; crcs[b] was preset to R_init(0^n) ^ ~0
// on the host side of the launch.  No ordering between workgroups is
// needed, so every CU works on a table at once.  A table of at most 16 KiB
// (Single, the common shard index size) needs no atomic and no preset fill:
// it gets the next power of two of its segment count in lanes, so small
// tables pack 256 >> lgp to a workgroup (1 KiB tables: 16), and its first
// lane stores R0(M) ^ preset after a lane-group XOR.
template <bool Single>
__global__ __launch_bounds__(kCrcThreadsPerWg) void
crc32c_kernel(const uint8_t* __restrict__ data, uint64_t nbytes, uint64_t stride, uint32_t wgs,
              uint32_t n_buffers, uint32_t lgp, CrcPow pw, uint32_t preset,
              uint32_t* __restrict__ crcs)
{
    __shared__ uint32_t table[8][256];
    __shared__ uint32_t wave_x[kCrcThreadsPerWg / 64];
    const uint32_t tid = threadIdx.x;
    {
        uint32_t c = tid;
        for (int k = 0; k < 8; ++k)
            c = (c >> 1) ^ (kCrc32cPoly & (0u - (c & 1u)));
        table[0][tid] = c;
    }
    __syncthreads();
    for (int k = 1; k < 8; ++k) {
        const uint32_t prev = table[k - 1][tid];
        table[k][tid] = (prev >> 8) ^ table[0][prev & 0xFFu];
    }
    __syncthreads();

    // Single: 2^lgp lanes per table (lgp <= 8), 256 >> lgp tables per workgroup
    const uint32_t lanes = Single ? (1u << lgp) : uint32_t(kCrcThreadsPerWg);
    const uint32_t b = Single ? blockIdx.x * (kCrcThreadsPerWg >> lgp) + (tid >> lgp)
                              : blockIdx.x / wgs;
    const uint32_t q = Single ? 0u : blockIdx.x % wgs;
    const uint32_t js = tid & (lanes - 1);                   // segment within the workgroup
    const uint8_t* buf = data + uint64_t(b) * stride;
    const uint64_t j = uint64_t(q) * kCrcThreadsPerWg + js; // segment, from the end
    uint32_t c = 0;                                          // zero-initialised register
    auto step8 = [&](const uint8_t* v) {                     // slicing-by-8
        const uint32_t lo = c ^ (uint32_t(v[0]) | uint32_t(v[1]) << 8 | uint32_t(v[2]) << 16 |
                                 uint32_t(v[3]) << 24);
        c = table[7][lo & 0xFFu] ^ table[6][(lo >> 8) & 0xFFu] ^ table[5][(lo >> 16) & 0xFFu] ^
            table[4][lo >> 24] ^ table[3][v[4]] ^ table[2][v[5]] ^ table[1][v[6]] ^
            table[0][v[7]];
    };
    if (b < n_buffers && kCrcSeg * j < nbytes) {
        const uint64_t end = nbytes - kCrcSeg * j;
        if (end >= kCrcSeg) {
            // a whole segment: four 16-byte loads in flight, any alignment
            // (shard index tables sit at 4-byte offsets after their CRC)
            const uint8_t* s = buf + end - kCrcSeg;
            u32x4 w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = *reinterpret_cast<const u32x4_u*>(s + 16 * k);
            uint8_t v[64];
            __builtin_memcpy(v, w, 64);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                step8(v + 8 * k);
        } else {
            // the buffer's first, short segment
            for (uint64_t i = 0; i < end; ++i)
                c = (c >> 8) ^ table[0][(c ^ buf[i]) & 0xFFu];
        }
        c = multmodp(pw.seg[js], c); // shift by the segments after it in this workgroup
    }
    // XOR over each table's lanes (the whole wave when a table spans waves)
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1)
        if (d < lanes)
            c ^= __shfl_xor(c, d);
    if (Single && lanes <= 64) {
        if (js == 0 && b < n_buffers)
            crcs[b] = c ^ preset;
        return;
    }
    if ((tid & 63) == 0)
        wave_x[tid >> 6] = c;
    __syncthreads();
    const uint32_t wpt = lanes / 64; // waves per table
    if (tid < kCrcThreadsPerWg / 64 / wpt) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < wpt; ++k)
            v ^= wave_x[tid * wpt + k];
        if constexpr (Single) {
            const uint32_t bt = blockIdx.x * (kCrcThreadsPerWg >> lgp) + tid;
            if (bt < n_buffers)
                crcs[bt] = v ^ preset;
        } else {
            // shift by the workgroups after this one: x^(8 * 16 KiB * q)
            for (int l = 0; l < kCrcWgLevels; ++l)
                if ((q >> l) & 1u)
                    v = multmodp(pw.wg[l], v);
            atomicXor(crcs + b, v);
        }
    }
}

} // namespace

hipError_t
launch_blosc_filter(int shuffle,
                    uint32_t typesize,
                    uint32_t blocksize,
                    const void* src,
                    uint64_t nbytes,
                    uint32_t n_buffers,
                    void* dst,
                    hipStream_t stream)
{
    if (typesize == 0 || blocksize == 0 || shuffle < 0 || shuffle > 2 || n_buffers == 0)
        return hipErrorInvalidValue;
    if (nbytes == 0)
        return hipSuccess;
    const auto* s = static_cast<const uint8_t*>(src);
    auto* d = static_cast<uint8_t*>(dst);
    const bool aligned = reinterpret_cast<uintptr_t>(s) % 16 == 0 &&
                         reinterpret_cast<uintptr_t>(d) % 16 == 0 &&
                         (n_buffers == 1 || nbytes % 16 == 0);
    const uint64_t full = nbytes / blocksize;
    const uint32_t leftover = uint32_t(nbytes % blocksize);
    if (full * n_buffers >= (1ull << 32))
        return hipErrorInvalidValue;
    if (full) {
        const BlockRun run{ nbytes, 0, uint32_t(full), blocksize, 0 };
        hipError_t e = filter_run(shuffle, typesize, s, d, run, uint32_t(full * n_buffers),
                                  aligned, stream);
        if (e != hipSuccess)
            return e;
    }
    if (leftover) {
        const BlockRun run{ nbytes, full * blocksize, 1, leftover, 0 };
        return filter_run(shuffle, typesize, s, d, run, n_buffers,
                          aligned && (full * blocksize) % 16 == 0, stream);
    }
    return hipSuccess;
}

hipError_t
launch_crc32c(const void* data, uint64_t nbytes, uint64_t stride, uint32_t n_buffers,
              uint32_t* crcs, hipStream_t stream)
{
    if (n_buffers == 0 || n_buffers >= (1u << 31))
        return hipErrorInvalidValue;
    const uint64_t wgs = (nbytes + kCrcWgBytes - 1) / kCrcWgBytes;
    if (wgs >= (1ull << kCrcWgLevels) || wgs * n_buffers >= (1ull << 31))
        return hipErrorInvalidValue;
    // crcs[b] = R_init(0^n) ^ ~0; the kernel XORs R0(M) in
    const uint32_t preset = multmodp(x8nmodp(nbytes), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
    if (wgs <= 1) {
        // empty tables: the CRC is the preset; else one workgroup per table
        // writes R0(M) ^ preset and nothing needs filling first
        if (wgs == 0)
            return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(crcs), int(preset),
                                     n_buffers, stream);
    } else {
        hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(crcs), int(preset),
                                         n_buffers, stream);
        if (e != hipSuccess)
            return e;
    }
    // the shift powers do not depend on the launch: computed once
    static const CrcPow pw = [] {
        CrcPow p;
        const uint32_t seg = x8nmodp(kCrcSeg);
        p.seg[0] = 1u << 31; // x^0
        for (int t = 1; t < kCrcThreadsPerWg; ++t)
            p.seg[t] = multmodp(seg, p.seg[t - 1]);
        p.wg[0] = x8nmodp(kCrcWgBytes);
        for (int l = 1; l < kCrcWgLevels; ++l)
            p.wg[l] = multmodp(p.wg[l - 1], p.wg[l - 1]);
        return p;
    }();
    if (wgs == 1) {
        uint32_t lgp = 0; // lanes per table: next power of two of its segments
        while ((uint64_t(kCrcSeg) << lgp) < nbytes)
            ++lgp;
        const uint32_t per_wg = uint32_t(kCrcThreadsPerWg) >> lgp;
        hipLaunchKernelGGL(crc32c_kernel<true>, dim3((n_buffers + per_wg - 1) / per_wg),
                           dim3(kCrcThreadsPerWg), 0, stream,
                           static_cast<const uint8_t*>(data), nbytes, stride, uint32_t(wgs),
                           n_buffers, lgp, pw, preset, crcs);
    } else {
        hipLaunchKernelGGL(crc32c_kernel<false>, dim3(uint32_t(wgs * n_buffers)),
                           dim3(kCrcThreadsPerWg), 0, stream, static_cast<const uint8_t*>(data),
                           nbytes, stride, uint32_t(wgs), n_buffers, 8u, pw, preset, crcs);
    }
    return hipGetLastError();
}

// ---- lz4 splits and blosc frames --------------------------------------------
//
// The entropy stage of a blosc+LZ4 chunk on the device: one wave per split
// runs the encoder lz4_block.hh states serially, and one workgroup per chunk
// lays the frame out as blocks_frame / write_frame do on the host
// (blosc_frame.cpp).  Every value that steers the encoder is wave-uniform
// (ballots, lane reads, loads of one address), so all 64 lanes take the same
// path; the lanes share the table clear, the probes of a search, the match
// count and the copies.

namespace {

using lz4::kTableBytes;

__device__ __forceinline__ uint32_t
uni(uint32_t v)
{
    return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ uint32_t
lane_read(uint32_t v, uint32_t lane)
{
    return __builtin_amdgcn_readlane(v, uni(lane));
}

__device__ __forceinline__ void
store32(uint8_t* p, uint32_t v)
{
    __builtin_memcpy(p, &v, 4);
}

// dst[0, len) = src[0, len), any alignment, by the whole wave
__device__ __forceinline__ void
wave_copy(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t lane)
{
    const uint32_t words = len >> 2;
    for (uint32_t i = lane; i < words; i += 64)
        store32(dst + 4 * i, lz4::read32(src + 4 * i));
    for (uint32_t i = (words << 2) + lane; i < len; i += 64)
        dst[i] = src[i];
}

// the bytes after a token nibble of 15 (lz4::put_length), by the whole wave
__device__ __forceinline__ uint32_t
wave_put_length(uint8_t* dst, uint32_t len, uint32_t lane)
{
    const uint32_t m = len - 15, q = m / 255;
    for (uint32_t i = lane; i < q; i += 64)
        dst[i] = 255;
    if (lane == 0)
        dst[q] = uint8_t(m - q * 255);
    return q + 1;
}

// equal bytes of src[a...] and src[b...] (b < a) before `limit`: four bytes a
// lane, 256 a step, the first lane that stops found by ballot
__device__ __forceinline__ uint32_t
wave_count(const uint8_t* src, uint32_t a, uint32_t b, uint32_t limit, uint32_t lane)
{
    uint32_t total = 0;
    for (;;) {
        const uint32_t pos = a + total + 4 * lane;
        const uint32_t ref = b + total + 4 * lane;
        uint32_t c = 0;
        if (pos + 4 <= limit) {
            const uint32_t x = lz4::read32(src + pos) ^ lz4::read32(src + ref);
            c = x ? uint32_t(__builtin_ctz(x)) >> 3 : 4u;
        } else {
            while (c < 3 && pos + c < limit && src[pos + c] == src[ref + c])
                ++c;
        }
        const uint64_t stop = __ballot(c < 4);
        if (stop) {
            const uint32_t l = uint32_t(__ffsll(static_cast<long long>(stop))) - 1;
            return total + 4 * l + lane_read(c, l);
        }
        total += 256; // every lane had four bytes before limit: pos advances
    }
}

// sum over t < x of t >> 6: the bytes the step schedule skips
__device__ __forceinline__ uint64_t
skip_sum(uint32_t x)
{
    const uint64_t q = x >> 6, r = x & 63;
    return 32 * q * (q - 1) + q * r;
}

enum SearchEnd
{
    kSearchInputEnd = 0, // the next probe would pass end - 11: last literals
    kSearchFound = 1,
    kSearchMore = 2 // `max_probes` probes made, none matched
};

// One search, one probe at a time (the A/B form, and the first probes of the
// batched form): lane 0 owns the table.
template<typename T>
__device__ __forceinline__ SearchEnd
search_serial(const uint8_t* src, T* table, uint32_t ip, uint32_t mflimit1, uint32_t accel,
              uint32_t lane, uint32_t max_probes, uint32_t* p_out, uint32_t* cand_out)
{
    uint32_t next = ip, step = 1, nb = accel << lz4::kSkipTrigger;
    for (uint32_t g = 0; g < max_probes; ++g) {
        const uint32_t p = next;
        next += step; // step >= 1: accel >= 1
        step = nb++ >> lz4::kSkipTrigger;
        if (next > mflimit1)
            return kSearchInputEnd;
        const lz4::Table<T> tab{ table };
        const uint32_t h = uni(tab.hash(src + p));
        const uint32_t v = uni(lz4::read32(src + p));
        uint32_t c = 0;
        if (lane == 0) {
            c = table[h];
            table[h] = T(p);
        }
        const uint32_t cand = uni(c);
        if (lz4::Table<T>::near(cand, p) && uni(lz4::read32(src + cand)) == v) {
            *p_out = p;
            *cand_out = cand;
            return kSearchFound;
        }
    }
    return kSearchMore;
}

// Probes a batched search makes one at a time before it goes 64 wide: in
// compressible data most searches end within their first few probes, and a
// batch costs a 64-step conflict scan on top of the two loads.  A search that
// has missed this often is likely a long one (incompressible data, where the
// steps grow), which is what the batches are for.
constexpr uint32_t kSerialLead = 8;

// One search, 64 probes at a time.  The probe positions do not depend on the
// data, so lane i takes probe g0 + i.  A lane whose bucket an earlier lane of
// the batch also probes gets that lane's position as its candidate (the
// nearest one), which is what the serial order of lookups and stores yields;
// the first lane whose candidate passes is the match, and only the lanes up to
// it store, the latest of a bucket winning.
template<typename T>
__device__ __forceinline__ bool
search_batch(const uint8_t* src, T* table, uint32_t ip, uint32_t mflimit1, uint32_t accel,
             uint32_t lane, uint32_t* p_out, uint32_t* cand_out)
{
    const uint32_t nb0 = accel << lz4::kSkipTrigger;
    const uint64_t f0 = skip_sum(nb0);
    const lz4::Table<T> tab{ table };
    const SearchEnd lead =
      search_serial<T>(src, table, ip, mflimit1, accel, lane, kSerialLead, p_out, cand_out);
    if (lead != kSearchMore)
        return lead == kSearchFound;
    for (uint32_t g0 = kSerialLead;; g0 += 64) {
        __syncthreads(); // earlier stores, by any lane, before these lookups
        const uint32_t g = g0 + lane;
        const uint64_t at = ip + (g ? 1 + skip_sum(nb0 + g - 1) - f0 : 0);
        const uint64_t nxt_at = ip + 1 + skip_sum(nb0 + g) - f0;
        const bool valid = nxt_at <= mflimit1; // a prefix of the lanes
        const uint32_t p = valid ? uint32_t(at) : 0;
        uint32_t h = 0xFFFFFFFFu, v = 0, c = 0;
        if (valid) {
            h = tab.hash(src + p);
            v = lz4::read32(src + p);
            c = table[h];
        }
        int prev = -1, nxt = 64;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const uint32_t hj = __builtin_amdgcn_readlane(h, j);
            if (hj == h) {
                if (j < int(lane))
                    prev = j;
                else if (j > int(lane) && nxt == 64)
                    nxt = j;
            }
        }
        const uint32_t pc = __shfl(p, prev < 0 ? 0 : prev);
        const uint32_t pv = __shfl(v, prev < 0 ? 0 : prev);
        uint32_t cv = pv;
        if (prev >= 0)
            c = pc;
        else if (valid)
            cv = lz4::read32(src + c);
        const bool hit = valid && lz4::Table<T>::near(c, p) && cv == v;
        const uint64_t hits = __ballot(hit);
        const uint64_t invalid = __ballot(!valid);
        const uint32_t m = hits ? uint32_t(__ffsll(static_cast<long long>(hits))) - 1 : 63u;
        if (valid && lane <= m && nxt > int(m))
            table[h] = T(p);
        if (hits) {
            __syncthreads();
            *p_out = lane_read(p, m);
            *cand_out = lane_read(c, m);
            return true;
        }
        if (invalid)
            return false;
        // 64 valid probes: the next batch starts at least 64 bytes further on
    }
}

struct Lz4Run
{
    uint64_t stride;   // bytes between chunks
    uint64_t first;    // offset of the run's first split within a chunk
    uint32_t per;      // splits of the run per chunk
    uint32_t len;      // bytes per split
    uint32_t row0;     // the run's first row among a chunk's rows
    uint32_t rows_per; // rows per chunk
    uint32_t accel;
};

// One wave per split: slot = the split's own bytes in `comp`, row = (csize,
// need), csize 0 when need passed the split size.
template<typename T, bool BATCH>
__global__ __launch_bounds__(64) void
lz4_split_kernel(const uint8_t* __restrict__ filt, uint8_t* __restrict__ comp,
                 uint2* __restrict__ rows, Lz4Run run)
{
    __shared__ T table[kTableBytes / sizeof(T)];
    const uint32_t lane = threadIdx.x;
    const uint32_t k = blockIdx.x / run.per, j = blockIdx.x % run.per;
    const uint64_t base = uint64_t(k) * run.stride + run.first + uint64_t(j) * run.len;
    const uint8_t* src = filt + base;
    uint8_t* dst = comp + base;
    const uint32_t n = run.len, cap = run.len;
    {
        auto* w = reinterpret_cast<uint32_t*>(table);
        for (uint32_t i = lane; i < kTableBytes / 4; i += 64)
            w[i] = 0;
    }
    __syncthreads();
    const lz4::Table<T> tab{ table };
    uint64_t need = 0;
    uint32_t op = 0, anchor = 0;
    bool fits = true;
    auto over = [&](uint64_t x) {
        need = x > need ? x : need;
        return x > cap;
    };
    if (n >= lz4::kMinInput) {
        const uint32_t mflimit1 = n - lz4::kMfLimit;
        const uint32_t matchlimit = n - lz4::kLastLiterals;
        // position 0 goes into the table: the cleared entry already says so
        uint32_t ip = 1;
        for (;;) {
            uint32_t p = 0, cand = 0;
            const bool found =
              BATCH ? search_batch<T>(src, table, ip, mflimit1, run.accel, lane, &p, &cand)
                    : search_serial<T>(src, table, ip, mflimit1, run.accel, lane, 0xFFFFFFFFu, &p,
                                       &cand) == kSearchFound;
            if (!found)
                break;
            // backwards to the anchor, 64 bytes a step
            for (uint32_t back = 0;;) {
                const uint32_t room = (p - anchor < cand ? p - anchor : cand) - back;
                if (room == 0) {
                    p -= back;
                    cand -= back;
                    break;
                }
                bool eq = false;
                if (lane < room)
                    eq = src[p - 1 - back - lane] == src[cand - 1 - back - lane];
                const uint64_t stop = __ballot(!eq);
                const uint32_t c = stop ? uint32_t(__ffsll(static_cast<long long>(stop))) - 1 : 64u;
                back += c; // c <= room
                if (c < 64) {
                    p -= back;
                    cand -= back;
                    break;
                }
            }
            const uint32_t lit = p - anchor;
            if (over(op + lz4::bound_literals(lit))) {
                fits = false;
                break;
            }
            uint32_t token_at = op++;
            uint32_t token = lit >= 15 ? 0xF0u : lit << 4;
            if (lit >= 15)
                op += wave_put_length(dst + op, lit, lane);
            wave_copy(dst + op, src + anchor, lit, lane);
            op += lit;
            for (;;) {
                const uint32_t off = p - cand;
                if (lane == 0) {
                    dst[op] = uint8_t(off);
                    dst[op + 1] = uint8_t(off >> 8);
                }
                op += 2;
                const uint32_t count = wave_count(src, p + 4, cand + 4, matchlimit, lane);
                if (over(op + lz4::bound_match(count))) {
                    fits = false;
                    break;
                }
                if (count >= 15) {
                    token |= 15;
                    op += wave_put_length(dst + op, count, lane);
                } else {
                    token |= count;
                }
                if (lane == 0)
                    dst[token_at] = uint8_t(token);
                anchor = ip = p + 4 + count;
                if (ip >= mflimit1)
                    break;
                // store ip - 2, then look ip up and store it
                const uint32_t h2 = uni(tab.hash(src + ip - 2));
                const uint32_t h = uni(tab.hash(src + ip));
                const uint32_t v = uni(lz4::read32(src + ip));
                uint32_t c = 0;
                if (lane == 0) {
                    table[h2] = T(ip - 2);
                    c = table[h];
                    table[h] = T(ip);
                }
                cand = uni(c);
                if (!(lz4::Table<T>::near(cand, ip) && uni(lz4::read32(src + cand)) == v))
                    break;
                p = ip;
                token_at = op++;
                token = 0;
            }
            if (!fits || ip >= mflimit1)
                break;
            ++ip;
        }
    }
    if (fits) {
        const uint32_t last = n - anchor;
        if (over(op + lz4::bound_last(last))) {
            fits = false;
        } else {
            if (lane == 0)
                dst[op] = uint8_t(last >= 15 ? 0xF0u : last << 4);
            ++op;
            if (last >= 15)
                op += wave_put_length(dst + op, last, lane);
            wave_copy(dst + op, src + anchor, last, lane);
            op += last;
        }
    }
    if (lane == 0)
        rows[uint64_t(k) * run.rows_per + run.row0 + j] =
          make_uint2(fits ? op : 0u, need > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(need));
}

// dst[0, len) = src[0, len), any alignment, by a 256-thread workgroup
__device__ __forceinline__ void
wg_copy(uint8_t* dst, const uint8_t* src, uint64_t len, uint32_t t)
{
    const uint64_t vecs = len >> 4;
    for (uint64_t i = t; i < vecs; i += 256)
        *reinterpret_cast<u32x4_u*>(dst + 16 * i) = *reinterpret_cast<const u32x4_u*>(src + 16 * i);
    for (uint64_t i = (vecs << 4) + t; i < len; i += 256)
        dst[i] = src[i];
}

__device__ __forceinline__ void
put32_dev(uint8_t* d, uint32_t v)
{
    d[0] = uint8_t(v);
    d[1] = uint8_t(v >> 8);
    d[2] = uint8_t(v >> 16);
    d[3] = uint8_t(v >> 24);
}

// One workgroup per chunk.  Every thread walks the chunk's rows the way
// blocks_frame does (blosc_frame.cpp), once to learn whether c-blosc would
// fall back to the memcpy frame and once to place the splits; the workgroup
// copies each payload.  `memcpy_only`: clevel 0 or nbytes < 128.
__global__ __launch_bounds__(256) void
blosc_frame_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ filt,
                   const uint8_t* __restrict__ comp, const uint2* __restrict__ rows,
                   uint8_t* __restrict__ dst, uint32_t* __restrict__ sizes, BloscFrameLayout lay)
{
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    uint8_t* out = dst + uint64_t(k) * lay.dst_stride;
    const uint64_t chunk = uint64_t(k) * lay.nbytes;
    const uint2* row = rows + uint64_t(k) * lay.rows_per;
    const uint64_t destsize = lay.nbytes + 16;
    const uint32_t nblocks = uint32_t((lay.nbytes + lay.blocksize - 1) / lay.blocksize);
    // pass 0 decides, pass 1 writes
    bool fallback = lay.memcpy_only;
    uint64_t total = 0;
    for (int pass = 0; pass < 2 && !fallback; ++pass) {
        uint64_t nt = 16 + 4 * uint64_t(nblocks);
        if (nt > destsize) {
            fallback = true;
            break;
        }
        uint32_t r = 0;
        for (uint32_t b = 0; b < nblocks && !fallback; ++b) {
            const uint64_t off = uint64_t(b) * lay.blocksize;
            const uint64_t bsize = lay.nbytes - off < lay.blocksize ? lay.nbytes - off : lay.blocksize;
            const uint32_t nsplits = bsize < lay.blocksize ? 1u : lay.nsplits;
            const uint64_t neb = bsize / nsplits;
            if (pass && t == 0)
                put32_dev(out + 16 + 4 * b, uint32_t(nt));
            for (uint32_t j = 0; j < nsplits; ++j, ++r) {
                nt += 4;
                if (nt >= destsize) {
                    fallback = true;
                    break;
                }
                const uint64_t cap = neb < destsize - nt ? neb : destsize - nt;
                const uint2 cn = row[r];
                const bool packed = cn.x != 0 && cn.y <= cap && cn.x != neb;
                if (!packed && nt + neb > destsize) {
                    fallback = true;
                    break;
                }
                const uint64_t c = packed ? cn.x : neb;
                if (pass) {
                    if (t == 0)
                        put32_dev(out + nt - 4, uint32_t(c));
                    const uint64_t piece = chunk + off + uint64_t(j) * neb;
                    wg_copy(out + nt, (packed ? comp : filt) + piece, c, t);
                }
                nt += c;
            }
        }
        total = nt;
    }
    uint8_t flags = lay.flags;
    if (fallback) {
        flags |= 0x2;
        total = destsize;
        wg_copy(out + 16, src + chunk, lay.nbytes, t);
    }
    if (t == 0) {
        out[0] = 2; // BLOSC_VERSION_FORMAT
        out[1] = 1; // versionlz of lz4
        out[2] = flags;
        out[3] = lay.typesize;
        put32_dev(out + 4, uint32_t(lay.nbytes));
        put32_dev(out + 8, lay.blocksize);
        put32_dev(out + 12, uint32_t(total));
        sizes[k] = uint32_t(total);
    }
}

// frame k (sizes[k] bytes at frames + k * stride) to packed + offsets[k]
__global__ __launch_bounds__(256) void
pack_frames_kernel(const uint8_t* __restrict__ frames, uint64_t stride,
                   const uint32_t* __restrict__ sizes, const uint64_t* __restrict__ offsets,
                   uint8_t* __restrict__ packed)
{
    const uint32_t k = blockIdx.x;
    wg_copy(packed + offsets[k], frames + uint64_t(k) * stride, sizes[k], threadIdx.x);
}

template<typename T>
void
launch_split_run(const uint8_t* filt, uint8_t* comp, uint2* rows, const Lz4Run& run, uint32_t grid,
                 bool serial, hipStream_t stream)
{
    if (launch_log_on())
        launch_log_record("family=lz4 table=%s probe=%s streams=%u grid=%u block=64 len=%u "
                          "accel=%u",
                          sizeof(T) == 2 ? "u16" : "u32", serial ? "serial" : "batch", grid, grid,
                          run.len, run.accel);
    if (serial)
        hipLaunchKernelGGL((lz4_split_kernel<T, false>), dim3(grid), dim3(64), 0, stream, filt,
                           comp, rows, run);
    else
        hipLaunchKernelGGL((lz4_split_kernel<T, true>), dim3(grid), dim3(64), 0, stream, filt, comp,
                           rows, run);
}

} // namespace

uint32_t
lz4_rows_per_chunk(uint64_t nbytes, uint32_t blocksize, uint32_t nsplits)
{
    return uint32_t(nbytes / blocksize) * nsplits + (nbytes % blocksize ? 1u : 0u);
}

hipError_t
launch_lz4_splits(const void* filtered, void* comp, void* rows, uint64_t nbytes,
                  uint32_t n_buffers, uint32_t blocksize, uint32_t nsplits, int accel,
                  bool serial_probe, hipStream_t stream)
{
    if (blocksize == 0 || nsplits == 0 || n_buffers == 0 || nbytes == 0 || blocksize % nsplits)
        return hipErrorInvalidValue;
    const uint64_t full = nbytes / blocksize;
    const uint32_t leftover = uint32_t(nbytes % blocksize);
    const uint64_t rows_per = full * nsplits + (leftover ? 1 : 0);
    if (rows_per * n_buffers >= (1ull << 31))
        return hipErrorInvalidValue;
    const auto* f = static_cast<const uint8_t*>(filtered);
    auto* c = static_cast<uint8_t*>(comp);
    auto* r = static_cast<uint2*>(rows);
    const uint32_t acc = uint32_t(lz4::clamp_accel(accel));
    auto go = [&](const Lz4Run& run) {
        const uint32_t grid = run.per * n_buffers;
        if (run.len < lz4::kU16Limit)
            launch_split_run<uint16_t>(f, c, r, run, grid, serial_probe, stream);
        else
            launch_split_run<uint32_t>(f, c, r, run, grid, serial_probe, stream);
        return hipGetLastError();
    };
    if (full) {
        const Lz4Run run{ nbytes, 0, uint32_t(full * nsplits), blocksize / nsplits, 0,
                          uint32_t(rows_per), acc };
        if (const hipError_t e = go(run); e != hipSuccess)
            return e;
    }
    if (leftover) {
        const Lz4Run run{ nbytes, full * blocksize, 1, leftover, uint32_t(full * nsplits),
                          uint32_t(rows_per), acc };
        return go(run);
    }
    return hipSuccess;
}

hipError_t
launch_blosc_frames(const void* src, const void* filtered, const void* comp, const void* rows,
                    void* dst, uint32_t* sizes, uint32_t n_buffers, const BloscFrameLayout& layout,
                    hipStream_t stream)
{
    if (n_buffers == 0 || n_buffers >= (1u << 31) || layout.blocksize == 0 || layout.nsplits == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(blosc_frame_kernel, dim3(n_buffers), dim3(256), 0, stream,
                       static_cast<const uint8_t*>(src), static_cast<const uint8_t*>(filtered),
                       static_cast<const uint8_t*>(comp), static_cast<const uint2*>(rows),
                       static_cast<uint8_t*>(dst), sizes, layout);
    return hipGetLastError();
}

hipError_t
launch_pack_frames(const void* frames, uint64_t stride, const uint32_t* sizes,
                   const uint64_t* offsets, void* packed, uint32_t n_buffers, hipStream_t stream)
{
    if (n_buffers == 0 || n_buffers >= (1u << 31))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_frames_kernel, dim3(n_buffers), dim3(256), 0, stream,
                       static_cast<const uint8_t*>(frames), stride, sizes, offsets,
                       static_cast<uint8_t*>(packed));
    return hipGetLastError();
}

// ---- reading blosc+LZ4 frames back -------------------------------------------
//
// blosc_decode.hh states the frame walk, the LZ4 block decoder and the
// unfilter serially.  Here one wave decodes one split: the token walk is
// wave-uniform (every value that steers it comes out of a lane read), and the
// 64 lanes share the literal and match copies.  Every bound is checked before
// the copy it guards, as in the serial decoder, so a malformed stream ends in
// a status.
//
// A match reads bytes this wave may just have stored, through other lanes.
// The output lives in global memory; a workgroup-scope fence (one wave sits on
// one CU) orders those stores before the loads, and is paid only when the
// match's source reaches past `visible`, the position up to which an earlier
// fence already covers.  No non-temporal stores: the region is read again.
// DESIGN.md §12.13 has the reasons against an LDS window.

namespace {

typedef unsigned long long u64_u __attribute__((aligned(1)));
typedef unsigned int u32_u __attribute__((aligned(1)));

// 256 bytes of a split's input held by the wave, four per lane; a byte is a
// lane read away.  `i` is wave-uniform.
struct InWindow
{
    const uint8_t* src;
    uint32_t n, lane, base, word;

    __device__ __forceinline__ void fill(uint32_t at)
    {
        base = at;
        const uint32_t p = at + 4 * lane; // at < n <= 2^31
        uint32_t w = 0;
        if (p + 4 <= n) {
            w = lz4::read32(src + p);
        } else {
            for (uint32_t k = 0; k < 4 && p + k < n; ++k)
                w |= uint32_t(src[p + k]) << (8 * k);
        }
        word = w;
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t i)
    {
        i = uni(i);
        if (i - base >= 256u)
            fill(i);
        const uint32_t d = i - base;
        return (lane_read(word, d >> 2) >> (8 * (d & 3))) & 0xFFu;
    }
};

// dst[0, len) = src[0, len), ranges apart, any alignment: 16 bytes a lane,
// the last 15 or fewer one byte a lane
__device__ __forceinline__ void
wave_copy16(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t lane)
{
    const uint32_t vecs = len >> 4;
    for (uint32_t i = lane; i < vecs; i += 64)
        *reinterpret_cast<u32x4_u*>(dst + 16 * uint64_t(i)) =
          *reinterpret_cast<const u32x4_u*>(src + 16 * uint64_t(i));
    const uint32_t t = (vecs << 4) + lane;
    if (t < len)
        dst[t] = src[t];
}

// out[pos + i] = out[pos - off + i % off], i < len, for a match that overlaps
// itself (off < len): every source lies before pos, so one pass suffices.
// Four bytes a lane; i % off is divided once and stepped from there.
__device__ __forceinline__ void
wave_copy_periodic(uint8_t* out, uint32_t pos, uint32_t off, uint32_t len, uint32_t lane)
{
    const uint8_t* pat = out + (pos - off);
    uint8_t* to = out + pos;
    uint32_t r = (4 * lane) % off;
    const uint32_t step = 256 % off;
    for (uint32_t i0 = 4 * lane; i0 < len; i0 += 256) {
        uint32_t q = r, w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w |= uint32_t(pat[q]) << (8 * k);
            q = q + 1 == off ? 0 : q + 1;
        }
        if (i0 + 4 <= len) {
            store32(to + i0, w);
        } else {
            for (uint32_t k = 0; i0 + k < len; ++k)
                to[i0 + k] = uint8_t(w >> (8 * k));
        }
        r += step;
        if (r >= off)
            r -= off;
    }
}

// lz4::decode_block by one wave; the result is wave-uniform.
__device__ __forceinline__ int32_t
wave_decode_block(const uint8_t* src, uint32_t n, uint8_t* out, uint32_t cap, uint32_t lane)
{
    if (n == 0)
        return lz4::kDecEmpty;
    if (cap > 0x7FFFFFFFu)
        cap = 0x7FFFFFFFu;
    InWindow rd{ src, n, lane, 0, 0 };
    rd.fill(0);
    uint32_t ip = 0, op = 0, visible = 0;
    for (;;) {
        const uint32_t token = rd(ip++);
        uint64_t lit;
        if (const int32_t e = lz4::read_run(rd, ip, n, token >> 4, lit))
            return e;
        if (lit > n - ip)
            return lz4::kDecLiteralsInput;
        if (lit > cap - op)
            return lz4::kDecLiteralsOutput;
        wave_copy16(out + op, src + ip, uint32_t(lit), lane);
        ip += uint32_t(lit);
        op += uint32_t(lit);
        if (ip == n)
            return int32_t(op);
        if (n - ip < 2)
            return lz4::kDecTruncated;
        const uint32_t off = rd(ip) | (rd(ip + 1) << 8);
        ip += 2;
        uint64_t ml64;
        if (const int32_t e = lz4::read_run(rd, ip, n, token & 15, ml64))
            return e;
        ml64 += 4;
        if (off == 0)
            return lz4::kDecOffsetZero;
        if (off > op)
            return lz4::kDecOffsetBefore;
        if (ml64 > cap - op)
            return lz4::kDecMatchOutput;
        const uint32_t ml = uint32_t(ml64);
        // the source is out[op - off, op - off + min(off, ml)): fence when it
        // holds bytes stored since the last fence
        if (op - off + (off < ml ? off : ml) > visible) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            visible = op;
        }
        if (off >= ml)
            wave_copy16(out + op, out + (op - off), ml, lane);
        else
            wave_copy_periodic(out, op, off, ml, lane);
        op += ml;
        if (ip >= n)
            return lz4::kDecEndsInMatch;
    }
}

__global__ __launch_bounds__(64) void
lz4_decode_blocks_kernel(const uint8_t* comp, const uint64_t* __restrict__ comp_offsets,
                         const uint32_t* __restrict__ csize, uint8_t* out,
                         const uint64_t* __restrict__ out_offsets,
                         const uint32_t* __restrict__ cap, int32_t* __restrict__ results)
{
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const int32_t r =
      wave_decode_block(comp + comp_offsets[k], csize[k], out + out_offsets[k], cap[k], lane);
    if (lane == 0)
        results[k] = r;
}

__device__ __forceinline__ void
wave_zero(uint8_t* dst, uint32_t len, uint32_t lane)
{
    const uint32_t vecs = len >> 4;
    const u32x4 z = { 0u, 0u, 0u, 0u };
    for (uint32_t i = lane; i < vecs; i += 64)
        *reinterpret_cast<u32x4_u*>(dst + 16 * uint64_t(i)) = z;
    const uint32_t t = (vecs << 4) + lane;
    if (t < len)
        dst[t] = 0;
}

constexpr uint32_t kUnfilterSkip = 0; // meta pair: nothing to unfilter
constexpr uint32_t kUnfilterCopy = 3; // uniform form, shuffle 0

// Wave w of frame k: the header (every wave of a frame parses it and comes
// to the same answer), then splits w, w + waves, ... of the frame.  Statuses
// meet in status[k] by atomicMax on top of the 0 (kOk) queued before the
// kernel: they are numbered in the order of detection, and whatever one wave
// finds beyond kOk is the frame's.
__global__ __launch_bounds__(64) void
blosc_decode_kernel(BloscDecodeCall c, uint32_t k0, uint32_t waves)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t k = k0 + blockIdx.x / waves, w = blockIdx.x % waves;
    uint8_t* dst = c.dst + uint64_t(k) * c.dst_stride;
    // this wave's slice of a whole-chunk copy or fill
    const uint32_t slice = ((c.nbytes + waves - 1) / waves + 15u) & ~15u;
    const uint64_t s0 = uint64_t(w) * slice;
    const uint32_t slen = s0 >= c.nbytes ? 0u : (c.nbytes - uint32_t(s0) < slice ? c.nbytes - uint32_t(s0) : slice);

    blosc::FrameSpan span;
    blosc::Status st = c.table ? blosc::span_shard(c.table, k, c.frame_stride, c.base, &span)
                               : blosc::span_strided(c.frames, c.frame_stride, c.frame_bytes, k, &span);
    blosc::FrameInfo fi{};
    const uint8_t* f = c.frames + span.offset;
    if (st == blosc::kAbsent)
        wave_zero(dst + s0, slen, lane); // Zarr's fill value here
    else if (st == blosc::kOk)
        st = blosc::parse_header(f, span.extent, c.typesize, c.nbytes, &fi);
    const bool filtered = st == blosc::kOk && !fi.memcpyed && fi.filter != blosc::kNoFilter;
    if (w == 0 && lane == 0) {
        c.meta[2 * uint64_t(k)] = filtered ? fi.filter : kUnfilterSkip;
        c.meta[2 * uint64_t(k) + 1] = fi.blocksize;
        if (st != blosc::kOk)
            atomicMax(c.status + k, uint32_t(st));
    }
    if (st != blosc::kOk)
        return;
    if (fi.memcpyed) {
        wave_copy16(dst + s0, f + blosc::kHeaderBytes + s0, slen, lane);
        return;
    }
    uint8_t* out = filtered ? c.scratch + uint64_t(k) * c.nbytes : dst;
    for (uint32_t s = w; s < fi.total_splits; s += waves) {
        blosc::SplitRef r;
        bool ok = blosc::locate_split(fi, f, span.extent, s, &r) == blosc::kOk;
        if (ok) {
            if (r.csize == r.neb)
                wave_copy16(out + r.dst, f + r.src, r.neb, lane);
            else
                ok = wave_decode_block(f + r.src, r.csize, out + r.dst, r.neb, lane) ==
                     int32_t(r.neb);
        }
        if (!ok) {
            if (lane == 0)
                atomicMax(c.status + k, uint32_t(blosc::kCorrupt));
            return;
        }
    }
}

// ---- unfilter ----------------------------------------------------------------
//
// A buffer's blocks are cut into units of E elements: 8 for the byte
// unshuffle (TS 8-byte plane loads in, 8 * TS contiguous bytes out), 64 or 32
// for the bit unshuffle (8 * TS row loads of 8 or 4 bytes), 16 bytes for
// copied blocks.  A block's last unit also copies its blocksize % typesize
// tail.  Threads stride over a buffer's units, so any block size a header
// names is covered by a grid sized from (typesize, nbytes) alone.  TS 0: any
// typesize, byte by byte.

template<int TS>
constexpr uint32_t kBitUnitElems = (TS == 1 || TS == 2 || TS == 4) ? 64u : (TS == 8 ? 32u : 8u);

struct UnfilterCall
{
    const uint8_t* src;
    uint64_t src_stride;
    uint8_t* dst;
    uint64_t dst_stride;
    const uint32_t* meta; // null: mode and bs below
    uint32_t mode;        // 1 byte, 2 bit, kUnfilterCopy
    uint32_t bs;
    uint32_t ts;
    uint32_t nbytes;
    uint32_t blocks_per; // workgroups per buffer
    uint32_t k0;
};

template<int TS>
__device__ __forceinline__ void
unshuffle_unit(const uint8_t* sb, uint8_t* db, uint32_t ts, uint32_t ne, uint32_t q)
{
    const uint32_t e0 = q * 8;
    const uint32_t cnt = ne - e0 < 8 ? ne - e0 : 8;
    if constexpr (TS >= 2) {
        if (cnt == 8) {
            uint64_t plane[TS];
#pragma unroll
            for (int j = 0; j < TS; ++j)
                plane[j] = *reinterpret_cast<const u64_u*>(sb + uint64_t(j) * ne + e0);
            uint8_t e[8 * TS];
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int j = 0; j < TS; ++j)
                    e[k * TS + j] = uint8_t(plane[j] >> (8 * k));
            u32x4 v[TS / 2];
            __builtin_memcpy(v, e, sizeof(e));
            auto* d = reinterpret_cast<u32x4_u*>(db + uint64_t(e0) * TS);
#pragma unroll
            for (int i = 0; i < TS / 2; ++i)
                d[i] = v[i];
            return;
        }
    }
    for (uint32_t k = 0; k < cnt; ++k)
        for (uint32_t j = 0; j < ts; ++j)
            db[uint64_t(e0 + k) * ts + j] = sb[uint64_t(j) * ne + e0 + k];
}

template<int TS>
__device__ __forceinline__ void
unbitshuffle_unit(const uint8_t* sb, uint8_t* db, uint32_t ts, uint32_t ne, uint32_t q)
{
    constexpr uint32_t E = kBitUnitElems<TS>;
    constexpr uint32_t GB = E / 8; // bytes of every bit row a unit takes
    const uint32_t row = ne / 8;
    const uint32_t g0 = q * GB;
    const uint32_t cnt = row - g0 < GB ? row - g0 : GB;
    if constexpr (TS == 1 || TS == 2 || TS == 4 || TS == 8) {
        if (cnt == GB) {
            uint64_t rows[8 * TS];
#pragma unroll
            for (int r = 0; r < 8 * TS; ++r) {
                const uint8_t* p = sb + uint64_t(r) * row + g0;
                if constexpr (GB == 8)
                    rows[r] = *reinterpret_cast<const u64_u*>(p);
                else
                    rows[r] = *reinterpret_cast<const u32_u*>(p);
            }
            uint8_t e[E * TS];
#pragma unroll
            for (int j = 0; j < TS; ++j)
#pragma unroll
                for (uint32_t g = 0; g < GB; ++g) {
                    // byte b = bit row j * 8 + b of this group: bit 8b + k is
                    // bit b of byte j of element 8g + k; the transpose turns
                    // byte k into that element's byte
                    uint64_t x = 0;
#pragma unroll
                    for (int b = 0; b < 8; ++b)
                        x |= ((rows[j * 8 + b] >> (8 * g)) & 0xFFull) << (8 * b);
                    x = trans_bit_8x8(x);
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        e[(g * 8 + k) * TS + j] = uint8_t(x >> (8 * k));
                }
            u32x4 v[E * TS / 16];
            __builtin_memcpy(v, e, sizeof(e));
            auto* d = reinterpret_cast<u32x4_u*>(db + uint64_t(g0) * 8 * TS);
#pragma unroll
            for (uint32_t i = 0; i < E * TS / 16; ++i)
                d[i] = v[i];
            return;
        }
    }
    for (uint32_t g = 0; g < cnt; ++g)
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t m = g0 + g;
            for (uint32_t j = 0; j < ts; ++j) {
                uint32_t v = 0;
                for (uint32_t b = 0; b < 8; ++b)
                    v |= ((uint32_t(sb[uint64_t(j * 8 + b) * row + m]) >> k) & 1u) << b;
                db[uint64_t(m * 8 + k) * ts + j] = uint8_t(v);
            }
        }
}

template<int TS>
__global__ __launch_bounds__(256) void
blosc_unfilter_kernel(UnfilterCall c)
{
    const uint32_t ts = TS ? uint32_t(TS) : c.ts;
    const uint32_t k = c.k0 + blockIdx.x / c.blocks_per;
    const uint32_t t0 = (blockIdx.x % c.blocks_per) * 256 + threadIdx.x;
    const uint32_t T = c.blocks_per * 256;
    uint32_t mode = c.mode, bs = c.bs;
    if (c.meta) {
        mode = c.meta[2 * uint64_t(k)];
        bs = c.meta[2 * uint64_t(k) + 1];
        if (mode == kUnfilterSkip || bs == 0)
            return;
    }
    const uint8_t* s = c.src + uint64_t(k) * c.src_stride;
    uint8_t* d = c.dst + uint64_t(k) * c.dst_stride;
    const uint32_t full = c.nbytes / bs, left = c.nbytes % bs;
    // what a block of `bsz` bytes went through, and its units
    auto kind_of = [&](uint32_t bsz) {
        return mode == kUnfilterCopy ? uint32_t(blosc::kNoFilter) : blosc::block_filter(mode, ts, bsz);
    };
    auto units_of = [&](uint32_t bsz, uint32_t kind) {
        const uint32_t n = kind == blosc::kNoFilter ? (bsz + 15) / 16
                                                    : (bsz / ts + (kind == blosc::kByteShuffle ? 7u : kBitUnitElems<TS> - 1)) /
                                                        (kind == blosc::kByteShuffle ? 8u : kBitUnitElems<TS>);
        return n ? n : 1u;
    };
    const uint32_t kind_full = kind_of(bs), upb = units_of(bs, kind_full);
    const uint32_t kind_left = kind_of(left), upl = left ? units_of(left, kind_left) : 0u;
    const uint64_t units = uint64_t(full) * upb + upl;
    for (uint64_t u = t0; u < units; u += T) {
        uint32_t b, q, bsz, kind, n_units;
        if (u < uint64_t(full) * upb) {
            b = uint32_t(u / upb);
            q = uint32_t(u % upb);
            bsz = bs;
            kind = kind_full;
            n_units = upb;
        } else {
            b = full;
            q = uint32_t(u - uint64_t(full) * upb);
            bsz = left;
            kind = kind_left;
            n_units = upl;
        }
        const uint8_t* sb = s + uint64_t(b) * bs;
        uint8_t* db = d + uint64_t(b) * bs;
        if (kind == blosc::kNoFilter) {
            const uint32_t o = q * 16;
            if (bsz - o >= 16) {
                *reinterpret_cast<u32x4_u*>(db + o) = *reinterpret_cast<const u32x4_u*>(sb + o);
            } else {
                for (uint32_t i = o; i < bsz; ++i)
                    db[i] = sb[i];
            }
            continue;
        }
        const uint32_t ne = bsz / ts;
        if (kind == blosc::kByteShuffle)
            unshuffle_unit<TS>(sb, db, ts, ne, q);
        else
            unbitshuffle_unit<TS>(sb, db, ts, ne, q);
        if (q == n_units - 1) // the blocksize % typesize tail
            for (uint32_t o = ne * ts; o < bsz; ++o)
                db[o] = sb[o];
    }
}

// `per` workgroups for each of n buffers, in launches of fewer than 2^31
// workgroups: launch(k0, nk)
template<typename L>
hipError_t
for_buffer_slices(uint32_t n, uint32_t per, L&& launch)
{
    const uint32_t cap = 0x7FFFFFFFu / per;
    if (cap == 0)
        return hipErrorInvalidValue;
    for (uint64_t k0 = 0; k0 < n; k0 += cap) {
        launch(uint32_t(k0), uint32_t(n - k0 < cap ? n - k0 : cap));
        if (const hipError_t e = hipGetLastError(); e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace

hipError_t
launch_blosc_unfilter(int shuffle, uint32_t typesize, uint32_t blocksize, const void* src,
                      uint64_t src_stride, uint32_t nbytes, uint32_t n_buffers, void* dst,
                      uint64_t dst_stride, const uint32_t* meta, hipStream_t stream)
{
    if (typesize == 0 || (!meta && blocksize == 0) || shuffle < 0 || shuffle > 2 ||
        n_buffers == 0 || nbytes > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    if (nbytes == 0)
        return hipSuccess;
    // a thread for every 8 elements (or 16 bytes): larger units stride less
    const uint32_t unit = typesize > 2 ? 8 * typesize : 16;
    const uint64_t threads = (uint64_t(nbytes) + unit - 1) / unit;
    UnfilterCall c{ static_cast<const uint8_t*>(src), src_stride, static_cast<uint8_t*>(dst),
                    dst_stride, meta, shuffle ? uint32_t(shuffle) : kUnfilterCopy, blocksize,
                    typesize, nbytes, uint32_t((threads + 255) / 256), 0 };
    return for_buffer_slices(n_buffers, c.blocks_per, [&](uint32_t k0, uint32_t nk) {
        c.k0 = k0;
        const dim3 grid(nk * c.blocks_per), block(256);
        if (launch_log_on())
            launch_log_record("family=unfilter dtype=%u method=%d n_out=1 grid=%u block=256 "
                              "form=%s per_frame=%d",
                              typesize, shuffle, grid.x,
                              (typesize == 1 || typesize == 2 || typesize == 4 || typesize == 8 ||
                               typesize == 16)
                                ? "vec"
                                : "generic",
                              meta ? 1 : 0);
        switch (typesize) {
            case 1: hipLaunchKernelGGL(blosc_unfilter_kernel<1>, grid, block, 0, stream, c); break;
            case 2: hipLaunchKernelGGL(blosc_unfilter_kernel<2>, grid, block, 0, stream, c); break;
            case 4: hipLaunchKernelGGL(blosc_unfilter_kernel<4>, grid, block, 0, stream, c); break;
            case 8: hipLaunchKernelGGL(blosc_unfilter_kernel<8>, grid, block, 0, stream, c); break;
            case 16: hipLaunchKernelGGL(blosc_unfilter_kernel<16>, grid, block, 0, stream, c); break;
            default: hipLaunchKernelGGL(blosc_unfilter_kernel<0>, grid, block, 0, stream, c); break;
        }
    });
}

hipError_t
launch_lz4_decode_blocks(const void* comp, const uint64_t* comp_offsets, const uint32_t* csize,
                         void* out, const uint64_t* out_offsets, const uint32_t* cap, int32_t* results,
                         uint32_t n_splits, hipStream_t stream)
{
    if (n_splits == 0 || n_splits >= (1u << 31))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(lz4_decode_blocks_kernel, dim3(n_splits), dim3(64), 0, stream,
                       static_cast<const uint8_t*>(comp), comp_offsets, csize,
                       static_cast<uint8_t*>(out), out_offsets, cap, results);
    return hipGetLastError();
}

hipError_t
launch_blosc_decode(const BloscDecodeCall& call, uint32_t n_frames, hipStream_t stream)
{
    if (n_frames == 0 || call.nbytes == 0 || call.typesize == 0 || call.nbytes > blosc::kMaxBuffer)
        return hipErrorInvalidValue;
    if (const hipError_t e = hipMemsetAsync(call.status, 0, sizeof(uint32_t) * uint64_t(n_frames), stream);
        e != hipSuccess)
        return e;
    // a wave for every 8 KiB of a chunk, 32 at the most: c-blosc's splits are
    // 16 KiB and up, and a wave without a split ends at once
    const uint32_t waves = call.nbytes / 8192 < 1 ? 1u : (call.nbytes / 8192 > 32 ? 32u : call.nbytes / 8192);
    if (const hipError_t e = for_buffer_slices(n_frames, waves, [&](uint32_t k0, uint32_t nk) {
            if (launch_log_on())
                launch_log_record("family=blosc_decode dtype=%u grid=%u block=64 waves=%u "
                                  "frames=%u shard=%d",
                                  call.typesize, nk * waves, waves, nk, call.table ? 1 : 0);
            hipLaunchKernelGGL(blosc_decode_kernel, dim3(nk * waves), dim3(64), 0, stream, call,
                               k0, waves);
        });
        e != hipSuccess)
        return e;
    return launch_blosc_unfilter(1, call.typesize > 255 ? 1u : call.typesize, 0, call.scratch,
                                 call.nbytes, call.nbytes, n_frames, call.dst, call.dst_stride,
                                 call.meta, stream);
}

} // namespace aqz
