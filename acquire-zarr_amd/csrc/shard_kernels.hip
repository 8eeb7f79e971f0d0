// shard_kernels.hip — Zarr v3 shard assembly on gfx950 (include/aqz_shard.h,
// DESIGN.md §12.10): the scans that place a layer's chunk frames in their
// shards, the pack kernel that moves the bytes (the HBM-bound part), the
// index-table writer and the per-chunk has_data reduction.
#include "shard_kernels.hh"

#include "launch_log.hh"

namespace aqz {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1))); // any byte alignment (gfx950 global loads)
typedef uint32_t u32_u __attribute__((aligned(1)));

constexpr uint64_t kSentinel = ~0ull; // kUnwrittenSentinel (shard.hh)
constexpr uint32_t kBlock = 256;

// Bytes of frame c: its entry of the size table, never more than the stride
// (a frame is read inside [frame, frame + stride) whatever the table holds).
__device__ __forceinline__ uint64_t
frame_len(const ShardLayerArgs& a, uint32_t c)
{
    if (!a.sizes)
        return a.stride;
    const uint64_t n = a.sizes[c];
    return n < a.stride ? n : a.stride;
}

// inclusive scan over the 64 lanes of a wave, cross-lane
__device__ __forceinline__ uint64_t
wave_inclusive_scan(uint64_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up(static_cast<unsigned long long>(v), d);
        if (lane >= d)
            v += up;
    }
    return v;
}

// Exclusive scan over the 256 threads of a workgroup: within a wave by
// shuffles, across the four waves through `lds`.  *total: the sum of all.
// Every thread of the workgroup must call it (two barriers).
__device__ __forceinline__ uint64_t
block_exclusive_scan(uint64_t v, uint64_t* total, uint64_t* lds)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t incl = wave_inclusive_scan(v, lane);
    if (lane == 63)
        lds[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < kBlock / 64; ++k) {
        const uint64_t t = lds[k];
        before += k < wave ? t : 0;
        all += t;
    }
    __syncthreads(); // lds is written again by the next tile
    *total = all;
    return before + incl - v;
}

// One workgroup per shard: exclusive scan of (present ? size : 0) over the
// layer's slots in slot order, 256 slots a tile with a running carry, so any
// slot count.  Writes the layer's table pairs, each chunk's byte offset in
// its shard's segment, the segment's bytes and file offset, and the shard's
// new running offset (only thread 0 touches file_off[s]).
__global__ __launch_bounds__(kBlock) void
shard_scan_slots_kernel(ShardLayerArgs a, ShardGeometry g, uint32_t layer)
{
    __shared__ uint64_t lds[kBlock / 64];
    __shared__ uint64_t file0_s;
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    if (tid == 0)
        file0_s = a.file_off[s];
    __syncthreads();
    const uint64_t file0 = file0_s;
    const uint32_t spl = g.slots_per_layer;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < spl; base += kBlock) { // uniform trip count
        const uint32_t j = base + tid;
        const int32_t c = j < spl ? a.slot_chunk[uint64_t(s) * spl + j] : -1;
        const bool present = c >= 0 && (!a.has_data || a.has_data[c] != 0);
        const uint64_t len = present ? frame_len(a, uint32_t(c)) : 0;
        uint64_t total;
        const uint64_t at = carry + block_exclusive_scan(len, &total, lds);
        if (j < spl) {
            uint64_t* p =
              a.pairs + (uint64_t(s) * g.chunks_per_shard + uint64_t(layer) * spl + j) * 2;
            p[0] = present ? file0 + at : kSentinel;
            p[1] = present ? len : kSentinel;
            if (c >= 0)
                a.chunk_rel[c] = at;
        }
        carry += total;
    }
    if (tid == 0) {
        a.segments[3 * uint64_t(s) + 1] = carry;
        a.segments[3 * uint64_t(s) + 2] = file0;
        a.file_off[s] = file0 + carry;
    }
}

// One workgroup: exclusive scan of the segments' bytes over the shards, the
// same tiles and carry; the segments' starts in `out` and the total.
__global__ __launch_bounds__(kBlock) void
shard_scan_shards_kernel(uint64_t* segments, uint32_t n_shards)
{
    __shared__ uint64_t lds[kBlock / 64];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n_shards; base += kBlock) {
        const uint32_t s = base + tid;
        const uint64_t bytes = s < n_shards ? segments[3 * uint64_t(s) + 1] : 0;
        uint64_t total;
        const uint64_t at = carry + block_exclusive_scan(bytes, &total, lds);
        if (s < n_shards)
            segments[3 * uint64_t(s)] = at;
        carry += total;
    }
    if (tid == 0)
        segments[3 * uint64_t(n_shards)] = carry;
}

template<bool NT>
__device__ __forceinline__ u32x4
load16(const uint8_t* p)
{
    if constexpr (NT)
        return __builtin_nontemporal_load(reinterpret_cast<const u32x4_u*>(p));
    else
        return *reinterpret_cast<const u32x4_u*>(p);
}

template<bool NT>
__device__ __forceinline__ void
store16(uint8_t* p, u32x4 v)
{
    if constexpr (NT)
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
    else
        *reinterpret_cast<u32x4*>(p) = v;
}

// dst[0, n) = src[0, n) by a 256-thread workgroup, both at any byte address:
// the bytes up to dst's next 16-byte boundary one by one, then 16-byte
// vectors stored aligned and loaded wherever the source falls, four in
// flight per thread, then the last n % 16 bytes one by one.  Nothing outside
// src[0, n) is read and nothing outside dst[0, n) is written.
template<bool NT>
__device__ __forceinline__ void
copy_piece(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t t)
{
    uint32_t head = uint32_t(-reinterpret_cast<uintptr_t>(dst)) & 15u;
    head = head < n ? head : n;
    if (t < head)
        dst[t] = src[t];
    const uint8_t* s = src + head;
    uint8_t* d = dst + head;
    const uint32_t body = n - head, vecs = body >> 4;
    uint32_t i = t;
    for (; i + 3 * kBlock < vecs; i += 4 * kBlock) {
        u32x4 v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            v[k] = load16<NT>(s + 16ull * (i + k * kBlock));
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            store16<NT>(d + 16ull * (i + k * kBlock), v[k]);
    }
    for (; i < vecs; i += kBlock)
        store16<NT>(d + 16ull * i, load16<NT>(s + 16ull * i));
    const uint32_t done = vecs << 4;
    if (t < body - done)
        d[done + t] = s[done + t];
}

// Workgroup (c, p) = (blockIdx.x / pieces, blockIdx.x % pieces) copies piece p
// of frame c into its shard's segment, or exits when the chunk is absent or
// the frame ends before the piece: the grid needs no size on the host.
template<bool NT>
__global__ __launch_bounds__(kBlock) void
shard_pack_kernel(ShardLayerArgs a, uint32_t pieces, uint32_t piece)
{
    const uint32_t c = blockIdx.x / pieces, p = blockIdx.x % pieces;
    if (a.has_data && a.has_data[c] == 0)
        return;
    const uint64_t len = frame_len(a, c);
    const uint64_t beg = uint64_t(p) * piece;
    if (beg >= len)
        return;
    const uint64_t left = len - beg;
    const uint32_t n = left < piece ? uint32_t(left) : piece;
    const uint8_t* src = a.frames + uint64_t(c) * a.stride + beg;
    uint8_t* dst = a.out + a.segments[3 * uint64_t(a.chunk_shard[c])] + a.chunk_rel[c] + beg;
    copy_piece<NT>(dst, src, n, threadIdx.x);
}

// Table s = the shard's pairs, then their CRC-32C (Shard::write_table_,
// shard.cpp:145-165): one thread per 32-bit word of the tables, which lie
// 16 * chunks_per_shard + 4 bytes apart, so at 4-byte steps from any base.
__global__ __launch_bounds__(kBlock) void
shard_tables_kernel(const uint32_t* __restrict__ pair_words, const uint32_t* __restrict__ crcs,
                    const uint64_t* __restrict__ file_off, uint8_t* __restrict__ tables,
                    uint64_t* __restrict__ table_offsets, uint64_t words_per, uint64_t total_words)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= total_words)
        return;
    const uint64_t s = i / words_per, w = i % words_per;
    const uint32_t v = w + 1 < words_per ? pair_words[s * (words_per - 1) + w] : crcs[s];
    *reinterpret_cast<u32_u*>(tables + 4 * i) = v;
    if (w == 0)
        table_offsets[s] = file_off[s];
}

struct FlagBases
{
    uint32_t base[kShardFlagFrames];
};

// Thread (t, k): tile t of the launch's frame k.  Writers of one chunk's
// byte all store the same 1.
__global__ __launch_bounds__(kBlock) void
shard_chunk_flags_kernel(const uint8_t* __restrict__ flags, uint32_t n_tiles, uint32_t slots,
                         FlagBases bases, uint8_t* __restrict__ has_data)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x, k = blockIdx.y;
    if (t >= n_tiles)
        return;
    const uint8_t* f = flags + (uint64_t(k) * n_tiles + t) * slots;
    uint32_t any = 0;
    for (uint32_t i = 0; i < slots; ++i)
        any |= f[i];
    if (any)
        has_data[uint64_t(bases.base[k]) + t] = 1;
}

} // namespace

hipError_t
launch_shard_scan(const ShardLayerArgs& a, const ShardGeometry& g, uint32_t layer,
                  hipStream_t stream)
{
    if (g.n_shards == 0 || g.n_shards >= (1u << 31) || g.slots_per_layer == 0)
        return hipErrorInvalidValue;
    if (launch_log_on())
        launch_log_record("family=shard kernel=scan_slots grid=%u block=%u slots=%u shards=%u "
                          "piece=0",
                          g.n_shards, kBlock, g.slots_per_layer, g.n_shards);
    hipLaunchKernelGGL(shard_scan_slots_kernel, dim3(g.n_shards), dim3(kBlock), 0, stream, a, g,
                       layer);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    if (launch_log_on())
        launch_log_record("family=shard kernel=scan_shards grid=1 block=%u slots=%u shards=%u "
                          "piece=0",
                          kBlock, g.slots_per_layer, g.n_shards);
    hipLaunchKernelGGL(shard_scan_shards_kernel, dim3(1), dim3(kBlock), 0, stream, a.segments,
                       g.n_shards);
    return hipGetLastError();
}

hipError_t
launch_shard_pack(const ShardLayerArgs& a, const ShardGeometry& g, uint32_t piece,
                  bool nontemporal, hipStream_t stream)
{
    if (piece == 0 || a.stride == 0 || g.chunks_per_layer == 0)
        return hipErrorInvalidValue;
    const uint64_t pieces = (a.stride + piece - 1) / piece;
    if (pieces * g.chunks_per_layer >= (1ull << 31))
        return hipErrorInvalidValue;
    const uint32_t grid = uint32_t(pieces * g.chunks_per_layer);
    if (launch_log_on())
        launch_log_record("family=shard kernel=pack%s grid=%u block=%u slots=%u shards=%u "
                          "piece=%u",
                          nontemporal ? "_nt" : "", grid, kBlock, g.slots_per_layer, g.n_shards,
                          piece);
    if (nontemporal)
        hipLaunchKernelGGL(shard_pack_kernel<true>, dim3(grid), dim3(kBlock), 0, stream, a,
                           uint32_t(pieces), piece);
    else
        hipLaunchKernelGGL(shard_pack_kernel<false>, dim3(grid), dim3(kBlock), 0, stream, a,
                           uint32_t(pieces), piece);
    return hipGetLastError();
}

hipError_t
launch_shard_tables(const uint64_t* pairs, const uint32_t* crcs, const uint64_t* file_off,
                    uint8_t* tables, uint64_t* table_offsets, const ShardGeometry& g,
                    hipStream_t stream)
{
    const uint64_t words_per = 4ull * g.chunks_per_shard + 1;
    const uint64_t total = words_per * g.n_shards;
    const uint64_t grid = (total + kBlock - 1) / kBlock;
    if (g.n_shards == 0 || grid >= (1ull << 31))
        return hipErrorInvalidValue;
    if (launch_log_on())
        launch_log_record("family=shard kernel=tables grid=%u block=%u slots=%u shards=%u piece=0",
                          uint32_t(grid), kBlock, g.slots_per_layer, g.n_shards);
    hipLaunchKernelGGL(shard_tables_kernel, dim3(uint32_t(grid)), dim3(kBlock), 0, stream,
                       reinterpret_cast<const uint32_t*>(pairs), crcs, file_off, tables,
                       table_offsets, words_per, total);
    return hipGetLastError();
}

hipError_t
launch_shard_chunk_flags(const uint8_t* tile_nonzero, uint32_t n_frames, uint32_t n_tiles,
                         uint32_t flag_slots, const uint32_t* host_base, uint8_t* has_data,
                         hipStream_t stream)
{
    if (n_frames == 0 || n_tiles == 0 || flag_slots == 0 || n_tiles >= (1u << 31))
        return hipErrorInvalidValue;
    const uint32_t gx = (n_tiles + kBlock - 1) / kBlock;
    for (uint32_t k0 = 0; k0 < n_frames; k0 += kShardFlagFrames) {
        const uint32_t n = n_frames - k0 < kShardFlagFrames ? n_frames - k0 : kShardFlagFrames;
        FlagBases b{};
        for (uint32_t k = 0; k < n; ++k)
            b.base[k] = host_base[k0 + k];
        if (launch_log_on())
            launch_log_record("family=shard kernel=chunk_flags grid=%u block=%u slots=%u "
                              "shards=0 piece=0",
                              gx * n, kBlock, flag_slots);
        hipLaunchKernelGGL(shard_chunk_flags_kernel, dim3(gx, n), dim3(kBlock), 0, stream,
                           tile_nonzero + uint64_t(k0) * n_tiles * flag_slots, n_tiles, flag_slots,
                           b, has_data);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace aqz
