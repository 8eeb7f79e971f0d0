// ds_kernels.hip — CDNA4 (gfx950) kernels for the acquire-zarr multiscale
// pyramid.  See ds_kernels.hh for the contract and DESIGN.md for the
// roofline analysis.
//
// Semantics restated from acquire-zarr v0.8.1 src/streaming/downsampler.cpp:
//   reducers        :39-137 (decimate/mean/min/max, 4- and 2-operand forms)
//   scale_image<T>  :139-206 (2x2 reduce, odd right/bottom edge replicated)
//   average_two_frames<T> :208-246 (dst = f(earlier, current))
// The arithmetic is bit-exact with the reference binary: narrow integers are
// promoted to int, 32/64-bit integer sums wrap, floats sum left to right and
// divide by 4 (exact as a multiply by 0.25), min/max are compare-select
// chains seeded with the first operand so NaN order matches.
//
// Design: this is an HBM-bound stencil, not a contraction — no MFMA.  Each
// wave owns a tile of 64 lanes x 16 bytes wide and 2^NL rows tall, issues
// all 2^NL row loads (16 B per lane, 1 KiB per wave instruction) before any
// arithmetic, and reduces the pyramid in registers: in-lane while a lane
// still holds >= 2 columns of a level, then across lanes with __shfl_down at
// doubling strides.  Every level of the run is written from the same pass,
// so the base frame is read exactly once.  LDS only assembles stores: the
// band kernels (cascade_band_kernel) stage each level's rows of a whole row
// band in LDS so that they leave as full 64-byte bursts, and
// transpose_kernel turns its tiles through LDS.
#include "ds_kernels.hh"

// What the fused launchers launch is decided on the host (ds_plan.cpp);
// ds_dispatch.cpp hands the plan to run_cascade, run_cascade_tiled, run_volume.
// The launchers' decision log (launch_log.hh, launch_log.cpp) is part of the
// library build, which always sets AQZ_SHARDS; a tools/ probe that includes
// this file directly builds alone and records nothing.
#ifdef AQZ_SHARDS
#include "launch_log.hh"
#else
namespace aqz {
inline bool
launch_log_on()
{
    return false;
}
inline void
launch_log_record(const char*, ...)
{
}
} // namespace aqz
#endif

// Build sharding (acquire-zarr_amd/Makefile): the library compiles this file
// AQZ_SHARDS times; shard k instantiates the kernels of the dtypes whose
// code % AQZ_SHARDS == k, and its dtype-dispatching launchers are named
// <launcher>_shard<k>.  ds_dispatch.cpp routes each call to its shard; the
// dtype-independent helpers are ds_plan.cpp's.  The shards compile in
// parallel: one unit held over a thousand kernel instantiations.  Included
// directly (the tools/ probes, followed by ds_plan.cpp and ds_dispatch.cpp),
// the file builds unsharded.
#ifndef AQZ_SHARDS
#define AQZ_SHARDS 1
#endif
#ifndef AQZ_SHARD
#define AQZ_SHARD 0
#endif
#if AQZ_SHARDS > 1
#define AQZ_CAT2_(a, b) a##b
#define AQZ_CAT_(a, b) AQZ_CAT2_(a, b)
#define AQZ_SHARDED(name) AQZ_CAT_(name##_shard, AQZ_SHARD)
#else
#define AQZ_SHARDED(name) name
#endif

#include <algorithm>
#include <type_traits>

namespace aqz {
namespace {

// Native 16-byte vector (HIP's uint4 is a struct; the builtins want this).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The same widths at byte alignment, for the fused kernels' frame accesses:
// a batch of odd-width frames puts rows (and frames) at any byte offset.
// gfx950 global loads/stores take unaligned addresses (the compiler emits the
// same global_load_dwordx4 / global_store_dwordx2 for these types); the
// bytes a wave touches are unchanged, so HBM traffic is unchanged.
typedef u32x4 u32x4_u __attribute__((aligned(1)));
typedef uint64_t u64_u __attribute__((aligned(1)));
typedef uint32_t u32_u __attribute__((aligned(1)));
typedef uint16_t u16_u __attribute__((aligned(1)));

// ---- reducers --------------------------------------------------------------

// NaN payloads exactly as the reference binary makes them.  IEEE 754 leaves
// a NaN result's payload open; the reference's compiled float mean (x86 SSE
// addss/divss, downsampler.cpp:48-51,108-112) returns the FIRST source
// operand's NaN, quieted, when it is a NaN, else the second's, and for an
// invalid sum (inf + -inf) the negative "default NaN" (sign and quiet bits
// set, zero payload).  gfx950's v_add/v_div pick differently (inf - inf
// gives the positive quiet NaN), so the kernels keep
// the plain arithmetic and rebuild the bits only where the result is a NaN:
// one compare per output in the common case, the walk below when a wave has
// a NaN lane.  The walk selects on bits (integer ops) so nothing
// canonicalises the payload; divide by 4 or 2 keeps a quiet NaN unchanged on
// x86.  The
// oracle states the same rule (oracle/ds_oracle.c add_<T>).
template<typename T>
struct float_bits;
template<>
struct float_bits<float>
{
    using U = uint32_t;
    static constexpr U quiet() { return 0x00400000u; }
    static constexpr U default_nan() { return 0xFFC00000u; }
};
template<>
struct float_bits<double>
{
    using U = uint64_t;
    static constexpr U quiet() { return 0x0008000000000000ull; }
    static constexpr U default_nan() { return 0xFFF8000000000000ull; }
};

// x86 `x + y` with its NaN rule (x the first source), as selects on bits.
template<typename T>
__device__ __forceinline__ T
x86_add(T x, T y)
{
    using FB = float_bits<T>;
    using U = typename FB::U;
    const T s = x + y;
    const U bx = __builtin_bit_cast(U, x) | FB::quiet();
    const U by = __builtin_bit_cast(U, y) | FB::quiet();
    const U bs = (s != s) ? FB::default_nan() : __builtin_bit_cast(U, s);
    return __builtin_bit_cast(T, (x != x) ? bx : ((y != y) ? by : bs));
}

// Whether any lane of the wave holds a NaN result.  The fix-up runs behind a
// wave-uniform branch.  A lane-divergent one (only the NaN lanes inside) gave
// wrong outputs in edge tiles of 16-byte f32 tiles on 4 of 256 fuzz cases
// (round 5): in-range lanes read the next row's chunk as zero or stale bits.
// Round 6 (tools/divergent/) narrowed it to the divergent
// branch together with exec-masked edge loads (load_chunk); either one alone
// is exact, and tests/test_gpu_divergent.py reruns round 5's launch.
__device__ __forceinline__ bool
wave_any(bool p)
{
    return __builtin_amdgcn_ballot_w64(p) != 0;
}

#ifdef AQZ_NAN_FIXUP_DIVERGENT
// The round-5 lane-divergent form (branches on the NaN lanes only), kept for
// the regression probe (tools/divergent/, tests/test_gpu_divergent.py).
template<typename T>
__device__ __forceinline__ T
x86_add_branchy(T x, T y)
{
    using FB = float_bits<T>;
    using U = typename FB::U;
    const T s = x + y;
    U r;
    if (x != x)
        r = __builtin_bit_cast(U, x) | FB::quiet();
    else if (y != y)
        r = __builtin_bit_cast(U, y) | FB::quiet();
    else if (s != s)
        r = FB::default_nan();
    else
        return s;
    return __builtin_bit_cast(T, r);
}
#endif

template<typename T>
__device__ __forceinline__ T
mean4(T a, T b, T c, T d)
{
    if constexpr (std::is_floating_point_v<T>) {
        const T r = (((a + b) + c) + d) / T(4);
#ifdef AQZ_NAN_FIXUP_DIVERGENT
        if (__builtin_expect(r != r, 0))
            return x86_add_branchy(x86_add_branchy(x86_add_branchy(a, b), c), d);
        return r;
#endif
        if (__builtin_expect(wave_any(r != r), 0)) {
            // the chain's first NaN is the value (x86 keeps it through the
            // later adds and the divide); other lanes keep theirs
            const T n = x86_add(x86_add(x86_add(a, b), c), d);
            return (r != r) ? n : r;
        }
        return r;
    } else if constexpr (sizeof(T) < sizeof(int)) {
        return T((int(a) + int(b) + int(c) + int(d)) / 4);
    } else {
        using U = std::make_unsigned_t<T>;
        const T s = T(U(a) + U(b) + U(c) + U(d));
        return T(s / T(4));
    }
}

template<typename T>
__device__ __forceinline__ T
mean2(T a, T b)
{
    if constexpr (std::is_floating_point_v<T>) {
        const T r = (a + b) / T(2);
#ifdef AQZ_NAN_FIXUP_DIVERGENT
        if (__builtin_expect(r != r, 0))
            return x86_add_branchy(a, b);
        return r;
#endif
        if (__builtin_expect(wave_any(r != r), 0)) {
            const T n = x86_add(a, b);
            return (r != r) ? n : r;
        }
        return r;
    } else if constexpr (sizeof(T) < sizeof(int)) {
        return T((int(a) + int(b)) / 2);
    } else {
        using U = std::make_unsigned_t<T>;
        const T s = T(U(a) + U(b));
        return T(s / T(2));
    }
}

template<typename T, int M>
__device__ __forceinline__ T
reduce4(T a, T b, T c, T d)
{
    if constexpr (M == kDecimate) {
        return a;
    } else if constexpr (M == kMean) {
        return mean4(a, b, c, d);
    } else if constexpr (M == kMin) {
        T v = a;
        v = (b < v) ? b : v;
        v = (c < v) ? c : v;
        v = (d < v) ? d : v;
        return v;
    } else {
        T v = a;
        v = (b > v) ? b : v;
        v = (c > v) ? c : v;
        v = (d > v) ? d : v;
        return v;
    }
}

template<typename T, int M>
__device__ __forceinline__ T
reduce2(T a, T b)
{
    if constexpr (M == kDecimate) {
        return a;
    } else if constexpr (M == kMean) {
        return mean2(a, b);
    } else if constexpr (M == kMin) {
        return a < b ? a : b;
    } else {
        return a > b ? a : b;
    }
}

// ---- cross-lane move of any 1/2/4/8-byte element ---------------------------

template<typename T>
__device__ __forceinline__ T
shfl_down_any(T v, int delta)
{
    if constexpr (sizeof(T) <= 4) {
        uint32_t x = 0;
        __builtin_memcpy(&x, &v, sizeof(T));
        x = __shfl_down(x, (unsigned)delta);
        T r;
        __builtin_memcpy(&r, &x, sizeof(T));
        return r;
    } else {
        unsigned long long x;
        __builtin_memcpy(&x, &v, 8);
        x = __shfl_down(x, (unsigned)delta);
        T r;
        __builtin_memcpy(&r, &x, 8);
        return r;
    }
}

// Store N contiguous elements of T as one access at any byte alignment
// (optionally non-temporal: write-once pyramid levels).
template<typename T, int N, bool NT = false>
__device__ __forceinline__ void
store_vec(T* dst, const T (&v)[N])
{
    constexpr int B = int(sizeof(T)) * N;
    static_assert(B == 1 || B == 2 || B == 4 || B == 8 || B == 16 || B == 32, "width");
    if constexpr (B == 32) {
        // a lane's whole 32-byte load (the tiled base store): two accesses
        T half[2][N / 2];
        __builtin_memcpy(half, v, 32);
        store_vec<T, N / 2, NT>(dst, half[0]);
        store_vec<T, N / 2, NT>(dst + N / 2, half[1]);
    } else if constexpr (B == 16) {
        u32x4 q;
        __builtin_memcpy(&q, v, 16);
        u32x4_u* d = reinterpret_cast<u32x4_u*>(dst); // typedef keeps align 1
        if constexpr (NT)
            __builtin_nontemporal_store(q, d);
        else
            *d = q;
    } else if constexpr (B == 8) {
        uint64_t q;
        __builtin_memcpy(&q, v, 8);
        u64_u* d = reinterpret_cast<u64_u*>(dst); // typedef keeps align 1
        if constexpr (NT)
            __builtin_nontemporal_store(q, d);
        else
            *d = q;
    } else if constexpr (B == 4) {
        uint32_t q;
        __builtin_memcpy(&q, v, 4);
        u32_u* d = reinterpret_cast<u32_u*>(dst); // typedef keeps align 1
        if constexpr (NT)
            __builtin_nontemporal_store(q, d);
        else
            *d = q;
    } else if constexpr (B == 2) {
        uint16_t q;
        __builtin_memcpy(&q, v, 2);
        u16_u* d = reinterpret_cast<u16_u*>(dst); // typedef keeps align 1
        if constexpr (NT)
            __builtin_nontemporal_store(q, d);
        else
            *d = q;
    } else {
        uint8_t q;
        __builtin_memcpy(&q, v, 1);
        uint8_t* d = reinterpret_cast<uint8_t*>(dst);
        if constexpr (NT)
            __builtin_nontemporal_store(q, d);
        else
            *d = q;
    }
}

#ifdef AQZ_EDGE_SHIFT_ASM
// probe variants (tools/divergent): the 64-bit shifts as
// inline asm, =2 with two wait states after each one
__device__ __forceinline__ uint64_t
probe_shr64(uint64_t x, uint32_t n)
{
    uint64_t r;
#if AQZ_EDGE_SHIFT_ASM == 2
    asm volatile("v_lshrrev_b64 %0, %1, %2\n\ts_nop 1" : "=v"(r) : "v"(n), "v"(x));
#else
    asm volatile("v_lshrrev_b64 %0, %1, %2" : "=v"(r) : "v"(n), "v"(x));
#endif
    return r;
}
__device__ __forceinline__ uint64_t
probe_shl64(uint64_t x, uint32_t n)
{
    uint64_t r;
#if AQZ_EDGE_SHIFT_ASM == 2
    asm volatile("v_lshlrev_b64 %0, %1, %2\n\ts_nop 1" : "=v"(r) : "v"(n), "v"(x));
#else
    asm volatile("v_lshlrev_b64 %0, %1, %2" : "=v"(r) : "v"(n), "v"(x));
#endif
    return r;
}
#endif

// Shift a little-endian LB-byte vector down by `bytes` (0 <= bytes < LB).
template<int LB>
__device__ __forceinline__ void
shift_down(uint64_t (&q)[LB / 8], uint32_t bytes)
{
#ifdef AQZ_EDGE_SHIFT32
    // probe variant (tools/divergent): the same shift in
    // 32-bit words, no 64-bit shifts; `bytes` >= LB gives zero
    if constexpr (LB == 16) {
        uint32_t w[4], o[4];
        __builtin_memcpy(w, q, 16);
        const uint32_t k = bytes >> 2, r = (bytes & 3u) * 8u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t j = uint32_t(i) + k;
            const uint32_t a = j == 0 ? w[0] : j == 1 ? w[1] : j == 2 ? w[2] : j == 3 ? w[3] : 0u;
            const uint32_t b = j == 0 ? w[1] : j == 1 ? w[2] : j == 2 ? w[3] : 0u;
            o[i] = r ? (a >> r) | (b << (32u - r)) : a;
        }
        __builtin_memcpy(q, o, 16);
        return;
    }
#endif
    const uint32_t n = 8 * bytes;
#ifdef AQZ_EDGE_SHIFT_ASM
    if constexpr (LB == 16) {
        uint64_t lo = q[0], hi = q[1];
        if (n >= 64) {
            lo = probe_shr64(hi, n - 64);
            hi = 0;
        } else if (n) {
            lo = probe_shr64(lo, n) | probe_shl64(hi, 64 - n);
            hi = probe_shr64(hi, n);
        }
        q[0] = lo;
        q[1] = hi;
        return;
    }
#endif
    if constexpr (LB == 8) {
        q[0] = n ? q[0] >> n : q[0];
    } else {
        uint64_t lo = q[0], hi = q[1];
        if (n >= 64) {
            lo = hi >> (n - 64);
            hi = 0;
        } else if (n) {
            lo = (lo >> n) | (hi << (64 - n));
            hi >>= n;
        }
        q[0] = lo;
        q[1] = hi;
    }
}

// E elements of T from row `row` starting at column `col`, as one LB-byte
// vector load at any alignment.  EDGE (tiles that touch the frame's right or
// bottom edge): rows past the frame (`row_ok` false) and chunks starting at
// or past `W` read as zero.  A chunk that straddles the row end is loaded
// whole when the bytes past the row end are still inside the buffer
// (`tail_safe`: they belong to the next row or frame; the kernel replaces
// those columns by edge replication anyway).  On the batch's last row it is
// loaded instead as the row's last E elements and shifted down in registers,
// so nothing outside the buffer is read.  Needs W >= E (cascade_fits).
// Every lane issues one vector load either way: no divergent element loads,
// and the edge path costs the interior path no registers.
//
// Out-of-range chunks (rows past the frame, columns past W) are skipped by
// an exec-masked load and read as zero.  AQZ_EDGE_LOAD_SELECT (probe builds,
// tools/divergent/) loads on every lane instead — from the row's last chunk,
// or from `safe` (the frame's first elements) for rows past the frame — and
// selects the zero afterwards.  That form cures the round-5 divergent-branch
// build, but it gave one wrong pixel in one default fuzz
// run, so the product keeps the masked form with its long clean record.
template<typename T, int E, bool NT, bool EDGE>
__device__ __forceinline__ void
load_chunk(T* out, const T* row, uint32_t col, uint32_t W, bool row_ok, bool tail_safe,
           const T* safe)
{
    constexpr int LB = E * int(sizeof(T));
    static_assert(LB == 16 || LB == 8, "fused loads are 8 or 16 bytes");
    uint32_t at = col;
    bool ok = true;
    if constexpr (EDGE) {
        ok = row_ok && col < W;
        if (col + E > W && !tail_safe)
            at = W - E;
    }
    uint64_t q[LB / 8] = {};
#ifdef AQZ_EDGE_LOAD_SELECT
    if constexpr (EDGE) {
        // past the row end: the row's last chunk, whose line the wave's last
        // in-range lane reads anyway (=1), or `safe` (=2); past the frame's
        // last row: `safe`
        const T* a0 = ok ? row + at : (row_ok && AQZ_EDGE_LOAD_SELECT == 1) ? row + (W - E) : safe;
        uint64_t w[LB / 8];
        if constexpr (LB == 16) {
            const u32x4 v = NT ? __builtin_nontemporal_load(reinterpret_cast<const u32x4_u*>(a0))
                               : *reinterpret_cast<const u32x4_u*>(a0);
            __builtin_memcpy(w, &v, 16);
        } else {
            w[0] = NT ? __builtin_nontemporal_load(reinterpret_cast<const u64_u*>(a0))
                      : *reinterpret_cast<const u64_u*>(a0);
        }
#pragma unroll
        for (int i = 0; i < LB / 8; ++i)
            q[i] = ok ? w[i] : 0ull;
        shift_down<LB>(q, (col - at) * uint32_t(sizeof(T)));
        __builtin_memcpy(out, q, LB);
        return;
    }
#endif
    (void)safe;
    if (ok) {
        // explicit byte-aligned pointer types (a template argument would drop
        // the typedef's alignment)
        if constexpr (LB == 16) {
            const u32x4_u* a = reinterpret_cast<const u32x4_u*>(row + at);
            const u32x4 v = NT ? __builtin_nontemporal_load(a) : *a;
            __builtin_memcpy(q, &v, 16);
        } else {
            const u64_u* a = reinterpret_cast<const u64_u*>(row + at);
            q[0] = NT ? __builtin_nontemporal_load(a) : *a;
        }
    }
#ifdef AQZ_EDGE_DEBUG
    // probe variant (tools/divergent): report in-range edge chunks that
    // loaded as all-zero bits (the round-5 failure's signature)
    if constexpr (EDGE) {
        bool zero = true;
#pragma unroll
        for (int i = 0; i < LB / 8; ++i)
            zero = zero && q[i] == 0;
        if (ok && zero)
            printf("AQZDBG blk %u lane %u row %p col %u at %u W %u tail %d\n", blockIdx.x,
                   threadIdx.x, (const void*)row, col, at, W, int(tail_safe));
    }
#endif
    if constexpr (EDGE)
        shift_down<LB>(q, (col - at) * uint32_t(sizeof(T)));
    __builtin_memcpy(out, q, LB);
}

// ---- fused cascade ---------------------------------------------------------

// Division by a runtime constant as a multiply-high and shifts (Granlund &
// Montgomery; exact for every 32-bit n).  The tiled stores divide row and
// column indices by the chunk shape: per block, not per element, but on
// small frames a block is a few KiB and a 32-bit division's ~40 scalar
// instructions showed up (512^2 u8 tiled).
struct FastDiv
{
    uint32_t d = 1, m = 0, s = 0; // d == 1: m = 0, q = n

    static FastDiv make(uint32_t d)
    {
        FastDiv f;
        f.d = d ? d : 1;
        if (f.d == 1)
            return f;
        uint32_t l = 0;
        while ((1ull << l) < f.d)
            ++l;
        f.m = uint32_t(((uint64_t(1) << 32) * ((uint64_t(1) << l) - f.d)) / f.d + 1);
        f.s = l - 1;
        return f;
    }
    __device__ __forceinline__ uint32_t div(uint32_t n) const
    {
        if (d == 1)
            return n;
        const uint32_t t = __umulhi(n, m);
        return (t + ((n - t) >> 1)) >> s;
    }
};

// One chunk-tiled output level of the tiled cascade.  Frame f's tile
// t = ty * ntx + tx (tr x tc elements, row-major; the padded level is pw x ph)
// at tdst + base(f) + t * tstride, where base(f) = f * tframe_elems and
// tstride = tr * tc (tiles back to back), or — for a chunk lattice
// (launch_cascade_tiled with TiledOut::frame_offsets) — base(f) = foff[f] and
// tstride = the distance between neighbouring chunks: the reference's
// chunks_[tile + tile_group_offset(f)] at chunk_internal_offset(f)
// (array.cpp:563-617, array.dimensions.cpp:265-314).
// Zero scan.  slots > 0 (wave blocks and tiles nest): tile t owns `slots`
// flag bytes, one per (block, tile) pair (slots_x across), and every byte is
// written exactly once — by its wave, or as 0 by the zero-fill waves for
// blocks past the grid — so nothing is cleared first.  slots == 0: one byte
// per tile, cleared before the launch, set to 1 by every wave storing a
// nonzero byte into the tile.
// Zero-fill waves (wave ids past the grid's blocks): the padded area the
// blocks do not reach — columns >= cov_w, and rows >= cov_h — per
// (frame, level, padded row) item (zrows items per frame here), plus the
// slot flags of those blocks.
struct TiledLevel
{
    uint8_t* tdst;
    uint8_t* flags;
    uint64_t tframe_elems;
    const uint64_t* foff; // per-frame element offsets (chunk lattice), or null
    uint64_t tstride;     // elements from one tile to the next
    uint32_t tr, tc, ntx, pw, ph;
    uint32_t slots, slots_x, flags_frame;
    uint32_t cov_w, cov_h, zrows;
    FastDiv dr, dc; // by tr, by tc
};

// Element offset of frame f's tile 0 (wave-uniform f: a scalar load).
__device__ __forceinline__ uint64_t
tiled_frame_base(const TiledLevel& t, uint32_t f)
{
    return t.foff ? t.foff[f] : uint64_t(f) * t.tframe_elems;
}

struct CascadeParams
{
    const uint8_t* src;
    uint64_t src_frame_elems;
    uint32_t W, H;         // input level geometry
    uint32_t units_x;      // column tiles per frame
    uint32_t units_y;      // row tiles per frame
    uint32_t total_units;  // units_x * units_y * n_frames
    uint8_t* dst[kMaxFusedLevels];
    uint64_t dst_frame_elems[kMaxFusedLevels];
    uint32_t w[kMaxFusedLevels];
    uint32_t h[kMaxFusedLevels];
    // Chunk-tiled outputs (cascade_kernel<..., TILED>, launch_cascade_tiled), one
    // TiledLevel per level; dst[J-1] may then be null (no row-major copy).
    TiledLevel tl[kMaxFusedLevels];
    uint32_t zitems;                 // items per frame, all levels
    FastDiv zdiv;                    // by zitems
    uint32_t zwaves;                 // zero-fill waves: the grid's first zwaves / (waves per block) blocks
    uint32_t main_blocks;            // blocks of cascade waves after them
    uint32_t remap;                  // 1: XCD-contiguous block order (cascade_kernel)
    uint32_t wb;                     // bit J-1: level J's row-major stores write-back, not nt
    uint32_t order;                  // unit order: 0 columns fastest, 1 frames, 2 row bands
    uint32_t seg_w;                  // > 0: a workgroup is seg_w column tiles of one row band
    uint32_t nt;                     // launcher's choice of load policy (load_nt)
    uint32_t band_last;              // K > 0: the band's last K waves to finish store it (no barrier)
    uint32_t seg_rowwise;            // 1: band segments of misaligned rows (StageCtx::rowb)
    uint32_t upw;                    // units per wave (cascade_kernel, columns-fastest order)
};

// cascade_base_kernel (launch_cascade_tiled with a base): the input level goes
// out chunk-tiled as well, as tl0 (its size is W x H).  A kernel argument of
// its own beside CascadeParams, so that every other kernel keeps its
// arguments, and the levels' code its parameter block, as they are.
struct BaseLevel
{
    TiledLevel tl0;
    FastDiv zdiv0; // by tl0.zrows (zero_fill_base); zitems counts the levels alone
};

// Columns of T per lane in the fused cascade: 16 bytes for 1- and 2-byte
// types, 32 bytes (two 16-byte loads per row) for 4- and 8-byte types, which
// keeps levels 1-3 in-lane and halves the cross-lane shuffles.  A/B on
// MI355X (tools/microbench.hip f32): 4096^2 f32 x64 batch 1083 -> 975 us,
// bit-identical; the same widening measured slower for u16 (562 vs 470 us).
template<typename T>
constexpr int kCascadeCols = sizeof(T) >= 4 ? 32 / int(sizeof(T)) : 16 / int(sizeof(T));

// Lanes per column group at level J when each lane starts with C columns.
template<int C, int J>
constexpr int kLaneStride = ((1 << J) >= C) ? ((1 << J) / C) : 1;

// One XY level in registers: level J (1-based within the run) from level J-1
// held as RI rows x CI columns per lane.  CI == 1 means the lane holds one
// column of a column group spread over kLaneStride<C, J-1> lanes (only the
// group's first lane is meaningful); the right-hand neighbour then comes
// from that many lanes up.  `win`/`hin` are level J-1's size, `cin0`/`rin0`
// the lane's first column/row there (edge replication needs them).
template<typename T, int M, int C, int J, int RI, int CI, bool EDGE>
__device__ __forceinline__ void
xy_step(const T (&in)[RI][CI],
        T (&out)[RI / 2][(CI >= 2) ? CI / 2 : 1],
        uint32_t win,
        uint32_t hin,
        uint32_t cin0,
        uint32_t rin0)
{
    constexpr int RO = RI / 2;
    constexpr bool kInLane = CI >= 2;
    constexpr int CO = kInLane ? CI / 2 : 1;
    constexpr int SI = kLaneStride<C, J - 1>;
#pragma unroll
    for (int r = 0; r < RO; ++r) {
#pragma unroll
        for (int c = 0; c < CO; ++c) {
            T here, right, down, diag;
            if constexpr (kInLane) {
                here = in[2 * r][2 * c];
                right = in[2 * r][2 * c + 1];
                down = in[2 * r + 1][2 * c];
                diag = in[2 * r + 1][2 * c + 1];
            } else {
                here = in[2 * r][0];
                down = in[2 * r + 1][0];
                right = shfl_down_any(here, SI);
                diag = shfl_down_any(down, SI);
            }
            if constexpr (EDGE) {
                // scale_image edge replication (downsampler.cpp:186-197):
                // last column of an odd width / last row of an odd height.
                const uint32_t col = cin0 + (kInLane ? 2u * c : 0u);
                const bool pw = col + 1 >= win;
                const bool ph = rin0 + 2u * r + 1 >= hin;
                const T r_ = pw ? here : right;
                const T g_ = ph ? r_ : (pw ? down : diag);
                const T d_ = ph ? here : down;
                right = r_;
                down = d_;
                diag = g_;
            }
            out[r][c] = reduce4<T, M>(here, right, down, diag);
        }
    }
}

// Write the lane's RO x CO block of level J (frame base `dst`, row pitch
// `wout`); only column-group leaders store, edge tiles clip to the level.
template<typename T, int C, int J, int RO, int CO, bool EDGE, bool NTS>
__device__ __forceinline__ void
store_level(T* dst,
            const T (&out)[RO][CO],
            uint32_t wout,
            uint32_t hout,
            uint32_t col0,
            uint32_t row0,
            int lane)
{
    constexpr int SO = kLaneStride<C, J>;
    const uint32_t cout0 = col0 >> J;
    const uint32_t rout0 = row0 >> J;
    const bool leader = (SO == 1) || ((lane & (SO - 1)) == 0);
#pragma unroll
    for (int r = 0; r < RO; ++r) {
        bool ok = leader;
        if constexpr (EDGE) {
            ok = ok && (rout0 + r < hout) && (cout0 < wout);
        }
        if (!ok)
            continue;
        T* d = dst + uint64_t(rout0 + r) * wout + cout0;
        if (!EDGE || cout0 + CO <= wout) {
            store_vec<T, CO, NTS>(d, out[r]);
        } else {
            // the lane's block overhangs the row end (any-width frames)
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                if (cout0 + c < wout) {
                    const T one[1] = { out[r][c] };
                    store_vec<T, 1, NTS>(d + c, one);
                }
            }
        }
    }
}

// Any nonzero byte (the chunk zero scan is byte-wise: -0.0 counts).
template<typename T>
__device__ __forceinline__ bool
nonzero_bits(T x)
{
    if constexpr (sizeof(T) == 8) {
        uint64_t b;
        __builtin_memcpy(&b, &x, 8);
        return b != 0;
    } else {
        uint32_t b = 0;
        __builtin_memcpy(&b, &x, sizeof(T));
        return b != 0;
    }
}

// Write the lane's RO x CO block of level J in chunk-tile order (the layout
// Array::write_frame_to_chunks_ fills, array.cpp:507-622): element (row, col)
// goes to tile (row / tr, col / tc) at (row % tr) * tc + col % tc.  Positions
// past the level inside the padded pw x ph area are stored as zero — the
// bytes Chunk::write_tile_rows leaves in an overhanging tile slot
// (chunk.cpp:17-58) — and positions past the padding are skipped.  `wc0` is
// the wave's first level-0 column (uniform).  Flags: see TiledLevel.  P is
// the kernel's parameter block (CascadeParams, VolumeTiledParams): it supplies
// the level sizes w[], h[] and the TiledLevel array tl[].
template<typename T, int C, int J, int RO, int CO, bool EDGE, int MODE, typename P>
__device__ __forceinline__ void
store_level_tiled(const P& p,
                  const T (&out)[RO][CO],
                  uint32_t f,
                  uint32_t wc0,
                  uint32_t row0,
                  int lane)
{
    constexpr int SO = kLaneStride<C, J>;
    constexpr int I = J - 1;
    const TiledLevel t = p.tl[I]; // one kernarg block load
    const uint32_t w = p.w[I], h = p.h[I], tr = t.tr, tc = t.tc;
    const uint32_t pw = t.pw, ph = t.ph;
    const uint32_t lc = (uint32_t(lane) * C) >> J; // lane's column offset in the block
    const uint32_t bc = wc0 >> J;                    // block's first level column (uniform)
    const uint32_t br = row0 >> J;                   // block's first level row (uniform)
    const uint32_t cout0 = bc + lc;
    const bool leader = (SO == 1) || ((lane & (SO - 1)) == 0);
    const uint64_t tile_elems = t.tstride;
    T* base = reinterpret_cast<T*>(t.tdst) + tiled_frame_base(t, f);
    uint8_t* flags = t.flags ? t.flags + uint64_t(f) * t.flags_frame : nullptr;
    auto nested = [&]() {
        const uint32_t K = t.slots;
        // Blocks and tiles nest: the block lies in one tile (its columns at
        // offset bx there), or spans whole tiles side by side (bx = 0).
        // Row and tile coordinates are wave-uniform; lanes add their column.
        constexpr uint32_t BW = (64u * C) >> J; // block columns at this level
        if (br >= ph || bc >= pw)
            return; // past the padding (uniform): no tile, no slot
        const uint32_t ty = t.dr.div(br), tx0 = t.dc.div(bc);
        const uint32_t ry0 = br - ty * tr, bx = bc - tx0 * tc;
        const uint32_t ltx = BW > tc ? t.dc.div(lc) : 0u; // lane's tile within the block
        const uint32_t cx = bx + lc - ltx * tc;
        T* tile = base + (uint64_t(ty) * t.ntx + tx0 + ltx) * tile_elems;
        const bool in_pad = cout0 < pw; // a block spanning tiles may pass the padding
        const bool act = leader && in_pad;
        // Values (zero past the level) and the vote first, so the flag store
        // goes out ahead of the block's data stores: a wave with little data
        // retires only when its last store completes.
        T v[RO][CO];
        bool nz = false;
#pragma unroll
        for (int r = 0; r < RO; ++r) {
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                T x = out[r][c];
                if constexpr (EDGE) {
                    if (br + r >= h || cout0 + c >= w)
                        x = T(0);
                }
                v[r][c] = x;
                nz = nz || (act && nonzero_bits(x));
            }
        }
        const uint64_t votes = __ballot(nz); // every lane reaches the vote
        if (flags && lane == 0) {
            const uint32_t srow = (ry0 / RO) * t.slots_x;
            uint8_t* f0 = flags + (uint64_t(ty) * t.ntx + tx0) * K + srow;
            if (BW <= tc) {
                f0[bx / BW] = votes != 0 ? 1 : 0;
            } else {
                // one slot per tile the block spans: the lanes of tile q are
                // those whose columns fall in [q * tc, (q + 1) * tc)
                const uint32_t lanes = (tc << J) / C; // lanes per tile (<= 64)
                const uint64_t m = lanes >= 64 ? ~0ull : ((1ull << lanes) - 1);
                for (uint32_t q = 0; q * lanes < 64 && tx0 + q < t.ntx; ++q)
                    f0[uint64_t(q) * K] = ((votes >> (q * lanes)) & m) != 0 ? 1 : 0;
            }
        }
        if (act) {
#pragma unroll
            for (int r = 0; r < RO; ++r)
                store_vec<T, CO, true>(tile + uint64_t(ry0 + r) * tc + cx, v[r]);
        }
    };
    auto general = [&]() {
    // General geometry: per-row tile coordinates, per-lane tile columns.
    const uint32_t tx = t.dc.div(cout0);
    const uint32_t cx = cout0 - tx * tc;
#pragma unroll
    for (int r = 0; r < RO; ++r) {
        const uint32_t row = br + r;
        bool ok = leader;
        if constexpr (EDGE) {
            ok = ok && row < ph && cout0 < pw;
        }
        if (!ok)
            continue;
        const uint32_t ty = t.dr.div(row);
        T* trow = base + uint64_t(ty) * t.ntx * tile_elems + uint64_t(row - ty * tr) * tc;
        T v[CO];
        bool rnz = false;
#pragma unroll
        for (int c = 0; c < CO; ++c) {
            T x = out[r][c];
            if constexpr (EDGE) {
                if (row >= h || cout0 + c >= w)
                    x = T(0);
            }
            v[c] = x;
            rnz = rnz || nonzero_bits(x);
        }
        if (cx + CO <= tc) {
            store_vec<T, CO, true>(trow + tx * tile_elems + cx, v);
            if (rnz && flags)
                flags[ty * t.ntx + tx] = 1;
        } else {
            // the lane's columns cross a tile edge (tc not a multiple of CO)
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                const uint32_t col = cout0 + c;
                if (col >= pw)
                    continue;
                const uint32_t ctx = t.dc.div(col);
                const T one[1] = { v[c] };
                store_vec<T, 1, true>(trow + ctx * tile_elems + (col - ctx * tc), one);
                if (flags && nonzero_bits(v[c]))
                    flags[ty * t.ntx + ctx] = 1;
            }
        }
    }

    };
    if constexpr (MODE == 1) {
        nested();
    } else {
        // per level: nested blocks keep their clear-free slots
        if (t.slots)
            nested();
        else
            general();
    }
}

// Level I's TiledLevel with compile-time kernarg offsets (indexing p.tl with
// a runtime I would copy the array to scratch).
template<typename P>
__device__ __forceinline__ TiledLevel
tiled_level(const P& p, int I)
{
    static_assert(kMaxFusedLevels == 4, "tiled_level");
    return I == 0 ? p.tl[0] : I == 1 ? p.tl[1] : I == 2 ? p.tl[2] : p.tl[3];
}

// NLV > 0: the fused volume's run of NLV levels.  `n_frames` then counts
// plane groups, level I + 1 emits 2^(NLV-1-I) planes per group, and a group's
// items are every level's zrows once per such plane (plan_volume_tiled).
template<typename T, int NLV = 0, typename P>
__device__ __forceinline__ void
zero_fill_tiled(const P& p, uint32_t z, uint32_t nz, int lane, int n_out,
                uint32_t n_frames)
{
    constexpr int E = 16 / int(sizeof(T));
    const uint32_t items = p.zitems * n_frames; // < 2^32: checked at launch
    for (uint32_t it = z; it < items; it += nz) {
        uint32_t f = p.zdiv.div(it);
        uint32_t rem = it - f * p.zitems;
        int I = 0;
#pragma unroll
        for (int k = 0; k < kMaxFusedLevels - 1; ++k) {
            uint32_t zr = k == 0 ? p.tl[0].zrows : k == 1 ? p.tl[1].zrows : p.tl[2].zrows;
            if constexpr (NLV > 0)
                zr <<= (NLV - 1 - k > 0 ? NLV - 1 - k : 0);
            if (I == k && I + 1 < n_out && rem >= zr) {
                rem -= zr;
                ++I;
            }
        }
        const TiledLevel t = tiled_level(p, I);
        if constexpr (NLV > 0) {
            // the level's plane within the group, then the row item within it
            const uint32_t zz = rem / t.zrows;
            rem -= zz * t.zrows;
            f = (f << (NLV - 1 - I)) + zz;
        }
        const uint32_t tr = t.tr, tc = t.tc, pw = t.pw;
        const uint32_t cw = min(t.cov_w, pw), chh = min(t.cov_h, t.ph);
        const uint32_t row = cw < pw ? rem : chh + rem;
        const uint32_t a = row >= chh ? 0u : cw;
        const uint64_t tile_elems = t.tstride;
        const uint32_t ty = t.dr.div(row);
        T* trow = reinterpret_cast<T*>(t.tdst) + tiled_frame_base(t, f) +
                  uint64_t(ty) * t.ntx * tile_elems + uint64_t(row - ty * tr) * tc;
        for (uint32_t tx = t.dc.div(a); tx * tc < pw; ++tx) {
            const uint32_t c0 = max(a, tx * tc) - tx * tc; // segment [c0, tc) in the tile row
            T* seg = trow + tx * tile_elems + c0;
            const uint32_t len = tc - c0;
            for (uint32_t i = uint32_t(lane) * E; i < len; i += 64u * E) {
                if (i + E <= len) {
                    const T zeros[E] = {};
                    store_vec<T, E, true>(seg + i, zeros);
                } else {
                    for (uint32_t k = i; k < len; ++k) {
                        const T zero[1] = { T(0) };
                        store_vec<T, 1, true>(seg + k, zero);
                    }
                }
            }
        }
    }
    // slot flags of blocks no wave of the grid owns (rows >= cov_h or
    // columns >= cov_w at their level)
#pragma unroll
    for (int I = 0; I < kMaxFusedLevels; ++I) {
        if (I >= n_out)
            break;
        const TiledLevel t = p.tl[I];
        if (!t.slots || !t.flags || (t.cov_w >= t.pw && t.cov_h >= t.ph))
            continue;
        const uint32_t K = t.slots, kx = t.slots_x, ky = K / kx;
        const uint32_t bh = t.tr / ky, bw = t.tc / kx; // slot size at the level
        const uint64_t per_frame = t.flags_frame;
        const uint64_t total = per_frame * n_frames;
        for (uint64_t q = uint64_t(z) * 64 + lane; q < total; q += uint64_t(nz) * 64) {
            const uint32_t f = uint32_t(q / per_frame);
            const uint32_t s = uint32_t(q - uint64_t(f) * per_frame);
            const uint32_t tile = s / K, slot = s - tile * K;
            const uint32_t ty = tile / t.ntx, tx = tile - ty * t.ntx;
            const uint32_t r0 = ty * t.tr + (slot / kx) * bh;
            const uint32_t c0 = tx * t.tc + (slot % kx) * bw;
            if (r0 >= t.cov_h || c0 >= t.cov_w)
                t.flags[q] = 0;
        }
    }
}

// Level 0 of a run in chunk-tile order (cascade_base_kernel): the
// lane's loaded block v[R][C] goes out as store_level_tiled writes a level,
// with the block 2^NL rows by 64 * C columns and a lane store the lane's
// whole load — same layout, same zeros past the level inside the padded
// area, nothing past it, same flags (BaseLevel::tl0).  On edge units a lane's
// columns past the row end hold the next row's (or frame's) bytes and rows
// past the frame a shifted or skipped load: both are masked to zero here,
// on the packed words as loaded (a byte mask per lane, a uniform test per
// row), so that 1- and 2-byte pixels are never unpacked.  A function of its
// own, so that the levels' store keeps its code in every other kernel.
//
// A lane's row as 32-bit words, zero past the frame: `mask` the lane's bytes
// inside the row, `in` (uniform) the row inside the frame.
template<typename T, int C, bool EDGE>
__device__ __forceinline__ void
base_row_words(const T (&row)[C], const uint32_t (&mask)[C * int(sizeof(T)) / 4], bool in,
               uint32_t (&wd)[C * int(sizeof(T)) / 4])
{
    __builtin_memcpy(wd, row, C * sizeof(T));
    if constexpr (EDGE) {
#pragma unroll
        for (int i = 0; i < C * int(sizeof(T)) / 4; ++i)
            wd[i] = in ? (wd[i] & mask[i]) : 0u;
    }
}

template<typename T, int C>
__device__ __forceinline__ void
base_store_row(T* d, const uint32_t (&wd)[C * int(sizeof(T)) / 4])
{
    T x[C];
    __builtin_memcpy(x, wd, C * sizeof(T));
    store_vec<T, C, true>(d, x);
}

// `t0`: BaseLevel::tl0; w x h: the frame.
template<typename T, int C, int R, bool EDGE, int MODE>
__device__ __forceinline__ void
store_base_tiled(const TiledLevel& t0,
                 uint32_t w,
                 uint32_t h,
                 const T (&v)[R][C],
                 uint32_t f,
                 uint32_t wc0,
                 uint32_t row0,
                 int lane)
{
    constexpr int RB = C * int(sizeof(T)); // a lane's bytes per row
    constexpr int NW = RB / 4;
    static_assert(RB == 8 || RB == 16 || RB == 32, "a lane's load");
    const TiledLevel t = t0; // one kernarg block load
    const uint32_t tr = t.tr, tc = t.tc;
    const uint32_t pw = t.pw, ph = t.ph;
    const uint32_t lc = uint32_t(lane) * C; // lane's column offset in the block
    const uint32_t cout0 = wc0 + lc;
    const uint64_t tile_elems = t.tstride;
    T* base = reinterpret_cast<T*>(t.tdst) + tiled_frame_base(t, f);
    uint8_t* flags = t.flags ? t.flags + uint64_t(f) * t.flags_frame : nullptr;
    // the lane's bytes inside the frame, as a mask per 32-bit word of its row
    uint32_t mask[NW] = {};
    if constexpr (EDGE) {
        const uint32_t nvb =
          (cout0 < w ? min(w - cout0, uint32_t(C)) : 0u) * uint32_t(sizeof(T));
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const uint32_t lo = 4u * uint32_t(i);
            mask[i] = nvb >= lo + 4u ? ~0u : nvb <= lo ? 0u : (1u << (8u * ((nvb - lo) & 3u))) - 1u;
        }
    }
    if (MODE == 1 || t.slots) {
        const uint32_t K = t.slots;
        // as store_level_tiled's nested form, at J = 0
        constexpr uint32_t BW = 64u * C;
        if (row0 >= ph || wc0 >= pw)
            return; // past the padding (uniform): no tile, no slot
        const uint32_t ty = t.dr.div(row0), tx0 = t.dc.div(wc0);
        const uint32_t ry0 = row0 - ty * tr, bx = wc0 - tx0 * tc;
        const uint32_t ltx = BW > tc ? t.dc.div(lc) : 0u; // lane's tile within the block
        const uint32_t cx = bx + lc - ltx * tc;
        T* tile = base + (uint64_t(ty) * t.ntx + tx0 + ltx) * tile_elems;
        const bool act = cout0 < pw; // a block spanning tiles may pass the padding
        // the vote and the flag store ahead of the data stores
        // (the mask is the same for every row, so the vote ORs the rows'
        // words as loaded — rows inside the frame only — and masks the sum:
        // no masked copy of the block exists beside the block itself)
        uint32_t acc[NW] = {};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            uint32_t wd[NW];
            __builtin_memcpy(wd, v[r], RB);
            const bool in = !EDGE || row0 + uint32_t(r) < h; // uniform
#pragma unroll
            for (int i = 0; i < NW; ++i)
                acc[i] |= in ? wd[i] : 0u;
        }
        uint32_t any = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i)
            any |= EDGE ? (acc[i] & mask[i]) : acc[i];
        const uint64_t votes = __ballot(act && any != 0); // every lane reaches the vote
        if (flags && lane == 0) {
            const uint32_t srow = (ry0 / uint32_t(R)) * t.slots_x;
            uint8_t* f0 = flags + (uint64_t(ty) * t.ntx + tx0) * K + srow;
            if (BW <= tc) {
                f0[bx / BW] = votes != 0 ? 1 : 0;
            } else {
                const uint32_t lanes = tc / C; // lanes per tile (<= 64)
                const uint64_t m = lanes >= 64 ? ~0ull : ((1ull << lanes) - 1);
                for (uint32_t q = 0; q * lanes < 64 && tx0 + q < t.ntx; ++q)
                    f0[uint64_t(q) * K] = ((votes >> (q * lanes)) & m) != 0 ? 1 : 0;
            }
        }
        if (act) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                uint32_t wd[NW];
                base_row_words<T, C, EDGE>(v[r], mask, row0 + uint32_t(r) < h, wd);
                base_store_row<T, C>(tile + uint64_t(ry0 + r) * tc + cx, wd);
            }
        }
    } else if constexpr (MODE != 1) {
        // per-row tile coordinates, per-lane tile columns
        const uint32_t tx = t.dc.div(cout0);
        const uint32_t cx = cout0 - tx * tc;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t row = row0 + uint32_t(r);
            if constexpr (EDGE) {
                if (!(row < ph && cout0 < pw))
                    continue;
            }
            const uint32_t ty = t.dr.div(row);
            T* trow = base + uint64_t(ty) * t.ntx * tile_elems + uint64_t(row - ty * tr) * tc;
            uint32_t wd[NW];
            base_row_words<T, C, EDGE>(v[r], mask, row < h, wd);
            if (cx + C <= tc) {
                uint32_t any = 0;
#pragma unroll
                for (int i = 0; i < NW; ++i)
                    any |= wd[i];
                base_store_row<T, C>(trow + tx * tile_elems + cx, wd);
                if (any && flags)
                    flags[ty * t.ntx + tx] = 1;
            } else {
                // the lane's columns cross a tile edge (tc not a multiple of C)
                T x[C];
                __builtin_memcpy(x, wd, RB);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const uint32_t col = cout0 + c;
                    if (col >= pw)
                        continue;
                    const uint32_t ctx = t.dc.div(col);
                    const T one[1] = { x[c] };
                    store_vec<T, 1, true>(trow + ctx * tile_elems + (col - ctx * tc), one);
                    if (flags && nonzero_bits(x[c]))
                        flags[ty * t.ntx + ctx] = 1;
                }
            }
        }
    }
}

// zero_fill_tiled's work for level 0 of such a run: the padded base area the
// units do not reach, per (frame, padded row) item (tl0.zrows a frame), and
// the slot flags of blocks no wave owns.  The levels keep zero_fill_tiled.
template<typename T>
__device__ __forceinline__ void
zero_fill_base(const BaseLevel& b, uint32_t z, uint32_t nz, int lane, uint32_t n_frames)
{
    constexpr int E = 16 / int(sizeof(T));
    const TiledLevel t = b.tl0;
    const uint32_t items = t.zrows * n_frames; // < 2^32: checked at launch
    const uint32_t tr = t.tr, tc = t.tc, pw = t.pw;
    const uint32_t cw = min(t.cov_w, pw), chh = min(t.cov_h, t.ph);
    const uint64_t tile_elems = t.tstride;
    for (uint32_t it = z; it < items; it += nz) {
        const uint32_t f = b.zdiv0.div(it);
        const uint32_t rem = it - f * t.zrows;
        const uint32_t row = cw < pw ? rem : chh + rem;
        const uint32_t a = row >= chh ? 0u : cw;
        const uint32_t ty = t.dr.div(row);
        T* trow = reinterpret_cast<T*>(t.tdst) + tiled_frame_base(t, f) +
                  uint64_t(ty) * t.ntx * tile_elems + uint64_t(row - ty * tr) * tc;
        for (uint32_t tx = t.dc.div(a); tx * tc < pw; ++tx) {
            const uint32_t c0 = max(a, tx * tc) - tx * tc; // segment [c0, tc) in the tile row
            T* seg = trow + tx * tile_elems + c0;
            const uint32_t len = tc - c0;
            for (uint32_t i = uint32_t(lane) * E; i < len; i += 64u * E) {
                if (i + E <= len) {
                    const T zeros[E] = {};
                    store_vec<T, E, true>(seg + i, zeros);
                } else {
                    for (uint32_t k = i; k < len; ++k) {
                        const T zero[1] = { T(0) };
                        store_vec<T, 1, true>(seg + k, zero);
                    }
                }
            }
        }
    }
    if (!t.slots || !t.flags || (t.cov_w >= t.pw && t.cov_h >= t.ph))
        return;
    const uint32_t K = t.slots, kx = t.slots_x, ky = K / kx;
    const uint32_t bh = t.tr / ky, bw = t.tc / kx; // slot size
    const uint64_t per_frame = t.flags_frame;
    const uint64_t total = per_frame * n_frames;
    for (uint64_t q = uint64_t(z) * 64 + lane; q < total; q += uint64_t(nz) * 64) {
        const uint32_t f = uint32_t(q / per_frame);
        const uint32_t s = uint32_t(q - uint64_t(f) * per_frame);
        const uint32_t tile = s / K, slot = s - tile * K;
        const uint32_t ty = tile / t.ntx, tx = tile - ty * t.ntx;
        const uint32_t r0 = ty * t.tr + (slot / kx) * bh;
        const uint32_t c0 = tx * t.tc + (slot % kx) * bw;
        if (r0 >= t.cov_h || c0 >= t.cov_w)
            t.flags[q] = 0;
    }
}

// Row-band staging (cascade_band_kernel): levels whose rows split 64-byte
// DRAM bursts are written to LDS first, so that one workgroup — which owns
// a whole row band of the frame — stores each level's band as one
// contiguous span in whole 16-byte chunks.  lds[J-1] maps byte 0 to the
// span start rounded down to 16 bytes (`head` bytes before the span).
struct StageCtx
{
    uint8_t* lds[kMaxFusedLevels];
    uint32_t head[kMaxFusedLevels];
    uint32_t mask; // bit J-1: level J is staged
    // LDS row stride (elements) and first staged column per level: the
    // level width and 0 for a whole band, the segment's for a segmented one
    uint32_t stride[kMaxFusedLevels];
    uint32_t scol[kMaxFusedLevels];
    // Misaligned segments (rowb > 0): each level row of the segment is its
    // own piece in LDS, rowb bytes apart, placed at the same offset modulo
    // 16 as its global address, so that it leaves in aligned 16-byte chunks:
    // row r's piece starts (head + r * hstep) % 16 bytes into its slot.
    uint32_t rowb[kMaxFusedLevels];
    uint32_t hstep[kMaxFusedLevels];
};

template<typename T, int C, int J, int RO, int CO, bool EDGE, bool ROWS = false>
__device__ __forceinline__ void
stage_level(const StageCtx& sc,
            const T (&out)[RO][CO],
            uint32_t wout,
            uint32_t hout,
            uint32_t col0,
            uint32_t row0,
            uint32_t band_row0,
            int lane)
{
    constexpr int SO = kLaneStride<C, J>;
    const uint32_t cout0 = col0 >> J;
    const uint32_t rout0 = row0 >> J;
    const bool leader = (SO == 1) || ((lane & (SO - 1)) == 0);
    uint8_t* base = sc.lds[J - 1] + sc.head[J - 1];
#pragma unroll
    for (int r = 0; r < RO; ++r) {
        bool ok = leader;
        if constexpr (EDGE) {
            ok = ok && (rout0 + r < hout) && (cout0 < wout);
        }
        if (!ok)
            continue;
        const uint32_t rr = rout0 + r - (band_row0 >> J); // row within the band
        T* d;
        if constexpr (ROWS) {
            d = reinterpret_cast<T*>(sc.lds[J - 1] + rr * sc.rowb[J - 1] +
                                     ((sc.head[J - 1] + rr * sc.hstep[J - 1]) & 15u)) +
                (cout0 - sc.scol[J - 1]);
        } else {
            d = reinterpret_cast<T*>(base) + uint64_t(rr) * sc.stride[J - 1] +
                (cout0 - sc.scol[J - 1]);
        }
        // A lane's CO elements as one LDS vector write where they are whole
        // and aligned (every row of an aligned band): element writes put the
        // lanes 16 B apart for f32 level 1, a 4-way bank conflict (60% of
        // LDS cycles, profiles/r03/f32/); the element path stays for edges
        // and unaligned bands.
        constexpr int VB = CO * int(sizeof(T));
        if constexpr (VB == 16 || VB == 8 || VB == 4) {
            if ((!EDGE || cout0 + CO <= wout) &&
                (reinterpret_cast<uintptr_t>(d) & uintptr_t(VB - 1)) == 0) {
                if constexpr (VB == 16) {
                    u32x4 v;
                    __builtin_memcpy(&v, out[r], 16);
                    *reinterpret_cast<u32x4*>(d) = v;
                } else if constexpr (VB == 8) {
                    uint64_t v;
                    __builtin_memcpy(&v, out[r], 8);
                    *reinterpret_cast<uint64_t*>(d) = v;
                } else {
                    uint32_t v;
                    __builtin_memcpy(&v, out[r], 4);
                    *reinterpret_cast<uint32_t*>(d) = v;
                }
                continue;
            }
        }
#pragma unroll
        for (int c = 0; c < CO; ++c) {
            if (!EDGE || cout0 + c < wout)
                d[c] = out[r][c];
        }
    }
}

// Level J of the 2-D cascade: reduce, store, recurse to J+1.
template<typename T, int M, int C, int J, int NL, int RI, int CI, bool EDGE,
         bool NTS = false, int STAGED = 0, int TILED = 0>
__device__ __forceinline__ void
cascade_level(const CascadeParams& p,
              const T (&in)[RI][CI],
              uint32_t f,
              uint32_t row0,
              uint32_t col0,
              int lane,
              const StageCtx* sc = nullptr)
{
    constexpr int RO = RI / 2;
    constexpr int CO = (CI >= 2) ? CI / 2 : 1;
    const uint32_t win = (J == 1) ? p.W : p.w[J - 2];
    const uint32_t hin = (J == 1) ? p.H : p.h[J - 2];

    T out[RO][CO];
    xy_step<T, M, C, J, RI, CI, EDGE>(in, out, win, hin, col0 >> (J - 1),
                                      row0 >> (J - 1));
    T* dst = reinterpret_cast<T*>(p.dst[J - 1]) +
             uint64_t(f) * p.dst_frame_elems[J - 1];
    if constexpr (TILED) {
        // a row-major copy only where the next launch reads this level
        if (p.dst[J - 1])
            store_level<T, C, J, RO, CO, EDGE, NTS>(dst, out, p.w[J - 1], p.h[J - 1],
                                                    col0, row0, lane);
        store_level_tiled<T, C, J, RO, CO, EDGE, TILED>(p, out, f, col0 - uint32_t(lane) * C,
                                                        row0, lane);
    } else if constexpr (STAGED) {
        if ((sc->mask >> (J - 1)) & 1u) {
            // the band's rows start at row0 - row0 % 2^NL: one band per block
            stage_level<T, C, J, RO, CO, EDGE, STAGED == 2>(*sc, out, p.w[J - 1], p.h[J - 1],
                                                            col0, row0,
                                                            row0 & ~((1u << NL) - 1u), lane);
        } else {
            store_level<T, C, J, RO, CO, EDGE, NTS>(dst, out, p.w[J - 1], p.h[J - 1],
                                                    col0, row0, lane);
        }
    } else if ((p.wb >> (J - 1)) & 1u) {
        // write-back: partial 64-B bursts of neighbouring waves merge in L2
        store_level<T, C, J, RO, CO, EDGE, false>(dst, out, p.w[J - 1], p.h[J - 1], col0, row0,
                                                  lane);
    } else {
        store_level<T, C, J, RO, CO, EDGE, NTS>(dst, out, p.w[J - 1], p.h[J - 1],
                                                col0, row0, lane);
    }
    if constexpr (J < NL) {
        cascade_level<T, M, C, J + 1, NL, RO, CO, EDGE, NTS, STAGED, TILED>(p, out, f, row0,
                                                                           col0, lane, sc);
    }
}

// C = columns per lane (a multiple of 16 bytes of T); NT / NTS = non-temporal
// loads / stores.  Every byte of the pyramid is touched exactly once, so both
// streams are marked non-temporal: measured on MI355X (tools/microbench.hip,
// profiles/r01) the headline batch drops from ~530 to ~475 us with NT stores.
//
// SPLIT (two 16-byte loads per lane and row, i.e. 4- and 8-byte types at the
// wide tile): the wave's 64 x 32-byte row segment is loaded as two halves of
// 64 x 16 contiguous bytes — load k covers bytes [k KiB, (k+1) KiB) of the
// segment, lane i bytes 16i.. of it — instead of lane i taking bytes 32i..
// in both loads.  Each load instruction then reads whole 128-byte lines, and
// no line is requested by two instructions, which L2 did not always merge
// (F config Min/Max fetched 2.3-2.7% more than the frame).
// The halves are two tiles of E columns per lane, reduced and stored
// (staged) one after the other by the E-column cascade.
//
// TILED 3 / 4 (cascade_base_kernel, `base` set): TILED 1 / 2 with the loaded
// block itself stored as level 0's chunk tiles first — the same bytes for
// every method, since the store sees only the loads.
template<typename T, int M, int NL, int C, bool NT, bool EDGE, bool NTS = true,
         int STAGED = 0, int TILED = 0, bool SPLIT = false>
__device__ __forceinline__ void
cascade_unit(const CascadeParams& p,
             uint32_t f,
             uint32_t row0,
             uint32_t col0,
             int lane,
             const StageCtx* sc = nullptr,
             const BaseLevel* base = nullptr)
{
    constexpr int R = 1 << NL;
    constexpr int RB = C * int(sizeof(T));   // bytes per lane per row
    constexpr int LB = RB >= 16 ? 16 : RB;   // bytes per load (8 for narrow tiles)
    constexpr int V = RB / LB;               // loads per row
    constexpr int E = LB / int(sizeof(T));   // elements per load
    const T* src =
      reinterpret_cast<const T*>(p.src) + uint64_t(f) * p.src_frame_elems;
    if constexpr (SPLIT) {
        static_assert(V == 2 && TILED == 0, "SPLIT: two loads per row, row-major/staged levels");
        const uint32_t wc0 = col0 - uint32_t(lane) * C; // the wave's first column
        const bool last_frame = f + 1 == p.total_units / (p.units_x * p.units_y);
        T h[2][R][E];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                load_chunk<T, E, NT, EDGE>(&h[k][r][0], src + uint64_t(row0 + r) * p.W,
                                           wc0 + uint32_t(k) * 64u * E + uint32_t(lane) * E, p.W,
                                           row0 + r < p.H, !last_frame || row0 + r + 1 < p.H, src);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            cascade_level<T, M, E, 1, NL, R, E, EDGE, NTS, STAGED, TILED>(
              p, h[k], f, row0, wc0 + uint32_t(k) * 64u * E + uint32_t(lane) * E, lane, sc);
        }
        return;
    }

    T v[R][C];
    // All row loads are issued before any arithmetic: 2^NL * V outstanding
    // loads per lane (1 KiB per wave instruction at 16 B).
    // reading past a row end stays in the buffer except on the batch's last row
    const bool last_frame = f + 1 == p.total_units / (p.units_x * p.units_y);
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            load_chunk<T, E, NT, EDGE>(&v[r][k * E], src + uint64_t(row0 + r) * p.W,
                                       col0 + uint32_t(k) * E, p.W, row0 + r < p.H,
                                       !last_frame || row0 + r + 1 < p.H, src);
        }
    }
    // keep every load above the reductions (the scheduler would otherwise
    // hold back the last rows' loads to save registers)
    __builtin_amdgcn_sched_barrier(0);
    constexpr bool kBase = TILED >= 3;
    if constexpr (kBase)
        store_base_tiled<T, C, R, EDGE, TILED - 2>(base->tl0, p.W, p.H, v, f,
                                                   col0 - uint32_t(lane) * C, row0, lane);
    cascade_level<T, M, C, 1, NL, R, C, EDGE, NTS, STAGED, kBase ? TILED - 2 : TILED>(
      p, v, f, row0, col0, lane, sc);
}

// TILED (1: blocks and tiles nest, 2: any chunk shape): every level goes out
// in chunk-tile order (store_level_tiled); the grid's first blocks zero-fill
// the tile overhang its cascade blocks do not reach (zero_fill_tiled).
template<typename T, int M, int NL, int C = kCascadeCols<T>, bool NT = true, int TILED = 0>
__global__ __launch_bounds__(512) void
cascade_kernel(CascadeParams p)
{
    // one tile per wave, the grid covers every tile (no grid-stride loop:
    // measured 2-4% faster for f32 than the looped form), except that small
    // units go p.upw consecutive ones per wave (below)
    constexpr int R = 1 << NL;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t blk = blockIdx.x;
    if constexpr (TILED) {
        // The first blocks zero-fill the tile overhang (dispatched round-robin
        // over the XCDs like any blocks); the cascade blocks follow.
        const uint32_t wpb = blockDim.x >> 6;
        const uint32_t zb = p.zwaves / wpb;
        if (blk < zb) {
            zero_fill_tiled<T>(p, blk * wpb + wave, p.zwaves, lane, NL,
                               p.total_units / (p.units_x * p.units_y));
            return;
        }
        blk -= zb;
    }
    if (p.remap) {
        // XCD-contiguous order ($AQZ_XCD_REMAP=1, off by default): workgroup
        // i runs on XCD i % 8, so remapping i to (i % 8) * (n / 8) + i / 8
        // gives XCD x a contiguous eighth of the units (whole frames for
        // batches of >= 8).  Same-box A/B (profiles/r02/remap_ab.log): +2-4%
        // for 5472x3648, -1-5% for 3000^2, within noise at the headline.
        const uint32_t nb8 = p.main_blocks & ~7u;
        if (blk < nb8)
            blk = (blk & 7u) * (nb8 >> 3) + (blk >> 3);
    }
    if constexpr (TILED) {
        // one unit per wave (the loop below, even run once, cost the tiled
        // instantiations 40-70% more VGPRs: headline 60 -> 100, half the
        // occupancy, 3000^2 tiled 539 -> 710 us)
        uint32_t ux, uy, f;
        if (p.seg_w) {
            // band-aligned workgroups (rows that split 128-B lines): the
            // waves sharing a line run on one CU, so it is fetched once
            const uint32_t segs = (p.units_x + p.seg_w - 1) / p.seg_w;
            const uint32_t band = blk / segs;
            ux = (blk - band * segs) * p.seg_w + wave;
            if (ux >= p.units_x || band >= p.total_units / p.units_x)
                return;
            uy = band % p.units_y;
            f = band / p.units_y;
        } else {
            const uint32_t u = blk * (blockDim.x >> 6) + wave;
            if (u >= p.total_units)
                return;
            ux = u % p.units_x;
            const uint32_t t = u / p.units_x;
            uy = t % p.units_y;
            f = t / p.units_y;
        }
        const uint32_t row0 = uy * R;
        const uint32_t tile_col0 = ux * (64u * C);
        const uint32_t col0 = tile_col0 + uint32_t(lane) * C;
        if ((tile_col0 + 64u * C <= p.W) && (row0 + R <= p.H))
            cascade_unit<T, M, NL, C, NT, false, true, 0, TILED>(p, f, row0, col0, lane);
        else
            cascade_unit<T, M, NL, C, NT, true, true, 0, TILED>(p, f, row0, col0, lane);
        return;
    }
    // p.upw > 1 (columns-fastest order, no band workgroups): each wave takes
    // that many consecutive units, for launches whose units move only a few
    // KiB (Decimate of narrow frames reads 2 of 4 rows of 512 B)
    const uint32_t upw = (!p.seg_w && p.order == 0) ? max(p.upw, 1u) : 1u;
    for (uint32_t it = 0; it < upw; ++it) {
        uint32_t ux, uy, f;
        if (p.seg_w) {
            // band-aligned workgroups: the waves that share a row's partial
            // 64-B bursts run on one CU, so the halves meet in its L2
            const uint32_t segs = (p.units_x + p.seg_w - 1) / p.seg_w;
            const uint32_t band = blk / segs;
            ux = (blk - band * segs) * p.seg_w + wave;
            if (ux >= p.units_x || band >= p.total_units / p.units_x)
                return;
            uy = band % p.units_y;
            f = band / p.units_y;
        } else if (const uint32_t u = (blk * (blockDim.x >> 6) + wave) * upw + it;
                   u >= p.total_units) {
            return;
        } else if (p.order == 0) {
            ux = u % p.units_x;
            const uint32_t t = u / p.units_x;
            uy = t % p.units_y;
            f = t / p.units_y;
        } else if (p.order == 1) {
            const uint32_t nf = p.total_units / (p.units_x * p.units_y);
            f = u % nf;
            const uint32_t t = u / nf;
            ux = t % p.units_x;
            uy = t / p.units_x;
        } else {
            uy = u % p.units_y;
            const uint32_t t = u / p.units_y;
            ux = t % p.units_x;
            f = t / p.units_x;
        }
        const uint32_t row0 = uy * R;
        const uint32_t tile_col0 = ux * (64u * C);
        const uint32_t col0 = tile_col0 + uint32_t(lane) * C;
        // wave-uniform: interior tiles take the edge-free path
        if ((tile_col0 + 64u * C <= p.W) && (row0 + R <= p.H)) {
            cascade_unit<T, M, NL, C, NT, false, true, 0, 0>(p, f, row0, col0, lane);
        } else {
            cascade_unit<T, M, NL, C, NT, true, true, 0, 0>(p, f, row0, col0, lane);
        }
    }
}

// cascade_kernel<..., TILED = MODE> with the input level written as chunk
// tiles too (launch_cascade_tiled with a base; MODE 1: every level, the base
// included, nests with the wave blocks, 2: any chunk shape).  The zero-fill
// blocks do the base's items first, then the levels'; the cascade blocks map
// one unit per wave as there, and each stores its loaded block as tiles
// before it reduces it (cascade_unit TILED 3 / 4).  A kernel of its own: the
// tiled instantiations without a base stay as they are.
template<typename T, int M, int NL, int C, bool NT, int MODE>
__global__ __launch_bounds__(512) void
cascade_base_kernel(CascadeParams p, BaseLevel b)
{
    constexpr int R = 1 << NL;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t blk = blockIdx.x;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t zb = p.zwaves / wpb;
    if (blk < zb) {
        zero_fill_base<T>(b, blk * wpb + wave, p.zwaves, lane,
                          p.total_units / (p.units_x * p.units_y));
        zero_fill_tiled<T>(p, blk * wpb + wave, p.zwaves, lane, NL,
                           p.total_units / (p.units_x * p.units_y));
        return;
    }
    blk -= zb;
    if (p.remap) {
        const uint32_t nb8 = p.main_blocks & ~7u;
        if (blk < nb8)
            blk = (blk & 7u) * (nb8 >> 3) + (blk >> 3);
    }
    uint32_t ux, uy, f;
    if (p.seg_w) {
        const uint32_t segs = (p.units_x + p.seg_w - 1) / p.seg_w;
        const uint32_t band = blk / segs;
        ux = (blk - band * segs) * p.seg_w + wave;
        if (ux >= p.units_x || band >= p.total_units / p.units_x)
            return;
        uy = band % p.units_y;
        f = band / p.units_y;
    } else {
        const uint32_t u = blk * wpb + wave;
        if (u >= p.total_units)
            return;
        ux = u % p.units_x;
        const uint32_t t = u / p.units_x;
        uy = t % p.units_y;
        f = t / p.units_y;
    }
    const uint32_t row0 = uy * R;
    const uint32_t tile_col0 = ux * (64u * C);
    const uint32_t col0 = tile_col0 + uint32_t(lane) * C;
    if ((tile_col0 + 64u * C <= p.W) && (row0 + R <= p.H))
        cascade_unit<T, M, NL, C, NT, false, true, 0, MODE + 2>(p, f, row0, col0, lane, nullptr,
                                                                &b);
    else
        cascade_unit<T, M, NL, C, NT, true, true, 0, MODE + 2>(p, f, row0, col0, lane, nullptr,
                                                               &b);
}

// Band-staged cascade: one workgroup per row band of one frame, one wave per
// column tile.  Staged levels (StageCtx) go to LDS; after one barrier the
// workgroup writes each staged level's band — consecutive level rows are
// adjacent in memory — as one span of whole, 16-byte-aligned chunks, so only
// the span's first and last chunk share bursts with the neighbouring bands.
// Used for frames whose level rows split 64-byte bursts (widths like 2000 or
// 3000 px, bands of <= 4 tiles, <= 6 for 2-byte types: partial-burst writes
// measured 30% slower than whole ones, tools/pitchbench.hip), where the
// band's last wave stores it instead of a barrier (CascadeParams::band_last),
// and for aligned bands of 5-8 tiles (row-major rows at >= 4 KiB pitch
// written 512 B per wave ran 15% slow on most boxes).  seg_tiles > 0
// (aligned frames only): a band wider than that
// is split into segments of seg_tiles tiles, one workgroup each, every level
// row of a segment one contiguous piece; waves past the last tile only join
// the barrier.
template<typename T, int M, int NL, int C, bool NT = true, bool ROWS = false, bool SPLIT = false>
__global__ __launch_bounds__(512)
// 2-byte Min / Max on line-aligned rows (NT loads): held to 80 VGPRs, 6
// waves per SIMD instead of 5 at 81 (headline Min 481 -> 470 us, Max 483
// -> 470); the same hint on misaligned bands stored by their last wave cost
// 3000^2 Max 546 -> 584 us, and Mean would spill at 80
// (profiles/r03/occupancy/)
__attribute__((amdgpu_waves_per_eu(
  sizeof(T) == 2 && (M == kMin || M == kMax) && NT ? 6 : 1))) void
cascade_band_kernel(CascadeParams p, uint32_t stage_mask, uint32_t seg_tiles)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t band_lds[];
    constexpr int R = 1 << NL;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t segs = seg_tiles ? (p.units_x + seg_tiles - 1) / seg_tiles : 1u;
    const uint32_t seg = blockIdx.x % segs;
    const uint32_t band = blockIdx.x / segs;
    const uint32_t uy = band % p.units_y;
    const uint32_t f = band / p.units_y;
    const uint32_t row0 = uy * R;
    const uint32_t ux = seg * seg_tiles + wave;
    const uint32_t seg_col0 = seg * seg_tiles * 64u * C; // level-0 column

    // LDS regions of the staged levels (same arithmetic in every thread)
    StageCtx sc{};
    sc.mask = stage_mask;
    uint32_t len[kMaxFusedLevels] = {};  // bytes per level row piece x rows
    uint32_t rows_of[kMaxFusedLevels] = {};
    uint32_t piece[kMaxFusedLevels] = {}; // bytes of one row's piece (segmented)
    uint8_t* span[kMaxFusedLevels] = {};
    uint32_t off = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        if (!((stage_mask >> i) & 1u))
            continue;
        const uint32_t r0 = row0 >> (i + 1);
        const uint32_t rows = min(uint32_t(R >> (i + 1)), p.h[i] - min(r0, p.h[i]));
        rows_of[i] = rows;
        if (seg_tiles) {
            const uint32_t c0 = seg_col0 >> (i + 1);
            const uint32_t cw = min((seg_tiles * 64u * C) >> (i + 1), p.w[i] - min(c0, p.w[i]));
            sc.stride[i] = cw;
            sc.scol[i] = c0;
            piece[i] = cw * uint32_t(sizeof(T));
            span[i] = p.dst[i] +
                      (uint64_t(f) * p.dst_frame_elems[i] + uint64_t(r0) * p.w[i] + c0) * sizeof(T);
            len[i] = rows * piece[i];
            if constexpr (ROWS) {
                // misaligned rows: one LDS slot per row (StageCtx::rowb)
                sc.head[i] = uint32_t(reinterpret_cast<uintptr_t>(span[i]) & 15u);
                sc.hstep[i] = (p.w[i] * uint32_t(sizeof(T))) & 15u;
                sc.rowb[i] = (piece[i] + 30u) & ~15u;
                sc.lds[i] = band_lds + off;
                off += rows * sc.rowb[i];
                continue;
            }
            sc.head[i] = 0; // aligned frames: every piece starts on 16 bytes
        } else {
            sc.stride[i] = p.w[i];
            sc.scol[i] = 0;
            span[i] = p.dst[i] + (uint64_t(f) * p.dst_frame_elems[i] + uint64_t(r0) * p.w[i]) *
                                   sizeof(T);
            len[i] = rows * p.w[i] * uint32_t(sizeof(T));
            sc.head[i] = uint32_t(reinterpret_cast<uintptr_t>(span[i]) & 15u);
        }
        sc.lds[i] = band_lds + off;
        off += (sc.head[i] + len[i] + 15u) & ~15u;
    }

    // p.band_last: no barrier before the stores.  Each wave counts itself
    // in once its LDS writes are done, and the last one to arrive stores the
    // whole band, so no wave waits for a slower one (the band's partial edge
    // tile; profiles/r02/band8/misaligned_pmc/).
    __shared__ uint32_t band_arrivals;
    const bool last_mode = p.band_last != 0; // uniform
    if (last_mode) {
        if (threadIdx.x == 0)
            band_arrivals = 0;
        __syncthreads();
    }

    if (ux < p.units_x) { // wave-uniform
        const uint32_t col0 = ux * (64u * C) + uint32_t(lane) * C;
        const bool interior = (ux * 64u * C + 64u * C <= p.W) && (row0 + R <= p.H);
        if (interior)
            cascade_unit<T, M, NL, C, NT, false, true, ROWS ? 2 : 1, 0, SPLIT>(p, f, row0, col0,
                                                                           lane, &sc);
        else
            cascade_unit<T, M, NL, C, NT, true, true, ROWS ? 2 : 1, 0, SPLIT>(p, f, row0, col0,
                                                                          lane, &sc);
    }
    uint32_t tid = threadIdx.x, nth = blockDim.x;
    if (last_mode) {
        // release: this wave's LDS writes complete before its count lands;
        // acquire: the storing waves then see every other wave's.  The last
        // K = p.band_last waves to arrive store the band together; all but
        // the very last wait for the stragglers among them (the workgroup's
        // waves are co-resident, so the count always completes).
        const uint32_t nw = blockDim.x >> 6;
        const uint32_t K = min(p.band_last, nw);
        uint32_t old = 0;
        if (lane == 0)
            old = __hip_atomic_fetch_add(&band_arrivals, 1u, __ATOMIC_ACQ_REL,
                                         __HIP_MEMORY_SCOPE_WORKGROUP);
        old = __builtin_amdgcn_readfirstlane(old);
        if (old + K < nw)
            return;
        if (old + 1u < nw) {
            while (__hip_atomic_load(&band_arrivals, __ATOMIC_ACQUIRE,
                                     __HIP_MEMORY_SCOPE_WORKGROUP) < nw)
                __builtin_amdgcn_s_sleep(1);
        }
        tid = (old + K - nw) * 64u + uint32_t(lane);
        nth = K * 64u;
    } else {
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < NL; ++i) {
        if (!((stage_mask >> i) & 1u) || len[i] == 0)
            continue;
        if constexpr (ROWS) {
            // misaligned segment: row r's piece leaves in the 16-byte chunks
            // of its own global span, whole ones as vectors, the two ends
            // (shared with the neighbouring segments) byte by byte
            const uint32_t cmax = sc.rowb[i] / 16u;
            const uint32_t chunks = rows_of[i] * cmax;
            const uint64_t pitch = uint64_t(p.w[i]) * sizeof(T);
            for (uint32_t k = tid; k < chunks; k += nth) {
                const uint32_t r = k / cmax, c = k - r * cmax;
                const uint32_t h = (sc.head[i] + r * sc.hstep[i]) & 15u;
                const uint32_t end = h + piece[i];
                const uint32_t a = c * 16u, b = a + 16u;
                if (a >= end)
                    continue;
                const uint8_t* l = sc.lds[i] + r * sc.rowb[i];
                uint8_t* g = span[i] + r * pitch - h;
                if (a >= h && b <= end) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(l + a);
                    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(g + a));
                } else {
                    for (uint32_t x = max(a, h); x < min(b, end); ++x)
                        g[x] = l[x];
                }
            }
            continue;
        }
        if (seg_tiles) {
            // rows_of[i] pieces of piece[i] bytes, level pitch apart
            const uint32_t cpr = piece[i] / 16u;
            const uint32_t chunks = rows_of[i] * cpr;
            const uint64_t pitch = uint64_t(p.w[i]) * sizeof(T);
            for (uint32_t k = tid; k < chunks; k += nth) {
                const uint32_t r = k / cpr, c = k - r * cpr;
                const u32x4 v = *reinterpret_cast<const u32x4*>(sc.lds[i] + r * piece[i] + c * 16u);
                __builtin_nontemporal_store(
                  v, reinterpret_cast<u32x4*>(span[i] + r * pitch + c * 16u));
            }
            continue;
        }
        const uint32_t head = sc.head[i];
        const uint32_t end = head + len[i];
        const uint32_t chunks = (end + 15u) / 16u;
        uint8_t* g = span[i] - head;
        for (uint32_t k = tid; k < chunks; k += nth) {
            const uint32_t a = k * 16u, b = a + 16u;
            if (a >= head && b <= end) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(sc.lds[i] + a);
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(g + a));
            } else {
                // first / last chunk of the span: only the band's own bytes
                for (uint32_t x = max(a, head); x < min(b, end); ++x)
                    g[x] = sc.lds[i][x];
            }
        }
    }
}

// ---- fused volume (2x2x2, two-stage) ----------------------------------------
//
// For pyramids whose every level halves XY *and* Z (3-D stacks, BASELINE
// config V): the reference reduces each plane 2x2 in XY (scale_image), then
// pairs consecutive reduced planes (average_two_frames, dst = earlier plane,
// src = current) — two truncations, not an 8-way mean.
// One wave owns 2^NL planes x 2^NL rows x (64 lanes x 16 B) and produces
// every level of the run from registers.

struct VolumeParams
{
    const uint8_t* src;
    uint64_t src_frame_elems;
    uint32_t W, H;
    uint32_t units_x;
    uint32_t units_y;
    uint32_t total_units; // units_x * units_y * plane groups
    uint8_t* dst[kMaxVolumeLevels];
    uint64_t dst_frame_elems[kMaxVolumeLevels];
    uint32_t w[kMaxVolumeLevels];
    uint32_t h[kMaxVolumeLevels];
};

// volume_kernel<..., TILED>: every level also (dst[J-1] null: only) goes out in
// chunk-tile order, plane k of level J as frame k of tl[J-1]; one flag byte
// per tile, cleared before the launch (TiledLevel::slots == 0).  The grid's
// first zwaves / (waves per block) blocks zero-fill the tile overhang the
// units do not reach (zero_fill_tiled<T, NL>).  tl[] has the cascade's length
// so that both parameter blocks feed the same tiled stores; a run uses its
// first n_out entries.
struct VolumeTiledParams : VolumeParams
{
    TiledLevel tl[kMaxFusedLevels];
    uint32_t zitems; // zero-fill items per plane group, all levels
    FastDiv zdiv;    // by zitems
    uint32_t zwaves;
};

template<typename T, int M, int C, int J, int NL, int ZI, int RI, int CI,
         bool EDGE, bool NTS, bool TILED = false, typename P = VolumeParams>
__device__ __forceinline__ void
volume_level(const P& p,
             const T (&in)[ZI][RI][CI],
             uint32_t g,
             uint32_t row0,
             uint32_t col0,
             int lane)
{
    constexpr int RO = RI / 2;
    constexpr int CO = (CI >= 2) ? CI / 2 : 1;
    constexpr int ZO = ZI / 2;
    const uint32_t win = (J == 1) ? p.W : p.w[J - 2];
    const uint32_t hin = (J == 1) ? p.H : p.h[J - 2];

    T xy[ZI][RO][CO];
#pragma unroll
    for (int z = 0; z < ZI; ++z) {
        xy_step<T, M, C, J, RI, CI, EDGE>(in[z], xy[z], win, hin,
                                          col0 >> (J - 1), row0 >> (J - 1));
    }
    T out[ZO][RO][CO];
#pragma unroll
    for (int z = 0; z < ZO; ++z) {
#pragma unroll
        for (int r = 0; r < RO; ++r) {
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                out[z][r][c] = reduce2<T, M>(xy[2 * z][r][c], xy[2 * z + 1][r][c]);
            }
        }
    }
#pragma unroll
    for (int z = 0; z < ZO; ++z) {
        // level-J frame index: plane group g covers 2^(NL-J) frames there
        T* dst = reinterpret_cast<T*>(p.dst[J - 1]) +
                 (uint64_t(g) * ZO + z) * p.dst_frame_elems[J - 1];
        if constexpr (TILED) {
            // a row-major copy only where the next launch reads this level
            if (p.dst[J - 1])
                store_level<T, C, J, RO, CO, EDGE, NTS>(dst, out[z], p.w[J - 1],
                                                        p.h[J - 1], col0, row0, lane);
            store_level_tiled<T, C, J, RO, CO, EDGE, 2>(p, out[z], g * uint32_t(ZO) + z,
                                                        col0 - uint32_t(lane) * C, row0, lane);
        } else {
            store_level<T, C, J, RO, CO, EDGE, NTS>(dst, out[z], p.w[J - 1],
                                                    p.h[J - 1], col0, row0, lane);
        }
    }
    if constexpr (J < NL) {
        volume_level<T, M, C, J + 1, NL, ZO, RO, CO, EDGE, NTS, TILED>(p, out, g, row0,
                                                                      col0, lane);
    }
}

// C = columns per lane (V = C*sizeof(T)/16 loads per row).  NTL: loads
// nontemporal.  Decimate reads planes 0 and 2 and rows 0 and 2 of the unit
// only (the other loads have no use and are dropped by the compiler).
template<typename T, int M, int NL, int C, bool EDGE, bool NTL>
__device__ __forceinline__ void
volume_load(const VolumeParams& p,
            uint32_t g,
            uint32_t row0,
            uint32_t col0,
            T (&v)[1 << NL][1 << NL][C])
{
    constexpr int R = 1 << NL;
    constexpr int Z = 1 << NL;
    constexpr int V = C * int(sizeof(T)) / 16;
    const bool last_group = g + 1 == p.total_units / (p.units_x * p.units_y);
#pragma unroll
    for (int z = 0; z < Z; ++z) {
        const T* src = reinterpret_cast<const T*>(p.src) +
                       (uint64_t(g) * Z + z) * p.src_frame_elems;
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                constexpr int E = 16 / int(sizeof(T));
                load_chunk<T, E, NTL, EDGE>(&v[z][r][k * E], src + uint64_t(row0 + r) * p.W,
                                            col0 + uint32_t(k) * E, p.W, row0 + r < p.H,
                                            !(last_group && z == Z - 1) ||
                                              row0 + r + 1 < p.H,
                                            src);
            }
        }
    }
}

template<typename T, int M, int NL, int C, bool EDGE, bool NTL, bool TILED = false,
         typename P = VolumeParams>
__device__ __forceinline__ void
volume_unit(const P& p,
            uint32_t g,
            uint32_t row0,
            uint32_t col0,
            int lane)
{
    constexpr int R = 1 << NL;
    T v[R][R][C];
    volume_load<T, M, NL, C, EDGE, NTL>(p, g, row0, col0, v);
    volume_level<T, M, C, 1, NL, R, R, C, EDGE, true, TILED>(p, v, g, row0, col0, lane);
}

// Unit u's plane group, first row and this lane's first column; true when
// the unit lies wholly inside the frame.  ZFAST puts the plane group
// innermost in the unit order.
template<int NL, int C, bool ZFAST>
__device__ __forceinline__ bool
volume_coords(const VolumeParams& p, uint32_t u, int lane, uint32_t& g, uint32_t& row0,
              uint32_t& col0)
{
    uint32_t ux, uy;
    if constexpr (ZFAST) {
        const uint32_t groups = p.total_units / (p.units_x * p.units_y);
        g = u % groups;
        const uint32_t t = u / groups;
        ux = t % p.units_x;
        uy = t / p.units_x;
    } else {
        ux = u % p.units_x;
        const uint32_t t = u / p.units_x;
        uy = t % p.units_y;
        g = t / p.units_y;
    }
    row0 = uy * (1u << NL);
    const uint32_t tile_col0 = ux * (64u * C);
    col0 = tile_col0 + uint32_t(lane) * C;
    return (tile_col0 + 64u * C <= p.W) && (row0 + (1u << NL) <= p.H);
}

// NTL: nontemporal loads.  UPW units per wave (consecutive, columns first):
// with UPW > 1 and every unit inside the frame, all of them are loaded
// before the first is reduced, so a wave has UPW units' loads in flight —
// Decimate's units read only 4 KiB.  Round 5: with the
// volume in HBM, Decimate's launch runs at 0.59-0.60 of spec with
// nontemporal loads and 0.55-0.56 with plain ones; the 0.82 once measured
// with plain loads came from the Infinity Cache holding the launch's
// 128 MiB read set between launches.
//
// TILED (launch_volume_tiled; one unit per wave, columns first, nontemporal
// loads): the levels go out in chunk-tile order — VolumeTiledParams.
template<typename T, int M, int NL, bool NTL, int UPW, int C = 16 / int(sizeof(T)),
         bool ZFAST = false, bool TILED = false>
__global__ __launch_bounds__(256) void
volume_kernel(std::conditional_t<TILED, VolumeTiledParams, VolumeParams> p)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t blk = blockIdx.x;
    if constexpr (TILED) {
        static_assert(UPW == 1 && !ZFAST && NTL, "the tiled volume kernel's one form");
        // The first blocks zero-fill the tile overhang, as in cascade_kernel.
        const uint32_t wpb = blockDim.x >> 6;
        const uint32_t zb = p.zwaves / wpb;
        if (blk < zb) {
            zero_fill_tiled<T, NL>(p, blk * wpb + wave, p.zwaves, lane, NL,
                                   p.total_units / (p.units_x * p.units_y));
            return;
        }
        blk -= zb;
    }
    const uint32_t w = blk * (blockDim.x >> 6) + wave;
    if constexpr (UPW == 1) {
        if (w >= p.total_units)
            return;
        uint32_t g, row0, col0;
        if (volume_coords<NL, C, ZFAST>(p, w, lane, g, row0, col0))
            volume_unit<T, M, NL, C, false, NTL, TILED>(p, g, row0, col0, lane);
        else
            volume_unit<T, M, NL, C, true, NTL, TILED>(p, g, row0, col0, lane);
    } else {
        constexpr int R = 1 << NL;
        const uint32_t u0 = w * UPW;
        if (u0 >= p.total_units)
            return;
        uint32_t g[UPW], row0[UPW], col0[UPW];
        bool inside = u0 + UPW <= p.total_units;
#pragma unroll
        for (int i = 0; i < UPW; ++i) {
            const uint32_t u = min(u0 + uint32_t(i), p.total_units - 1);
            inside = volume_coords<NL, C, ZFAST>(p, u, lane, g[i], row0[i], col0[i]) && inside;
        }
        if (inside) {
            T v[UPW][R][R][C];
#pragma unroll
            for (int i = 0; i < UPW; ++i)
                volume_load<T, M, NL, C, false, NTL>(p, g[i], row0[i], col0[i], v[i]);
#pragma unroll
            for (int i = 0; i < UPW; ++i)
                volume_level<T, M, C, 1, NL, R, R, C, false, true>(p, v[i], g[i], row0[i],
                                                                   col0[i], lane);
        } else {
            for (int i = 0; i < UPW && u0 + uint32_t(i) < p.total_units; ++i) {
                uint32_t gg, r0, c0;
                if (volume_coords<NL, C, ZFAST>(p, u0 + uint32_t(i), lane, gg, r0, c0))
                    volume_unit<T, M, NL, C, false, NTL>(p, gg, r0, c0, lane);
                else
                    volume_unit<T, M, NL, C, true, NTL>(p, gg, r0, c0, lane);
            }
        }
    }
}

// ---- generic single level --------------------------------------------------

template<typename T, int M>
__global__ __launch_bounds__(256) void
xy_generic_kernel(const T* __restrict__ src,
                  uint64_t src_frame_elems,
                  uint32_t w,
                  uint32_t h,
                  T* __restrict__ dst,
                  uint64_t dst_frame_elems,
                  uint32_t wo,
                  uint32_t ho,
                  uint64_t total)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
         i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t c = uint32_t(i % wo);
        const uint64_t t = i / wo;
        const uint32_t r = uint32_t(t % ho);
        const uint64_t f = t / ho;
        const uint32_t col = 2 * c, row = 2 * r;
        const bool pw = col + 1 >= w;
        const bool ph = row + 1 >= h;
        const T* s = src + f * src_frame_elems + uint64_t(row) * w + col;
        const uint32_t dr = pw ? 0 : 1;
        const uint64_t dd = ph ? 0 : w;
        const T here = s[0];
        const T right = s[dr];
        const T down = s[dd];
        const T diag = s[dd + dr];
        dst[f * dst_frame_elems + uint64_t(r) * wo + c] =
          reduce4<T, M>(here, right, down, diag);
    }
}

// ---- Z pair ----------------------------------------------------------------

template<typename T, int M, bool VEC>
__global__ __launch_bounds__(256) void
zpair_kernel(T* out, const T* earlier, const T* current, uint64_t n)
{
    constexpr int C = 16 / int(sizeof(T));
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    const uint64_t tid = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    uint64_t done = 0;
    if constexpr (VEC) {
        // all three pointers 16-byte aligned: 16 B per lane per operand
        const uint64_t nvec = n / C;
        for (uint64_t i = tid; i < nvec; i += stride) {
            const u32x4 qa = reinterpret_cast<const u32x4*>(earlier)[i];
            const u32x4 qb = reinterpret_cast<const u32x4*>(current)[i];
            T a[C], b[C], o[C];
            __builtin_memcpy(a, &qa, 16);
            __builtin_memcpy(b, &qb, 16);
#pragma unroll
            for (int k = 0; k < C; ++k) {
                o[k] = reduce2<T, M>(a[k], b[k]);
            }
            store_vec<T, C>(out + i * C, o);
        }
        done = nvec * C;
    }
    for (uint64_t i = done + tid; i < n; i += stride) {
        out[i] = reduce2<T, M>(earlier[i], current[i]);
    }
}

// ---- Z run -------------------------------------------------------------------
//
// Up to kMaxZLevels consecutive levels that halve Z alone (w x h unchanged),
// for a batch of whole plane groups: level j's plane k is
// reduce2(earlier, current) of level j-1's planes 2k and 2k+1, each level
// from the truncated one before it — volume_level's Z step without its XY
// step.  A wave takes one plane group (2^NL consecutive input planes) by one
// span of 64 lanes x kZRunVecs 16-byte vectors (ZRunPlan); a lane holds the
// same vectors of every plane of the group, so the whole tree is in-lane.
// Planes of any element count sit at any byte offset: loads and stores are
// 16 bytes at byte alignment, counted from each plane's own start, and the
// elements behind a plane's last whole vector go one to a lane from the span
// that ends the plane.  Decimate reads the even planes only (plane 2k is
// level 1's plane k; the odd planes feed nothing).
struct ZRunParams
{
    const uint8_t* src;
    uint64_t src_frame_elems;
    uint64_t elems; // of one plane
    uint32_t spans, total_units;
    uint8_t* dst[kMaxZLevels];
    uint64_t dst_frame_elems[kMaxZLevels];
};

// Levels 1..NL of the N = 2^NL values v[] (one per plane of the group), each
// written through st(level, plane within the group's share of it, value).
template<typename T, int M, int NL, int J = 1, typename V, typename St>
__device__ __forceinline__ void
zrun_tree(const V (&v)[1 << (NL - J + 1)], St&& st)
{
    constexpr int N = 1 << (NL - J);
    V o[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if constexpr (std::is_same_v<V, T>) {
            o[k] = reduce2<T, M>(v[2 * k], v[2 * k + 1]);
        } else {
#pragma unroll
            for (int c = 0; c < int(sizeof(V) / sizeof(T)); ++c)
                o[k].e[c] = reduce2<T, M>(v[2 * k].e[c], v[2 * k + 1].e[c]);
        }
        st(J, k, o[k]);
    }
    if constexpr (J < NL)
        zrun_tree<T, M, NL, J + 1>(o, st);
}

template<typename T, int C>
struct ZRunVec
{
    T e[C];
};

// EDGE: the span reaches past the plane's last whole vector — lanes past it
// skip their loads and stores (exec mask); the reductions run on every lane,
// so mean2's wave_any branch stays wave-uniform (§12.1's pattern).
template<typename T, int M, int NL, bool EDGE>
__device__ __forceinline__ void
zrun_vectors(const ZRunParams& p, uint32_t g, uint64_t vec0, uint64_t nvec)
{
    constexpr int C = 16 / int(sizeof(T));
    constexpr int P = 1 << NL;
    constexpr int U = int(kZRunVecs);
    using V = ZRunVec<T, C>;
    const T* src = reinterpret_cast<const T*>(p.src) + uint64_t(g) * P * p.src_frame_elems;
    V v[U][P] = {};
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        in[u] = !EDGE || vec0 + uint64_t(u) * 64 < nvec;
    // every load of the unit before the first reduction
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (in[u]) {
#pragma unroll
            for (int z = 0; z < P; ++z) {
                if (M == kDecimate && z % 2 != 0)
                    continue;
                const T* a = src + uint64_t(z) * p.src_frame_elems + (vec0 + uint64_t(u) * 64) * C;
                const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4_u*>(a));
                __builtin_memcpy(&v[u][z], &q, 16);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t e0 = (vec0 + uint64_t(u) * 64) * C;
        zrun_tree<T, M, NL>(v[u], [&](int j, int k, const V& o) {
            if (in[u]) {
                T* d = reinterpret_cast<T*>(p.dst[j - 1]) +
                       (uint64_t(g) * (P >> j) + uint32_t(k)) * p.dst_frame_elems[j - 1] + e0;
                store_vec<T, C, true>(d, o.e);
            }
        });
    }
}

template<typename T, int M, int NL>
__global__ __launch_bounds__(256) void
zrun_kernel(ZRunParams p)
{
    constexpr int C = 16 / int(sizeof(T));
    constexpr int P = 1 << NL;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t unit = blockIdx.x * (blockDim.x >> 6) + wave;
    if (unit >= p.total_units)
        return;
    // spans fastest, then plane groups
    const uint32_t g = unit / p.spans;
    const uint32_t s = unit - g * p.spans;
    const uint64_t nvec = p.elems / C;
    const uint64_t span0 = uint64_t(s) * (64u * kZRunVecs);
    if (span0 + 64u * kZRunVecs <= nvec)
        zrun_vectors<T, M, NL, false>(p, g, span0 + lane, nvec);
    else if (span0 < nvec)
        zrun_vectors<T, M, NL, true>(p, g, span0 + lane, nvec);
    if (C > 1 && s + 1 == p.spans) {
        // the 1..C-1 elements behind the last whole vector, one to a lane
        const uint32_t tail = uint32_t(p.elems - nvec * C);
        if (tail == 0)
            return;
        const bool in = lane < tail;
        const uint64_t e0 = nvec * C + lane;
        const T* src = reinterpret_cast<const T*>(p.src) + uint64_t(g) * P * p.src_frame_elems;
        T v[P] = {};
        if (in) {
#pragma unroll
            for (int z = 0; z < P; ++z) {
                if (M == kDecimate && z % 2 != 0)
                    continue;
                v[z] = src[uint64_t(z) * p.src_frame_elems + e0];
            }
        }
        zrun_tree<T, M, NL>(v, [&](int j, int k, T o) {
            if (in)
                reinterpret_cast<T*>(p.dst[j - 1])[(uint64_t(g) * (P >> j) + uint32_t(k)) *
                                                     p.dst_frame_elems[j - 1] +
                                                   e0] = o;
        });
    }
}

// ---- Z run, chunk-tiled ------------------------------------------------------
//
// zrun_kernel with every level also (dst[j] null: only) written in chunk-tile
// order, plane k of level j + 1 as frame k of tl[j] (launch_zrun_tiled).  The
// planes are W x H (elems = W * H); units, loads and the tree are
// zrun_kernel's.  A lane turns its vector's first element e into
// (y, x) = (e / W, e % W): the span's first element is divided once per wave
// (uniform), the lane's offset behind it — below 2^12 — by FastDiv.  Per
// level, with that level's own tile shape, a vector whose C elements lie in
// one frame row and one tile row is one 16-byte store; any other goes element
// by element, the address worked out anew only where a frame row or a tile
// row ends.  The stores cover exactly the frame; the grid's first zwaves /
// (waves per block) blocks zero-fill the rest of the padded area
// (zero_fill_tiled<T, NL>, cov_w = W and cov_h = H).  One flag byte per tile,
// cleared before the launch, set to 1 by every lane storing a nonzero bit
// pattern into the tile.  tl[] has the cascade's length for zero_fill_tiled.
struct ZRunTiledParams : ZRunParams
{
    uint32_t W;
    FastDiv dw; // by W
    TiledLevel tl[kMaxFusedLevels];
    uint32_t zitems; // zero-fill items per plane group, all levels
    FastDiv zdiv;    // by zitems
    uint32_t zwaves;
};

// Row and column of plane element `base` (wave-uniform).
__device__ __forceinline__ void
zrun_row_col(const ZRunTiledParams& p, uint64_t base, uint32_t& y, uint32_t& x)
{
    if ((p.elems >> 32) == 0) {
        y = p.dw.div(uint32_t(base));
        x = uint32_t(base) - y * p.W;
    } else {
        const uint64_t q = base / p.W;
        y = uint32_t(q);
        x = uint32_t(base - q * p.W);
    }
}

// N consecutive plane elements e[], the first at (y, x), into frame `plane`
// of tiled level t.  Every element lies inside the plane.
template<typename T, int N>
__device__ __forceinline__ void
zrun_store_tiled(const TiledLevel& t, uint32_t W, uint32_t plane, uint32_t y, uint32_t x,
                 const T (&e)[N])
{
    T* base = reinterpret_cast<T*>(t.tdst) + tiled_frame_base(t, plane);
    uint8_t* flags = t.flags ? t.flags + uint64_t(plane) * t.flags_frame : nullptr;
    uint32_t ty = t.dr.div(y), tx = t.dc.div(x);
    uint32_t ry = y - ty * t.tr, cx = x - tx * t.tc;
    const auto at = [&]() {
        return base + (uint64_t(ty) * t.ntx + tx) * t.tstride + uint64_t(ry) * t.tc + cx;
    };
    if (N == 1 || (x + N <= W && cx + N <= t.tc)) {
        bool nz = false;
#pragma unroll
        for (int c = 0; c < N; ++c)
            nz = nz || nonzero_bits(e[c]);
        store_vec<T, N, true>(at(), e);
        if (flags && nz)
            flags[ty * t.ntx + tx] = 1;
        return;
    }
    if constexpr (N > 1) {
        // a rolled loop over the 16 bytes as one integer, the next element
        // shifted down each turn: no register is indexed by the counter
        static_assert(N * sizeof(T) == 16, "a lane's vector");
        unsigned __int128 q;
        __builtin_memcpy(&q, e, 16);
        T* d = at();
#pragma clang loop unroll(disable)
        for (int c = 0; c < N; ++c) {
            const uint64_t lo = uint64_t(q);
            T one[1];
            __builtin_memcpy(one, &lo, sizeof(T));
            store_vec<T, 1, true>(d, one);
            if (flags && nonzero_bits(one[0]))
                flags[ty * t.ntx + tx] = 1;
            q >>= 8 * sizeof(T);
            ++x;
            ++cx;
            ++d;
            if (x == W) {
                // the frame row ends: the next row's first tile
                x = 0;
                ++y;
                ty = t.dr.div(y);
                ry = y - ty * t.tr;
                tx = 0;
                cx = 0;
                d = at();
            } else if (cx == t.tc) {
                // the tile row ends: the same row of the next tile
                ++tx;
                cx = 0;
                d = at();
            }
        }
    }
}

// Level I + 1 of a unit's outputs (levels[j][k]: level j + 1, plane k of the
// group's share), N elements a lane store, row-major where dst[I] is set and
// as tiles.  One level after the other, each with its TiledLevel at a
// compile-time place in the kernel arguments, so that one level's scalars are
// live at a time.
template<typename T, int NL, int N, int U, int I = 0, typename V>
__device__ __forceinline__ void
zrun_store_levels(const ZRunTiledParams& p, uint32_t g, const V (&levels)[U][NL][(1 << NL) / 2],
                  const bool (&in)[U], const uint64_t (&e0)[U], const uint32_t (&y)[U],
                  const uint32_t (&x)[U])
{
    if constexpr (I < NL) {
        constexpr int PL = (1 << NL) >> (I + 1); // the level's planes per group
        const TiledLevel t = p.tl[I];            // one kernarg block load
        T* rm = reinterpret_cast<T*>(p.dst[I]);
        const uint64_t rm_frame = p.dst_frame_elems[I];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (in[u]) {
#pragma unroll
                for (int k = 0; k < PL; ++k) {
                    const uint32_t plane = g * uint32_t(PL) + uint32_t(k);
                    T e[N];
                    __builtin_memcpy(e, &levels[u][I][k], sizeof(e));
                    if (rm)
                        store_vec<T, N, true>(rm + uint64_t(plane) * rm_frame + e0[u], e);
                    zrun_store_tiled<T, N>(t, p.W, plane, y[u], x[u], e);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        zrun_store_levels<T, NL, N, U, I + 1>(p, g, levels, in, e0, y, x);
    }
}

// zrun_vectors with the tiled stores.  (y0, x0): row and column of the span's
// first element (uniform); x0 + the lane's offset stays below 2^31 + 2^12.
template<typename T, int M, int NL, bool EDGE>
__device__ __forceinline__ void
zrun_tiled_vectors(const ZRunTiledParams& p, uint32_t g, uint64_t vec0, uint64_t nvec,
                   uint32_t y0, uint32_t x0, uint32_t lane)
{
    constexpr int C = 16 / int(sizeof(T));
    constexpr int P = 1 << NL;
    constexpr int U = int(kZRunVecs);
    using V = ZRunVec<T, C>;
    const T* src = reinterpret_cast<const T*>(p.src) + uint64_t(g) * P * p.src_frame_elems;
    V v[U][P] = {};
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        in[u] = !EDGE || vec0 + uint64_t(u) * 64 < nvec;
    // every load of the unit before the first reduction
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (in[u]) {
#pragma unroll
            for (int z = 0; z < P; ++z) {
                if (M == kDecimate && z % 2 != 0)
                    continue;
                const T* a = src + uint64_t(z) * p.src_frame_elems + (vec0 + uint64_t(u) * 64) * C;
                const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4_u*>(a));
                __builtin_memcpy(&v[u][z], &q, 16);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // the whole tree on every lane, then the stores, masked
    V levels[U][NL][P / 2];
    uint64_t e0[U];
    uint32_t y[U], x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        zrun_tree<T, M, NL>(v[u], [&](int j, int k, const V& o)
                                    __attribute__((always_inline)) { levels[u][j - 1][k] = o; });
        e0[u] = (vec0 + uint64_t(u) * 64) * C;
        // the vector's first element as (y, x): one division by W
        const uint32_t xx = x0 + (lane + uint32_t(u) * 64) * uint32_t(C);
        const uint32_t dy = p.dw.div(xx);
        y[u] = y0 + dy;
        x[u] = xx - dy * p.W;
    }
    zrun_store_levels<T, NL, C, U>(p, g, levels, in, e0, y, x);
}

template<typename T, int M, int NL>
__global__ __launch_bounds__(256) void
zrun_tiled_kernel(ZRunTiledParams p)
{
    constexpr int C = 16 / int(sizeof(T));
    constexpr int P = 1 << NL;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wpb = blockDim.x >> 6;
    uint32_t blk = blockIdx.x;
    // The first blocks zero-fill the tile overhang, as in volume_kernel.
    const uint32_t zb = p.zwaves / wpb;
    if (blk < zb) {
        zero_fill_tiled<T, NL>(p, blk * wpb + wave, p.zwaves, int(lane), NL,
                               p.total_units / p.spans);
        return;
    }
    blk -= zb;
    const uint32_t unit = blk * wpb + wave;
    if (unit >= p.total_units)
        return;
    // spans fastest, then plane groups
    const uint32_t g = unit / p.spans;
    const uint32_t s = unit - g * p.spans;
    const uint64_t nvec = p.elems / C;
    const uint64_t span0 = uint64_t(s) * (64u * kZRunVecs);
    if (span0 < nvec) {
        uint32_t y0, x0;
        zrun_row_col(p, span0 * C, y0, x0);
        if (span0 + 64u * kZRunVecs <= nvec)
            zrun_tiled_vectors<T, M, NL, false>(p, g, span0 + lane, nvec, y0, x0, lane);
        else
            zrun_tiled_vectors<T, M, NL, true>(p, g, span0 + lane, nvec, y0, x0, lane);
    }
    if (C > 1 && s + 1 == p.spans) {
        // the 1..C-1 elements behind the last whole vector, one to a lane
        const uint32_t tail = uint32_t(p.elems - nvec * C);
        if (tail == 0)
            return;
        const bool in = lane < tail;
        const uint64_t e0 = nvec * C + lane;
        uint32_t y0, x0;
        zrun_row_col(p, nvec * C, y0, x0);
        const uint32_t xx = x0 + lane;
        const uint32_t dy = p.dw.div(xx);
        const uint32_t y = y0 + dy, x = xx - dy * p.W;
        const T* src = reinterpret_cast<const T*>(p.src) + uint64_t(g) * P * p.src_frame_elems;
        T v[P] = {};
        if (in) {
#pragma unroll
            for (int z = 0; z < P; ++z) {
                if (M == kDecimate && z % 2 != 0)
                    continue;
                v[z] = src[uint64_t(z) * p.src_frame_elems + e0];
            }
        }
        T levels[1][NL][P / 2];
        zrun_tree<T, M, NL>(v, [&](int j, int k, T o)
                                 __attribute__((always_inline)) { levels[0][j - 1][k] = o; });
        const bool in1[1] = { in };
        const uint64_t e1[1] = { e0 };
        const uint32_t y1[1] = { y }, x1[1] = { x };
        zrun_store_levels<T, NL, 1, 1>(p, g, levels, in1, e1, y1, x1);
    }
}

// ---- chunk tiling --------------------------------------
//
// Array::write_frame_to_chunks_ (array.cpp:507-622) copies each frame tile's
// rows into its chunk buffer at stride tile_cols*bpp (Chunk::write_tile_rows,
// chunk.cpp:17-58), leaving the overhang zero, and byte-scans the copied rows
// for the all-zero-chunk skip.  This kernel emits the frame already in that
// tile order (zero-padded) plus the scan result, so the host does one
// contiguous copy per tile and no scan.  Grid: `slices` blocks per tile, one
// block-wide OR per block.

// SLICE_FLAGS: every block writes its own flag byte (flags[t*slices + s]),
// no atomics and no pre-clear; otherwise one u32 per tile, OR-ed atomically
// (the caller clears it).
template<typename T, bool SLICE_FLAGS>
__global__ __launch_bounds__(256) void
tile_kernel(const T* __restrict__ src,
            uint32_t W,
            uint32_t H,
            uint32_t tile_rows,
            uint32_t tile_cols,
            uint32_t n_tiles_x,
            uint32_t slices,
            T* __restrict__ dst,
            void* __restrict__ flags)
{
    const uint32_t t = blockIdx.x / slices;
    const uint32_t s = blockIdx.x % slices;
    const uint32_t ty = t / n_tiles_x, tx = t % n_tiles_x;
    const uint32_t tile_elems = tile_rows * tile_cols; // < 2^31, checked by the launcher
    const uint32_t per = (tile_elems + slices - 1) / slices;
    const uint32_t e0 = s * per;
    const uint32_t e1 = e0 + per < tile_elems ? e0 + per : tile_elems;
    T* out = dst + uint64_t(t) * tile_elems;
    bool any = false;
    for (uint32_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const uint32_t r = e / tile_cols;
        const uint32_t c = e % tile_cols;
        const uint32_t row = ty * tile_rows + r;
        const uint32_t col = tx * tile_cols + c;
        T v = T(0);
        if (row < H && col < W) {
            v = src[uint64_t(row) * W + col];
            any = any || nonzero_bits(v);
        }
        out[e] = v;
    }
    const bool block_any = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        if constexpr (SLICE_FLAGS) {
            static_cast<uint8_t*>(flags)[blockIdx.x] = block_any ? 1 : 0;
        } else if (block_any) {
            atomicOr(static_cast<uint32_t*>(flags) + t, 1u);
        }
    }
}

// 16-B vector form for frames whose rows and tiles are 16-B multiples (so a
// vector is entirely inside or entirely outside the frame): block = one
// (tile, slice of rows); lane = one 16-B vector of a tile row.
__device__ __forceinline__ bool
nonzero_vec(u32x4 v)
{
    return (v.x | v.y | v.z | v.w) != 0;
}

template<bool SLICE_FLAGS>
__global__ __launch_bounds__(256) void
tile_kernel_vec(const u32x4* __restrict__ src,
                uint32_t row_vecs,   // W * bpp / 16
                uint32_t H,
                uint32_t tile_rows,
                uint32_t tile_vecs,  // tile_cols * bpp / 16
                uint32_t n_tiles_x,
                uint32_t slices,
                u32x4* __restrict__ dst,
                void* __restrict__ flags)
{
    const uint32_t t = blockIdx.x / slices;
    const uint32_t s = blockIdx.x % slices;
    const uint32_t ty = t / n_tiles_x, tx = t % n_tiles_x;
    const uint32_t rows_per = (tile_rows + slices - 1) / slices;
    const uint32_t r0 = s * rows_per;
    const uint32_t r1 = r0 + rows_per < tile_rows ? r0 + rows_per : tile_rows;
    // 32-bit in-slice indices (the launcher keeps a tile below 2^31 vectors)
    const uint32_t n = (r1 > r0 ? r1 - r0 : 0) * tile_vecs;
    u32x4* out = dst + uint64_t(t) * tile_rows * tile_vecs + uint64_t(r0) * tile_vecs;
    const uint32_t col_v0 = tx * tile_vecs;
    bool any = false;
    // U vectors per lane per round, all loads issued before the stores
    constexpr uint32_t U = 8;
    for (uint32_t e0 = threadIdx.x; e0 < n; e0 += U * blockDim.x) {
        u32x4 v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t e = e0 + u * blockDim.x;
            const uint32_t r = r0 + e / tile_vecs;
            const uint32_t cv = col_v0 + e % tile_vecs;
            const uint32_t row = ty * tile_rows + r;
            v[u] = u32x4{ 0u, 0u, 0u, 0u };
            if (e < n && row < H && cv < row_vecs)
                v[u] = __builtin_nontemporal_load(src + uint64_t(row) * row_vecs + cv);
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t e = e0 + u * blockDim.x;
            if (e < n) {
                any = any || nonzero_vec(v[u]);
                __builtin_nontemporal_store(v[u], out + e);
            }
        }
    }
    const bool block_any = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        if constexpr (SLICE_FLAGS) {
            static_cast<uint8_t*>(flags)[blockIdx.x] = block_any ? 1 : 0;
        } else if (block_any) {
            atomicOr(static_cast<uint32_t*>(flags) + t, 1u);
        }
    }
}

// ---- transpose_frame (array.cpp:488-504) ------------------------------------
//
// Y x X -> X x Y of a row-major `rows` x `cols` frame, for arrays whose
// storage order swaps the two spatial dimensions (Array::write_frame_to_chunks_
// transposes level 0 before chunking, array.cpp:517-530, and the downsampler
// then sees the transposed frame).  Pure data movement, HBM-bound:
// 2 * rows * cols * sizeof(T) bytes.  One block per kTransposeSub tiles of
// kTransposeTile^2 elements,
// staged through LDS so both the global reads (source rows) and the global
// writes (destination rows) are contiguous; with VEC each lane moves 16 B per
// access on interior tiles.  Edge tiles (and VEC=false frames, whose rows are
// not 16-B aligned) move one element per access.

// tile edge in elements: 256-B row segments on both sides (128 B for u8)
template<typename T>
constexpr int kTransposeTile = sizeof(T) == 1 ? 128 : 256 / int(sizeof(T));

template<typename T>
constexpr int kTransposePitch = kTransposeTile<T> + (sizeof(T) >= 4 ? 1 : 4 / int(sizeof(T)));

// tiles per block, stacked along the source rows: 32 KiB per block for every
// dtype (a lone 64 x 64 f32 tile moved 16 KiB and measured 84% of a D2D copy)
template<typename T>
constexpr int kTransposeSub =
  32768 / (kTransposeTile<T> * kTransposeTile<T> * int(sizeof(T))) > 1
    ? 32768 / (kTransposeTile<T> * kTransposeTile<T> * int(sizeof(T)))
    : 1;

template<typename T, bool VEC>
__global__ __launch_bounds__(256) void
transpose_kernel(const T* __restrict__ src, uint32_t rows, uint32_t cols, T* __restrict__ dst)
{
    constexpr int TD = kTransposeTile<T>;
    constexpr int P = kTransposePitch<T>;
    constexpr int S = kTransposeSub<T>;
    __shared__ T tile[S][TD * P];
    const uint32_t c0 = blockIdx.x * TD;     // source columns = destination rows
    const uint32_t rb = blockIdx.y * TD * S; // source rows = destination columns
    const int tid = threadIdx.x;
    const bool interior = VEC && rb + TD * S <= rows && c0 + TD <= cols;
    if (interior) {
        constexpr int V = 16 / int(sizeof(T));
        constexpr int VPR = TD / V;       // vectors per tile row
        constexpr int RPP = 256 / VPR;    // tile rows per pass
        const int v = tid % VPR;
        if constexpr (S > 1) {
            // every sub-tile's loads before the first LDS store (f32 84% ->
            // 91% of a D2D copy, u8 likewise; the lone u16 tile measured
            // faster with each load followed by its LDS store, below)
            u32x4 x[S][TD / RPP];
#pragma unroll
            for (int t = 0; t < S; ++t) {
#pragma unroll
                for (int i = 0; i < TD / RPP; ++i) {
                    const int r = tid / VPR + i * RPP;
                    x[t][i] = __builtin_nontemporal_load(
                      reinterpret_cast<const u32x4*>(src + uint64_t(rb + t * TD + r) * cols + c0) +
                      v);
                }
            }
#pragma unroll
            for (int t = 0; t < S; ++t) {
#pragma unroll
                for (int i = 0; i < TD / RPP; ++i) {
                    const int r = tid / VPR + i * RPP;
                    T e[V];
                    __builtin_memcpy(e, &x[t][i], 16);
#pragma unroll
                    for (int k = 0; k < V; ++k)
                        tile[t][r * P + v * V + k] = e[k];
                }
            }
        } else {
#pragma unroll
            for (int r = tid / VPR; r < TD; r += RPP) {
                const u32x4 x = __builtin_nontemporal_load(
                  reinterpret_cast<const u32x4*>(src + uint64_t(rb + r) * cols + c0) + v);
                T e[V];
                __builtin_memcpy(e, &x, 16);
#pragma unroll
                for (int k = 0; k < V; ++k)
                    tile[0][r * P + v * V + k] = e[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < S; ++t) {
#pragma unroll
            for (int c = tid / VPR; c < TD; c += RPP) {
                T e[V];
#pragma unroll
                for (int k = 0; k < V; ++k)
                    e[k] = tile[t][(v * V + k) * P + c];
                u32x4 y;
                __builtin_memcpy(&y, e, 16);
                auto* q =
                  reinterpret_cast<u32x4*>(dst + uint64_t(c0 + c) * rows + rb + t * TD) + v;
                __builtin_nontemporal_store(y, q);
            }
        }
    } else {
        // one element per access; lanes sweep rows so accesses stay contiguous
        const int x = tid % TD;
        for (int t = 0; t < S; ++t) {
            const uint32_t r0 = rb + t * TD;
            for (int r = tid / TD; r < TD; r += 256 / TD) {
                if (r0 + r < rows && c0 + x < cols)
                    tile[t][r * P + x] = src[uint64_t(r0 + r) * cols + c0 + x];
            }
        }
        __syncthreads();
        for (int t = 0; t < S; ++t) {
            const uint32_t r0 = rb + t * TD;
            for (int c = tid / TD; c < TD; c += 256 / TD) {
                if (c0 + c < cols && r0 + x < rows)
                    dst[uint64_t(c0 + c) * rows + r0 + x] = tile[t][x * P + c];
            }
        }
    }
}

// ---- dispatch ---------------------------------------------------------------

template<typename F>
hipError_t
with_dtype(int dtype, F&& f)
{
    // only this shard's dtypes are instantiated
    switch (dtype) {
        case 0:
            if constexpr (0 % AQZ_SHARDS == AQZ_SHARD)
                return f(uint8_t{});
            return hipErrorInvalidValue;
        case 1:
            if constexpr (1 % AQZ_SHARDS == AQZ_SHARD)
                return f(uint16_t{});
            return hipErrorInvalidValue;
        case 2:
            if constexpr (2 % AQZ_SHARDS == AQZ_SHARD)
                return f(uint32_t{});
            return hipErrorInvalidValue;
        case 3:
            if constexpr (3 % AQZ_SHARDS == AQZ_SHARD)
                return f(uint64_t{});
            return hipErrorInvalidValue;
        case 4:
            if constexpr (4 % AQZ_SHARDS == AQZ_SHARD)
                return f(int8_t{});
            return hipErrorInvalidValue;
        case 5:
            if constexpr (5 % AQZ_SHARDS == AQZ_SHARD)
                return f(int16_t{});
            return hipErrorInvalidValue;
        case 6:
            if constexpr (6 % AQZ_SHARDS == AQZ_SHARD)
                return f(int32_t{});
            return hipErrorInvalidValue;
        case 7:
            if constexpr (7 % AQZ_SHARDS == AQZ_SHARD)
                return f(int64_t{});
            return hipErrorInvalidValue;
        case 8:
            if constexpr (8 % AQZ_SHARDS == AQZ_SHARD)
                return f(float{});
            return hipErrorInvalidValue;
        case 9:
            if constexpr (9 % AQZ_SHARDS == AQZ_SHARD)
                return f(double{});
            return hipErrorInvalidValue;
        default:
            return hipErrorInvalidValue;
    }
}

template<typename F>
hipError_t
with_method(int method, F&& f)
{
    switch (method) {
        case kDecimate:
            return f(std::integral_constant<int, kDecimate>{});
        case kMean:
            return f(std::integral_constant<int, kMean>{});
        case kMin:
            return f(std::integral_constant<int, kMin>{});
        case kMax:
            return f(std::integral_constant<int, kMax>{});
        default:
            return hipErrorInvalidValue;
    }
}

// The fused launches write 1..kMaxFusedLevels levels.
template<typename F>
hipError_t
with_levels(int n_out, F&& f)
{
    switch (n_out) {
        case 1:
            return f(std::integral_constant<int, 1>{});
        case 2:
            return f(std::integral_constant<int, 2>{});
        case 3:
            return f(std::integral_constant<int, 3>{});
        case 4:
            return f(std::integral_constant<int, 4>{});
        default:
            return hipErrorInvalidValue;
    }
}

template<typename F>
hipError_t
with_flag(bool on, F&& f)
{
    return on ? f(std::true_type{}) : f(std::false_type{});
}

template<int K>
using int_tag = std::integral_constant<int, K>;

// The source, units and row-major levels of CascadeParams / VolumeParams.
template<typename P, typename Plan>
void
fill_frames(P& p, const Plan& pl, const void* src, uint64_t src_frame_elems, uint32_t W,
            uint32_t H, const LevelOut* outs)
{
    p.src = static_cast<const uint8_t*>(src);
    p.src_frame_elems = src_frame_elems;
    p.W = W;
    p.H = H;
    p.units_x = pl.units_x;
    p.units_y = pl.units_y;
    p.total_units = pl.total_units;
    for (int i = 0; i < pl.n_out; ++i) {
        p.dst[i] = static_cast<uint8_t*>(outs[i].ptr);
        p.dst_frame_elems[i] = outs[i].frame_elems;
        p.w[i] = outs[i].w;
        p.h[i] = outs[i].h;
    }
}

// Fill level i's TiledLevel from its plan and output.
void
fill_tiled_level(TiledLevel& q, const TiledLevelPlan& l, const TiledOut& t)
{
    q.tdst = static_cast<uint8_t*>(t.ptr);
    q.flags = t.nonzero;
    q.tframe_elems = l.tframe_elems;
    q.foff = t.frame_offsets;
    q.tstride = l.tstride;
    q.tr = t.tile_rows;
    q.tc = t.tile_cols;
    q.ntx = l.ntx;
    q.pw = l.pw;
    q.ph = l.ph;
    q.slots = l.slots;
    q.slots_x = l.slots_x;
    q.flags_frame = l.flags_frame;
    q.cov_w = l.cov_w;
    q.cov_h = l.cov_h;
    q.zrows = l.zrows;
    q.dr = FastDiv::make(t.tile_rows);
    q.dc = FastDiv::make(t.tile_cols);
}

} // namespace

// The planned launchers: the plan (ds_plan.hh) has decided everything;
// these fill the kernel parameters from it and pick the instantiation its
// selector fields name.  A selector value no kernel is built for is an error,
// never another kernel.

hipError_t
AQZ_SHARDED(run_cascade)(const CascadePlan& pl, const void* src, uint64_t src_frame_elems,
                         uint32_t W, uint32_t H, const LevelOut* outs, hipStream_t stream)
{
    if (!pl.valid)
        return hipErrorInvalidValue;
    CascadeParams p{};
    fill_frames(p, pl, src, src_frame_elems, W, H, outs);
    p.main_blocks = pl.main_blocks;
    p.remap = pl.remap;
    p.wb = pl.wb;
    p.order = pl.order;
    p.seg_w = pl.seg_w;
    p.nt = pl.nt;
    p.band_last = pl.band_last;
    p.seg_rowwise = pl.seg_rowwise;
    p.upw = pl.upw;
    const dim3 grid(pl.grid), block(pl.block);
    return with_dtype(pl.dtype, [&](auto tag) -> hipError_t {
        using T = decltype(tag);
        constexpr int CW = kCascadeCols<T>;
        constexpr int CN = CW / 2;
        auto go = [&](auto mtag, auto ltag, auto nttag, auto ctag) -> hipError_t {
            constexpr int M = decltype(mtag)::value;
            constexpr int NL = decltype(ltag)::value;
            constexpr bool NT = decltype(nttag)::value;
            constexpr int C = decltype(ctag)::value;
            if (!pl.band) {
                hipLaunchKernelGGL((cascade_kernel<T, M, NL, C, NT>), grid, block, 0, stream, p);
                return hipGetLastError();
            }
            auto band = [&](auto rtag, auto stag) -> hipError_t {
                constexpr bool RW = decltype(rtag)::value;
                constexpr bool SP = decltype(stag)::value;
                if (pl.lds > 65536) // above the default per-workgroup LDS
                    (void)hipFuncSetAttribute(
                      reinterpret_cast<const void*>(&cascade_band_kernel<T, M, NL, C, NT, RW, SP>),
                      hipFuncAttributeMaxDynamicSharedMemorySize, int(pl.lds));
                hipLaunchKernelGGL((cascade_band_kernel<T, M, NL, C, NT, RW, SP>), grid, block,
                                   pl.lds, stream, p, pl.stage_mask, pl.seg_tiles);
                return hipGetLastError();
            };
            // misaligned segments: a separate instantiation, so that
            // whole bands keep their code (a runtime branch per row
            // cost 3000^2 / 2600^2 u16 8-9%), for 2- and 4-byte types
            // at the wide tile only (where the planner picks them)
            if (pl.seg_rowwise) {
                if constexpr ((sizeof(T) == 2 || sizeof(T) == 4) &&
                              (C == CW || (sizeof(T) == 4 && C == CN)))
                    return band(std::true_type{}, std::false_type{});
                else
                    return hipErrorInvalidValue;
            }
            // whole-line loads for 4- and 8-byte types at the wide tile
            // (cascade_unit SPLIT)
            if (pl.split) {
                if constexpr (sizeof(T) >= 4 && C == CW)
                    return band(std::false_type{}, std::true_type{});
                else
                    return hipErrorInvalidValue;
            }
            return band(std::false_type{}, std::false_type{});
        };
        return with_method(pl.method, [&](auto mtag) -> hipError_t {
            return with_levels(pl.n_out, [&](auto ltag) -> hipError_t {
                return with_flag(pl.nt != 0, [&](auto nttag) -> hipError_t {
                    if (pl.cols == uint32_t(CW))
                        return go(mtag, ltag, nttag, int_tag<CW>{});
                    if (pl.cols == uint32_t(CN))
                        return go(mtag, ltag, nttag, int_tag<CN>{});
                    return hipErrorInvalidValue;
                });
            });
        });
    });
}

hipError_t
AQZ_SHARDED(run_cascade_tiled)(const TiledPlan& pl, const void* src, uint64_t src_frame_elems,
                               uint32_t W, uint32_t H, const LevelOut* outs,
                               const TiledOut* touts, const TiledOut* tbase, hipStream_t stream)
{
    if (!pl.valid || pl.base != (tbase != nullptr))
        return hipErrorInvalidValue;
    CascadeParams p{};
    BaseLevel b{};
    fill_frames(p, pl, src, src_frame_elems, W, H, outs);
    if (pl.base) {
        fill_tiled_level(b.tl0, pl.base_lv, *tbase);
        b.zdiv0 = FastDiv::make(pl.base_lv.zrows ? pl.base_lv.zrows : 1);
        if (pl.base_lv.clear_flags) {
            const hipError_t e = hipMemsetAsync(
              tbase->nonzero, 0, size_t(pl.n_frames) * pl.base_lv.ntx * pl.base_lv.nty, stream);
            if (e != hipSuccess)
                return e;
        }
    }
    for (int i = 0; i < pl.n_out; ++i) {
        const TiledOut& t = touts[i];
        const TiledLevelPlan& l = pl.lv[i];
        fill_tiled_level(p.tl[i], l, t);
        if (l.clear_flags) {
            const hipError_t e =
              hipMemsetAsync(t.nonzero, 0, size_t(pl.n_frames) * l.ntx * l.nty, stream);
            if (e != hipSuccess)
                return e;
        }
    }
    p.zitems = pl.zitems;
    p.zdiv = FastDiv::make(pl.zitems ? pl.zitems : 1);
    p.zwaves = pl.zwaves;
    p.main_blocks = pl.main_blocks;
    p.remap = pl.remap;
    p.seg_w = pl.seg_w;
    p.nt = pl.nt;
    const dim3 grid(pl.grid), block(pl.block);
    return with_dtype(pl.dtype, [&](auto tag) -> hipError_t {
        using T = decltype(tag);
        constexpr int CW = kCascadeCols<T>;
        constexpr int CN = CW / 2;
        auto go = [&](auto mtag, auto ltag, auto nttag, auto ctag, auto mdtag) -> hipError_t {
            constexpr int MD = decltype(mdtag)::value;
            if constexpr (MD >= 3)
                hipLaunchKernelGGL(
                  (cascade_base_kernel<T, decltype(mtag)::value, decltype(ltag)::value,
                                       decltype(ctag)::value, decltype(nttag)::value, MD - 2>),
                  grid, block, 0, stream, p, b);
            else
                hipLaunchKernelGGL(
                  (cascade_kernel<T, decltype(mtag)::value, decltype(ltag)::value,
                                  decltype(ctag)::value, decltype(nttag)::value, MD>),
                  grid, block, 0, stream, p);
            return hipGetLastError();
        };
        return with_method(pl.method, [&](auto mtag) -> hipError_t {
            return with_levels(pl.n_out, [&](auto ltag) -> hipError_t {
                return with_flag(pl.nt != 0, [&](auto nttag) -> hipError_t {
                    // tiled mode 1: wave blocks and tiles nest; 2: they do not;
                    // 3 / 4: the same with the base level written as tiles too
                    auto go_c = [&](auto ctag) -> hipError_t {
                        if (pl.base)
                            return pl.nested ? go(mtag, ltag, nttag, ctag, int_tag<3>{})
                                             : go(mtag, ltag, nttag, ctag, int_tag<4>{});
                        return pl.nested ? go(mtag, ltag, nttag, ctag, int_tag<1>{})
                                         : go(mtag, ltag, nttag, ctag, int_tag<2>{});
                    };
                    if (pl.cols == uint32_t(CW))
                        return go_c(int_tag<CW>{});
                    if (pl.cols == uint32_t(CN))
                        return go_c(int_tag<CN>{});
                    return hipErrorInvalidValue;
                });
            });
        });
    });
}

hipError_t
AQZ_SHARDED(run_volume)(const VolumePlan& pl, const void* src, uint64_t src_frame_elems,
                        uint32_t W, uint32_t H, const LevelOut* outs, hipStream_t stream)
{
    if (!pl.valid)
        return hipErrorInvalidValue;
    VolumeParams p{};
    fill_frames(p, pl, src, src_frame_elems, W, H, outs);
    const dim3 grid(pl.grid), block(pl.block);
    return with_dtype(pl.dtype, [&](auto tag) -> hipError_t {
        using T = decltype(tag);
        constexpr int CZ = 16 / int(sizeof(T));
        return with_method(pl.method, [&](auto mtag) -> hipError_t {
            constexpr int M = decltype(mtag)::value;
            auto go = [&](auto nltag) -> hipError_t {
                auto run = [&](auto ntltag, auto upwtag, auto zftag) -> hipError_t {
                    hipLaunchKernelGGL((volume_kernel<T, M, decltype(nltag)::value,
                                                      decltype(ntltag)::value,
                                                      decltype(upwtag)::value, CZ,
                                                      decltype(zftag)::value>),
                                       grid, block, 0, stream, p);
                    return hipGetLastError();
                };
                // Decimate alone has kernels of two and four units per wave;
                // four, and the plane-groups-fastest order, only with
                // nontemporal loads
                if constexpr (M == kDecimate) {
                    if (pl.upw == 4 && pl.ntl)
                        return with_flag(pl.zfast, [&](auto zftag) -> hipError_t {
                            return run(std::true_type{}, int_tag<4>{}, zftag);
                        });
                    if (pl.upw == 2 && pl.zfast && pl.ntl)
                        return run(std::true_type{}, int_tag<2>{}, std::true_type{});
                    if (pl.upw == 2 && !pl.zfast)
                        return with_flag(pl.ntl, [&](auto ntltag) -> hipError_t {
                            return run(ntltag, int_tag<2>{}, std::false_type{});
                        });
                }
                if (pl.upw != 1 || pl.zfast)
                    return hipErrorInvalidValue;
                return with_flag(pl.ntl, [&](auto ntltag) -> hipError_t {
                    return run(ntltag, int_tag<1>{}, std::false_type{});
                });
            };
            if (pl.n_out == 1)
                return go(int_tag<1>{});
            if (pl.n_out == 2)
                return go(int_tag<2>{});
            return hipErrorInvalidValue;
        });
    });
}

hipError_t
AQZ_SHARDED(run_volume_tiled)(const VolumeTiledPlan& pl, const void* src,
                              uint64_t src_frame_elems, uint32_t W, uint32_t H,
                              const LevelOut* outs, const TiledOut* touts, hipStream_t stream)
{
    if (!pl.valid)
        return hipErrorInvalidValue;
    VolumeTiledParams p{};
    fill_frames(p, pl, src, src_frame_elems, W, H, outs);
    for (int i = 0; i < pl.n_out; ++i) {
        fill_tiled_level(p.tl[i], pl.lv[i], touts[i]);
        if (pl.lv[i].clear_flags) {
            // level i + 1 emits n_planes >> (i + 1) planes
            const hipError_t e = hipMemsetAsync(
              touts[i].nonzero, 0, size_t(pl.n_planes >> (i + 1)) * pl.lv[i].flags_frame, stream);
            if (e != hipSuccess)
                return e;
        }
    }
    p.zitems = pl.zitems;
    p.zdiv = FastDiv::make(pl.zitems ? pl.zitems : 1);
    p.zwaves = pl.zwaves;
    const dim3 grid(pl.grid), block(pl.block);
    return with_dtype(pl.dtype, [&](auto tag) -> hipError_t {
        using T = decltype(tag);
        constexpr int CZ = 16 / int(sizeof(T));
        return with_method(pl.method, [&](auto mtag) -> hipError_t {
            constexpr int M = decltype(mtag)::value;
            auto go = [&](auto nltag) -> hipError_t {
                hipLaunchKernelGGL(
                  (volume_kernel<T, M, decltype(nltag)::value, true, 1, CZ, false, true>), grid,
                  block, 0, stream, p);
                return hipGetLastError();
            };
            if (pl.n_out == 1)
                return go(int_tag<1>{});
            if (pl.n_out == 2)
                return go(int_tag<2>{});
            return hipErrorInvalidValue;
        });
    });
}

namespace {

hipError_t
launch_tile_impl(int dtype,
                 const void* src,
                 uint32_t W,
                 uint32_t H,
                 uint32_t tile_rows,
                 uint32_t tile_cols,
                 void* dst,
                 void* flags,
                 bool slice_flags,
                 hipStream_t stream)
{
    if (W == 0 || H == 0 || tile_rows == 0 || tile_cols == 0 ||
        uint64_t(tile_rows) * tile_cols >= (1ull << 31))
        return hipErrorInvalidValue;
    const uint32_t ntx = (W + tile_cols - 1) / tile_cols;
    const uint32_t nty = (H + tile_rows - 1) / tile_rows;
    const uint32_t slices = tile_slices(tile_rows, tile_cols);
    const uint64_t blocks = uint64_t(ntx) * nty * slices;
    if (blocks >= (1ull << 31))
        return hipErrorInvalidValue;
    if (!slice_flags) {
        hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t) * ntx * nty, stream);
        if (e != hipSuccess)
            return e;
    }
    const size_t bpp = dtype_bytes(dtype);
    if ((uint64_t(W) * bpp) % 16 == 0 && (uint64_t(tile_cols) * bpp) % 16 == 0 &&
        reinterpret_cast<uintptr_t>(src) % 16 == 0 &&
        reinterpret_cast<uintptr_t>(dst) % 16 == 0) {
        const uint32_t rv = uint32_t(uint64_t(W) * bpp / 16);
        const uint32_t tv = uint32_t(uint64_t(tile_cols) * bpp / 16);
        const auto* s16 = static_cast<const u32x4*>(src);
        auto* d16 = static_cast<u32x4*>(dst);
        if (slice_flags)
            hipLaunchKernelGGL((tile_kernel_vec<true>), dim3(uint32_t(blocks)), dim3(256), 0,
                               stream, s16, rv, H, tile_rows, tv, ntx, slices, d16, flags);
        else
            hipLaunchKernelGGL((tile_kernel_vec<false>), dim3(uint32_t(blocks)), dim3(256), 0,
                               stream, s16, rv, H, tile_rows, tv, ntx, slices, d16, flags);
        return hipGetLastError();
    }
    return with_dtype(dtype, [&](auto tag) -> hipError_t {
        using T = decltype(tag);
        if (slice_flags)
            hipLaunchKernelGGL((tile_kernel<T, true>), dim3(uint32_t(blocks)), dim3(256),
                               0, stream, static_cast<const T*>(src), W, H, tile_rows,
                               tile_cols, ntx, slices, static_cast<T*>(dst), flags);
        else
            hipLaunchKernelGGL((tile_kernel<T, false>), dim3(uint32_t(blocks)), dim3(256),
                               0, stream, static_cast<const T*>(src), W, H, tile_rows,
                               tile_cols, ntx, slices, static_cast<T*>(dst), flags);
        return hipGetLastError();
    });
}

} // namespace

hipError_t
AQZ_SHARDED(launch_tile_frame)(int dtype,
                  const void* src,
                  uint32_t W,
                  uint32_t H,
                  uint32_t tile_rows,
                  uint32_t tile_cols,
                  void* dst,
                  uint32_t* nonzero,
                  hipStream_t stream)
{
    return launch_tile_impl(dtype, src, W, H, tile_rows, tile_cols, dst, nonzero,
                            false, stream);
}

hipError_t
AQZ_SHARDED(launch_tile_frame_sliced)(int dtype,
                         const void* src,
                         uint32_t W,
                         uint32_t H,
                         uint32_t tile_rows,
                         uint32_t tile_cols,
                         void* dst,
                         uint8_t* slice_flags,
                         hipStream_t stream)
{
    return launch_tile_impl(dtype, src, W, H, tile_rows, tile_cols, dst, slice_flags,
                            true, stream);
}

hipError_t
AQZ_SHARDED(launch_transpose)(int dtype,
                 const void* src,
                 uint32_t rows,
                 uint32_t cols,
                 void* dst,
                 hipStream_t stream)
{
    if (rows == 0 || cols == 0)
        return hipErrorInvalidValue;
    return with_dtype(dtype, [&](auto tag) -> hipError_t {
        using T = decltype(tag);
        constexpr uint32_t TD = kTransposeTile<T>;
        constexpr uint32_t TR = TD * kTransposeSub<T>; // source rows per block
        const uint32_t bx = (cols + TD - 1) / TD;
        const uint32_t by = (rows + TR - 1) / TR;
        if (by > 65535)
            return hipErrorInvalidValue;
        // 16-B vectors need 16-B aligned bases and row pitches on both sides
        const bool vec = (reinterpret_cast<uintptr_t>(src) % 16) == 0 &&
                         (reinterpret_cast<uintptr_t>(dst) % 16) == 0 &&
                         (uint64_t(cols) * sizeof(T)) % 16 == 0 &&
                         (uint64_t(rows) * sizeof(T)) % 16 == 0;
        if (vec)
            hipLaunchKernelGGL((transpose_kernel<T, true>), dim3(bx, by), dim3(256), 0,
                               stream, static_cast<const T*>(src), rows, cols,
                               static_cast<T*>(dst));
        else
            hipLaunchKernelGGL((transpose_kernel<T, false>), dim3(bx, by), dim3(256), 0,
                               stream, static_cast<const T*>(src), rows, cols,
                               static_cast<T*>(dst));
        return hipGetLastError();
    });
}

hipError_t
AQZ_SHARDED(launch_xy_generic)(int dtype,
                  int method,
                  const void* src,
                  uint64_t src_frame_elems,
                  uint32_t w,
                  uint32_t h,
                  const LevelOut& out,
                  uint32_t n_frames,
                  hipStream_t stream)
{
    if (w == 0 || h == 0 || n_frames == 0)
        return hipErrorInvalidValue;
    if (out.w != (w + 1) / 2 || out.h != (h + 1) / 2)
        return hipErrorInvalidValue;
    const uint64_t total = uint64_t(out.w) * out.h * n_frames;
    const uint32_t grid = grid_for(total, 256, 8192);
    return with_dtype(dtype, [&](auto tag) -> hipError_t {
        using T = decltype(tag);
        return with_method(method, [&](auto mtag) -> hipError_t {
            constexpr int M = decltype(mtag)::value;
            if (launch_log_on())
                launch_log_record("family=generic dtype=%d method=%d n_out=1 grid=%u block=256",
                                  int(sizeof(T)), M, grid);
            hipLaunchKernelGGL((xy_generic_kernel<T, M>),
                               dim3(grid), dim3(256), 0, stream,
                               static_cast<const T*>(src), src_frame_elems, w,
                               h, static_cast<T*>(out.ptr), out.frame_elems,
                               out.w, out.h, total);
            return hipGetLastError();
        });
    });
}

hipError_t
AQZ_SHARDED(launch_zpair)(int dtype,
             int method,
             void* out,
             const void* earlier,
             const void* current,
             uint64_t n,
             hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    const size_t b = dtype_bytes(dtype);
    if (!b)
        return hipErrorInvalidValue;
    // batch slots of odd-sized levels need not be 16-byte aligned
    const bool vec = ((reinterpret_cast<uintptr_t>(out) |
                       reinterpret_cast<uintptr_t>(earlier) |
                       reinterpret_cast<uintptr_t>(current)) %
                      16) == 0;
    const uint64_t items = vec ? (n * b + 15) / 16 : n;
    const uint32_t grid = grid_for(items, 256, 8192);
    return with_dtype(dtype, [&](auto tag) -> hipError_t {
        using T = decltype(tag);
        return with_method(method, [&](auto mtag) -> hipError_t {
            constexpr int M = decltype(mtag)::value;
            if (launch_log_on())
                launch_log_record(
                  "family=zpair dtype=%d method=%d n_out=1 grid=%u block=256 vec=%d",
                  int(sizeof(T)), M, grid, int(vec));
            if (vec)
                hipLaunchKernelGGL((zpair_kernel<T, M, true>), dim3(grid),
                                   dim3(256), 0, stream, static_cast<T*>(out),
                                   static_cast<const T*>(earlier),
                                   static_cast<const T*>(current), n);
            else
                hipLaunchKernelGGL((zpair_kernel<T, M, false>), dim3(grid),
                                   dim3(256), 0, stream, static_cast<T*>(out),
                                   static_cast<const T*>(earlier),
                                   static_cast<const T*>(current), n);
            return hipGetLastError();
        });
    });
}

hipError_t
AQZ_SHARDED(launch_zrun)(int dtype,
            int method,
            const void* src,
            uint64_t src_frame_elems,
            uint64_t elems,
            const LevelOut* outs,
            int n_out,
            uint32_t planes,
            hipStream_t stream)
{
    const ZRunPlan pl = plan_zrun(dtype, method, src, src_frame_elems, elems, outs, n_out, planes);
    if (!pl.valid)
        return hipErrorInvalidValue;
    ZRunParams p{};
    p.src = static_cast<const uint8_t*>(src);
    p.src_frame_elems = src_frame_elems;
    p.elems = elems;
    p.spans = pl.spans;
    p.total_units = pl.groups * pl.spans;
    for (int i = 0; i < n_out; ++i) {
        p.dst[i] = static_cast<uint8_t*>(outs[i].ptr);
        p.dst_frame_elems[i] = outs[i].frame_elems;
    }
    const dim3 grid(pl.grid), block(pl.block);
    return with_dtype(dtype, [&](auto tag) -> hipError_t {
        using T = decltype(tag);
        return with_method(method, [&](auto mtag) -> hipError_t {
            constexpr int M = decltype(mtag)::value;
            if (launch_log_on())
                launch_log_record("%s", format_plan(pl).c_str());
            auto go = [&](auto nltag) -> hipError_t {
                hipLaunchKernelGGL((zrun_kernel<T, M, decltype(nltag)::value>), grid, block, 0,
                                   stream, p);
                return hipGetLastError();
            };
            if (n_out == 1)
                return go(int_tag<1>{});
            if (n_out == 2)
                return go(int_tag<2>{});
            return go(int_tag<3>{});
        });
    });
}

hipError_t
AQZ_SHARDED(launch_zrun_tiled)(int dtype,
                  int method,
                  const void* src,
                  uint64_t src_frame_elems,
                  uint32_t W,
                  uint32_t H,
                  const LevelOut* outs,
                  const TiledOut* touts,
                  int n_out,
                  uint32_t planes,
                  hipStream_t stream)
{
    const ZRunTiledPlan pl =
      plan_zrun_tiled(dtype, method, src, src_frame_elems, W, H, outs, touts, n_out, planes);
    if (!pl.valid)
        return hipErrorInvalidValue;
    ZRunTiledParams p{};
    p.src = static_cast<const uint8_t*>(src);
    p.src_frame_elems = src_frame_elems;
    p.elems = pl.elems;
    p.spans = pl.spans;
    p.total_units = pl.groups * pl.spans;
    p.W = W;
    p.dw = FastDiv::make(W);
    for (int i = 0; i < n_out; ++i) {
        p.dst[i] = static_cast<uint8_t*>(outs[i].ptr);
        p.dst_frame_elems[i] = outs[i].frame_elems;
        fill_tiled_level(p.tl[i], pl.lv[i], touts[i]);
        if (pl.lv[i].clear_flags) {
            // level i + 1 emits planes >> (i + 1) planes
            const hipError_t e = hipMemsetAsync(
              touts[i].nonzero, 0, size_t(planes >> (i + 1)) * pl.lv[i].flags_frame, stream);
            if (e != hipSuccess)
                return e;
        }
    }
    p.zitems = pl.zitems;
    p.zdiv = FastDiv::make(pl.zitems ? pl.zitems : 1);
    p.zwaves = pl.zwaves;
    const dim3 grid(pl.grid), block(pl.block);
    return with_dtype(dtype, [&](auto tag) -> hipError_t {
        using T = decltype(tag);
        return with_method(method, [&](auto mtag) -> hipError_t {
            constexpr int M = decltype(mtag)::value;
            if (launch_log_on())
                launch_log_record("%s", format_plan(pl).c_str());
            auto go = [&](auto nltag) -> hipError_t {
                hipLaunchKernelGGL((zrun_tiled_kernel<T, M, decltype(nltag)::value>), grid, block,
                                   0, stream, p);
                return hipGetLastError();
            };
            if (n_out == 1)
                return go(int_tag<1>{});
            if (n_out == 2)
                return go(int_tag<2>{});
            return go(int_tag<3>{});
        });
    });
}

} // namespace aqz
