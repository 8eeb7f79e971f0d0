// gather_kernels.hip — chunk buffers back into row-major frames on gfx950
// (include/aqz_shard.h): the inverse of the tiling, organised
// around the destination.  A workgroup owns one frame and a band of its rows;
// consecutive lanes own consecutive aligned 16-byte vectors of the frame.  The
// kernels move bytes: they take the element size, not a type.
#include "gather_kernels.hh"

#include "launch_log.hh"

namespace aqz {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1))); // any byte alignment (gfx950 global loads)

constexpr uint32_t kBlock = 256;
constexpr uint32_t kAbsent = 0xFFFFFFFFu; // AQZ_CHUNK_SLOT_ABSENT

struct GatherPlaces
{
    uint64_t internal[kGatherFrames];
    uint32_t base[kGatherFrames];
};

// Where pixel (y, x) of a frame lies in the chunk buffers, or null when its
// chunk's slot is absent or not a slot (the latter raises the flag).
__device__ __forceinline__ const uint8_t*
pixel_src(const GatherArgs& a, uint32_t base, uint64_t internal, uint32_t y, uint32_t x)
{
    const uint32_t ty = y / a.tile_rows, ry = y - ty * a.tile_rows;
    const uint32_t tx = x / a.tile_cols, cx = x - tx * a.tile_cols;
    const uint32_t c = base + ty * a.n_tiles_x + tx;
    const uint32_t s = a.slot ? a.slot[c] : c;
    if (s >= a.n_slots) {
        if (s != kAbsent && a.bad_slot)
            *a.bad_slot = 1u;
        return nullptr;
    }
    // ry * tile_cols + cx < 2^31: an element of one tile
    return a.chunks + uint64_t(s) * a.chunk_stride + internal +
           (uint64_t(ry * a.tile_cols + cx) << a.bpp_log2);
}

__device__ __forceinline__ uint64_t
load_elem(const uint8_t* p, uint32_t lg)
{
    switch (lg) {
        case 0:
            return __builtin_nontemporal_load(p);
        case 1:
            return __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p));
        case 2:
            return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
        default:
            return __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(p));
    }
}

__device__ __forceinline__ void
store_elem(uint8_t* p, uint64_t v, uint32_t lg)
{
    switch (lg) {
        case 0:
            __builtin_nontemporal_store(uint8_t(v), p);
            break;
        case 1:
            __builtin_nontemporal_store(uint16_t(v), reinterpret_cast<uint16_t*>(p));
            break;
        case 2:
            __builtin_nontemporal_store(uint32_t(v), reinterpret_cast<uint32_t*>(p));
            break;
        default:
            __builtin_nontemporal_store(v, reinterpret_cast<uint64_t*>(p));
            break;
    }
}

// pixel p (row-major) of the frame at dst, one element
__device__ __forceinline__ void
copy_pixel(const GatherArgs& a, uint32_t base, uint64_t internal, uint8_t* dst, uint64_t p)
{
    const uint32_t y = uint32_t(p / a.W), x = uint32_t(p % a.W);
    const uint8_t* s = pixel_src(a, base, internal, y, x);
    store_elem(dst + (p << a.bpp_log2), s ? load_elem(s, a.bpp_log2) : 0ull, a.bpp_log2);
}

// The element form: thread (p, k) = pixel p of the launch's frame k.  For
// geometries where no 16-byte vector fits a tile row.
__global__ __launch_bounds__(kBlock) void
gather_elem_kernel(GatherArgs a, GatherPlaces pl, uint64_t n_px)
{
    const uint32_t k = blockIdx.y;
    const uint64_t p = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= n_px)
        return;
    copy_pixel(a, pl.base[k], pl.internal[k], a.frames + uint64_t(k) * a.frame_stride, p);
}

// The 16 bytes from pixel (y, x) on in row-major order, element by element:
// a destination vector that crosses a tile edge or a row end.  It never reads
// past a tile row: a new address is worked out wherever a tile row or the
// frame row ends, and only there (the one place that divides).  Every load is
// issued before the first value is used, so a lane waits for memory once and
// not once an element.
template<uint32_t LG>
__device__ __forceinline__ u32x4
assemble_elems(const GatherArgs& a, uint32_t base, uint64_t internal, uint32_t y, uint32_t x)
{
    constexpr uint32_t EPV = 16u >> LG;
    uint64_t v[EPV];
    const uint8_t* p = nullptr;
    uint32_t left = 0; // elements up to the end of this tile row or frame row
#pragma unroll
    for (uint32_t e = 0; e < EPV; ++e) {
        if (left == 0) {
            p = pixel_src(a, base, internal, y, x);
            const uint32_t in_tile = a.tile_cols - x % a.tile_cols, in_row = a.W - x;
            left = in_tile < in_row ? in_tile : in_row;
        }
        v[e] = p ? load_elem(p, LG) : 0ull;
        p = p ? p + (1u << LG) : p;
        --left;
        if (++x == a.W) {
            x = 0;
            ++y;
        }
    }
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (uint32_t e = 0; e < EPV; ++e) {
        constexpr uint32_t kBits = 8u << LG;
        if (e * kBits < 64)
            lo |= v[e] << (e * kBits % 64);
        else
            hi |= v[e] << (e * kBits % 64);
    }
    return u32x4{ uint32_t(lo), uint32_t(lo >> 32), uint32_t(hi), uint32_t(hi >> 32) };
}

__device__ __forceinline__ u32x4
assemble_vec(const GatherArgs& a, uint32_t base, uint64_t internal, uint32_t y, uint32_t x)
{
    switch (a.bpp_log2) { // uniform over the launch
        case 0:
            return assemble_elems<0>(a, base, internal, y, x);
        case 1:
            return assemble_elems<1>(a, base, internal, y, x);
        case 2:
            return assemble_elems<2>(a, base, internal, y, x);
        default:
            return assemble_elems<3>(a, base, internal, y, x);
    }
}

// The vector form.  Workgroup (j, k): rows [j * band_rows, (j + 1) * band_rows)
// of the launch's frame k.  The frame is N = W * H * bpp bytes from dst; its
// aligned vectors start `head` bytes in (dst's distance to a 16-byte boundary)
// and the workgroup owns those that start inside its band.  A vector whose
// elements all lie in one tile row is one 16-byte load, from wherever the tile
// row puts it, and one aligned 16-byte store: U of them a lane a round, every
// load of the round issued before its first store.  Any other vector is
// assembled, in a second pass over the band.  The head goes element by element
// in band 0 and the N - head mod 16 bytes behind the last vector in the last
// band.
__global__ __launch_bounds__(kBlock) void
gather_vec_kernel(GatherArgs a, GatherPlaces pl, uint32_t band_rows)
{
    const uint32_t k = blockIdx.y, t = threadIdx.x, lg = a.bpp_log2;
    const uint32_t base = pl.base[k];
    const uint64_t internal = pl.internal[k];
    uint8_t* dst = a.frames + uint64_t(k) * a.frame_stride;
    const uint32_t row_bytes = a.W << lg; // < 2^31 (gather_form)
    const uint64_t N = uint64_t(row_bytes) * a.H;
    uint64_t head = uint64_t(-reinterpret_cast<uintptr_t>(dst)) & 15u;
    head = head < N ? head : N;
    const uint64_t nv = (N - head) >> 4;
    const uint32_t y0 = blockIdx.x * band_rows; // < H
    const uint32_t y1 = a.H - y0 > band_rows ? y0 + band_rows : a.H;
    const uint64_t B0 = uint64_t(y0) * row_bytes, B1 = uint64_t(y1) * row_bytes;
    // vector v starts at byte head + 16 v: those with B0 <= start < B1
    const uint64_t v0 = B0 > head ? (B0 - head + 15) >> 4 : 0;
    uint64_t v1 = B1 > head ? (B1 - head + 15) >> 4 : 0;
    v1 = v1 < nv ? v1 : nv;
    // a band is below 2^32 bytes (launch_chunk_gather), so 32-bit from here
    const uint32_t n = v1 > v0 ? uint32_t(v1 - v0) : 0;
    const uint32_t rb0 = n ? uint32_t(head + (v0 << 4) - B0) : 0;
    uint8_t* vdst = dst + head + (v0 << 4);
    const uint32_t epv = 16u >> lg;

    // round 1: the vectors that lie in one tile row
    constexpr uint32_t U = 8;
    for (uint32_t i0 = t; i0 < n; i0 += U * kBlock) {
        u32x4 v[U];
        bool whole[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t i = i0 + u * kBlock;
            v[u] = u32x4{ 0u, 0u, 0u, 0u };
            whole[u] = false;
            if (i < n) {
                const uint32_t rb = rb0 + (i << 4);
                const uint32_t r = rb / row_bytes, xb = rb - r * row_bytes;
                const uint32_t y = y0 + r, x = xb >> lg;
                const uint32_t cx = x % a.tile_cols;
                whole[u] = cx + epv <= a.tile_cols && x + epv <= a.W;
                if (whole[u]) {
                    const uint8_t* s = pixel_src(a, base, internal, y, x);
                    if (s)
                        v[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_u*>(s));
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t i = i0 + u * kBlock;
            if (whole[u])
                __builtin_nontemporal_store(v[u],
                                            reinterpret_cast<u32x4*>(vdst + (uint64_t(i) << 4)));
        }
    }
    // round 2: the vectors that cross a tile edge or a row end, one a lane a
    // turn, so that the lanes of round 1 never wait for an assembly.  None
    // exists where the frame's rows, its tile rows and its start are all
    // 16-byte multiples (the same for every lane of the launch's frame).
    const bool aligned = (row_bytes & 15u) == 0 && head == 0 &&
                         (a.tile_cols >= a.W || ((uint64_t(a.tile_cols) << lg) & 15u) == 0);
    if (!aligned) {
        for (uint32_t i = t; i < n; i += kBlock) {
            const uint32_t rb = rb0 + (i << 4);
            const uint32_t r = rb / row_bytes, xb = rb - r * row_bytes;
            const uint32_t y = y0 + r, x = xb >> lg;
            const uint32_t cx = x % a.tile_cols;
            if (cx + epv <= a.tile_cols && x + epv <= a.W)
                continue;
            __builtin_nontemporal_store(assemble_vec(a, base, internal, y, x),
                                        reinterpret_cast<u32x4*>(vdst + (uint64_t(i) << 4)));
        }
    }
    if (blockIdx.x == 0 && t < uint32_t(head >> lg))
        copy_pixel(a, base, internal, dst, t);
    if (blockIdx.x == gridDim.x - 1) {
        const uint64_t tail = head + (nv << 4);
        if (t < uint32_t((N - tail) >> lg))
            copy_pixel(a, base, internal, dst, (tail >> lg) + t);
    }
}

uint32_t
gather_band_rows(const GatherArgs& a)
{
    const uint32_t row_bytes = a.W << a.bpp_log2;
    const uint32_t rows = (kGatherBandBytes + row_bytes - 1) / row_bytes;
    return rows < a.H ? rows : a.H;
}

} // namespace

int
gather_form(uint32_t width, uint32_t tile_cols, uint32_t bpp_log2)
{
    return (uint64_t(tile_cols) << bpp_log2) >= 16 && (uint64_t(width) << bpp_log2) < (1ull << 31);
}

hipError_t
launch_chunk_gather(const GatherArgs& a, const uint32_t* host_base, const uint64_t* host_internal,
                    uint32_t n_frames, hipStream_t stream)
{
    if (n_frames == 0 || a.W == 0 || a.H == 0 || a.tile_rows == 0 || a.tile_cols == 0 ||
        a.bpp_log2 > 3)
        return hipErrorInvalidValue;
    const bool vec = gather_form(a.W, a.tile_cols, a.bpp_log2) != 0;
    const uint64_t n_px = uint64_t(a.W) * a.H;
    // a band's rows * row bytes stay below 2^32: at most kGatherBandBytes
    // rounded up to a row, and a row is below 2^31 bytes in this form
    const uint32_t band_rows = vec ? gather_band_rows(a) : 0;
    const uint64_t gx = vec ? (uint64_t(a.H) + band_rows - 1) / band_rows : (n_px + kBlock - 1) / kBlock;
    const uint32_t per = n_frames < kGatherFrames ? n_frames : kGatherFrames;
    if (gx * per >= (1ull << 31))
        return hipErrorInvalidValue;
    const uint32_t launches = (n_frames + kGatherFrames - 1) / kGatherFrames;
    if (launch_log_on())
        launch_log_record("family=gather form=%s frames_per_launch=%u launches=%u frames=%u "
                          "grid=%u block=%u band_rows=%u",
                          vec ? "vec" : "elem", kGatherFrames, launches, n_frames, uint32_t(gx),
                          kBlock, band_rows);
    for (uint32_t k0 = 0; k0 < n_frames; k0 += kGatherFrames) {
        const uint32_t n = n_frames - k0 < kGatherFrames ? n_frames - k0 : kGatherFrames;
        GatherPlaces pl{};
        for (uint32_t k = 0; k < n; ++k) {
            pl.base[k] = host_base[k0 + k];
            pl.internal[k] = host_internal[k0 + k];
        }
        GatherArgs b = a;
        b.frames = a.frames + uint64_t(k0) * a.frame_stride;
        if (vec)
            hipLaunchKernelGGL(gather_vec_kernel, dim3(uint32_t(gx), n), dim3(kBlock), 0, stream,
                               b, pl, band_rows);
        else
            hipLaunchKernelGGL(gather_elem_kernel, dim3(uint32_t(gx), n), dim3(kBlock), 0, stream,
                               b, pl, n_px);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace aqz
