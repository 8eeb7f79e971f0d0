// shard_layout_sweep.cpp — csrc/shard_layout.cpp (host only, no HIP) on random
// N-D dimension sets with ragged shards, against the per-chunk statement of
// ArrayDimensions::shard_index_for_chunk_ / shard_internal_index_
// (array.dimensions.cpp:461-548: strides, modulo and divide per chunk index),
// built with the host sanitizers:
//   make -C acquire-zarr_amd shardsweep && tests/cpp/bin/shard_layout_sweep
// Output arrays are exactly chunks_per_layer long, so a write past the end is
// an AddressSanitizer report.
#include "aqz_shard.h"

#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

namespace {

int failures = 0;

#define CHECK_THAT(cond)                                                                           \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);                        \
            ++failures;                                                                            \
        }                                                                                          \
    } while (0)

uint64_t
ceil_div(uint64_t a, uint64_t b)
{
    return (a + b - 1) / b;
}

void
one_case(std::mt19937_64& rng)
{
    auto pick = [&](uint32_t lo, uint32_t hi) {
        return uint32_t(lo + rng() % (hi - lo + 1));
    };
    const uint32_t nd = pick(3, 6);
    std::vector<aqz_dimension> dims(nd);
    for (uint32_t i = 0; i < nd; ++i) {
        const uint32_t chunk = pick(1, 8), n_chunks = pick(1, 5);
        uint32_t size = n_chunks * chunk - pick(0, chunk - 1);
        if (i == 0 && (rng() & 1))
            size = 0; // the unbounded append dimension
        dims[i] = aqz_dimension{ int32_t(pick(0, 3)), size ? size : (i ? 1u : 0u), chunk,
                                 pick(1, 4), 1.0 };
    }
    const uint32_t layer = pick(0, dims[0].shard_size_chunks - 1);
    aqz_zarr_shard_geometry geo{};
    CHECK_THAT(aqz_zarr_shard_layout(dims.data(), nd, layer, &geo, nullptr, nullptr) == AQZ_OK);
    std::vector<uint32_t> shard_of(geo.chunks_per_layer), internal_of(geo.chunks_per_layer);
    CHECK_THAT(aqz_zarr_shard_layout(dims.data(), nd, layer, &geo, shard_of.data(),
                                     internal_of.data()) == AQZ_OK);

    std::vector<uint64_t> chunk_stride(nd, 1), shard_stride(nd, 1), internal_stride(nd, 1);
    uint64_t per_shard = dims[0].shard_size_chunks, n_shards = 1;
    for (uint32_t i = nd - 1; i > 0; --i) {
        const uint64_t n = ceil_div(dims[i].array_size_px, dims[i].chunk_size_px);
        chunk_stride[i - 1] = chunk_stride[i] * n;
        shard_stride[i - 1] = shard_stride[i] * ceil_div(n, dims[i].shard_size_chunks);
        internal_stride[i - 1] = internal_stride[i] * dims[i].shard_size_chunks;
        per_shard *= dims[i].shard_size_chunks;
        n_shards *= ceil_div(n, dims[i].shard_size_chunks);
    }
    CHECK_THAT(geo.chunks_per_layer == chunk_stride[0]);
    CHECK_THAT(geo.chunks_per_shard == per_shard);
    CHECK_THAT(geo.n_shards == n_shards);
    CHECK_THAT(geo.layers_per_shard == dims[0].shard_size_chunks);
    const uint64_t spl = per_shard / geo.layers_per_shard;
    std::vector<std::set<uint32_t>> seen(geo.n_shards);
    for (uint64_t c = 0; c < geo.chunks_per_layer; ++c) {
        const uint64_t index = uint64_t(layer) * geo.chunks_per_layer + c;
        uint64_t shard = 0, internal = (index / chunk_stride[0]) % dims[0].shard_size_chunks *
                                       internal_stride[0];
        for (uint32_t i = nd - 1; i > 0; --i) {
            const uint64_t at = index % chunk_stride[i - 1] / chunk_stride[i];
            shard += at / dims[i].shard_size_chunks * shard_stride[i];
            internal += at % dims[i].shard_size_chunks * internal_stride[i];
        }
        CHECK_THAT(shard_of[c] == shard);
        CHECK_THAT(internal_of[c] == internal);
        CHECK_THAT(internal >= layer * spl && internal < (layer + 1) * spl);
        // each internal index once, ascending with the chunk index
        auto& s = seen[shard_of[c]];
        CHECK_THAT(s.empty() || *s.rbegin() < internal_of[c]);
        s.insert(internal_of[c]);
    }
}

} // namespace

int
main()
{
    std::mt19937_64 rng(20);
    for (int i = 0; i < 20000; ++i)
        one_case(rng);
    // refusals
    aqz_dimension d[3] = { { 2, 0, 4, 2, 1.0 }, { 0, 64, 16, 2, 1.0 }, { 0, 64, 16, 2, 1.0 } };
    aqz_zarr_shard_geometry geo{};
    CHECK_THAT(aqz_zarr_shard_layout(d, 3, 2, &geo, nullptr, nullptr) == AQZ_INVALID_ARGUMENT);
    CHECK_THAT(aqz_zarr_shard_layout(d, 2, 0, &geo, nullptr, nullptr) == AQZ_INVALID_ARGUMENT);
    CHECK_THAT(aqz_zarr_shard_layout(nullptr, 3, 0, &geo, nullptr, nullptr) ==
               AQZ_INVALID_ARGUMENT);
    d[1] = { 0, 1u << 16, 1, 1, 1.0 };
    d[2] = { 0, 1u << 16, 1, 1, 1.0 };
    CHECK_THAT(aqz_zarr_shard_layout(d, 3, 0, &geo, nullptr, nullptr) == AQZ_OVERFLOW);
    d[1] = { 0, 0xFFFFFFFFu, 1, 0xFFFFFFFFu, 1.0 };
    d[2] = { 0, 0xFFFFFFFFu, 1, 0xFFFFFFFFu, 1.0 };
    CHECK_THAT(aqz_zarr_shard_layout(d, 3, 0, &geo, nullptr, nullptr) == AQZ_OVERFLOW);
    if (failures) {
        std::fprintf(stderr, "shard_layout_sweep: %d failures\n", failures);
        return 1;
    }
    std::printf("shard_layout_sweep ok: 20000 dimension sets\n");
    return 0;
}
