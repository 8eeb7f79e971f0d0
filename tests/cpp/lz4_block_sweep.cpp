// lz4_block_sweep — the serial encoder of csrc/lz4_block.hh against
// LZ4_compress_fast of the liblz4 given on the command line (default
// liblz4.so.1), return value and bytes, over a seeded sweep.  Host code only;
// meant to be built with -fsanitize=address,undefined (`make lz4sweep`): every
// source and destination is an exact-size heap block, so a read past src + n
// or a write past dst + cap is reported.
//
//   lz4_block_sweep [liblz4 path] [cases per group]
#include "lz4_block.hh"

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace {

using Lz4Fn = int (*)(const char*, char*, int, int, int);

std::vector<uint8_t>
make_data(std::mt19937_64& rng, int kind, size_t n)
{
    std::vector<uint8_t> v(n);
    switch (kind) {
        case 0: // random
            for (auto& b : v)
                b = uint8_t(rng());
            break;
        case 1: // sparse
            for (auto& b : v)
                b = (rng() % 16 == 0) ? uint8_t(rng()) : 0;
            break;
        case 2: { // periodic with noise
            const size_t period = 1 + rng() % 300;
            for (size_t i = 0; i < n; ++i)
                v[i] = uint8_t((i % period) * 7 + ((rng() % 64 == 0) ? rng() : 0));
            break;
        }
        case 3: { // far repeats: a random prefix copied at random distances
            size_t i = 0;
            while (i < n) {
                const size_t len = 1 + rng() % 200;
                if (i > 8 && rng() % 2) {
                    const size_t back = 1 + rng() % (i < 200000 ? i : 200000);
                    for (size_t k = 0; k < len && i < n; ++k, ++i)
                        v[i] = v[i - back];
                } else {
                    for (size_t k = 0; k < len && i < n; ++k, ++i)
                        v[i] = uint8_t(rng());
                }
            }
            break;
        }
        default: { // runs
            size_t i = 0;
            while (i < n) {
                const size_t len = 1 + rng() % 5000;
                const uint8_t b = uint8_t(rng());
                for (size_t k = 0; k < len && i < n; ++k, ++i)
                    v[i] = b;
            }
            break;
        }
    }
    return v;
}

long g_cases = 0, g_bad = 0, g_zero = 0;

void
check(Lz4Fn lz4, const std::vector<uint8_t>& data, int cap, int accel, void* table)
{
    const int n = int(data.size());
    // exact-size blocks
    uint8_t* src = static_cast<uint8_t*>(std::malloc(n ? n : 1));
    if (n)
        std::memcpy(src, data.data(), n);
    uint8_t* mine = static_cast<uint8_t*>(std::malloc(cap ? cap : 1));
    // the library may write a few bytes past what it returns, never past cap
    std::vector<uint8_t> theirs(size_t(cap) + 1);
    uint32_t need = 0;
    const uint32_t got = aqz::lz4::encode_block(src, uint32_t(n), mine, uint32_t(cap), accel,
                                                table, &need);
    const int want = lz4(reinterpret_cast<const char*>(data.data()),
                         reinterpret_cast<char*>(theirs.data()), n, cap, accel);
    ++g_cases;
    if (want == 0)
        ++g_zero;
    const bool ok = int(got) == want && (want == 0 || std::memcmp(mine, theirs.data(), want) == 0) &&
                    ((need <= uint32_t(cap)) == (want != 0));
    if (!ok) {
        if (++g_bad <= 10)
            std::fprintf(stderr, "MISMATCH n=%d cap=%d accel=%d got=%u want=%d need=%u\n", n, cap,
                         accel, got, want, need);
    }
    std::free(src);
    std::free(mine);
}

} // namespace

int
main(int argc, char** argv)
{
    const char* path = argc > 1 ? argv[1] : "liblz4.so.1";
    const int per = argc > 2 ? std::atoi(argv[2]) : 40;
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) {
        std::fprintf(stderr, "cannot load %s\n", path);
        return 2;
    }
    auto lz4 = reinterpret_cast<Lz4Fn>(dlsym(h, "LZ4_compress_fast"));
    if (!lz4)
        return 2;
    std::vector<uint32_t> table(aqz::lz4::kTableBytes / 4);
    std::mt19937_64 rng(20240607);
    std::vector<size_t> sizes;
    for (size_t n = 0; n <= 64; ++n)
        sizes.push_back(n);
    for (size_t n : { 65535u, 65545u, 65546u, 65547u, 65548u, 70000u, 131072u, 200001u })
        sizes.push_back(n);
    for (int k = 0; k < per; ++k)
        sizes.push_back(65 + rng() % 40000);
    sizes.push_back(1u << 20);
    for (size_t n : sizes) {
        for (int kind = 0; kind < 5; ++kind) {
            const auto data = make_data(rng, kind, n);
            const int accel = 1 + int(rng() % 10);
            // the capacity this input needs, then capacities around it
            uint32_t need = 0;
            std::vector<uint8_t> big(n + n / 200 + 64);
            aqz::lz4::encode_block(data.data(), uint32_t(n), big.data(), uint32_t(big.size()),
                                   accel, table.data(), &need);
            std::vector<int> caps = { int(n + n / 255 + 16), int(n), int(need), int(need) - 1,
                                      int(need) + 1, int(n / 2), int(n) - 1, 0, 1 };
            if (n > 20)
                caps.push_back(int(rng() % n));
            for (int cap : caps)
                if (cap >= 0)
                    check(lz4, data, cap, accel, table.data());
        }
    }
    std::printf("%ld cases, %ld library zeros, %ld mismatches\n", g_cases, g_zero, g_bad);
    return g_bad ? 1 : 0;
}
