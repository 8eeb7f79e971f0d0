// hip_raii_check.cpp — csrc/hip_raii.hh under the host sanitizers, on a
// machine WITHOUT a GPU, where every HIP allocation and creation fails: the
// failure paths are the ones no GPU test reaches.
//   * a failed reserve leaves the buffer empty (null, capacity 0);
//   * a second reserve after a failure tries again (it fails again, it does
//     not report a stale capacity);
//   * moving and destroying empty and moved-from owners is clean.
// With a GPU present the allocations succeed; the program then checks the
// success side of the same rules (grow, no-op, move) and frees everything.
//
// Build and run: make raiicheck && tests/cpp/bin/hip_raii_check
#include "hip_raii.hh"

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__,        \
                         __LINE__, #cond);                                     \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

namespace {

template<class B>
void
check_buf(const char* name)
{
    B b;
    CHECK(!b && b.get() == nullptr && b.capacity() == 0);
    CHECK(b.reserve(0) == hipSuccess); // nothing to do, nothing allocated
    CHECK(!b && b.capacity() == 0);

    const hipError_t first = b.reserve(4096);
    if (first != hipSuccess) {
        CHECK(!b && b.get() == nullptr && b.capacity() == 0);
        // not "already large enough": the allocation is attempted again
        CHECK(b.reserve(4096) != hipSuccess);
        CHECK(b.reserve(1) != hipSuccess);
        CHECK(!b && b.capacity() == 0);
    } else {
        void* p = b.get();
        CHECK(p && b.capacity() == 4096);
        CHECK(b.reserve(100) == hipSuccess && b.get() == p && b.capacity() == 4096);
        CHECK(b.reserve(8192) == hipSuccess && b.capacity() == 8192);
    }
    const size_t cap = b.capacity();

    B moved(std::move(b));
    CHECK(!b && b.capacity() == 0); // moved-from: empty
    CHECK(moved.capacity() == cap);
    b = std::move(moved);           // assign into a moved-from owner
    CHECK(!moved && moved.capacity() == 0 && b.capacity() == cap);
    B& self = b;
    b = std::move(self);            // self-assignment keeps the buffer
    CHECK(b.capacity() == cap);
    moved.reset();                  // reset of an empty owner
    (void)moved.reserve(64);        // a moved-from owner is usable again

    std::vector<B> v(3);            // what a handle's level table does
    (void)v[1].reserve(256);
    v.resize(8);
    v.clear();
    std::printf("%s: %s\n", name,
                first == hipSuccess ? "allocations succeeded" : "allocations failed");
}

template<class H>
void
check_handle(const char* name)
{
    H h;
    CHECK(!h && h.get() == nullptr);
    const hipError_t first = h.create();
    if (first != hipSuccess) {
        CHECK(!h);
        CHECK(h.create() != hipSuccess); // tried again
        CHECK(!h);
    } else {
        auto raw = h.get();
        CHECK(raw && h.create() == hipSuccess && h.get() == raw); // created once
    }
    auto raw = h.get();
    H moved(std::move(h));
    CHECK(!h && moved.get() == raw);
    h = std::move(moved);
    CHECK(!moved && h.get() == raw);
    H& self = h;
    h = std::move(self);
    CHECK(h.get() == raw);
    moved.reset();
    std::printf("%s: %s\n", name, first == hipSuccess ? "creation succeeded" : "creation failed");
}

} // namespace

int
main()
{
    check_buf<aqz::DeviceBuf>("DeviceBuf");
    check_buf<aqz::PinnedBuf>("PinnedBuf");
    check_handle<aqz::Event>("Event");
    check_handle<aqz::Stream>("Stream");
    std::printf("hip_raii_check ok\n");
    return 0;
}
