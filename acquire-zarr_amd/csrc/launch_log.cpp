// launch_log.cpp — the launchers' decision log (launch_log.hh).
#include "launch_log.hh"

#include "abi_guard.hh"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace aqz {

namespace {

constexpr size_t kLines = 512;
constexpr size_t kLineLen = 320;

struct Ring
{
    std::mutex mu;
    size_t head = 0;  // oldest line
    size_t count = 0; // lines held
    char line[kLines][kLineLen];
};

Ring&
ring()
{
    static Ring r;
    return r;
}

} // namespace

bool
launch_log_on()
{
    static const bool on = [] {
        const char* e = std::getenv("AQZ_LAUNCH_LOG");
        return e && std::strcmp(e, "1") == 0;
    }();
    return on;
}

void
launch_log_record(const char* fmt, ...)
{
    char tmp[kLineLen];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(tmp, sizeof(tmp), fmt, ap);
    va_end(ap);
    Ring& r = ring();
    std::lock_guard<std::mutex> lock(r.mu);
    size_t slot;
    if (r.count == kLines) {
        slot = r.head;
        r.head = (r.head + 1) % kLines;
    } else {
        slot = (r.head + r.count) % kLines;
        ++r.count;
    }
    std::memcpy(r.line[slot], tmp, kLineLen);
}

int
launch_log_drain(char* buf, size_t cap)
{
    if (!buf || cap == 0)
        return AQZ_INVALID_ARGUMENT;
    Ring& r = ring();
    std::lock_guard<std::mutex> lock(r.mu);
    size_t need = 1;
    for (size_t i = 0; i < r.count; ++i)
        need += std::strlen(r.line[(r.head + i) % kLines]) + 1;
    if (need > cap)
        return AQZ_OVERFLOW;
    size_t off = 0;
    for (size_t i = 0; i < r.count; ++i) {
        const char* s = r.line[(r.head + i) % kLines];
        const size_t n = std::strlen(s);
        std::memcpy(buf + off, s, n);
        off += n;
        buf[off++] = '\n';
    }
    buf[off] = '\0';
    r.head = r.count = 0;
    return AQZ_OK;
}

} // namespace aqz

extern "C" int
aqz_debug_launch_log(char* buf, size_t cap)
{
    try {
        return aqz::launch_log_drain(buf, cap);
    } catch (...) {
        return ABI_GUARD_FAIL(nullptr);
    }
}
