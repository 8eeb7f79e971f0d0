// hip_raii.hh — move-only owners of the HIP resources a handle holds:
// DeviceBuf, PinnedBuf (a pointer with its capacity), Event, Stream.  Each
// destructor frees what it owns and waits for nothing: whoever destroys an
// owner has already synchronised the work that uses it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>

namespace aqz {
namespace raii {

inline hipError_t
pinned_alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
inline hipError_t
event_create(hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }
inline hipError_t
stream_create(hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }

// A grow-only scratch buffer: the pointer and its capacity move together, so
// "the capacity says it fits" always means "the memory is there".
template<hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
class Buf
{
  public:
    Buf() = default;
    Buf(Buf&& o) noexcept { swap(o); }
    Buf& operator=(Buf&& o) noexcept
    {
        Buf(std::move(o)).swap(*this); // the old memory goes with the temporary
        return *this;
    }
    ~Buf() { reset(); }

    // Nothing when `bytes` already fit; else free, then allocate.  A failed
    // allocation leaves the buffer empty.  Never synchronises: the caller
    // waits first for whatever may still use the old memory.
    hipError_t reserve(size_t bytes)
    {
        if (cap_ >= bytes)
            return hipSuccess;
        reset();
        const hipError_t e = Alloc(&p_, bytes);
        if (e != hipSuccess)
            p_ = nullptr;
        else
            cap_ = bytes;
        return e;
    }
    void reset()
    {
        if (p_)
            (void)Free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    void* get() const { return p_; }
    uint8_t* bytes() const { return static_cast<uint8_t*>(p_); }
    size_t capacity() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }

  private:
    void swap(Buf& o)
    {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
    }
    void* p_ = nullptr;
    size_t cap_ = 0;
};

// An event or a stream, created on demand.
template<class T, hipError_t (*Create)(T*), hipError_t (*Destroy)(T)>
class Handle
{
  public:
    Handle() = default;
    Handle(Handle&& o) noexcept { std::swap(h_, o.h_); }
    Handle& operator=(Handle&& o) noexcept
    {
        Handle t(std::move(o));
        std::swap(h_, t.h_);
        return *this;
    }
    ~Handle() { reset(); }

    hipError_t create() { return h_ ? hipSuccess : Create(&h_); } // once
    void reset()
    {
        if (h_)
            (void)Destroy(h_);
        h_ = nullptr;
    }
    T get() const { return h_; }
    operator T() const { return h_; }

  private:
    T h_ = nullptr;
};

} // namespace raii

using DeviceBuf = raii::Buf<hipMalloc, hipFree>;
using PinnedBuf = raii::Buf<raii::pinned_alloc, hipHostFree>;
using Event = raii::Handle<hipEvent_t, raii::event_create, hipEventDestroy>;     // no timing
using Stream = raii::Handle<hipStream_t, raii::stream_create, hipStreamDestroy>; // non-blocking

} // namespace aqz
