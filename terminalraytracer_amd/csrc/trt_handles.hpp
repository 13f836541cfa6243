// trt_handles.hpp -- INTERNAL to libtrt_hip.so: owners of the HIP resources the host code holds.  Each frees its resource when
// it is destroyed, so no teardown lists them and no early return leaks one.  Host-only: trt_dist.hip includes it without the
// kernels of trt_context.hpp.  No owner may be static or global: its destructor would run at exit, after the HIP runtime's.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

namespace trt_impl
{

template <typename T>
struct DeviceBuffer
{
    T *ptr = nullptr;
    size_t capacity = 0; // elements

    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)), capacity(std::exchange(o.capacity, 0)) {}
    DeviceBuffer &operator=(DeviceBuffer o) noexcept // moves only; the old allocation goes with `o`
    {
        std::swap(ptr, o.ptr);
        std::swap(capacity, o.capacity);
        return *this;
    }
    ~DeviceBuffer()
    {
        if (ptr)
            (void)hipFree(ptr);
    }
    // room for at least n elements, and a ptr that is not null; growing does not keep the contents
    hipError_t reserve(size_t n)
    {
        if (n <= capacity && ptr)
            return hipSuccess;
        *this = DeviceBuffer();
        hipError_t e = hipMalloc((void **)&ptr, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess)
            capacity = std::max<size_t>(n, 1);
        return e;
    }
};

// pinned host memory: the staging area of copies from the device
struct PinnedBuffer
{
    void *ptr = nullptr;
    size_t bytes = 0;

    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer &) = delete;
    PinnedBuffer &operator=(const PinnedBuffer &) = delete;
    ~PinnedBuffer()
    {
        if (ptr)
            (void)hipHostFree(ptr);
    }
    // room for at least n bytes; growing does not keep the contents
    hipError_t reserve(size_t n)
    {
        if (n <= bytes)
            return hipSuccess;
        if (ptr)
            (void)hipHostFree(ptr);
        ptr = nullptr;
        bytes = 0;
        hipError_t e = hipHostMalloc(&ptr, n, hipHostMallocDefault);
        if (e == hipSuccess)
            bytes = n;
        return e;
    }
};

// Event and Stream own one handle each and read as it wherever HIP takes one.  create() is for an owner that holds none.
class Event
{
  public:
    Event() = default;
    Event(const Event &) = delete;
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    ~Event()
    {
        if (e_)
            (void)hipEventDestroy(e_);
    }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e_, flags); }
    operator hipEvent_t() const { return e_; }

  private:
    hipEvent_t e_ = nullptr;
};

class Stream
{
  public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream &operator=(Stream o) noexcept // moves only; the old stream goes with `o`
    {
        std::swap(s_, o.s_);
        return *this;
    }
    ~Stream()
    {
        if (s_)
            (void)hipStreamDestroy(s_);
    }
    hipError_t create() { return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
    // kernels on this stream run only on the compute units whose bits are set in mask[0 .. words - 1]
    hipError_t create(uint32_t words, const uint32_t *mask) { return hipExtStreamCreateWithCUMask(&s_, words, mask); }
    operator hipStream_t() const { return s_; }

  private:
    hipStream_t s_ = nullptr;
};

} // namespace trt_impl
