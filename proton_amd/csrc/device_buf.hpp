// device_buf.hpp -- the one owner of device memory the host side keeps beyond a call: the context's tables and buffers.
// (The temporaries of one host function are DeviceTmp's, device_tmp.hpp.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace pa {

// count elements of T on the device.  Move-only; frees in the destructor.  A group of these is released by assigning a fresh group.
template <class T>
class DeviceBuf {
public:
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    DeviceBuf(DeviceBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DeviceBuf() { reset(); }

    T *get() const { return p_; }
    size_t size() const { return n_; }            // elements asked for (0: empty, or one spare element behind a zero count)
    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; n_ = 0;
    }
    // room for count (at least one) T, in place of what was held
    hipError_t alloc(size_t count)
    {
        reset();
        const hipError_t e = hipMalloc((void **)&p_, (count ? count : 1) * sizeof(T));
        if (e != hipSuccess) { p_ = nullptr; return e; }
        n_ = count;
        return hipSuccess;
    }
    // alloc(v.size()) and the copy enqueued on `stream`: v must live until the stream has drained
    hipError_t upload(const std::vector<T> &v, hipStream_t stream)
    {
        const hipError_t e = alloc(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpyAsync(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream);
    }
    // at least count elements, contents not kept.  Work on `stream` may still be using the old buffer: the stream drains before
    // it is freed.
    hipError_t grow(size_t count, hipStream_t stream)
    {
        if (p_ && n_ >= count) return hipSuccess;
        if (p_) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
        }
        return alloc(count);
    }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace pa
