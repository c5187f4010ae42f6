// device_tmp.hpp -- what the host side of every symbolic phase repeats: the grid of a one-thread-per-item launch, device temporaries
// that go away on every path out of the function, and rocPRIM's two-phase exclusive scan with its total read back.
#pragma once

#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <cstddef>
#include <vector>

namespace pa {

inline unsigned blocks_for(size_t n) { return (unsigned)(n ? (n + 255) / 256 : 1); }

// The device temporaries of one host function.  ok() notes the first error; the destructor frees what alloc() handed out, after
// the stream has drained if an error is pending (kernels of the failed sequence may still be reading the temporaries).
class DeviceTmp {
public:
    explicit DeviceTmp(hipStream_t stream) : stream_(stream) {}
    DeviceTmp(const DeviceTmp &) = delete;
    DeviceTmp &operator=(const DeviceTmp &) = delete;
    ~DeviceTmp()
    {
        if (error_ != hipSuccess) (void)hipStreamSynchronize(stream_);
        for (void *p : held_) (void)hipFree(p);
    }
    bool ok(hipError_t e)
    {
        if (e != hipSuccess && error_ == hipSuccess) error_ = e;
        return e == hipSuccess;
    }
    hipError_t error() const { return error_; }
    // *p = room for count (at least one) T
    template <class T> bool alloc(T **p, size_t count)
    {
        void *q = nullptr;
        if (!ok(hipMalloc(&q, (count ? count : 1) * sizeof(T)))) return false;
        held_.push_back(q);
        *p = static_cast<T *>(q);
        return true;
    }

private:
    hipStream_t stream_;
    hipError_t error_ = hipSuccess;
    std::vector<void *> held_;
};

// out[i] = in[0] + ... + in[i - 1], i < n.  With in[n - 1] a sentinel (zero), out[n - 1] is the total of the n - 1 counts: if
// `total` is given it is copied there and the stream is synchronised.  The scan's work space comes from `tmp`, which notes an error.
template <class T>
hipError_t exclusive_scan_with_total(hipStream_t stream, const T *in, T *out, size_t n, DeviceTmp &tmp, T *total)
{
    size_t bytes = 0;
    char *work = nullptr;
    if (!tmp.ok(rocprim::exclusive_scan(nullptr, bytes, in, out, T(0), n, rocprim::plus<T>(), stream))) return tmp.error();
    if (!tmp.alloc(&work, bytes)) return tmp.error();
    if (!tmp.ok(rocprim::exclusive_scan(work, bytes, in, out, T(0), n, rocprim::plus<T>(), stream))) return tmp.error();
    if (total == nullptr) return hipSuccess;
    if (!tmp.ok(hipMemcpyAsync(total, out + (n - 1), sizeof(T), hipMemcpyDeviceToHost, stream))) return tmp.error();
    tmp.ok(hipStreamSynchronize(stream));
    return tmp.error();
}

}  // namespace pa
