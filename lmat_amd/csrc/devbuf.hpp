// devbuf.hpp -- DevBuf: a device buffer that grows on demand and frees itself; ensure_all for several at once.
// Needs the HIP runtime API only, so host translation units (lmat_api.cpp, collective.cpp) include it as well as the HIP ones.
#pragma once
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstddef>
#include <initializer_list>
#include <type_traits>
#include <utility>

namespace lmat_dev {

// Grow only, contents not kept: a buffer that is too small is freed (hipFree waits for the device, so a kernel of an earlier
// launch that still reads the old block is through by then) and allocated anew.  After a failed ensure the buffer is empty.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~DevBuf() { if (p) hipFree(p); }
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        if (p) { hipFree(p); p = nullptr; bytes = 0; }
        hipError_t e = hipMalloc(&p, std::max<size_t>(n, 256));
        if (e == hipSuccess) bytes = std::max<size_t>(n, 256);
        else p = nullptr;
        return e;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a copy would free the block twice");

inline hipError_t ensure_all(std::initializer_list<std::pair<DevBuf*, size_t>> need) {   // (buffer, bytes) ...
    for (const auto& n : need)
        if (const hipError_t e = n.first->ensure(n.second)) return e;
    return hipSuccess;
}

}  // namespace lmat_dev
