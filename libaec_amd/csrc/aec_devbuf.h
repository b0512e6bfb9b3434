// aec_devbuf.h -- a block of device memory (or of page-locked host memory) that grows on demand.  Every buffer the host
// layers hold between calls is one of these -- the context's workspaces (aec_gpu.hip), a stream's kit (aec_abi.cpp) -- so
// the allocator is called here and nowhere else in them.  No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace aec {

// what ensure() allocates for n bytes: a quarter more and 256 bytes, rounded up to a multiple of 256
inline size_t devbuf_room(size_t n) { return (n + n / 4 + 256 + 255) & ~(size_t)255; }

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool pinned = false;      // page-locked host memory (replace() only)

    DevBuf() = default;
    explicit DevBuf(bool host) : pinned(host) {}

    // Room for n bytes, the first `keep` of them surviving: the new block is allocated and filled BEFORE the old one is
    // freed, because the contents matter (a stream's undecoded input).  On failure nothing has changed.
    bool ensure(size_t n, size_t keep = 0)
    {
        if (n <= cap) return true;
        const size_t want = devbuf_room(n);
        void *q = nullptr;
        if (!alloc(&q, want)) return false;
        if (p && keep && hipMemcpy(q, p, keep, hipMemcpyDeviceToDevice) != hipSuccess) {
            (void)hipFree(q);
            return false;
        }
        if (p) (void)hipFree(p);
        p = q;
        cap = want;
        return true;
    }
    // Room for n bytes, `want` of them allocated, the contents dropped: the old block is freed BEFORE the new one is
    // allocated, because the two need not fit side by side (index tables reach 2.3 GB).  Freeing synchronises the device:
    // nothing still reads the old block.  On failure the buffer is empty.
    bool replace(size_t n, size_t want)
    {
        if (n <= cap) return true;
        release();
        if (!alloc(&p, want)) return false;
        cap = want;
        return true;
    }
    void release()
    {
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }

private:
    // a failed allocation leaves *q null and HIP's last error cleared
    bool alloc(void **q, size_t bytes) const
    {
        if ((pinned ? hipHostMalloc(q, bytes, hipHostMallocDefault) : hipMalloc(q, bytes)) == hipSuccess) return true;
        *q = nullptr;
        (void)hipGetLastError();
        return false;
    }
};

}  // namespace aec
