// devbuf.hpp -- the two memory holders of the host side: DevBuf, a growing device allocation, and
// PinnedRing, the pinned staging ring that large host <-> device copies go through.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

#include <utility>

namespace rt {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int device = 0;   // the device that holds p: the calling thread's when reserve allocated it
    ~DevBuf();
    hipError_t reserve(size_t n);   // grows (never shrinks); contents undefined after growth
    void release();                 // frees under 'device' (the calling thread's current device afterwards)
    template <class T> T* as() const { return static_cast<T*>(p); }
    // exchanges the allocations (a copy would free one buffer twice)
    void swap(DevBuf& o)
    {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        std::swap(device, o.device);
    }
};

// One 32-bit count of the stream's last kernels, on the host once they are done.
inline hipError_t read_u32(const void* dev, hipStream_t stream, unsigned& out)
{
    hipError_t e = hipMemcpyAsync(&out, dev, 4, hipMemcpyDeviceToHost, stream);
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
}

// DEPTH pinned chunks of CHUNK bytes with an event each, made by the first reserve() and kept: the host
// fills (or empties) one chunk while the DMA works on the others.  A slot is touched only after its event
// has passed, so one ring serves copies on any stream, one call at a time.
class PinnedRing {
public:
    static constexpr size_t CHUNK = 4u << 20;
    static constexpr int DEPTH = 4;
    struct Part {   // one array to read back
        void* host;
        const void* dev;
        size_t bytes;
    };
    ~PinnedRing();
    hipError_t reserve();
    // host -> dev in stream order; returns once the last chunk is enqueued (the host array is free again)
    hipError_t upload(void* dev, const void* host, size_t bytes, hipStream_t stream);
    // every part dev -> host behind the stream's work; returns once all of it is in the host arrays
    hipError_t readback(const Part* parts, int nparts, hipStream_t stream);

private:
    char* slot(size_t i) const { return buf_ + (i % DEPTH) * CHUNK; }
    hipError_t wait(size_t i) const { return used_[i % DEPTH] ? hipEventSynchronize(ev_[i % DEPTH]) : hipSuccess; }
    hipError_t mark(size_t i, hipStream_t stream)
    {
        used_[i % DEPTH] = true;
        return hipEventRecord(ev_[i % DEPTH], stream);
    }
    char* buf_ = nullptr;
    hipEvent_t ev_[DEPTH] = {};
    bool used_[DEPTH] = {};   // the slot's event has been recorded
};

}  // namespace rt
