// tri_geometry.hpp -- the triangles of a renderer: their count, the positions on the host and / or in
// d_tri9_ (caller order, [n][9]: what the device octree build and the raster path read), the object edits
// queued for the device copy, and the per-triangle attributes.  Which copy is current is a TriState
// (tri_state.hpp); nothing outside this class moves it.
//
// Kernels and the reads of their words run on the home stream given to init().  The owner knows nothing of
// frames in flight: calls marked [slots] write d_tri9_ where raster frames on other streams may read it, and
// the renderer waits for those frames (sync_slots) before it makes them.
//
// Calls that can fail return an RT_* code and leave the message in 'err'.
#pragma once

#include <stdint.h>

#include <array>
#include <string>
#include <vector>

#include "devbuf.hpp"
#include "tri_state.hpp"

namespace rt {

// Every non-null pointer of the list is device memory of 'device' (hipPointerGetAttributes on the address
// given: the range behind it is the caller's word), else RT_EINVAL with "<what>: ..." in err.  The check of
// the geometry input and of the device ray queries.
int check_device_pointers(const void* const* ptrs, int count, int device, const char* what, std::string& err);

class TriGeometry {
public:
    ~TriGeometry();
    void init(int device, hipStream_t home)
    {
        device_ = device;
        home_ = home;
    }

    int64_t count() const { return n_; }
    const std::vector<int32_t>& mat() const { return mat_; }
    const std::vector<float>& uv() const { return uv_; }
    // some material index lies outside [0, nmat) (the range is kept: no per-frame scan)
    bool mat_out_of_range(int nmat) const { return n_ > 0 && (mat_lo_ < 0 || mat_hi_ >= nmat); }
    int64_t ingests() const { return ingests_; }         // device inputs taken (rt_get_device_ingests)
    int64_t transforms() const { return transforms_; }   // matrices applied by the kernel (rt_get_device_transforms)

    // new triangles from host arrays; no triangles
    void set_host(const float* tri9, const int32_t* mat, const float* uv6, int64_t n);
    void clear() { set_host(nullptr, nullptr, nullptr, 0); }
    // the count, materials and texture coordinates alone (the positions: an ingest just before)
    void set_attributes(const int32_t* mat, const float* uv6, int64_t n);
    // a helper's copy of its lead's triangles, positions from the lead's host copy, which the caller has just
    // brought up to date (lead.host); no device state
    void copy_host_from(const TriGeometry& lead);

    // both arrays of a device input are memory of this device (a null one passes)
    int check_input(const void* d_verts, const void* d_idx, std::string& err);
    // [slots] positions of n triangles gathered from the caller's device arrays, in the order of 'stream': the
    // home stream waits for it, runs the kernel, and 'stream' waits for the kernel.  The queued edits are
    // dropped.  The kernel's word is read by the next check() or host().  A failure leaves no triangles.
    int ingest(const float* d_verts, int64_t nv, const int32_t* d_idx, int64_t n, hipStream_t stream, std::string& err);

    // The two ways of set_object_transform.  On the host: the host copy (current: host() just before) through
    // m.  On the device (while resident()): m queued; the queue runs one launch per matrix in call order
    // (composed matrices would round differently) at the next device(), host() or check().
    void transform_host(const float m[16]);
    void queue_transform(const float m[16]);
    bool resident() const { return st_.device_current(); }
    bool edits_queued() const { return !queue_.empty(); }

    // [slots] while edits_queued(): the host copy brought up to date (the queue, then one download, sized from
    // the count) and handed out
    int host(const std::vector<float>*& tri, std::string& err);
    // [slots] while edits_queued(): the device copy brought up to date (the queue; an upload on 'stream' when it
    // is not current) and handed out.  ring: the upload goes through the pinned ring, else it is one copy from
    // the pageable host copy (the raster path: nothing runs beside it there, and on sphere1m the ring cost it
    // 1 ms).  'what' names the caller in the messages.
    int device(hipStream_t stream, bool ring, const char* what, const float*& d_tri9, std::string& err);
    // [slots] while edits_queued(): the refusals before a build (the queue and the device input's word first):
    // a non-finite coordinate -- the host scan when the host copy is current, else the kernels' word -- and a
    // device input's index out of range
    int check(std::string& err);

    PinnedRing& ring() { return ring_; }   // (lent to the device octree build's readback)

private:
    int hip_fail(hipError_t e, const char* what, std::string& err) const;
    int apply_edits(std::string& err);
    int read_ingest_word(std::string& err);

    int device_ = 0;
    hipStream_t home_ = nullptr;
    int64_t n_ = 0;
    std::vector<float> tri_;   // [n][9] while st_.host_current() (else: of any size)
    std::vector<int32_t> mat_;
    int32_t mat_lo_ = INT32_MAX, mat_hi_ = INT32_MIN;   // range of mat_
    std::vector<float> uv_;
    TriState st_;
    DevBuf d_tri9_;
    std::vector<std::array<float, 16>> queue_;
    DevBuf d_edit_word_, d_ingest_word_;   // the kernels' words
    hipEvent_t ingest_ev_[2] = {nullptr, nullptr};   // the caller's stream -> home, and back
    PinnedRing ring_;
    int64_t ingests_ = 0, transforms_ = 0;
};

}  // namespace rt
