// tri_geometry.cpp -- rt::TriGeometry and rt::PinnedRing (see tri_geometry.hpp, devbuf.hpp).
#include "tri_geometry.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/rt_mi355x.h"
#include "host_scene.hpp"
#include "launch.hpp"

namespace rt {

PinnedRing::~PinnedRing()
{
    for (hipEvent_t ev : ev_)
        if (ev) (void)hipEventDestroy(ev);
    if (buf_) (void)hipHostFree(buf_);
}

hipError_t PinnedRing::reserve()
{
    hipError_t e = hipSuccess;
    if (!buf_ && (e = hipHostMalloc(reinterpret_cast<void**>(&buf_), DEPTH * CHUNK, hipHostMallocDefault)) != hipSuccess)
        buf_ = nullptr;
    for (int i = 0; i < DEPTH && e == hipSuccess; i++)
        if (!ev_[i]) e = hipEventCreateWithFlags(&ev_[i], hipEventDisableTiming);
    return e;
}

hipError_t PinnedRing::upload(void* dev, const void* host, size_t bytes, hipStream_t stream)
{
    hipError_t e = bytes ? reserve() : hipSuccess;
    for (size_t i = 0, off = 0; e == hipSuccess && off < bytes; i++, off += CHUNK) {
        const size_t len = std::min(CHUNK, bytes - off);
        if ((e = wait(i)) != hipSuccess)   // the slot's last copy has left it
            break;
        std::memcpy(slot(i), static_cast<const char*>(host) + off, len);
        if ((e = hipMemcpyAsync(static_cast<char*>(dev) + off, slot(i), len, hipMemcpyHostToDevice, stream)) == hipSuccess)
            e = mark(i, stream);
    }
    if (e != hipSuccess)
        (void)hipStreamSynchronize(stream);
    return e;
}

hipError_t PinnedRing::readback(const Part* parts, int nparts, hipStream_t stream)
{
    std::vector<Part> pieces;   // the parts in chunks
    for (int k = 0; k < nparts; k++)
        for (size_t off = 0; off < parts[k].bytes; off += CHUNK)
            pieces.push_back({static_cast<char*>(parts[k].host) + off, static_cast<const char*>(parts[k].dev) + off,
                              std::min(CHUNK, parts[k].bytes - off)});
    const size_t np = pieces.size();
    hipError_t e = reserve();
    for (size_t i = 0; e == hipSuccess && i < np + DEPTH; i++) {
        if ((e = wait(i)) != hipSuccess)
            break;
        if (i >= DEPTH)   // piece i - DEPTH has landed in the slot piece i takes next
            std::memcpy(pieces[i - DEPTH].host, slot(i), pieces[i - DEPTH].bytes);
        if (i < np && (e = hipMemcpyAsync(slot(i), pieces[i].dev, pieces[i].bytes, hipMemcpyDeviceToHost, stream)) == hipSuccess)
            e = mark(i, stream);
    }
    if (e != hipSuccess)
        (void)hipStreamSynchronize(stream);
    return e;
}

TriGeometry::~TriGeometry()
{
    for (hipEvent_t ev : ingest_ev_)
        if (ev) (void)hipEventDestroy(ev);
}

int TriGeometry::hip_fail(hipError_t e, const char* what, std::string& err) const
{
    err = std::string(what) + ": " + hipGetErrorString(e);
    return RT_EHIP;
}

void TriGeometry::set_host(const float* tri9, const int32_t* mat, const float* uv6, int64_t n)
{
    tri_.assign(tri9, tri9 + 9 * n);
    queue_.clear();
    st_.host_replaced();
    set_attributes(mat, uv6, n);
}

void TriGeometry::set_attributes(const int32_t* mat, const float* uv6, int64_t n)
{
    n_ = n;
    mat_.assign(mat, mat + n);
    // the material range, checked before every launch without re-reading the per-triangle indices (a
    // 1M-triangle scan per frame cost ~0.2 ms of host time)
    mat_lo_ = INT32_MAX;
    mat_hi_ = INT32_MIN;
    for (int32_t m : mat_) {
        mat_lo_ = std::min(mat_lo_, m);
        mat_hi_ = std::max(mat_hi_, m);
    }
    if (uv6)
        uv_.assign(uv6, uv6 + 6 * n);
    else
        uv_.clear();
}

void TriGeometry::copy_host_from(const TriGeometry& lead)
{
    tri_ = lead.tri_;
    queue_.clear();
    st_.host_replaced();
    n_ = lead.n_;
    mat_ = lead.mat_;
    mat_lo_ = lead.mat_lo_;
    mat_hi_ = lead.mat_hi_;
    uv_ = lead.uv_;
}

// (A pointer the runtime does not know leaves a sticky error behind: cleared.)
int check_device_pointers(const void* const* ptrs, int count, int device, const char* what, std::string& err)
{
    for (int i = 0; i < count; i++) {
        if (!ptrs[i])
            continue;
        hipPointerAttribute_t a{};
        const char* bad = nullptr;
        if (hipPointerGetAttributes(&a, ptrs[i]) != hipSuccess) {
            (void)hipGetLastError();
            bad = ": not a device pointer";
        } else if (a.type != hipMemoryTypeDevice)
            bad = ": not device memory";
        else if (a.device != device)
            bad = ": memory of another device";
        if (bad) {
            err = std::string(what) + bad;
            return RT_EINVAL;
        }
    }
    return RT_OK;
}

int TriGeometry::check_input(const void* d_verts, const void* d_idx, std::string& err)
{
    const void* const ptrs[] = {d_verts, d_idx};
    return check_device_pointers(ptrs, 2, device_, "geometry input", err);
}

int TriGeometry::ingest(const float* d_verts, int64_t nv, const int32_t* d_idx, int64_t n, hipStream_t stream,
                        std::string& err)
{
    hipError_t e;
    for (hipEvent_t& ev : ingest_ev_)
        if (!ev && (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess)
            return hip_fail(e, "hipEventCreate (geometry input)", err);
    if ((e = d_ingest_word_.reserve(4)) != hipSuccess)
        return hip_fail(e, "hipMalloc (geometry input)", err);
    // (from here the positions before are gone: growing d_tri9_ drops its contents)
    queue_.clear();
    if ((e = d_tri9_.reserve((size_t)n * 36)) == hipSuccess && (e = hipEventRecord(ingest_ev_[0], stream)) == hipSuccess &&
        (e = hipStreamWaitEvent(home_, ingest_ev_[0], 0)) == hipSuccess &&
        (e = hipMemsetAsync(d_ingest_word_.p, 0, 4, home_)) == hipSuccess &&
        (e = rt_launch_gather_points(d_verts, nv, d_idx, d_tri9_.as<float>(), 3 * n, d_ingest_word_.as<uint32_t>(),
                                     home_)) == hipSuccess &&
        (e = hipEventRecord(ingest_ev_[1], home_)) == hipSuccess)
        e = hipStreamWaitEvent(stream, ingest_ev_[1], 0);
    if (e != hipSuccess) {
        clear();   // (neither the old positions nor the new ones are whole)
        return hip_fail(e, "geometry input on the device", err);
    }
    ++ingests_;
    st_.ingested();
    return RT_OK;
}

// the device input's word, once per input, where the host waits for the home stream anyway
int TriGeometry::read_ingest_word(std::string& err)
{
    if (!st_.ingest_unread())
        return RT_OK;
    unsigned word = 0;
    hipError_t e = hipSetDevice(device_);
    if (e == hipSuccess)
        e = read_u32(d_ingest_word_.p, home_, word);
    if (e != hipSuccess)
        return hip_fail(e, "geometry input on the device", err);
    st_.ingest_word(word);
    return RT_OK;
}

void TriGeometry::transform_host(const float m[16])
{
    std::vector<float> out(tri_.size());
    mat::transform_points(m, tri_.data(), (int64_t)(tri_.size() / 3), out.data());
    tri_.swap(out);
    queue_.clear();
    st_.host_edited();
}

void TriGeometry::queue_transform(const float m[16])
{
    std::array<float, 16> q;
    std::memcpy(q.data(), m, sizeof(float) * 16);
    queue_.push_back(q);
    st_.edit_queued();
}

// the queued edits, applied to d_tri9_ where it lies, then the kernel's word
int TriGeometry::apply_edits(std::string& err)
{
    if (queue_.empty())
        return RT_OK;
    hipError_t e = hipSetDevice(device_);
    if (e != hipSuccess)
        return hip_fail(e, "hipSetDevice", err);
    if ((e = d_edit_word_.reserve(4)) != hipSuccess)
        return hip_fail(e, "hipMalloc (object transform)", err);
    e = hipMemsetAsync(d_edit_word_.p, 0, 4, home_);
    size_t applied = 0;
    while (e == hipSuccess && applied < queue_.size()) {
        e = rt_launch_xform_points(queue_[applied].data(), d_tri9_.as<float>(), 3 * n_, d_edit_word_.as<uint32_t>(), home_);
        if (e == hipSuccess)
            applied++;
    }
    // (a launch that failed leaves its matrix and the ones behind it queued)
    queue_.erase(queue_.begin(), queue_.begin() + applied);
    transforms_ += (int64_t)applied;
    unsigned word = 0;
    if (e == hipSuccess)
        e = read_u32(d_edit_word_.p, home_, word);
    if (e != hipSuccess)
        return hip_fail(e, "object transform on the device", err);
    st_.edit_word(word);
    return RT_OK;
}

int TriGeometry::host(const std::vector<float>*& tri, std::string& err)
{
    tri = &tri_;
    if (st_.host_current())
        return RT_OK;
    int rc = apply_edits(err);
    if (rc == RT_OK)
        rc = read_ingest_word(err);
    if (rc != RT_OK)
        return rc;
    tri_.resize(9 * (size_t)n_);   // (a device input leaves tri_ as it was, of any size)
    hipError_t e = hipSetDevice(device_);
    if (e == hipSuccess)
        e = hipStreamSynchronize(home_);
    if (e == hipSuccess && !tri_.empty())
        e = hipMemcpy(tri_.data(), d_tri9_.p, tri_.size() * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return hip_fail(e, "download (device-transformed triangles)", err);
    st_.downloaded();
    return RT_OK;
}

int TriGeometry::device(hipStream_t stream, bool ring, const char* what, const float*& d_tri9, std::string& err)
{
    int rc = apply_edits(err);
    if (rc != RT_OK)
        return rc;
    if (!st_.device_current()) {   // (else: resident from an upload before, a device input or a device transform)
        const size_t bytes = tri_.size() * 4;
        hipError_t e;
        if ((ring && bytes && (e = ring_.reserve()) != hipSuccess) || (e = d_tri9_.reserve(bytes)) != hipSuccess)
            return hip_fail(e, (std::string("hipMalloc (") + what + ")").c_str(), err);
        if (ring)
            e = ring_.upload(d_tri9_.p, tri_.data(), bytes, stream);
        else if (bytes)
            e = hipMemcpyAsync(d_tri9_.p, tri_.data(), bytes, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess)
            return hip_fail(e, (std::string("upload (") + what + ")").c_str(), err);
        st_.uploaded();   // (in stream order: every later reader of d_tri9_ follows 'stream' or waits for it)
    }
    d_tri9 = d_tri9_.as<float>();
    return RT_OK;
}

int TriGeometry::check(std::string& err)
{
    int rc = apply_edits(err);
    if (rc == RT_OK)
        rc = read_ingest_word(err);
    if (rc != RT_OK)
        return rc;
    // (while the host copy is stale the positions were written by a kernel, which kept the same test's word)
    bool finite = !st_.nonfinite();
    if (st_.host_current())
        for (float c : tri_)
            finite = finite && std::isfinite(c);
    if (finite && !st_.bad_index())
        return RT_OK;
    err = !finite ? "triangle with a non-finite vertex coordinate" : "vertex index out of range";
    return RT_EINVAL;
}

}  // namespace rt
