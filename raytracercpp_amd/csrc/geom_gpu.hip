// geom_gpu.hip -- the geometry edits on the device: Renderer::set_object_transform's pass over every
// vertex (renderer.cpp:214-224 of the reference) applied to the device-resident caller-order
// positions, so that an edit neither recomputes them on the host nor uploads them again
// (DESIGN.md 5.1).  The arithmetic is rt_math.hpp's xform_point, the expression the host runs
// (-ffp-contract=off, correctly rounded division on both sides): the same bytes, NaN payloads aside.
// Also the way in for positions that lie in device memory already (rt_set_triangles_device): a gather
// into the same resident array, a copy of words.
#include "launch.hpp"
#include "rt_math.hpp"

#include <algorithm>

namespace rt {

namespace {

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr int64_t MAX_BLOCKS = 2048;   // 8 blocks per CU; the points beyond them by a grid stride

struct Mat16 {
    float m[16];
};

// an infinity or a NaN: every exponent bit set
__device__ inline bool nonfinite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// One lane per point (a wave's 768 B are contiguous), in place.  *nonfinite gets bit 0 when a written
// coordinate is not finite (std::isfinite's test, as ensure_device_scene runs it on the host): one
// integer atomic per wave that saw one, none otherwise.
__global__ __launch_bounds__(BLOCK) void xform_points_kernel(Mat16 M, float* __restrict__ pts, int64_t n,
                                                             uint32_t* nonfinite)
{
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        float* p = pts + 3 * i;
        v3 q = xform_point(M.m, mk(p[0], p[1], p[2]));
        p[0] = q.x;
        p[1] = q.y;
        p[2] = q.z;
        bad = bad || nonfinite_bits(q.x) || nonfinite_bits(q.y) || nonfinite_bits(q.z);
    }
    // (the loop has ended for the whole wave: every lane is here)
    if (__any(bad) && threadIdx.x % WAVE == 0)
        atomicOr(nonfinite, 1u);
}

// Geometry given in device memory (rt_set_triangles_device): one lane per output point of
// tri9 [n][9], moved as three 32-bit words (no arithmetic: NaN payloads, signed zeros and denormals
// survive).  idx == nullptr: verts is [3 n][3] already, a copy.  Else point i is verts[idx[i]]; an index
// outside [0, nv) reads nothing, writes zeros and raises bit 1.  Bit 0 as in xform_points_kernel, for the
// written coordinates only.  One integer atomic per wave that saw either, none otherwise.
__global__ __launch_bounds__(BLOCK) void gather_points_kernel(const uint32_t* __restrict__ verts, int64_t nv,
                                                              const int32_t* __restrict__ idx,
                                                              uint32_t* __restrict__ out, int64_t npts,
                                                              uint32_t* flags)
{
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    uint32_t seen = 0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npts; i += stride) {
        int64_t v = i;
        if (idx)
            v = (int64_t)idx[i];
        uint32_t x = 0, y = 0, z = 0;
        if (v >= 0 && v < nv) {
            const uint32_t* p = verts + 3 * v;
            x = p[0];
            y = p[1];
            z = p[2];
        } else
            seen |= 2u;
        uint32_t* q = out + 3 * i;
        q[0] = x;
        q[1] = y;
        q[2] = z;
        if (nonfinite_bits(__uint_as_float(x)) || nonfinite_bits(__uint_as_float(y)) ||
            nonfinite_bits(__uint_as_float(z)))
            seen |= 1u;
    }
    // (the loop has ended for the whole wave: every lane is here)
    const bool b0 = __any(seen & 1u), b1 = __any(seen & 2u);
    if ((b0 || b1) && threadIdx.x % WAVE == 0)
        atomicOr(flags, (b0 ? 1u : 0u) | (b1 ? 2u : 0u));
}

}  // namespace

}  // namespace rt

hipError_t rt_launch_xform_points(const float m[16], float* pts, int64_t n, uint32_t* nonfinite, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    rt::Mat16 M;
    for (int k = 0; k < 16; k++) M.m[k] = m[k];
    const int64_t blocks = std::min<int64_t>((n + rt::BLOCK - 1) / rt::BLOCK, rt::MAX_BLOCKS);
    rt::xform_points_kernel<<<dim3((unsigned)blocks), dim3(rt::BLOCK), 0, stream>>>(M, pts, n, nonfinite);
    return hipGetLastError();
}

hipError_t rt_launch_gather_points(const float* verts, int64_t nv, const int32_t* idx, float* tri9, int64_t npts,
                                   uint32_t* flags, hipStream_t stream)
{
    if (npts <= 0)
        return hipSuccess;
    const int64_t blocks = std::min<int64_t>((npts + rt::BLOCK - 1) / rt::BLOCK, rt::MAX_BLOCKS);
    rt::gather_points_kernel<<<dim3((unsigned)blocks), dim3(rt::BLOCK), 0, stream>>>(
        reinterpret_cast<const uint32_t*>(verts), nv, idx, reinterpret_cast<uint32_t*>(tri9), npts, flags);
    return hipGetLastError();
}
