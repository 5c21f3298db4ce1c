// ray_stage.hpp -- where the arrays of a host ray query (rt_trace_rays, rt_wide_query, rt_trace_ray) lie inside
// the one device buffer the call stages them in, as a function of the call's list of arrays and its ray count.
// The renderer's stager (renderer.cpp RayStage) takes every offset and the total from here.  No HIP call: host
// programs include it.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rt {

enum : unsigned {
    STAGE_UP = 1,     // uploaded before the launch
    STAGE_DOWN = 2,   // downloaded after it
    STAGE_ONCE = 4,   // one element for the whole call, not one per ray (the shaded query's counts)
};

struct StageArray {
    void* host;      // the caller's array (an input is only read)
    uint64_t elem;   // bytes per ray
    unsigned flags;
};
inline StageArray stage_in(const void* host, uint64_t elem) { return {const_cast<void*>(host), elem, STAGE_UP}; }
inline StageArray stage_out(void* host, uint64_t elem) { return {host, elem, STAGE_DOWN}; }

constexpr int STAGE_MAX_ARRAYS = 12;
constexpr uint64_t STAGE_ALIGN = 16;   // (float4 stores: the shaded kernels' d_rgba rule)

// Array k takes bytes[k] at off[k]: the slots follow the list's order, each starts at a multiple of STAGE_ALIGN,
// and total is the last slot's end rounded up.  In 64 bits throughout: n goes up to 2^30, where the shaded
// query's list takes 50 B per ray.
struct StageLayout {
    uint64_t off[STAGE_MAX_ARRAYS], bytes[STAGE_MAX_ARRAYS], total;
};

inline StageLayout stage_layout(const StageArray* a, int count, uint64_t n)
{
    StageLayout L{};
    for (int k = 0; k < count; k++) {
        L.off[k] = L.total;
        L.bytes[k] = a[k].elem * ((a[k].flags & STAGE_ONCE) ? 1 : n);
        L.total = (L.off[k] + L.bytes[k] + STAGE_ALIGN - 1) / STAGE_ALIGN * STAGE_ALIGN;
    }
    return L;
}

}  // namespace rt
