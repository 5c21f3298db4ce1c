// wbvh_quick_gpu.hpp -- the quick wide BVH (wbvh.hpp build_wbvh_quick) built on the
// device from the device-built octree (octree_gpu.hpp), in place: the tree build_wbvh_quick makes of
// the same octree, byte for byte except where a code goes through acos / cos / sin.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "octree_gpu.hpp"
#include "wbvh.hpp"

namespace rt {

constexpr int WQ_GPU_MAX_DEPTH = 128;   // wide depths: two per octree level (a group node) plus a runs tree's

// the builder's running totals (device) and their host copy
struct WQuickDevInfo {
    int32_t depth_count[WQ_GPU_MAX_DEPTH];   // wide nodes per depth
    int32_t cursor[WQ_GPU_MAX_DEPTH];        // the depth lists' fill positions
    int32_t leaves, max_leaf, max_depth, nodes;
};

// O(n) temporaries, kept across rebuilds
struct WQuickGpuScratch {
    DevBuf sub;      // per octree node: its subtree's wide nodes W and triangles T, then its wide index I,
                     // first triangle F and wide depth D
    DevBuf plans;    // per wide node: its children (runs of triangles or nodes)
    DevBuf agg;      // per wide node: its aggregate as its parent's child (wbvh_quick.hpp QChild)
    DevBuf list;     // the wide nodes by depth
    DevBuf info;     // WQuickDevInfo
    void* pinned = nullptr;   // the phases' readbacks
    ~WQuickGpuScratch();
};

// true when build_wbvh_quick_device takes the octree build_flat_octree_device made of (n, max_depth)
bool wbvh_quick_device_supported(int64_t n, int max_depth);

// Builds the quick tree of the device-resident octree (d_nodes / d_tris, described by oi, the host copy
// of its OctreeDevInfo) on 'stream' and waits for it: wnodes = the WNode array, tmp = the slot maps
// (what rt_launch_wide_gather reads) and links = the risk walk's, both laid out by wide_layout.hpp for
// (stats[0], stats[2]): the three buffers of a renderer.hpp WideDev.  stats: WStats' nodes, leaves, tris, max_leaf, depth.  An empty octree is the empty tree (no
// launch).  Returns OCT_GPU_OK / OCT_GPU_UNSUPPORTED / OCT_GPU_HIP (*err: the HIP error).
int build_wbvh_quick_device(WQuickGpuScratch& S, const GNode* d_nodes, const GTri* d_tris, const OctreeDevInfo& oi,
                            DevBuf& wnodes, DevBuf& tmp, DevBuf& links, int64_t stats[5], hipStream_t stream,
                            hipError_t* err);

}  // namespace rt
