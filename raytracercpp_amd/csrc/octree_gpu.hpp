// octree_gpu.hpp -- the reference octree built on the device (octree_gpu.hip), byte for byte the
// arrays build_flat_octree / build_flat_octree_serial flatten (octree.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "octree.hpp"
#include "renderer.hpp"   // DevBuf

namespace rt {

constexpr int OCT_GPU_MAX_DEPTH = 30;            // levels 0 .. 30: the frames take at most 31 levels
constexpr int64_t OCT_GPU_MAX_TRIS = 1ll << 26;  // 8 children per inner node and every level's flat
                                                 // indices stay far inside 32 bits

// What the device build leaves beside the three arrays, in a device buffer the caller supplies
// (the builder's kernels keep their running totals in it) and, on return, in its host copy.
struct OctreeDevInfo {
    int64_t stats[6];       // OctreeStats: inner, leaves, empty_leaves, max_leaf, max_depth, nodes
    int32_t levels;         // FlatOctree::levels
    int32_t ordered_slabs;  // FlatOctree::ordered_slabs
    int64_t nodes, tris;    // flattened GNode and GTri counts
    int32_t level_base[OCT_GPU_MAX_DEPTH + 3];  // first flat index of each level's kept nodes
    int32_t slot_base[OCT_GPU_MAX_DEPTH + 3];   // first triangle slot of each level's leaves
    int32_t next[2];        // the level just classified: its inner nodes, the items they hold
    int32_t max_leaf;
};

// O(n) temporaries, kept across rebuilds
struct OctreeGpuScratch {
    DevBuf cx[2], cy[2], cz[2], tid[2];   // the items still above a leaf, ping-pong: centroid, triangle
    DevBuf key[2], pos[2];                // an item's node in its level; the sort's source positions
    DevBuf lnodes[2];                     // the current and the next level's nodes
    DevBuf flags, ranks;                  // per node: inner / kept / leaf triangles, and their exclusive sums
    DevBuf inner_node, parent_flat[2];    // per group of 8 children: the parent's node and flat index
    DevBuf partial;                       // the root box's per-block boxes
    DevBuf tmp;                           // hipcub
    void* pinned = nullptr;               // 8 bytes: the per-level readback
    ~OctreeGpuScratch();
};

enum { OCT_GPU_OK = 0, OCT_GPU_UNSUPPORTED = 1, OCT_GPU_HIP = 2 };

// true when build_flat_octree_device takes the input (else the caller builds on the host)
bool octree_device_supported(int64_t n, int max_depth);

// Builds the octree over d_tri9 ([n][9] world-space vertices with finite coordinates, on the
// current device) into nodes / tris / tri_id (grown as needed) on 'stream', and waits for it.
// n == 0 is the empty tree (no launch).  *err gets the HIP error of OCT_GPU_HIP.
int build_flat_octree_device(OctreeGpuScratch& S, const float* d_tri9, int64_t n, int max_depth,
                             int leaf_max_obj_count, DevBuf& nodes, DevBuf& tris, DevBuf& tri_id,
                             OctreeDevInfo* d_info, OctreeDevInfo* h_info, hipStream_t stream, hipError_t* err);

}  // namespace rt
