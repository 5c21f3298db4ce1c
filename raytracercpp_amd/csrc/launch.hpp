// launch.hpp -- the host-side launch wrappers kernels.hip defines and renderer.cpp calls, declared once:
// a definition whose parameters drift from these is a compile error, not a corrupted argument.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kparams.hpp"
#include "ocone.hpp"
#include "tile_lists.hpp"
#include "wbvh.hpp"

namespace rt {

// the reflection engine's passes over a chunk of frames (rt_launch_refl_stage)
enum class ReflStage {
    trace,     // gen + trace (refl_trace_feed_kernel with ReflArgs::feed, else refl_trace_kernel)
    long_,     // the deferred long traces
    pass1,     // pass1 (+ shadow list)
    shadow,    // shadow (+ spawn)
    resolve,
};

// the raster path's passes (rt_launch_raster_stage)
enum class RasterStage {
    count,
    write,
    fill,       // small pieces
    fill_big,   // big pieces
};

// the instances of shade_rays_kernel (rt_launch_shade_rays), in the order rt_get_device_shaded_queries reports
enum { SHADE_PLAIN = 0, SHADE_GENERIC = 1, SHADE_REFL = 2 };

}  // namespace rt

// internal to the library: C names, hidden from its exports
#define RT_LAUNCH extern "C" __attribute__((visibility("hidden"))) hipError_t

RT_LAUNCH rt_launch_ray_trace(const rt::KParams* P, hipStream_t stream);
RT_LAUNCH rt_launch_heavy_prep(const rt::KParams* P, uint32_t* cost, int ntiles, int32_t* list, uint32_t* bits,
                               int32_t* ctr, int32_t* ctr_next, const unsigned long long* stats_prev,
                               unsigned long long* stats_next, float split, int group, hipStream_t stream);
RT_LAUNCH rt_launch_trace_rays(const rt::KParams* P, const float* o, const float* d, int n, int32_t* id, float* t,
                               float* u, float* v, uint8_t* ret, hipStream_t stream);
RT_LAUNCH rt_launch_wide_query(const rt::KParams* P, const float* o, const float* d, int n, int kind, float* o_out,
                               float* d_out, int32_t* status, int32_t* id, float* t, float* u, float* v, uint8_t* sh,
                               hipStream_t stream);
// the ray queries over the caller's device memory (rt_trace_rays_device, rt_is_shadowed_device)
RT_LAUNCH rt_launch_closest_rays(const rt::KParams* P, const float* o, const float* d, int n, int32_t* id, float* t,
                                 float* u, float* v, uint8_t* ret, int64_t* counts, hipStream_t stream);
RT_LAUNCH rt_launch_shadow_points(const rt::KParams* P, const float* point, const float* normal, int n,
                                  const float light[3], uint8_t* shadowed, hipStream_t stream);
// the ray-segment queries (rt_occluded_device: record false, flag = the occlusion byte, id / t / u / v unused;
// rt_trace_segments_device: record true, flag = ret).  tmax [n] may be null: +inf for every ray
RT_LAUNCH rt_launch_segment_rays(const rt::KParams* P, bool record, const float* o, const float* d, const float* tmax,
                                 int n, int32_t* id, float* t, float* u, float* v, uint8_t* flag, int64_t* counts,
                                 hipStream_t stream);
// the visibility buffer of P's camera over the caller's device memory (rt_visibility_device): id / t [rh][rw], uv
// [rh][rw][2] (8-byte aligned), each may be null.  fast: the plain frame kernel's primary query with P's tile mask
// and entry sets (the host: P->wnodes, enable_bvh, no analytic shape), else the generic one.  P->counters: the
// launch's own zeroed counter block; no heavy list, tile costs or tile lists in P
RT_LAUNCH rt_launch_visibility(const rt::KParams* P, bool fast, int32_t* id, float* t, float* uv, hipStream_t stream);
// the shaded query over device memory (rt_trace_ray_device; rt_trace_ray's staged arrays): inst is rt::SHADE_*;
// every output but rgba may be null; the fill writes what trace_ray returns past max_recursion_depth
RT_LAUNCH rt_launch_shade_rays(const rt::KParams* P, int inst, const float* o, const float* d, int n,
                               uint32_t first_ray, float4* rgba, int32_t* src, float* t, uint8_t* found,
                               uint8_t* shadow, int64_t* counts, hipStream_t stream);
RT_LAUNCH rt_launch_shade_rays_fill(int n, float4* rgba, int32_t* src, float* t, uint8_t* found, uint8_t* shadow,
                                    hipStream_t stream);
RT_LAUNCH rt_launch_downscale(const uint32_t* in, int w, int h_rows, int f, uint32_t* out, hipStream_t stream);
RT_LAUNCH rt_launch_ssao(const rt::SsaoArgs* A, hipStream_t stream);

// the acceleration structures
RT_LAUNCH rt_launch_wide_gather(const rt::GTri* tris, const int32_t* slot, const uint32_t* leaf_of_slot,
                                const int32_t* tri_id, const int32_t* tri_mat, int n, rt::GTri* wtris, uint4* wmeta,
                                hipStream_t stream);
RT_LAUNCH rt_launch_risk_box_init(float* B, size_t nentries, hipStream_t stream);
RT_LAUNCH rt_launch_wide_risk(const rt::GTri* wtris, const uint4* wmeta, const rt::GNode* onodes,
                              const rt::WNode* wnodes, const uint32_t* tri_leaf, const uint32_t* parent, uint32_t* K,
                              float* B, unsigned long long* risk, int n, int nnodes, const rt::WRiskArgs* A,
                              uint32_t* cap, const float* cap_dir, hipStream_t stream);
// the tile mask (wbvh.hpp): the cut of the resident tree into buf (2 W_CUT_MAX + 1 words: the
// entries, scratch, the count), once per tree; the mask of one camera into words (bh x wpr), zeroed first
// (parent: WBvh::parent on the device, node -> its parent's entry)
RT_LAUNCH rt_launch_wide_cut(const rt::WNode* wnodes, int nnodes, int budget, int max_depth, uint32_t* buf, hipStream_t stream);
RT_LAUNCH rt_launch_wide_mask(const rt::WNode* wnodes, int nnodes, const uint32_t* parent, const uint32_t* cut, int budget,
                              const rt::WMaskCam* C, uint32_t* words, hipStream_t stream);
// the entry sets of the same camera (wbvh.hpp wbvh_entry_block) into out (bh x bw uint4), from
// the mask's words
RT_LAUNCH rt_launch_wide_entry(const rt::WNode* wnodes, int nnodes, const rt::WMaskCam* C, const uint32_t* words, int K,
                               int fan, int max_depth, uint4* out, hipStream_t stream);
// the tile lists of a launch (tile_lists.hpp) into lists (tile_lists_words(ntiles) words, 8-byte
// aligned), from the camera's mask words (L->mask, L->band_map: device memory)
RT_LAUNCH rt_launch_tile_lists(const rt::TileLayout* L, int32_t* lists, hipStream_t stream);
RT_LAUNCH rt_launch_ocone(const rt::OConeEnt* E, const rt::GTri* tris, const uint32_t* todo, int n, const float lo[3],
                          const int32_t dim[3], double h, double r, double slack, double QS, double cos_cap,
                          uint2* cells, size_t ncells, hipStream_t stream);

// geometry edits (geom_gpu.hip): xform_point over pts [n][3] in place; *nonfinite |= 1 when a written
// coordinate is not finite.  n <= 0: no launch
RT_LAUNCH rt_launch_xform_points(const float m[16], float* pts, int64_t n, uint32_t* nonfinite, hipStream_t stream);
// geometry from device memory: tri9 [npts][3] = verts[idx[i]] (idx null: verts[i], npts <= nv), bit for bit;
// *flags |= 1 when a written coordinate is not finite, |= 2 when an index is outside [0, nv) (zeros
// written, nothing read).  npts <= 0: no launch
RT_LAUNCH rt_launch_gather_points(const float* verts, int64_t nv, const int32_t* idx, float* tri9, int64_t npts,
                                  uint32_t* flags, hipStream_t stream);

// the reflection engine (renderer.cpp drives the levels)
RT_LAUNCH rt_launch_refl_level0(const rt::KParams* P, rt::FrameRec* fr1, unsigned int* nfr1, hipStream_t stream);
// level 0 over a batch of rays in the caller's device memory (rt_trace_ray_batch_device): P's outputs and found
// point at the batch's first ray, ray i is keyed as pixel first_ray + i; then the call's counts, counts[0..1] +=
// counters[0..1]
RT_LAUNCH rt_launch_refl_rays_level0(const rt::KParams* P, const float* o, const float* d, int n, uint32_t first_ray,
                                     rt::FrameRec* fr1, unsigned int* nfr1, uint8_t* found, hipStream_t stream);
RT_LAUNCH rt_launch_add_ray_counts(const unsigned long long* counters, int64_t* counts, hipStream_t stream);
RT_LAUNCH rt_launch_refl_stage(rt::ReflStage stage, const rt::KParams* P, const rt::ReflArgs* A, hipStream_t stream);
RT_LAUNCH rt_launch_refl_keys(const rt::KParams* P, const rt::FrameRec* fr, int n, uint32_t* keys, int32_t* idx,
                              hipStream_t stream);
RT_LAUNCH rt_launch_refl_sort_frames(const rt::FrameRec* fr, const int32_t* order, int n, rt::FrameRec* frs,
                                     hipStream_t stream);
RT_LAUNCH rt_launch_refl_shadow_keys(const rt::KParams* P, const rt::SampleRec* sm, const int32_t* list, int n,
                                     uint32_t* keys, hipStream_t stream);

// the raster path
RT_LAUNCH rt_launch_raster_stage(rt::RasterStage stage, const rt::KParams* P, const rt::RasterArgs* A, int npieces,
                                 hipStream_t stream);
RT_LAUNCH rt_launch_raster_shade(const rt::KParams* P, const rt::RasterArgs* A, rt::FrameRec* fr1, unsigned int* nfr1,
                                 hipStream_t stream);
