// renderer.hpp -- rt::Renderer, the host-side mirror of the reference's
// Renderer class (tp2/projets/renderer/renderer.h:20-355) for the ray-trace hot
// path.  Scene state lives on the host (as in the reference); the octree is
// built on the host and flattened, then nodes, triangles, materials and
// textures are kept resident in HBM, and ray_trace() runs the gfx950 kernels.
#pragma once

#include <stdint.h>

#include <array>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "devbuf.hpp"
#include "kparams.hpp"
#include "ocone.hpp"
#include "octree.hpp"
#include "tile_lists.hpp"
#include "tri_geometry.hpp"
#include "vis_slots.hpp"
#include "wbvh.hpp"
#include "wide_layout.hpp"

namespace rt {

struct OctreeGpuScratch;   // octree_gpu.hpp
struct OctreeDevInfo;
struct WQuickGpuScratch;   // wbvh_quick_gpu.hpp

// The device-resident wide BVH (wbvh.hpp) as one value: the nodes, the triangle records in its leaf order and
// their metadata (what frames read), the slot maps wide_gather_kernel reads (tmp) and the grazing-risk walk's
// links, with the counts they were sized for (0: no tree).  The offsets inside tmp and links are
// wide_layout.hpp's.  The renderer holds two: the resident tree, and the background build's, which only
// accel_thread_ writes until adoption swaps them.
struct WideDev {
    DevBuf b_nodes, b_tris, b_meta, b_tmp, b_links;
    int64_t nn = 0, nt = 0;   // nodes, triangle records
    WNode* nodes() const { return b_nodes.as<WNode>(); }
    GTri* tris() const { return b_tris.as<GTri>(); }
    uint4* meta() const { return b_meta.as<uint4>(); }
    int32_t* slot() const { return at<int32_t>(b_tmp, wide_tmp_slot_off((size_t)nn, (size_t)nt)); }
    uint32_t* leaf_of_slot() const { return at<uint32_t>(b_tmp, wide_tmp_leaf_of_slot_off((size_t)nn, (size_t)nt)); }
    uint32_t* tri_leaf() const { return at<uint32_t>(b_links, wide_links_tri_leaf_off((size_t)nn, (size_t)nt)); }
    uint32_t* parent() const { return at<uint32_t>(b_links, wide_links_parent_off((size_t)nn, (size_t)nt)); }
    // sizes the five buffers for a tree of these counts (the counts are the tree's from here on)
    hipError_t reserve(int64_t nodes, int64_t tris);
    void clear() { nn = nt = 0; }   // no tree (the allocations are kept for the next one)
    void swap(WideDev& o);

private:
    template <class T> static T* at(const DevBuf& b, size_t off) { return reinterpret_cast<T*>(b.as<char>() + off); }
};

// "Everything launched on a stream up to here has finished", for waits that may come after the caller has
// destroyed that stream: 'mark' is recorded on the caller's stream, the renderer's own fence stream waits
// on it, and 'done' is recorded there.  Later waits touch only 'done' (an event recorded on a stream that
// was destroyed since made hipEventSynchronize fail with a capture-state error).  Waits before the first
// record() pass at once.
struct Fence {
    hipError_t create()
    {
        hipError_t e = hipEventCreateWithFlags(&done_, hipEventDisableTiming);
        return e == hipSuccess ? hipEventCreateWithFlags(&mark_, hipEventDisableTiming) : e;
    }
    void destroy()
    {
        if (done_) hipEventDestroy(done_);
        if (mark_) hipEventDestroy(mark_);
        done_ = mark_ = nullptr;
        live_ = false;
    }
    hipError_t record(hipStream_t stream, hipStream_t fence_stream)
    {
        hipError_t e;
        if ((e = hipEventRecord(mark_, stream)) == hipSuccess && (e = hipStreamWaitEvent(fence_stream, mark_, 0)) == hipSuccess &&
            (e = hipEventRecord(done_, fence_stream)) == hipSuccess)
            live_ = true;
        return e;
    }
    // 'stream', or the host, waits for the last record()
    hipError_t wait_on(hipStream_t stream) const { return live_ ? hipStreamWaitEvent(stream, done_, 0) : hipSuccess; }
    hipError_t sync() const { return live_ ? hipEventSynchronize(done_) : hipSuccess; }
    bool live() const { return live_; }   // record() has been called
    // what the last record() follows is still running
    bool busy() const { return live_ && hipEventQuery(done_) == hipErrorNotReady; }

private:
    hipEvent_t mark_ = nullptr, done_ = nullptr;
    bool live_ = false;
};

struct HostTex {
    int w = 0, h = 0;
    std::vector<float> rgba;
};

// Diagnostic switches, read once from the environment when the renderer is created
// (rt_create); each selects an equivalent path (same framebuffer) for A/B runs and tests.
struct Knobs {
    bool wbvh = true;         // RT_WBVH=0: no wide BVH, every query walks the octree
    bool seg = true;          // RT_SEG=0: shadow queries have no segment end (5.2)
    bool seg_oct = false;     // RT_SEG_OCTREE=1: the octree walks only a shadow / reflection query's segment
                              // (5.2; off by default: it assumes no grazing report falls outside its volumes)
    bool cones = true;        // RT_CONES=0: no leaf normal cones (5.3; also turns the leaf slabs off)
    bool lslab = true;        // RT_LSLAB=0: no leaf slabs (5.4)
    bool plain = true;        // RT_PLAIN=0: no plain specialisation of ray_trace_kernel (5.6)
    bool quick_wbvh = true;   // RT_WBVH_QUICK_FIRST=0: no quick wide BVH after a geometry change (the frames
                              // before the SAH tree is resident walk the octree; 5.9)
    bool plain_octree = true; // RT_PLAIN_OCTREE=0: frames on the octree path (before the wide BVH is resident,
                              // exact mode) take the general kernel, not the plain one (5.8)
    bool shade_plain = true;  // RT_SHADE_PLAIN=0: rt_trace_ray_device sends plain scenes through its generic instance,
                              // not the frames' plain pixel (kernels.hip shade_rays_kernel)
    bool fused_ssaa = true;   // RT_FUSED_SSAA=0: band launches downscale in a separate pass (7)
    bool refl_engine = true;  // RT_REFL_ENGINE=0: the one-lane-per-pixel recursive kernel (9)
    int refl_chunk_log2 = 27; // RT_REFL_CHUNK_LOG2 (10..27): sample slots per engine chunk
    int shade_batch_log2 = 22; // RT_SHADE_BATCH_LOG2 (10..24): rays per engine batch of rt_trace_ray_batch_device
                              // (level 1 holds one FrameRec per ray of a batch; small values: tests)
    bool debug_waves = false; // RT_DEBUG_WAVES: per-wave records of diagnostic builds (rt_debug_read)
    bool exact = false;       // RT_EXACT=1 / rt_set_exact: wbvh and seg off
    bool risk = true;         // RT_WBVH_RISK=0: no per-frame grazing-risk bits (every child runs case (b), 5.6)
    bool heavy = true;        // RT_HEAVY_FIRST=0: tiles in queue order only (no heavy-first list, 5.6)
    int heavy_group = SPLIT_G; // RT_HEAVY_GROUP=0: no split tiles (else: the build's RT_SPLIT_G parts of a tile,
                              // each with that many lanes per pixel, kernels.hip trace_split_part)
    int split_parts = 0;      // RT_SPLIT_PARTS=n (G or 2 G): parts per split tile (0: G)
    float heavy_split_exp = 0.5f;  // RT_HEAVY_SPLIT_EXP=e: the bar below grows as (frame tiles / launch tiles)^e
    float heavy_split_exp_overlap = 0.7f;  // RT_HEAVY_SPLIT_EXP_OVERLAP: the same while other band launches are
                                           // in flight (the launch's tail overlaps them: fewer splits pay)
    float heavy_split = 0.5f; // RT_HEAVY_SPLIT=c: split the heavy tiles costing >= c x the launch's mean
                              // cycles per wave (heavy_prep_kernel)
    int refl_defer = 32;      // RT_REFL_DEFER=k (refl_feed = 0): reflection queries past k loop iterations
                              // finish in a pass of their own
    int refl_feed = 24;       // RT_REFL_FEED=k: the reflection queries by refl_trace_feed_kernel (lane refill at k
                              // waiting lanes of a wave; C5 16 / 24 / 32 / 48: 1,128 / 1,101 / 1,103 / 1,155 ms per
                              // frame, 1,195 without); 0: refl_trace_kernel with its deferral (RT_REFL_DEFER)
    bool refl_sample_major = true;  // RT_REFL_SAMPLE_MAJOR=0: the engine's slots frame-major (a frame's samples
                              // side by side) instead of sample-major (kernels.hip slot_of)
    bool refl_shadow_sort = true;  // RT_REFL_SHADOW_SORT=0: the engine's shadow pass takes its list in the order
                              // pass1 appended it, not sorted by hit point (kernels.hip refl_shadow_keys_kernel)
    bool refl_sorted_frames = true;  // RT_REFL_SORTED_FRAMES=0: the engine reads frames through the sort order
                              // instead of a sorted copy (kernels.hip refl_sort_frames_kernel)
    bool risk_cap = true;     // RT_RISK_CAP=0: no risk caps (camera / shadow rays into a silhouette's interior skip
                              // case (b), wbvh.hpp risk_cap_skip)
    bool scene_bound = true;  // RT_SCENE_BOUND=0: no scene bound (camera rays that miss the root's widened frame
                              // still run their root step, wbvh.hpp wbvh_scene_bound)
    bool tile_mask = true;    // RT_TILE_MASK=0: no tile mask (every background tile generates its rays and runs
                              // the scene bound, wbvh.hpp wbvh_mask_rect)
    bool tile_start = true;   // RT_TILE_START=0: no entry sets (every camera ray starts its wide query at the root,
                              // wbvh.hpp wbvh_entry_block); no mask, no entry sets
    bool entry_cull = true;   // RT_ENTRY_CULL=0: the entry search keeps the subtrees that face away from a whole block
                              // (wbvh.hpp wbvh_entry_backfacing): the sets of the search without it
    bool tile_list = true;    // RT_TILE_LIST=0: no tile lists (the queue hands out every tile and the masked ones are
                              // filled there, tile_lists.hpp)
    int cut_budget = W_CUT_BUDGET;  // RT_TILE_MASK_CUT=n (4 .. 65536): the largest cut the mask is computed from
    bool ocone = true;        // RT_OCONE=0: no origin cones (reflection queries always run case (b), ocone.hpp)
    int ocone_dim = 128;      // RT_OCONE_DIM=n: the origin-cone grid's cells along the scene's longest axis
    int inject_fail = 0;      // RT_INJECT_FRAME_FAIL=k (tests): the k-th ray_trace fails after its image start
    bool gpu_build = false;   // RT_GPU_BUILD=1 / rt_set_device_build: the octree is built on the device
                              // (octree_gpu.hpp; the same bytes as the host build)
    bool gpu_xform = true;    // RT_GPU_XFORM=0: with the device build on, set_object_transform still transforms
                              // the host copy and uploads it (else: the resident positions, geom_gpu.hip)
    bool async_accel = true;  // RT_ASYNC_ACCEL=0: the leaf cones / slabs and the wide BVH are built
                              // before the first frame instead of beside it
    bool accel_hold = false;  // RT_ACCEL_HOLD=1 (tests): frames keep the quick wide BVH until rt_finish_accel
                              // adopts the background's SAH tree
    bool accel_defer = false; // RT_ACCEL_DEFER=1 / rt_set_accel_deferred: a geometry change does not start the
                              // background build; rt_finish_accel, or the switch turned off, does
    static Knobs from_env();
};

// The shaded ray query's arguments as one value (rt_trace_ray_device's, in its order): n rays in memory of the
// renderer's device at current_recursion_depth 'depth', ray i keyed as pixel first_ray + i.  Every output but rgba
// may be null; counts (null or int64[2]) += the call's shadow and reflection rays.
struct ShadeRays {
    const float *orig, *dir;   // [n][3]
    int64_t n;
    int depth;
    int64_t first_ray;
    float* rgba;               // [n][4]
    int32_t* src;
    float* t;
    uint8_t *found, *shadow;
    int64_t* counts;
    // the rays from b0 on (in 64 bits: the kernels index ints within a launch); a null output stays null
    ShadeRays from(int64_t b0) const
    {
        return {orig + 3 * b0, dir + 3 * b0, n - b0, depth, first_ray + b0, rgba + 4 * b0, src ? src + b0 : nullptr,
                t ? t + b0 : nullptr, found ? found + b0 : nullptr, shadow ? shadow + b0 : nullptr, counts};
    }
};

// What the device ray queries count (query_calls_ / query_rays_, end_ray_query).  The three shaded kinds keep the
// order of rt::SHADE_* (launch.hpp), the order rt_get_device_shaded_queries reports.
enum QueryKind {
    Q_CLOSEST,           // trace_rays_device
    Q_SHADOW,            // is_shadowed_device
    Q_SHADED_PLAIN,      // trace_ray_device by instance of shade_rays_kernel
    Q_SHADED_GENERIC,
    Q_SHADED_REFL,
    Q_BATCH_ENGINE,      // trace_ray_batch_device through the frame engine
    Q_BATCH_DELEGATED,   // ... handed to trace_ray_device's code (counted there too)
    Q_VISIBILITY_FAST,     // visibility_device by instance of visibility_kernel (the "rays": pixels)
    Q_VISIBILITY_GENERIC,
    Q_OCCLUDED,          // occluded_device
    Q_SEGMENTS,          // trace_segments_device
    Q_KINDS,
    Q_NONE = -1,         // nothing was launched for the scene's rays: an empty call, or the fill past the depth limit
};

class Renderer {
public:
    explicit Renderer(int device);
    ~Renderer();
    int init(std::string& err);

    // ---- reference API (renderer.h) ----
    const rt_settings& render_settings() const { return s_; }
    int set_settings(const rt_settings& s);
    int set_exact(bool on);
    // the octree of the next geometry changes is built on the device (rt_set_device_build)
    void set_device_build(bool on) { knobs_.gpu_build = on; }
    int64_t device_builds() const { return device_builds_; }
    int64_t device_wide_builds() const { return device_wide_builds_; }
    int64_t device_transforms() const { return geo_.transforms(); }
    int64_t device_ingests() const { return geo_.ingests(); }
    int64_t accel_builds() const { return accel_builds_; }
    // geometry changes build the octree and the quick wide BVH only (rt_set_accel_deferred)
    void set_accel_deferred(bool on) { knobs_.accel_defer = on; }
    // set_triangles with the positions taken from memory of device_ (rt_set_triangles_device), and new
    // positions for the current triangles (rt_update_vertices_device)
    int set_triangles_device(const float* d_verts, int64_t nv, const int32_t* d_idx, const int32_t* mat,
                             const float* uv6, int64_t n, hipStream_t stream);
    int update_vertices_device(const float* d_verts, int64_t nv, const int32_t* d_idx, hipStream_t stream);
    // waits for the background build of the leaf cones / slabs and the wide BVH
    int finish_accel();
    bool exact() const { return knobs_.exact; }
    int change_render_size(int w, int h);
    int set_triangles(const float* tri9, const int32_t* mat, const float* uv6, int64_t n);
    int add_sphere(float cx, float cy, float cz, float r, int mat);
    int add_plane(float px, float py, float pz, float nx, float ny, float nz, int mat);
    int clear_geometry();
    int set_materials(const float* mats16, int n);
    int material_count() const { return (int)(mats_.size() / MAT_STRIDE); }
    int change_camera_fov(float fov);
    int change_camera_aspect_ratio(float aspect);
    int set_light_position(float x, float y, float z);
    int set_camera_transform(const float m[16]);
    int apply_transformation_to_camera(const float m[16]);
    int set_camera_matrices(const float pos[3], const float proj_inv[16], const float c2w[16]);
    void get_camera_matrices(float pos[3], float proj_inv[16], float c2w[16]) const;
    // Camera::_perspective_proj_mat / _world_to_camera_mat as the caller computed them (raster path)
    int set_camera_projection(const float proj[16], const float w2c[16]);
    // Camera::_fov / _aspect_ratio as the caller holds them (read by SSAO), matrices untouched
    int set_camera_lens(float fov, float aspect);
    int set_object_transform(const float m[16]);
    int reset_previous_transform();
    // Renderer::_triangles' positions (renderer.cpp:214-224) as they stand after every transform so far:
    // *n triangles, [n][9] into tri9 when it is not null (pending device edits are applied first)
    int get_triangles(float* tri9, int64_t* n);
    int set_texture(int slot, int w, int h, const float* rgba);
    int set_skybox(const int32_t w[6], const int32_t h[6], const float* const faces[6]);
    int reconstruct_bvh_new();
    int destroy_bvh();
    int ray_trace();
    // Renderer::raster_trace (renderer.cpp:869-1006): rasterised primary visibility,
    // trace_triangle shading (shadows / reflections through the octree)
    int raster_trace();
    int post_process();
    // Renderer::get_image (renderer.cpp:106-109); callable from another thread while this
    // handle renders (the display thread, QT/mainWindowThreads.cpp:6-23): it copies the image as
    // it stands in HBM on its own stream, so a frame in progress shows its finished tiles
    int get_image(uint32_t* argb, int32_t* w, int32_t* h);
    // Renderer::lock_image_mutex / unlock_image_mutex (renderer.h:41-42, renderer.cpp:96-104):
    // while held, no frame switches or reallocates the image (get_image takes it too)
    void lock_image() { image_mu_.lock(); }
    void unlock_image() { image_mu_.unlock(); }
    std::string display_error()
    {
        std::lock_guard<std::recursive_mutex> g(image_mu_);
        return display_err_;
    }
    // diagnostics: _z_buffer, _normal_buffer (xyz + pad) and the last SSAO pass's counts
    int get_ssao_buffers(float* z, float* n4, int32_t* ao);
    int request_aux(bool rgba, bool hit, bool shadow);
    int get_internal(uint32_t* argb, float* rgba, int32_t* hit_id, float* hit_t, uint8_t* shadow);
    int get_stats(rt_stats* out) const;

    // ---- multi-GPU strips ----
    int local_rows(int band_rows, int rank, int nranks) const;
    int render_bands_device(int band_rows, int rank, int nranks, uint32_t* d_out, hipStream_t stream);
    // the listed OUTPUT bands into consecutive local bands of d_out (cost-balanced strips, strips.py
    // assign_bands); render_bands_device is the list rank, rank + nranks, ...
    int render_band_list_device(int band_rows, const int32_t* bands, int nbands, uint32_t* d_out, hipStream_t stream);
    // per global output band, the shader cycles of its tiles in the last band launch on 'stream' (the
    // bands that launch did not render are left as they are)
    int band_costs(hipStream_t stream, double* costs, int nbands);
    // durations (ms) of the last n ray_trace_kernel launches of render_bands_device,
    // bracketed by HIP events on the launch stream (synchronises on them)
    int kernel_times(float* ms, int n);
    int band_counters(unsigned long long out[2]);
    int tile_mask(int src, uint32_t* out, int64_t cap, int32_t info[5]);   // rt_tile_mask
    int tile_lists(int src, int32_t* out, int64_t cap, int32_t info[5]);   // rt_tile_lists
    int tile_starts(int src, uint32_t* out, int64_t cap, int32_t info[3]); // rt_tile_starts
    int debug_read(uint64_t* out, int64_t n);   // diagnostic builds: the per-wave records of the last frame
    int tile_costs(uint32_t* out, int64_t n, int32_t* tiles_x, int32_t* tiles_y);   // trace_frame's last tile costs
    // the resident origin-cone grid (ocone.hpp; rt_ocone_read): its frame, and its words when out holds them
    int origin_cones(uint32_t* out, int64_t n, int32_t dims[3], float lo_ih[4]);
    // single-process multi-device rendering (rt_set_devices, multidev.hpp): render(Renderer&)
    // renders interleaved bands on every device and gathers them here with RCCL
    int set_devices(const int* ids, int n);
    bool multi_active() const { return multi_ != nullptr; }
    int render_multi();

    // BVH::intersect over n host rays (closest hit, reference semantics)
    int trace_rays(const float* orig, const float* dir, int64_t n, int32_t* id, float* t, float* u, float* v,
                   uint8_t* ret);
    // The ray queries over memory of device_, launched on the caller's stream (rt_trace_rays_device,
    // rt_is_shadowed_device): trace_rays' outputs through the frames' query, and
    // Renderer::is_shadowed (renderer.cpp:340-402) per (point, normal) pair towards 'light' (3 host floats,
    // null: the scene's).  The host does not wait for the kernel; query_fence_ follows it.
    int trace_rays_device(const float* d_orig, const float* d_dir, int64_t n, int32_t* d_id, float* d_t, float* d_u,
                          float* d_v, uint8_t* d_ret, int64_t* d_counts, hipStream_t stream);
    int is_shadowed_device(const float* d_point, const float* d_normal, int64_t n, const float* light,
                           uint8_t* d_shadowed, hipStream_t stream);
    // launches of the two kernels since rt_create and the rays given to them (rt_get_device_ray_queries)
    void device_ray_queries(int64_t calls[2], int64_t rays[2]) const;
    // The ray-segment queries (rt_occluded_device, rt_trace_segments_device): with trace_rays_device's
    // (id, t, u, v, ret) for ray i, hit_i = ret && t < d_tmax[i] (d_tmax null: +inf); the byte hit_i, or the record
    // where hit_i holds and (-1, -1, 1, 0, 0) elsewhere.  trace_rays_device's contract otherwise.
    int occluded_device(const float* d_orig, const float* d_dir, const float* d_tmax, int64_t n, uint8_t* d_occluded,
                        int64_t* d_counts, hipStream_t stream);
    int trace_segments_device(const float* d_orig, const float* d_dir, const float* d_tmax, int64_t n, int32_t* d_id,
                              float* d_t, float* d_u, float* d_v, uint8_t* d_ret, int64_t* d_counts, hipStream_t stream);
    // their launches and rays since rt_create: occluded, segments (rt_get_device_segment_queries)
    void device_segment_queries(int64_t calls[2], int64_t rays[2]) const;
    // Renderer::trace_ray (shaded) over q's rays in memory of device_, on the caller's stream (rt_trace_ray_device)
    int trace_ray_device(const ShadeRays& q, hipStream_t stream) { return shade_rays_device("trace_ray_device", q, stream); }
    // its launches and rays since rt_create by instance: plain, generic, reflective (rt_get_device_shaded_queries)
    void device_shaded_queries(int64_t calls[3], int64_t rays[3]) const;
    // trace_ray_device's arguments and per-ray results through the frame engine (rt_trace_ray_batch_device, DESIGN.md
    // 13): a scene with a reflective material, the BVH and the engine on is shaded level by level in batches of
    // 2^RT_SHADE_BATCH_LOG2 rays on the caller's stream; the host waits for the engine's counts, the call may
    // allocate, and the stream first waits for band launches and queries in flight.  Any other scene: trace_ray_device.
    int trace_ray_batch_device(const ShadeRays& q, hipStream_t stream);
    // its calls and rays since rt_create: [0] through the engine, [1] handed to trace_ray_device
    // (rt_get_device_shaded_batches)
    void device_shaded_batches(int64_t calls[2], int64_t rays[2]) const;
    // The visibility buffer of the current camera into memory of device_, on the caller's stream
    // (rt_visibility_device): per pixel of the internal image trace_ray's closest hit at depth 0 --
    // the source ray_trace leaves in hit_id, the record's t, and u / v where the source is a triangle.  Each output
    // may be null.  The ray queries' contract (query_fence_ follows the launch, the host does not wait), with a
    // slot of per-stream state (vis_slot_) that a stream's first call allocates.
    int visibility_device(int32_t* d_id, float* d_t, float* d_uv, hipStream_t stream);
    // its launches and pixels since rt_create by instance (fast, generic), and the launches that were given a tile
    // mask / entry sets (rt_get_device_visibility)
    void device_visibility(int64_t calls[2], int64_t pixels[2], int64_t used[2]) const;
    // the frames' wide-BVH query and its status over n host rays (rt_wide_query)
    int wide_query(const float* orig, const float* dir, int64_t n, int kind, float* o_out, float* d_out,
                   int32_t* status, int32_t* id, float* t, float* u, float* v, uint8_t* shadow);
    // the risk words for the current camera / light: src 0 the GPU's, 1 the host walk's (rt_risk_words)
    int risk_words(int src, uint64_t* out, int64_t cap, int64_t* count, int64_t* violations);
    // Renderer::trace_ray (shaded) over n host rays at current_recursion_depth 'depth'
    int trace_ray_colors(const float* orig, const float* dir, int64_t n, int depth, float* rgba, int32_t* src,
                         float* t, uint8_t* found, uint8_t* shadow);

    const std::string& error() const { return err_; }

private:
    int fail(int code, const std::string& msg);
    int hip_fail(hipError_t e, const char* what);
    void render_size(int& w, int& h) const;
    void update_camera_projection();
    int ensure_device_scene();
    // a geometry change on the lead (a helper's: adopt_from_lead) and its steps, in order
    int rebuild_geometry();
    int build_octree(int64_t n, bool& dev_built);
    int upload_octree_tables(bool dev_built, hipError_t& e);
    int build_quick_wide(bool dev_built, hipError_t& e);
    int upload_materials();
    int upload_textures();
    int validate() const;
    void fill_params(KParams& P) const;
    // the trace of one launch: the ray-trace kernel, or the reflection engine (frames by level)
    int launch_trace(const KParams& P, hipStream_t stream);
    // the raster path of one launch: clip + piece table, z-keys, shading, then the
    // reflection engine for the reflective pixels
    int launch_raster(const KParams& P, hipStream_t stream);
    int launch_frame(const KParams& P, hipStream_t stream)
    {
        return s_.hybrid_rasterization_tracing ? launch_raster(P, stream) : launch_trace(P, stream);
    }
    int check_frame() const;
    int launch_ssao();
    int trace_frame();
    int refl_level(const KParams& P, int level, int nframes, hipStream_t stream);
    // level 1 around the launch's shading pass: its frame buffer and zeroed count, then the count and refl_level
    int refl_level1_begin(const KParams& P, hipStream_t stream);
    int refl_level1_finish(const KParams& P, hipStream_t stream, const char* what, bool run_empty);
    // frames in flight (render_bands_device) and ray queries in flight on the callers' streams: make
    // 'stream' wait for every live slot's last launch and the last query, or the host for all of them
    // (before buffers that launches read are replaced)
    int wait_slots(hipStream_t stream);
    int sync_slots();
    // The device ray queries (trace_rays_device, is_shadowed_device, trace_ray_device).  query_fence_ follows the
    // last launch on any stream: fence_stream_ runs in order, so the last record() comes after every earlier one.
    Fence query_fence_;
    int64_t query_calls_[Q_KINDS] = {}, query_rays_[Q_KINDS] = {};
    int64_t vis_used_[2] = {};   // visibility launches given a tile mask, entry sets
    // before a query launch on 'stream': the count and the pointers (n_required of them must not be null when
    // n > 0; each must be memory of device_; nptrs 0: the renderer's own staging buffer, nothing to check), the
    // scene as a frame brings it up to date (shaded: validated first, with rt_trace_ray's codes and texts), P with
    // its risk words (reads_scene false: neither; the launch reads nothing of the scene)
    int begin_ray_query(const char* what, const void* const* ptrs, int nptrs, int n_required, int64_t n,
                        hipStream_t stream, KParams& P, bool shaded = false, bool reads_scene = true);
    // after it: the fence and the counters
    int end_ray_query(QueryKind kind, int64_t n, hipStream_t stream);
    // The start the shaded queries share ('what': the caller's name in the error texts): the argument checks,
    // begin_ray_query, and past the depth limit the fill.  launch: rays are left for the caller to shade.
    // staged: q is the host call's staging buffer (trace_ray_colors, which has checked its own arrays)
    int begin_shaded_query(const char* what, const ShadeRays& q, hipStream_t stream, KParams& P, bool& launch,
                           bool staged = false);
    // trace_ray_device under the caller's name; *kind: what it counted (Q_SHADED_*, or Q_NONE).  staged: the host
    // call's launch, which waits for the stream itself and is no device query -- never the plain instance, no
    // fence, nothing counted
    int shade_rays_device(const char* what, const ShadeRays& q, hipStream_t stream, QueryKind* kind = nullptr,
                          bool staged = false);
    // trace_ray_batch_device's engine passes over the batches (the fence follows, whatever they return)
    int shade_batches(KParams& P, const ShadeRays& q, hipStream_t stream);

    Knobs knobs_;
    int device_;
    // scene versions (bumped with the dirty flags): what a multi-device helper has mirrored
    uint64_t geom_ver_ = 0, mats_ver_ = 0, tex_ver_ = 0;
    uint64_t mir_geom_ = ~0ull, mir_mats_ = ~0ull, mir_tex_ = ~0ull;   // a helper: the lead's versions copied
    // The acceleration structures beside the octree: built on accel_thread_ after
    // the octree is uploaded, adopted by the first frame that starts after they are resident;
    // until then frames take the exact octree path (same results).
    std::thread accel_thread_;
    std::atomic<int> accel_state_{0};   // 0 idle, 1 building, 2 the tree built (the origin cones may follow), 3 failed
    std::atomic<bool> oc_done_{false};  // the background thread has finished (the origin cones included)
    bool tree_pending_ = false;         // the background's tree not adopted yet
    float oc_ms_ = 0.0f;                // the origin cones' build (background, after the tree)
    std::string accel_err_;
    hipStream_t accel_stream_ = nullptr;
    hipStream_t fence_stream_ = nullptr;   // every Fence's 'done' event is recorded here
    float accel_ms_[3] = {};            // cones + slabs, wide BVH, wide-BVH upload (background)
    bool cones_ready_ = false, wide_ready_ = false, lslab_ready_ = false;
    int wide_tree_ = 0;   // rt_stats.wide_tree: 0 none, 1 the quick tree, 2 the SAH tree, -1 its build failed
    uint64_t accel_ver_ = 0;   // bumped by install_wide: what a helper has copied (mir_accel_)
    // The one place a tree becomes resident (wide_, already written: the quick tree after a geometry change,
    // the SAH tree at adoption, a helper's copy of its lead's; wide_.nn == 0: the build left none).  Sets
    // wide_ready_ and wide_tree_ (tree, or 0 without one), sizes the risk buffer, invalidates what was derived
    // from the tree before (the risk words, the scene bound's root, the tile mask's cut), bumps accel_ver_.
    int install_wide(int tree);
    // The one place the geometry's acceleration structures are dropped (a geometry change, on the lead and on
    // a helper): frames take the exact octree path until the next install_wide.
    void drop_accel();
    void start_accel();
    // release: adopt even under RT_ACCEL_HOLD (rt_finish_accel, and before the geometry is replaced)
    int poll_accel(bool wait, bool release = false);
    int mirror_from(Renderer& lead);
    // a multi-device helper (rt_set_devices): the lead builds the octree, the leaf cones / slabs
    // and the wide BVH once; a helper copies the lead's device buffers to its own device
    const Renderer* lead_ = nullptr;
    uint64_t mir_accel_ = ~0ull;   // the lead's accel_ver_ copied
    int adopt_from_lead();
    int64_t host_builds_ = 0;      // host octree builds (rt_stats host_builds, helpers included)
    // the device octree build (knobs_.gpu_build): its temporaries and totals
    int64_t device_builds_ = 0;    // device octree builds (rt_get_device_builds)
    std::unique_ptr<OctreeGpuScratch> oct_gpu_;
    DevBuf d_oct_info_;
    // builds oct_ and d_nodes_ / d_tris_ / d_tri_id_ on the device; built stays false when the
    // builder does not take the input (the caller builds on the host)
    int build_octree_device(int64_t n, bool& built);
    // the quick wide BVH of a device-built octree, built there too (wbvh_quick_gpu.hpp):
    // wide_ written in place.  wb_ then stays empty (wb_on_device_) until a host reader asks for it
    // (host_wide: one download).
    int64_t device_wide_builds_ = 0;
    std::unique_ptr<OctreeDevInfo> oct_dev_info_;   // the last device octree build's totals
    std::unique_ptr<WQuickGpuScratch> wq_gpu_;
    bool wb_on_device_ = false;
    WStats wb_dev_stats_;
    int build_wide_device(bool& built);
    int host_wide();
    // The triangles: count, positions (host and / or device, with the queued object edits) and attributes
    // (tri_geometry.hpp; where the positions are: tri_state.hpp).  Its calls marked [slots]
    // come after sync_slots().
    TriGeometry geo_;
    // the geometry changed: the next frame rebuilds (geom_ver_: what a helper has mirrored)
    void touch_geometry() { geom_dirty_ = true, ++geom_ver_; }
    // geo_'s host copy, brought up to date (object edits queued for the device run first)
    int host_tris(const std::vector<float>*& tri);
    int ingest_positions(const float* d_verts, int64_t nv, const int32_t* d_idx, int64_t n, hipStream_t stream);
    // Deferred refinement (rt_set_accel_deferred): the resident octree has had no background build started
    bool unrefined_ = false;
    int64_t accel_builds_ = 0;        // start_accel calls (rt_get_accel_builds)
    struct MultiDev;
    std::unique_ptr<MultiDev> multi_;
    int num_cus_ = 256;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
    std::string err_;

    rt_settings s_;

    // scene (host copies; the reference Renderer copies its inputs too)
    std::vector<int32_t> shape_kind_;
    std::vector<float> shape_;
    std::vector<int32_t> shape_mat_;
    std::vector<float> mats_;
    float cam_pos_[3] = {0, 0, 0};
    float fov_ = 45.0f, near_ = 0.1f, far_ = 1000.0f, aspect_ = 1.0f;
    float proj_[16], proj_inv_[16], c2w_[16], w2c_[16];
    float light_[3] = {3, 3, 2};
    float prev_object_[16];
    HostTex tex_[TEX_SLOTS];
    HostTex sky_[6];
    bool has_bvh_ = false;   // Renderer::_bvh holds a built tree

    // device state
    FlatOctree oct_;
    // what the frames read of the octree on the host (a helper gets the lead's)
    int64_t oct_nn_ = 0, oct_nt_ = 0;
    int oct_levels_ = 0;
    GNode oct_root_{};
    OctreeStats oct_stats_{};
    bool has_uv_dev_ = false;   // d_tri_uv_ holds texcoords
    bool geom_dirty_ = true, mats_dirty_ = true, tex_dirty_ = true;
    DevBuf d_nodes_, d_tris_, d_tri_id_, d_tri_mat_, d_tri_uv_, d_mats_;
    DevBuf d_tex_[TEX_SLOTS], d_sky_[6];
    DevBuf d_internal_, d_image_, d_rgba_, d_hit_id_, d_hit_t_, d_shadow_, d_counters_;
    // SSAO: _z_buffer, _normal_buffer (float4) and the occlusion counts of the internal image
    DevBuf d_zbuf_, d_nbuf_, d_ao_;
    // leaf normal cones, [4] per GTri slot (renderer.cpp leaf_cones)
    std::vector<float> cones_;
    DevBuf d_cones_;
    // leaf slabs, [8] per GTri slot (renderer.cpp leaf_slab)
    std::vector<float> lslab_;
    DevBuf d_lslab_;
    std::vector<float> lsin_;   // per leaf (at its first slot): <= sin(angle at a) of its triangles
    DevBuf d_lsin_;
    // the resident wide BVH (wbvh.hpp): its host copy and its device buffers
    WBvh wb_;
    WideDev wide_;
    // the background build's (start_accel: accel_thread_ writes only these), swapped in at adoption
    // (poll_accel): the resident tree may be the quick one (wbvh.hpp build_wbvh_quick) that frames in flight
    // still read
    WBvh wb_next_;
    WideDev wide_next_;
    // the origin cones (ocone.hpp) of the resident SAH tree's triangles and the background build's
    OConeGrid ocg_, ocg_next_;
    DevBuf d_ocone_, d_ocone2_, d_oc_ent_, d_oc_todo_;
    bool ocone_ready_ = false;
    float risk_cap_dir_[2][3] = {};   // the risk caps' directions of the resident words (camera, light)
    // a wide BVH's upload into d on 'stream' (the gather of its triangle records and metadata from the
    // resident octree tables on the device)
    hipError_t upload_wide(const WBvh& w, WideDev& d, hipStream_t stream);
    int reserve_risk(size_t nodes);
    // the grazing-risk keys (KParams::wrisk; the buffer's layout: wide_layout.hpp), and the camera / light /
    // structure they were computed for; risk_fence_ follows their launch
    DevBuf d_wrisk_;
    bool risk_valid_ = false;
    // the resident wide BVH's root, for the scene bound (prepare_risk); false after every change of tree
    WNode sb_root_{};
    bool sb_root_valid_ = false;
    float risk_cam_[3] = {0, 0, 0}, risk_light_[3] = {0, 0, 0};
    float risk_G_ = 0.0f, risk_nl_ = 0.0f, risk_nu_ = 0.0f;
    Fence risk_fence_;
    // sets P.wrisk (and risk_G / risk_nl) for the frame's camera and light, recomputing the bits on
    // 'stream' when they changed; every launch that reads them waits for their computation
    int prepare_risk(KParams& P, hipStream_t stream);
    // the tile mask (wbvh.hpp wbvh_mask_rect): the resident tree's cut (d_cut_: 2 W_CUT_MAX + 1
    // words; false after every change of tree, as sb_root_valid_; cut_fence_ follows its computation, as
    // risk_fence_ the risk words') and, per launching stream, the mask of that stream's last camera: a launch
    // computes its mask on its own stream, so a moving camera does not make the frames in flight wait for
    // each other.  mask_last_: the mask the last launch was given (nullptr: none).
    struct MaskSlot {
        DevBuf words;
        // the blocks' entry sets (bh x bw uint4) from the words, computed at the stream's second
        // launch in a row with the same camera and cut (a camera that moves every launch never pays for them)
        DevBuf starts;
        bool starts_valid = false;
        uint32_t launches = 0; // the stream's launches in a row with these words
        WMaskCam cam{};        // the camera the words were computed for
        uint64_t cut_gen = 0;  // and the cut (0: no words yet)
        // the tile lists (tile_lists.hpp) of the stream's last launch with lists, behind the words
        // in the same allocation (at list_off 4-byte words; KParams::list_off): rebuilt on the stream when the
        // words were recomputed or the launch's layout (list_key, L: its band map on the device) changed
        bool lists_valid = false;
        uint64_t list_key = 0;
        int32_t list_off = 0;
        TileLayout L{};
        // whether the stream's launches take the lists (the list kernel) or leave them (the plain kernel): decided
        // once per resident tree from a launch's own figures, read back behind it without a wait (probe_lists):
        // -1 not decided yet (the lists are taken), 1 taken, 0 left
        int list_use = -1;
        uint64_t use_gen = 0;        // the cut the decision (or its absence) belongs to
        uint32_t list_launches = 0;  // launches given lists while undecided
        bool probe_pending = false;
        struct Probe {               // pinned: the launch's tile-cost sum and max, then the two list counts
            unsigned long long* host = nullptr;
            hipEvent_t ev = nullptr;
            ~Probe()
            {
                if (host) hipHostFree(host);
                if (ev) hipEventDestroy(ev);
            }
        } probe;
    };
    // The lists pay where the tickets they remove are a visible share of the launch's work: a removed ticket is
    // worth about LIST_TICKET_CYCLES wave-cycles (C4: ~3,300 in the masked tile's body, ~6,500 of dequeue, DESIGN.md
    // 5.14); below LIST_MIN_SHARE of the launch's tile cycles the list queue costs more than it saves (hair1m:
    // 0.6% estimated, 0.8% lost; C4: 15%, 4.8% won).
    static constexpr unsigned long long LIST_TICKET_CYCLES = 10000;
    static constexpr unsigned long long LIST_MIN_SHARE_INV = 50;   // 2%
    int probe_lists(const KParams& P, hipStream_t stream);
    MaskSlot* lists_slot_ = nullptr;   // the slot whose lists the launch in preparation was given
    DevBuf d_cut_;
    bool cut_valid_ = false, mask_seen_ = false;
    uint64_t cut_gen_ = 0;
    MaskSlot mask_main_;       // rt_ray_trace's (stream_)
    MaskSlot* mask_last_ = nullptr;
    bool lists_last_ = false;  // the last launch was given tile lists (mask_last_'s)
    bool starts_last_ = false; // the last launch was given entry sets (mask_last_->starts)
    Fence cut_fence_;
    // visibility (visibility_device): the mask and the entry sets alone, under the visibility kernel's weaker
    // condition (a wide tree, enable_bvh, no analytic shape: nothing of the shading matters), and nothing of what
    // the frames' getters report (mask_last_, starts_last_, lists_last_, lists_slot_, mask_seen_) moves
    int prepare_mask(KParams& P, hipStream_t stream, MaskSlot& M, uint64_t layout_key = 0, bool visibility = false);
    DevBuf d_dbg_;                          // diagnostic per-wave records (RT_DEBUG_WAVES)
    bool ssao_ready_ = false;   // the buffers hold the last frame's z / normals
    // raster path: per-triangle piece counts / offsets, the piece table and its texcoords, the z-key
    // buffer, the big-piece list, scan scratch (the caller-order triangles: geo_)
    DevBuf d_rcount_, d_roff_, d_pieces_, d_piece_uv_, d_zkey_, d_big_, d_scan_tmp_;
    bool want_rgba_ = false, want_hit_ = false, want_shadow_ = false;
    bool aux_valid_ = false;
    // current image (Renderer::_image): internal from the start of ray_trace, downscaled after
    // post_process.  image_mu_ (Renderer::_image_mutex) guards these fields and the image
    // buffers' (re)allocation against get_image on a display thread, which copies on its own
    // non-blocking stream through a pinned staging buffer.
    std::recursive_mutex image_mu_;
    hipStream_t display_stream_ = nullptr;
    hipEvent_t display_ev_[8] = {};   // get_image's chunks (renderer.cpp get_image)
    void* display_host_ = nullptr;
    size_t display_bytes_ = 0;
    std::vector<void*> display_old_;   // outgrown staging buffers (freed with the renderer)
    int frames_started_ = 0;           // (RT_INJECT_FRAME_FAIL)
    std::string display_err_;   // get_image's last failure (err_ belongs to the owning thread)
    // the image becomes the internal buffer of a frame about to launch (trace_frame)
    int begin_internal_image(int rw, int rh);
    int img_w_ = 0, img_h_ = 0;
    bool img_is_internal_ = false;
    bool rendered_ = false;

    // reflection engine buffers, per level (frames, results, chunk samples / hits, child counter)
    struct ReflLevel {
        DevBuf fr, ret, sm, hit, cnt, list, sort, sort_tmp, res, frs, slist;
    };
    static constexpr int REFL_LEVELS = 18;   // max_recursion_depth <= 15: frames at levels 1..16, +1 child slot
    ReflLevel refl_[REFL_LEVELS];

    // render_bands_device: per-stream tile-queue counters and SSAA band buffers, so that
    // frames launched on different streams can be in flight together.  Each
    // slot owns an event recorded after its last launch: launches that use buffers shared
    // across launches (reflection engine, raster path) and scene uploads wait on every
    // slot's fence, never on a stored stream handle (the caller may have destroyed it).
    // heavy tiles first (KParams::tile_cost / heavy_list): the last launch's tile costs of a layout
    struct TileCost {
        DevBuf cost, heavy;
        uint64_t key = 0;
        int ntiles = 0, tiles_x = 0, tiles_y = 0;   // the last launch's layout
        uint32_t parity = 0;   // which of the two tile-cost sums the last launch accumulated
        // its bands (band_costs): output rows per band, the SSAA factor, and the global band of each
        // local band
        int band_rows = 0, ssaa = 1;
        std::vector<int32_t> bands;
    };
    int prepare_heavy(KParams& P, TileCost& T, hipStream_t stream, uint64_t layout_key = 0, bool* zeroed = nullptr,
                      bool overlapped = false);
    int render_bands_impl(int band_rows, int rank, int nranks, const int32_t* bands, int nbands, uint32_t* d_out,
                          hipStream_t stream);
    const TileCost* last_tc_ = nullptr;   // the last launch's (rt_tile_costs)
    TileCost tc_main_;   // trace_frame's launches (stream_)
    struct BandSlot {
        hipStream_t stream = nullptr;
        DevBuf counters, tmp;
        TileCost tc;
        Fence fence;                 // follows the slot's last launch
        DevBuf map;                  // the band list of the slot's last list launch: map, then inverse
        std::vector<int32_t> map_host;
        int map_nb = 0;              // global bands of that list's image
        uint64_t used = 0;   // band_uses_ at the slot's last launch (least recently used is recycled)
        MaskSlot mask;       // the tile mask of the slot's last camera
    };
    static constexpr int BAND_SLOTS = 8;
    BandSlot band_slot_[BAND_SLOTS];
    int band_nslots_ = 0, band_last_ = -1;
    uint64_t band_uses_ = 0;
    // visibility_device: per launching stream the tile queue's counter block and the mask of that stream's last
    // camera, so that launches on different streams run concurrently; none of it is the band slots' (band_last_,
    // the tile costs and the slots' masks belong to frames).  vis_slots.hpp picks the slot.
    struct VisSlot {
        hipStream_t stream = nullptr;
        DevBuf counters;
        MaskSlot mask;
        Fence fence;         // follows the slot's last launch
        uint64_t used = 0;   // vis_uses_ at the slot's last launch
    };
    VisSlot vis_slot_[VIS_SLOTS];
    int vis_nslots_ = 0;
    uint64_t vis_uses_ = 0;
    // event ring for render_bands_device kernel timing
    static constexpr int EV_RING = 256;
    std::vector<hipEvent_t> ring_;
    int ring_next_ = 0, ring_count_ = 0;

    // stats
    int64_t last_primary_ = 0, last_shadow_ = 0, last_refl_ = 0;
    float last_seg_ = 0;   // KParams::seg_scale of the last frame
    int64_t last_work_[8] = {};   // RT_COUNT builds: counters[4..7], [10..12], [14] of the last frame (executed
                                  // k-DOP / MT tests: whole-line, segment; wide-BVH nodes, triangles, uncertified,
                                  // certificates)
    int64_t last_wave_[6] = {};     // RT_COUNT builds: counters[22..27], wide-BVH loop iterations (rt_stats)
    int64_t last_uncert_[6] = {};   // RT_COUNT builds: uncertified wide-BVH queries by reason
    void take_counters(const unsigned long long* cnt);
    float kernel_ms_ = 0, post_ms_ = 0, build_ms_ = 0;
    float build_split_ms_[4] = {};   // octree, leaf cones + slabs, wide BVH, upload
};

// render(Renderer&) (tp2/projets/utils/mainUtils.cpp:6-21): ray_trace then post_process;
// returns the elapsed milliseconds (*rc gets the status; on an error the remaining
// steps are skipped); raster_trace instead of ray_trace when hybrid_rasterization_tracing.
float render(Renderer& renderer, int* rc = nullptr);

}  // namespace rt
