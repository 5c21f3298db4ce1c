/*
 * rt_mi355x.h -- C ABI of the MI355X-native primary-ray + shadow-ray renderer
 * (librt_mi355x.so).  Drop-in for the hot path of TomClabault/RayTracerCPP:
 * each entry point replaces one member of the reference's Renderer class
 * (tp2/projets/renderer/renderer.h:20-355) or one free function it depends on;
 * the reference interface is cited next to each declaration.
 *
 * Conventions
 *   - plain pointers + sizes, no C++ types; every function is synchronous;
 *   - matrices are 16 floats, row-major (Transform::m[i][j] = m[4*i+j], tp2/src/mat.h:21-71);
 *   - triangles are [n][9] floats (a.xyz b.xyz c.xyz, world space as left by
 *     MeshIOUtils::create_triangles), material indices [n] int32, optional
 *     texture coordinates [n][6] floats (u0 u1 u2 v0 v1 v2 == Triangle::_tex_coords_u/_v);
 *   - materials are [n][16] floats: ambient_coeff rgb, diffuse rgb, specular rgb,
 *     emission rgb, reflection, roughness, ns, specular_threshold (Material, tp2/src/materials.h:14-38);
 *   - images are ARGB32 (0xAARRGGBB, QImage::Format_ARGB32), row-major, row 0 = NDC y = -1;
 *   - every function returns RT_OK (0) or a negative RT_E* code; rt_last_error()
 *     gives the message of the calling thread's last failure.  No exceptions
 *     cross this boundary.  The reference has no error reporting (asserts / UB):
 *     invalid material indices, absent textures and renders without geometry
 *     are rejected here up front with RT_EINVAL.
 *   - a handle belongs to one thread at a time (as Renderer does), except that rt_get_image,
 *     rt_lock_image and rt_unlock_image may be called from a second (display) thread while the
 *     owning thread renders (DisplayThread / RenderThread, QT/mainWindowThreads.cpp:6-65).
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_EINVAL (-1)
#define RT_EHIP (-2)
#define RT_ENOMEM (-3)
#define RT_ESTATE (-4)
#define RT_EUNSUPPORTED (-5)
#define RT_EIO (-6)

/* RenderSettings::ShadingMethod (rendererSettings.h:8-25) */
#define RT_SHADING_RT 0
#define RT_SHADING_ABS_NORMALS 1
#define RT_SHADING_PASTEL_NORMALS 2
#define RT_SHADING_BARYCENTRIC 3
#define RT_SHADING_VISUALIZE_AO 4

/* texture slots: Renderer::set_{ao,diffuse,normal,displacement,roughness}_map, set_skysphere (renderer.h:77-84) */
#define RT_TEX_AO 0
#define RT_TEX_DIFFUSE 1
#define RT_TEX_NORMAL 2
#define RT_TEX_DISPLACEMENT 3
#define RT_TEX_ROUGHNESS 4
#define RT_TEX_SKYSPHERE 5

/* RenderSettings, field for field (tp2/projets/renderer/rendererSettings.h:6-105);
 * every field is honoured (SSAO: full-frame rendering only). */
typedef struct rt_settings {
    int32_t image_width, image_height;
    int32_t enable_ssaa, ssaa_factor;
    int32_t enable_clipping;
    int32_t hybrid_rasterization_tracing;   /* rt_render: raster_trace instead of ray_trace */
    int32_t shading_method;
    int32_t compute_shadows;
    int32_t max_recursion_depth;
    int32_t enable_bvh, bvh_max_depth, bvh_leaf_object_count;
    int32_t enable_ssao;                    /* post_process: SSAO before SSAA (not with rt_render_bands_device) */
    int32_t ssao_sample_count;
    float ssao_radius, ssao_amount;
    int32_t enable_ambient, enable_diffuse, enable_specular, enable_emissive;
    int32_t rough_reflections_sample_count;
    int32_t enable_ao_mapping, enable_diffuse_mapping, enable_normal_mapping, enable_displacement_mapping;
    float displacement_mapping_strength;
    int32_t parallax_mapping_steps;
    int32_t enable_roughness_mapping;
    int32_t enable_skysphere, enable_skybox;
    uint32_t rng_seed;                      /* counter-based rough-reflection RNG seed (no reference equivalent) */
} rt_settings;

/* Per-render statistics (no reference equivalent; Renderer prints timings only). */
typedef struct rt_stats {
    int64_t primary_rays;      /* render_w * render_h of the last ray_trace */
    int64_t shadow_rays;       /* one per shaded hit with compute_shadows */
    int64_t reflection_rays;
    float kernel_ms;           /* GPU time of the last ray_trace kernel (HIP events) */
    float post_ms;             /* GPU time of the last post_process */
    float build_ms;            /* the last geometry change's blocking part: octree build + flatten + upload */
    int64_t octree_inner, octree_leaves, octree_empty_leaves, octree_max_leaf, octree_max_depth;
    int64_t gpu_nodes, gpu_tris;
    int32_t render_width, render_height;
    float seg_scale;           /* scene scale of the last frame's segment queries (kernels.hip seg_margin);
                                  0: shadow / reflection queries walked the whole line */
    int64_t work[4];           /* diagnostic builds (-DRT_COUNT=1) only, else 0: the last frame's k-DOP and
                                  Moller-Trumbore tests of whole-line queries, then of segment queries */
    int64_t work_wide[4];      /* diagnostic builds only: wide-BVH node visits, triangle tests, the queries it could
                                  not certify (traced through the octree instead), and the
                                  certificates' octree k-DOP tests */
    int64_t uncertified[6];    /* diagnostic builds only: uncertified wide-BVH queries by reason -- stack overflow,
                                  NaN hit, only overflowed hits, tie, minimum t outside (0, inf), failed
                                  certificate */
    int64_t wave_steps[6];     /* diagnostic builds only: wide-BVH traversal loop iterations of primary queries --
                                  summed over waves (each wave's longest lane), summed over lanes, wave calls --
                                  then the same for shadow queries (SIMD efficiency = lanes / (64 waves)) */
    float build_split_ms[4];   /* the last scene build, host milliseconds: octree build + flatten; leaf cones and
                                  slabs, and the wide BVH with its upload (both on the background thread,
                                  rt_finish_accel; 0 until adopted); the octree's upload */
    int64_t host_builds;       /* host octree builds since rt_create, over every device of rt_set_devices (its
                                  helpers copy the lead's build: one per geometry change, renderer.cpp:214-224) */
    int32_t wide_tree;         /* the wide BVH serving frames: 0 none (octree walk), 1 the quick tree built with the
                                  octree, 2 the SAH tree adopted after the background build, -1 that build failed
                                  (rt_finish_accel returned the error) and the quick tree keeps serving */
} rt_stats;

typedef struct rt_renderer rt_renderer;

/* RenderSettings() defaults (rendererSettings.h:27-102) */
void rt_default_settings(rt_settings *s);

/* Renderer::Renderer() (renderer.cpp:80): default Scene (Camera at origin, fov 45,
 * near 0.1, far 1000; PointLight (3,3,2)), RenderSettings(), no geometry.
 * device: HIP device ordinal.  Returns NULL on failure (see rt_last_error). */
rt_renderer *rt_create(int device);
void rt_destroy(rt_renderer *r);
const char *rt_last_error(void);

/* Renderer::render_settings() (renderer.h:46): read / replace the settings.
 * Replacing them re-creates the image (init_buffers, renderer.cpp:122-135) when the
 * render size changed and rebuilds the octree when the BVH parameters changed. */
int rt_get_settings(rt_renderer *r, rt_settings *out);
int rt_set_settings(rt_renderer *r, const rt_settings *s);

/* Exact mode (no reference counterpart).  on != 0: every BVH query walks
 * the octree over the whole ray line as BVH::intersect does (bvh.h:212-287), so every
 * result is the reference's by construction.  Off (default): closest hits come from the
 * wide BVH, whose child test is sound for every ray (grazing rays included, r04-r05), and
 * each answer is certified on the reference's own octree leaf; the few queries it cannot
 * certify (ties, NaN hits, overflowed stacks) walk the octree in place.  Both give the
 * same images; exact mode is slower.  Also RT_EXACT=1 at rt_create. */
int rt_set_exact(rt_renderer *r, int on);

/* Acceleration structures beside the octree (no reference counterpart): after a
 * geometry change the octree (the reference's BVH, renderer.cpp:214-224) is built and uploaded
 * before the next frame, together with a quick wide BVH (the octree's own hierarchy, O(n)); the
 * leaf cones / slabs and the SAH wide BVH are built on a background thread and replace it when
 * resident.  Frames certify their answers on either tree (the same images; without a wide BVH, as
 * in exact mode, they take the octree traversal).  rt_finish_accel waits for the background build
 * (RT_ASYNC_ACCEL=0 at rt_create: every geometry change waits for it; RT_WBVH_QUICK_FIRST=0: no
 * quick tree). */
int rt_finish_accel(rt_renderer *r);

/* Device octree build (no reference counterpart).  on != 0: after a geometry change
 * the octree is built on the GPU into the tables the frames read, and copied back for the host-side
 * structures built from it; the flattened arrays are byte for byte the host build's, so every frame
 * is the same.  Off (default): the host build.  Inputs the device builder does not take
 * (bvh_max_depth outside 0..30, more than 2^26 triangles) build on the host as before; brute-force
 * mode (enable_bvh off) never uses it.  Also RT_GPU_BUILD=1 at rt_create.
 * rt_get_device_builds: device octree builds since rt_create (rt_stats host_builds counts only the
 * host's). */
int rt_set_device_build(rt_renderer *r, int on);
int rt_get_device_builds(rt_renderer *r, int64_t *count);

/* The device builder alone: uploads tri9 ([n][9] world-space vertices) to 'device', builds and
 * flattens the octree there, copies the arrays back and returns rt_octree_digest's digest and
 * stats[7] (rt_mi355x_diag.h) of them.  ms (optional) = {the device build by HIP events, the whole
 * call on the host clock}.  RT_EUNSUPPORTED for an input the builder does not take (as above, or
 * a non-finite coordinate); RT_EHIP (rt_last_error) without a usable device. */
int rt_octree_build_device(int32_t device, const float *tri9, int64_t n, int32_t max_depth, int32_t leaf_max_obj_count,
                           uint64_t *digest, int64_t stats[7], float ms[2]);

/* The quick wide BVH on the device.  With the device build on, a rebuild whose
 * octree was built on the device also builds the quick wide BVH there, from the device-resident octree
 * into the tables the frames read: the same tree as the host's, byte for byte except the two codes
 * that go through acos / cos / sin, which may differ by one step (both sound).  Otherwise the host
 * builds it as before.  rt_get_device_wide_builds: such device builds since rt_create.
 * RT_ACCEL_HOLD=1 at rt_create (tests): frames keep the quick tree until rt_finish_accel adopts the
 * background's SAH tree. */
int rt_get_device_wide_builds(rt_renderer *r, int64_t *count);

/* The quick tree's builders alone.  rt_wbvh_quick_digest (host only): builds the octree and the quick
 * tree of tri9 on the host and returns six 64-bit FNV-1a digests (rt_octree_digest's hash): 0 the
 * nodes' exact fields (ox, oy, oz, exps, qlo, qhi, child), 1 s, slo, slab[] and bytes 0-2 of nrm[], 2
 * ext bytes 0, 1, 3 and ext2, 3 the transcendental bytes (nrm byte 3, the cone code; ext byte 2, sth),
 * 4 slot[] then leaf_of_slot[], 5 tri_leaf[] then parent[]; stats = nodes, leaves, tris, max_leaf,
 * depth; ms (optional) the two builds' time.
 * rt_wbvh_quick_build_device: the octree and the quick tree built on 'device' and downloaded: the
 * same digests and stats; check[0] = the downloaded tree's structural violations against the octree,
 * check[1] = transcendental bytes that differ from the host tree's, check[2] = the largest |code
 * difference| among them, check[3] = differing bytes elsewhere; ms (optional) = {the device quick
 * build by HIP events, the whole call}.  RT_EUNSUPPORTED / RT_EHIP as rt_octree_build_device. */
int rt_wbvh_quick_digest(const float *tri9, int64_t n, int32_t max_depth, int32_t leaf_max_obj_count, uint64_t digest[6],
                         int64_t stats[5], float *ms);
int rt_wbvh_quick_build_device(int32_t device, const float *tri9, int64_t n, int32_t max_depth,
                               int32_t leaf_max_obj_count, uint64_t digest[6], int64_t stats[5], int64_t check[4],
                               float ms[2]);

/* Object edits on the device.  With the device build on, rt_set_object_transform on a
 * handle whose positions are resident from the build before (not a helper of rt_set_devices) queues
 * its matrix; before the next build, or the next host reader of the positions (a host build,
 * brute-force mode, rt_get_triangles, a helper's copy), the queue runs on the GPU over the resident
 * positions in place, one launch per call in call order (geom_gpu.hip: Transform::operator()(Point),
 * mat.cpp:83-100, the host's expression: the same bytes), instead of a host pass and a new upload.
 * A non-finite result is reported by the next frame as the host path reports it (RT_EINVAL).
 * RT_GPU_XFORM=0 at rt_create keeps the host pass.  rt_get_device_transforms: the matrices applied
 * by the kernel since rt_create. */
int rt_get_device_transforms(rt_renderer *r, int64_t *count);

/* The kernel alone: uploads pts ([n][3]) to 'device', runs it with m and copies the points back into
 * out (which may be pts); *nonfinite = 1 when a written coordinate is not finite, else 0; ms
 * (optional) = {the kernel by HIP events, the whole call on the host clock}.  Against
 * rt_transform_points the bytes differ only where both are NaN (sign and payload).  RT_EINVAL for a
 * null pointer or n < 0; RT_EHIP (rt_last_error) without a usable device; n == 0: RT_OK, no launch. */
int rt_transform_points_device(int32_t device, const float m[16], const float *pts, int64_t n, float *out,
                               int32_t *nonfinite, float ms[2]);

/* Geometry from device memory (no reference counterpart; DESIGN.md 5.1 "Geometry input on the device").
 * rt_set_triangles_device is rt_set_triangles with the positions read from memory of the handle's device:
 * d_verts is [nv][3] floats and d_idx [n][3] int32 vertex indices, or with d_idx NULL d_verts is the
 * flat [n][9] (nv == 3 n).  mat ([n]) and uv6 ([n][6] or NULL) are host arrays as in rt_set_triangles;
 * the same limits on n; n == 0 is rt_set_triangles with n == 0 (no launch, pointers unread).
 * rt_update_vertices_device gives new positions for the current n triangles and keeps their materials
 * and texture coordinates: RT_ESTATE without geometry, or when the flat form's nv is not 3 n.
 * Neither touches the previous object transform (rt_set_object_transform composes as before).
 * hip_stream is the caller's hipStream_t (NULL: the null stream).  The call copies the positions on the
 * GPU in stream order (geom_gpu.hip, bit for bit): its kernel waits for the work queued on hip_stream
 * before the call, and hip_stream waits for the kernel, so the caller may reuse its buffers on
 * hip_stream as soon as the call returns.  The host does not wait for the GPU.
 * Both pointers must be device memory of the handle's device (hipPointerGetAttributes): else RT_EINVAL,
 * with the geometry unchanged.  A non-finite coordinate in a referenced vertex, or an index outside
 * [0, nv) (that corner becomes (0, 0, 0)), is found by the kernel and reported by the next frames with
 * RT_EINVAL until the geometry is replaced.  With the device build off the next build downloads the
 * positions once and builds on the host: the same frames.
 * rt_get_device_ingests: launches of that kernel since rt_create. */
int rt_set_triangles_device(rt_renderer *r, const float *d_verts, int64_t nv, const int32_t *d_idx, const int32_t *mat,
                            const float *uv6, int64_t n, void *hip_stream);
int rt_update_vertices_device(rt_renderer *r, const float *d_verts, int64_t nv, const int32_t *d_idx, void *hip_stream);
int rt_get_device_ingests(rt_renderer *r, int64_t *count);

/* The kernel alone on host arrays: uploads verts ([nv][3]) and idx ([n][3], or NULL for the flat form
 * with nv == 3 n) to 'device', gathers into out_tri9 ([n][9]) and copies it back; *flags bit 0: a
 * written coordinate is not finite, bit 1: an index outside [0, nv) (zeros written); ms (optional) =
 * {the kernel by HIP events, the whole call on the host clock}.  RT_EINVAL for a null pointer, a
 * negative count or a flat form with nv != 3 n; RT_EHIP (rt_last_error) without a usable device;
 * n == 0: RT_OK, no device touched. */
int rt_gather_triangles_device(int32_t device, const float *verts, int64_t nv, const int32_t *idx, int64_t n,
                               float *out_tri9, int32_t *flags, float ms[2]);

/* Deferred refinement.  on != 0: a geometry change builds what the next frame needs (the
 * octree and the quick wide BVH) and does not start the background build of the leaf cones / slabs, the
 * SAH wide BVH and the origin cones: frames stay on the quick tree (rt_stats.wide_tree 1; the octree, 0,
 * with RT_WBVH_QUICK_FIRST=0), the same images.  For geometry that changes every frame, whose
 * background build would be joined by the next change and dropped.  rt_finish_accel on a geometry not
 * refined yet starts that build, waits and adopts it; after on == 0 the next frame starts it.
 * Also RT_ACCEL_DEFER=1 at rt_create.  rt_get_accel_builds: background builds started since rt_create. */
int rt_set_accel_deferred(rt_renderer *r, int on);
int rt_get_accel_builds(rt_renderer *r, int64_t *count);

/* Single-process multi-device rendering (no reference counterpart: the reference renders on
 * one host, RenderThread::run, QT/mainWindowThreads.cpp:39-65).  ids[0] must be the handle's
 * device; n = 0 (or ids NULL) returns to one device.  rt_render then renders on every device
 * the interleaved bands of 8 output rows with band % n == its index in ids (the kernels of
 * rt_render_bands_device), sends them to ids[0] with RCCL (librccl, loaded at the first call
 * with n > 1) and re-assembles the frame there: rt_get_image returns the same image as on one
 * device.  Scene and settings changes on the handle reach the other devices before each
 * frame.  ids may instead repeat the handle's device n times (n renderers on one device, the
 * bands copied instead of sent: the same path without RCCL, for one-device machines).
 * Frames with enable_ssao render on ids[0] alone (SSAO reads across bands);
 * rt_ray_trace / rt_post_process / rt_get_internal are single-device as before.
 * The geometry is built once, on ids[0]; the other devices copy its device tables (rt_stats
 * host_builds).
 * EXPERIMENTAL: distinct device ids (the RCCL send / receive path) have not run on a multi-GPU
 * machine yet; they are refused with RT_EUNSUPPORTED unless RT_MULTIDEV_RCCL=1 is set in the
 * environment (tests/test_gpu_parity.py test_set_devices_distinct_rccl runs them where two or
 * more devices exist).  The repeated-device form is tested on every GPU run. */
int rt_set_devices(rt_renderer *r, const int32_t *ids, int32_t n);

/* Renderer::change_render_size (renderer.cpp:250-261) */
int rt_change_render_size(rt_renderer *r, int32_t width, int32_t height);

/* Renderer::set_triangles (renderer.cpp:137-144): copies, then builds the octree
 * BVH(&_triangles, bvh_max_depth, bvh_leaf_object_count) on the host, flattens
 * and uploads it.  uv6 may be NULL ((-1,-1,-1) texture coordinates). */
int rt_set_triangles(rt_renderer *r, const float *tri9, const int32_t *mat, const float *uv6, int64_t n);

/* Renderer::add_analytic_shape (renderer.cpp:146) with Sphere / Plane (analyticShape.h:20-53) */
int rt_add_sphere(rt_renderer *r, float cx, float cy, float cz, float radius, int32_t mat);
int rt_add_plane(rt_renderer *r, float px, float py, float pz, float nx, float ny, float nz, int32_t mat);

/* Renderer::clear_geometry (renderer.cpp:182-186) */
int rt_clear_geometry(rt_renderer *r);

/* Renderer::set_materials / get_materials (renderer.cpp:148-150) */
int rt_set_materials(rt_renderer *r, const float *mats16, int32_t n);
int rt_get_material_count(rt_renderer *r, int32_t *n);

/* Renderer::change_camera_fov / change_camera_aspect_ratio / set_light_position (renderer.cpp:188-190) */
int rt_change_camera_fov(rt_renderer *r, float fov);
int rt_change_camera_aspect_ratio(rt_renderer *r, float aspect);
int rt_set_light_position(rt_renderer *r, float x, float y, float z);

/* Renderer::set_camera_transform / apply_transformation_to_camera (renderer.cpp:226-241) */
int rt_set_camera_transform(rt_renderer *r, const float m[16]);
int rt_apply_transformation_to_camera(rt_renderer *r, const float m[16]);

/* Direct camera state (Camera::_position, _perspective_proj_mat_inv, _camera_to_world_mat,
 * scene/camera.h:19-30), for callers that computed the matrices themselves. */
int rt_set_camera_matrices(rt_renderer *r, const float pos[3], const float proj_inv[16], const float cam_to_world[16]);
int rt_get_camera_matrices(rt_renderer *r, float pos[3], float proj_inv[16], float cam_to_world[16]);

/* Camera::_perspective_proj_mat and Camera::_world_to_camera_mat (scene/camera.h:19-30),
 * which the raster path uses (renderer.cpp:833-838, 877-879), as the caller computed
 * them.  Default: perspective(fov, aspect) and the inverse of cam_to_world. */
int rt_set_camera_projection(rt_renderer *r, const float proj[16], const float world_to_cam[16]);

/* Camera::_fov and Camera::_aspect_ratio (scene/camera.h:22-23) as the caller holds them,
 * without recomputing any matrix: the SSAO pass reads them (renderer.cpp:1245, 1281-1282,
 * 1378-1379).  Default: the fov / aspect of the last change_camera_fov /
 * change_camera_aspect_ratio / change_render_size. */
int rt_set_camera_lens(rt_renderer *r, float fov, float aspect);

/* Renderer::set_object_transform / reset_previous_transform (renderer.cpp:212-224) */
int rt_set_object_transform(rt_renderer *r, const float m[16]);
int rt_reset_previous_transform(rt_renderer *r);
/* Renderer::_triangles' positions as rt_set_object_transform left them (renderer.cpp:214-224: every
 * vertex through object_transform x previous^-1): *n = the triangle count, and with tri9 != NULL the
 * world-space positions [n][9] in caller order, after every transform so far (object edits still
 * queued for the device, below, are applied first).  The same bytes in both build modes. */
int rt_get_triangles(rt_renderer *r, float *tri9, int64_t *n);

/* Renderer::set_*_map / set_skysphere and clear_*_map (renderer.cpp:192-205).
 * rgba: w*h*4 floats (Image texels); NULL clears the slot. */
int rt_set_texture(rt_renderer *r, int32_t slot, int32_t w, int32_t h, const float *rgba);

/* Renderer::set_skybox(Skybox(faces)) (renderer.cpp:199, skybox.h:12-16): faces
 * right, left, top, bottom, back, front. */
int rt_set_skybox(rt_renderer *r, const int32_t w[6], const int32_t h[6], const float *const faces[6]);

/* Renderer::reconstruct_bvh_new / destroy_bvh (renderer.cpp:243-248) */
int rt_reconstruct_bvh_new(rt_renderer *r);
int rt_destroy_bvh(rt_renderer *r);

/* Renderer::ray_trace (renderer.cpp:1068-1116): renders the render_w x render_h
 * internal image on the GPU (synchronous). */
int rt_ray_trace(rt_renderer *r);

/* Renderer::raster_trace (renderer.cpp:869-1006): the hybrid path -- primary visibility
 * by rasterising the clipped triangles (z-buffer; the sequential z-test's winner, first of
 * equal z), shading by trace_triangle (shadow and reflection rays through the octree).
 * Reflective materials need enable_bvh (RT_EUNSUPPORTED otherwise).  Same outputs as
 * rt_ray_trace: hit_id = the winning triangle, hit_t = its z-buffer depth. */
int rt_raster_trace(rt_renderer *r);

/* Diagnostics (no reference equivalent; Renderer::_z_buffer / _normal_buffer are private,
 * renderer.h:319-320): the internal-size z buffer, the normal buffer as 4 floats per pixel
 * (xyz, 0) and the occlusion counts of the last SSAO pass; any pointer may be NULL. */
int rt_get_ssao_buffers(rt_renderer *r, float *z, float *n4, int32_t *ao);

/* Renderer::post_process (renderer.cpp:1118-1124): post_process_ssao_SIMD (renderer.cpp:
 * 1229-1434) on the internal image when enable_ssao, then the SSAA downscale when enabled.
 * The z / normal buffers SSAO reads are those of the last rt_ray_trace / rt_raster_trace,
 * cleared before each (mainwindow.cpp:184-185); RT_ESTATE if that frame had SSAO off. */
int rt_post_process(rt_renderer *r);

/* Renderer::get_image (renderer.cpp:106-109): copies the current image
 * (image_width x image_height after post_process) to argb; w/h receive its size.
 * Progressive readback: from the start of a ray_trace / raster_trace the image is the frame's
 * internal (render_w x render_h) buffer, which the GPU fills tile by tile, as the reference's
 * ray_trace fills _image pixel by pixel.  Called from a display thread while the owning thread
 * renders, rt_get_image returns the image as it stands (finished tiles of the frame in progress,
 * elsewhere the previous frame or, for a re-created image -- size change, SSAA frame -- the
 * BACKGROUND_COLOR fill); it does not wait for the frame.  Frames rendered with rt_set_devices
 * appear whole, after their gather. */
int rt_get_image(rt_renderer *r, uint32_t *argb, int32_t *w, int32_t *h);

/* Renderer::lock_image_mutex / unlock_image_mutex (renderer.h:41-42, renderer.cpp:96-104): while a
 * thread holds the image lock, no frame of the handle switches or re-creates the image (the start
 * of a frame and post_process's SSAA swap wait for it); rt_get_image takes it too (recursive). */
int rt_lock_image(rt_renderer *r);
int rt_unlock_image(rt_renderer *r);

/* render(Renderer&) (utils/mainUtils.cpp:6-21): raster_trace (hybrid_rasterization_tracing)
 * or ray_trace, then post_process;
 * *ms receives the wall time in milliseconds (may be NULL). */
int rt_render(rt_renderer *r, float *ms);

/* Parity / debug buffers of the last ray_trace at internal resolution
 * (render_w x render_h); any pointer may be NULL.  Requesting them before the
 * render (rt_request_aux) makes the kernel write them. */
int rt_request_aux(rt_renderer *r, int32_t want_rgba, int32_t want_hit, int32_t want_shadow);
int rt_get_internal(rt_renderer *r, uint32_t *argb, float *rgba, int32_t *hit_id, float *hit_t, uint8_t *shadow);

int rt_get_stats(rt_renderer *r, rt_stats *out);

/* Image-strip rendering for multi-GPU (one process per GPU): renders the bands of
 * band_rows OUTPUT rows with band % nranks == rank into the device buffer d_out
 * (image_width x local_rows(...) ARGB32, final resolution, SSAA applied) on the
 * given HIP stream (NULL = the handle's stream).  Does not synchronise.
 *
 * Stream contract.  Every write to d_out is enqueued on hip_stream and ordered only by it:
 *   - the caller orders any earlier work on d_out (fills, copies, reads of the previous frame)
 *     before this call on hip_stream, e.g. with hipStreamWaitEvent; work that touches d_out
 *     on another stream afterwards must wait for an event recorded on hip_stream after this call;
 *   - launches on different streams may run concurrently (frames in flight); each stream has
 *     its own tile-queue counters and band buffer (up to 8 streams, the least recently used is
 *     recycled once its last launch is done);
 *   - the library orders its own shared state: a launch that uses buffers shared across
 *     launches (reflection engine, raster path) waits for every launch still in flight, and a
 *     scene, material or texture change waits for them on the host before it is uploaded. */
int rt_local_rows(rt_renderer *r, int32_t band_rows, int32_t rank, int32_t nranks, int32_t *rows_out);
int rt_render_bands_device(rt_renderer *r, int32_t band_rows, int32_t rank, int32_t nranks, uint32_t *d_out,
                           void *hip_stream);
/* Cost-balanced strips: renders the listed OUTPUT bands (bands[i] in [0, ceil(image_height /
 * band_rows)), each at most once) into d_out, local band i = rows [i * band_rows, (i + 1) *
 * band_rows) of an image_width x (nbands * band_rows) ARGB32 buffer; otherwise as
 * rt_render_bands_device (which renders the list rank, rank + nranks, ...), same stream contract.
 * A list that differs from the stream's previous one waits for that stream's last launch. */
int rt_render_band_list_device(rt_renderer *r, int32_t band_rows, const int32_t *bands, int32_t nbands,
                               uint32_t *d_out, void *hip_stream);
/* The cost of each OUTPUT band in the last band launch on hip_stream (NULL = the handle's stream):
 * the shader cycles of its 8x8 tiles (a tile is charged to the band of its first row), written to
 * costs[global band] for the bands that launch rendered; the others are left as they are, so that
 * ranks can sum their vectors.  Waits for that launch.  nbands >= ceil(image_height / band_rows).
 * RT_EINVAL before a band launch that records tile costs (reflections, raster, RT_HEAVY_FIRST=0). */
int rt_band_costs(rt_renderer *r, void *hip_stream, double *costs, int32_t nbands);

/* BVH::intersect (bvh.cpp:68-71; OctreeNode::intersect, bvh.h:212-287) for n arbitrary
 * rays (origins / directions [n][3]): the closest-hit query trace_ray and is_shadowed
 * issue, with the reference's visit order.  Outputs per ray: triangle index of the
 * query's HitInfo (-1 none), its t / u / v, and the boolean BVH::intersect returned.
 * Uses the brute-force loop when enable_bvh is 0. */
int rt_trace_rays(rt_renderer *r, const float *orig, const float *dir, int64_t n, int32_t *tri_id, float *t,
                  float *u, float *v, uint8_t *ret);

/* Ray queries on device memory (no reference counterpart).
 * rt_trace_rays_device is rt_trace_rays with every array in memory of the handle's device: d_orig / d_dir
 * [n][3] floats in, d_tri_id / d_t / d_u / d_v / d_ret [n] out.  Per ray it writes exactly what rt_trace_rays
 * writes for that ray in the same renderer state (the caller's triangle index or -1, the record's t / u / v --
 * -1, 1, 0 for a miss the wide BVH certifies -- and the boolean BVH::intersect returned), in every mode: the
 * resident wide BVH (quick or SAH tree), before one is resident, exact mode, RT_WBVH=0, enable_bvh 0.  It
 * takes the frames' query (the certified wide-BVH query, the exact octree walk for what that cannot certify;
 * DESIGN.md 5.6), where rt_trace_rays walks the octree for every ray.
 * d_counts (int64 [2] in device memory, or NULL; the caller zeroes it): the kernel adds to [0] the rays the
 * certified wide query answered and to [1] the rays traced through the octree walk or the brute-force loop;
 * one call's two increments sum to n.
 * rt_is_shadowed_device is Renderer::is_shadowed(inter_point, normal, light_position) (renderer.cpp:340-402)
 * for n (d_point, d_normal) pairs ([n][3] floats): d_shadowed[i] = 1 where it returns true, analytic shapes
 * included, else 0; all 0 with compute_shadows off, as the reference's function returns.  light: 3 host floats
 * read during the call, NULL = the scene's light (rt_set_light_position).  The scene is checked only as far
 * as is_shadowed reads it: no material or texture is needed.
 * hip_stream is the caller's hipStream_t (NULL: the null stream).  The kernel is launched on it, after the
 * work queued there before the call and before the work queued after it; only the caller's memory is
 * written, and the host does not wait for the kernel.  The call may block the host for what a frame would
 * block on (a pending geometry rebuild, a material upload) and allocates no device memory.  Whatever later
 * replaces what the kernel reads (geometry, materials, the wide BVH, the risk words) and rt_destroy first
 * wait for it, as for band launches, so the stream may be destroyed right after the call.
 * Every pointer must be device memory of the handle's device (hipPointerGetAttributes on the pointer itself:
 * that [n] elements lie behind it is the caller's word): else RT_EINVAL and no launch.  Outputs must not overlap the inputs or each other (not checked).  RT_EINVAL for a null pointer
 * with n > 0, n < 0 or n > 2^30; n == 0: RT_OK, no launch, pointers unread, counters unchanged.  Errors a
 * frame reports come back with the same codes (a non-finite ingested vertex, no usable device).  With
 * rt_set_devices the queries run on the handle's own device only, as rt_trace_rays.
 * rt_get_device_ray_queries: calls[0..1] = launches of the two kernels (closest hit, shadow) since
 * rt_create, rays[0..1] = the rays given to them. */
int rt_trace_rays_device(rt_renderer *r, const float *d_orig, const float *d_dir, int64_t n, int32_t *d_tri_id,
                         float *d_t, float *d_u, float *d_v, uint8_t *d_ret, int64_t *d_counts, void *hip_stream);
int rt_is_shadowed_device(rt_renderer *r, const float *d_point, const float *d_normal, int64_t n, const float *light,
                          uint8_t *d_shadowed, void *hip_stream);
int rt_get_device_ray_queries(rt_renderer *r, int64_t calls[2], int64_t rays[2]);

/* Ray-segment queries on device memory (no reference counterpart): is anything hit before
 * d_tmax[i] along ray i, and if so what.  The definition goes through rt_trace_rays_device: let (id, t, u, v,
 * ret) be what that call writes for ray i in the same renderer state, and hit_i = ret != 0 && t < d_tmax[i], a
 * float32 comparison: strict, and false for a NaN on either side.
 * rt_occluded_device writes d_occluded[i] = hit_i (1 or 0).
 * rt_trace_segments_device writes those five values bit for bit where hit_i holds and -1, -1.0f, 1.0f, 0.0f, 0
 * everywhere else, whatever stale record the whole-line query left.
 * d_tmax: [n] floats in memory of the handle's device; NULL means +inf for every ray.  Triangles only, as
 * rt_trace_rays_device: analytic shapes are not part of BVH::intersect and are ignored; compute_shadows is not
 * read.  This holds in every mode rt_trace_rays_device covers (the SAH or the quick tree, before one is
 * resident, exact mode, RT_WBVH=0, RT_SEG=0, enable_bvh 0, a scene with analytic shapes, non-finite rays).
 * The wide query stops at d_tmax[i] instead of walking the ray's whole line; so does its fallback, the octree
 * walk, with RT_SEG_OCTREE=1.  That switch is off by default and is the one exception to the definition: its
 * form assumes that no grazing hit is reported outside its triangle's volumes, so with
 * RT_SEG_OCTREE=1 the answer may differ from the definition for a ray the wide query does not certify whose
 * segment ends within an ulp of a grazing hit (14 of 20,000 rays of the grazing-plane stress set).
 * d_counts (int64 [2] in device memory, or NULL; the caller zeroes it): [0] += the rays the certified wide query
 * decided, [1] += the rays that went through the octree walk or the brute-force loop; one call's increments
 * sum to n.
 * Everything else is rt_trace_rays_device's contract: the stream order, no host wait, no allocation, every
 * pointer (d_tmax and d_counts included) checked to be memory of the handle's device, the wait of whatever
 * replaces what the kernel reads, RT_EINVAL for a null required pointer with n > 0, n < 0 or n > 2^30, and
 * n == 0: RT_OK with no launch.
 * rt_get_device_segment_queries: calls[0..1] = launches of the two queries (occluded, segments) since
 * rt_create, rays[0..1] = the rays given to them. */
int rt_occluded_device(rt_renderer *r, const float *d_orig, const float *d_dir, const float *d_tmax, int64_t n,
                       uint8_t *d_occluded, int64_t *d_counts, void *hip_stream);
int rt_trace_segments_device(rt_renderer *r, const float *d_orig, const float *d_dir, const float *d_tmax, int64_t n,
                             int32_t *d_tri_id, float *d_t, float *d_u, float *d_v, uint8_t *d_ret,
                             int64_t *d_counts, void *hip_stream);
int rt_get_device_segment_queries(rt_renderer *r, int64_t calls[2], int64_t rays[2]);

/* The shaded query on device memory (no reference counterpart).
 * rt_trace_ray_device is rt_trace_ray (below) with every array in memory of the handle's device: d_orig / d_dir
 * [n][3] floats in; d_rgba [n][4] floats out (required, 16-byte aligned: else RT_EINVAL); d_hit_src / d_t /
 * d_found / d_shadowed [n] out, each of which may be NULL and is then not written.  Per ray it writes exactly
 * what rt_trace_ray writes for that ray in the same renderer state, in every mode (quick or SAH wide BVH, before
 * one is resident, exact mode, RT_WBVH=0, enable_bvh 0, every shading method, analytic shapes, textures, sky,
 * reflections, rough reflections), with one exception: a scene the frames render with their plain pixel (no
 * texture map, sky, analytic shape, debug shading or reflective material, over a resident wide BVH) takes that
 * pixel's code, and its colour is the float RGBA a frame writes for the same ray (hit_src, t and the flags are
 * rt_trace_ray's bit for bit); RT_SHADE_PLAIN=0, read by rt_create, sends such scenes through the generic code.
 * first_ray: ray i draws the rough-reflection stream of pixel first_ray + i of a frame, so a batch split over
 * several calls gives the bytes of one call; first_ray 0 is rt_trace_ray's keying.  RT_EINVAL for first_ray < 0
 * or first_ray + n > 2^32.
 * current_recursion_depth as in rt_trace_ray; negative: RT_EINVAL.  Past max_recursion_depth every ray gets what
 * trace_ray returns there -- (0, 0, 0, 1), -1, -1.0f, 0, 0 -- from a fill kernel on hip_stream, and d_counts is
 * left as it is.
 * d_counts (int64 [2] in device memory, or NULL; the caller zeroes it): the kernel adds the call's shadow rays to
 * [0] and its reflection rays to [1], the numbers rt_get_stats reports after rt_trace_ray on the same rays.
 * rt_get_stats itself is not touched by this call, and the call shares nothing with band launches in flight.
 * The stream contract, the pointer check and the refusals are rt_trace_rays_device's: the kernel runs on
 * hip_stream in its order, only the caller's memory is written, the host does not wait and nothing is
 * allocated; whatever later replaces what the kernel reads (geometry, materials, textures, the skybox, the wide
 * BVH, the risk words) and rt_destroy first wait for it.  RT_EINVAL for a null d_orig / d_dir / d_rgba with
 * n > 0, n < 0 or n > 2^30; n == 0: RT_OK, no launch.  Outputs must not overlap the inputs or each other (not
 * checked).  The scene is validated as rt_trace_ray validates it, with the same codes (an enabled texture map
 * that is missing: RT_EINVAL; reflective materials with max_recursion_depth > 15: RT_EUNSUPPORTED).
 * rt_get_device_shaded_queries: calls[0..2] = launches of the shading kernel's three instances since rt_create
 * ([0] plain, [1] generic, [2] reflective), rays[0..2] = the rays given to them; the fill past the depth limit
 * counts in none. */
int rt_trace_ray_device(rt_renderer *r, const float *d_orig, const float *d_dir, int64_t n,
                        int32_t current_recursion_depth, int64_t first_ray,
                        float *d_rgba, int32_t *d_hit_src, float *d_t,
                        uint8_t *d_found, uint8_t *d_shadowed,
                        int64_t *d_counts, void *hip_stream);
int rt_get_device_shaded_queries(rt_renderer *r, int64_t calls[3], int64_t rays[3]);

/* Shaded ray batches through the frame engine (no reference counterpart).
 * rt_trace_ray_batch_device takes rt_trace_ray_device's arguments, in the same order and with the same meaning, and
 * writes per ray what that call writes for the ray in the same renderer state: d_hit_src, d_t, d_found and
 * d_shadowed bit for bit, d_counts[0..1] += the same shadow and reflection ray counts, d_rgba the colour the frame
 * engine computes for the ray (for a frame's camera rays, bit for bit the float RGBA an engine frame of the same
 * renderer writes; within the project's RGBA bar of the reference's trace_ray).  On a scene with a reflective
 * material rt_trace_ray_device walks each ray's whole compute_reflection recursion in one lane; this call shades
 * the batch level by level as the frames do, which is what a caller with many rays on a mirror or rough scene wants.
 * The optional outputs, first_ray, current_recursion_depth (past max_recursion_depth: the fill kernel), the pointer
 * check, every refusal and the scene's validation are rt_trace_ray_device's; n == 0: RT_OK, no launch.
 * The contract differs from rt_trace_ray_device's:
 *  - The work is ordered on hip_stream: it runs after what was queued there before the call, and what is queued
 *    after the call sees the outputs.  But the host blocks during the call: the engine reads its per-chunk counts
 *    back, at least once per level.  The last pass may still be in flight when the call returns.
 *  - The call may allocate device memory: the engine's level buffers grow as for frames (shared with them).
 *  - hip_stream first waits for band launches and ray queries in flight on other streams, and later band launches
 *    and frames wait for this call, as for any launch that uses the engine's buffers.
 *  - rt_get_stats, rt_band_counters and the image of a band launch around the call are what they are without it.
 * The n rays are shaded in batches of 2^RT_SHADE_BATCH_LOG2 (read by rt_create; 10..24, default 22).
 * Where the engine does not apply -- no reflective material, enable_bvh 0, RT_REFL_ENGINE=0 -- the call is
 * rt_trace_ray_device: the same code path, the same bytes, that call's contract, and its counters move.
 * No choice is made by n: for few rays, or rays that reflect once (a mirror), rt_trace_ray_device can be faster.
 * rt_get_device_shaded_batches: calls[0] / rays[0] = the calls the engine shaded since rt_create and their rays,
 * calls[1] / rays[1] = the calls handed to rt_trace_ray_device's code; the fill past the depth limit and an empty
 * call count in neither. */
int rt_trace_ray_batch_device(rt_renderer *r, const float *d_orig, const float *d_dir, int64_t n,
                              int32_t current_recursion_depth, int64_t first_ray,
                              float *d_rgba, int32_t *d_hit_src, float *d_t,
                              uint8_t *d_found, uint8_t *d_shadowed,
                              int64_t *d_counts, void *hip_stream);
int rt_get_device_shaded_batches(rt_renderer *r, int64_t calls[2], int64_t rays[2]);

/* The visibility buffer of the current camera on device memory (no reference counterpart).
 * rt_visibility_device answers, for every pixel of the internal image (render_w x render_h, SSAA applied; row 0 is
 * NDC y = -1, as everywhere), the closest-hit part of Renderer::trace_ray at depth 0 (renderer.cpp:1008-1040) for
 * that pixel's camera ray (renderer.cpp:1086-1098).  Nothing is shaded and no shadow ray is traced.  Outputs,
 * row-major [render_h][render_w], in memory of the handle's device; each may be NULL and is then not written, all
 * three NULL is RT_EINVAL:
 *   d_tri_id: the record's source when t > 0.1 (triangle index in caller order, or -2 - k for analytic shape k),
 *             else -1: exactly the hit_id rt_ray_trace leaves for rt_get_internal;
 *   d_t:      the record's t (-1 for a fresh record): rt_get_internal's hit_t, bit for bit;
 *   d_uv:     [..][2] floats, 8-byte aligned (else RT_EINVAL): where d_tri_id >= 0 the record's u, v, bit for bit
 *             what rt_trace_rays_device writes for that ray; (0, 0) everywhere else.
 * This holds in every mode (SAH or quick wide tree, before one is resident, exact mode, RT_WBVH=0, enable_bvh 0,
 * analytic shapes).  No shading setting is read: shading method, textures, sky, reflective materials, enable_ssao,
 * max_recursion_depth; hybrid_rasterization_tracing is ignored, as rt_ray_trace ignores it.  The scene is checked
 * only as far as the query reads it, as for rt_is_shadowed_device: no material or texture is needed.
 * Over a resident wide tree, with enable_bvh on and no analytic shape, the launch runs the frames' primary query
 * with their tile mask and per-block entry sets (the entry sets from a stream's second
 * launch in a row with one camera on), without the frame's shading and shadow query.
 * The contract is rt_trace_rays_device's: the work runs on hip_stream (NULL: the null stream) in its order, only
 * the caller's memory is written, the host does not wait for the GPU, whatever later replaces what the kernel reads
 * and rt_destroy wait for it, and the stream may be destroyed right after the call.  The call may block for what a
 * frame would block on (a pending rebuild).  Unlike the ray queries it may allocate device memory: each stream has
 * its own tile-queue counters and tile mask, allocated at the stream's first call and when the render size grows;
 * up to 8 streams keep theirs, a ninth takes over the least recently used stream's once that stream's last launch
 * is done (the host waits for it).  Launches on different streams run concurrently, among themselves and with band
 * launches; rt_tile_mask, rt_tile_starts, rt_tile_lists, rt_band_counters, rt_kernel_times, rt_band_costs and
 * rt_get_stats report what they would report without the call.
 * Every refusal happens before any launch: RT_EINVAL for a pointer that is not memory of the handle's device, a
 * misaligned d_uv, no output; the errors a frame reports come back with the same codes.  With rt_set_devices the
 * call runs on the handle's own device.
 * rt_get_device_visibility: calls[0..1] / pixels[0..1] = launches of the kernel's two instances since rt_create
 * ([0] the fast one over the wide tree, [1] the generic one) and their pixels; used[0] = launches that were given a
 * tile mask, used[1] = launches that were given entry sets. */
int rt_visibility_device(rt_renderer *r, int32_t *d_tri_id, float *d_t, float *d_uv, void *hip_stream);
int rt_get_device_visibility(rt_renderer *r, int64_t calls[2], int64_t pixels[2], int64_t used[2]);

/* Renderer::trace_ray(ray, hit_info, current_recursion_depth, intersection_found)
 * (renderer.h:144, renderer.cpp:1008-1066) for n arbitrary rays (origins / directions [n][3]),
 * each with a fresh HitInfo: rgba [n][4] = the Color trace_ray returns (shading, shadow ray,
 * compute_reflection recursion down to max_recursion_depth, sky / background on a miss);
 * hit_src = the record's source when intersection_found (triangle index, -2 - k for analytic
 * shape k), else -1; t = the record's t; intersection_found; shadowed = the hit's shadow ray was
 * blocked.  Ray i's rough-reflection samples draw from the stream of pixel i of a frame (the
 * counter-based RNG of rt_settings::rng_seed).  rt_get_stats reports the call's shadow and
 * reflection ray counts. */
int rt_trace_ray(rt_renderer *r, const float *orig, const float *dir, int64_t n, int32_t current_recursion_depth,
                 float *rgba, int32_t *hit_src, float *t, uint8_t *intersection_found, uint8_t *shadowed);

/* GPU durations (ms) of the ray-trace kernel of the last n rt_render_bands_device
 * calls, from HIP events recorded around each launch on its stream (waits for them). */
int rt_kernel_times(rt_renderer *r, float *ms, int32_t n);
/* shadow / reflection ray counts of the last rt_render_bands_device (waits for that launch);
 * RT_ESTATE before the first rt_render_bands_device call */
int rt_band_counters(rt_renderer *r, int64_t *shadow_rays, int64_t *reflection_rays);
/* the tile mask of the last frame launch (rt_ray_trace / rt_render_bands_device; RT_TILE_MASK=0: none): one bit
 * per 8 x 8 block of the internal image, block (bx, by) at bit bx & 31 of words[by * info[2] + (bx >> 5)]; a
 * clear bit: every pixel of the block is the background's and was written without a ray.  src 0: as the
 * device computed it; 1: recomputed on the host from the same wide-BVH nodes.  info: blocks per row, block
 * rows, words per row, 1 when the launch used the mask (0: it had none, every bit is set), the entries of the
 * tree cut it was computed from.  words may be NULL (info only); cap: its size in words.  RT_ESTATE before
 * the first frame launch */
int rt_tile_mask(rt_renderer *r, int32_t src, uint32_t *words, int64_t cap, int32_t info[5]);
/* the entry sets of the last frame launch (with its tile mask; RT_TILE_START=0: none): per 8 x 8 block of the
 * internal image, row-major, the four wide-BVH node links its camera rays' queries start at instead of the
 * root (0xFFFFFFFF in unused slots; {0, ...}: the root).  src 0: as the device computed them; 1: recomputed on
 * the host from the same nodes and mask.  info: blocks per row, block rows, 1 when the launch used entry sets
 * (0: every set is the root's).  sets may be NULL (info only); cap: its size in words (4 per block).
 * RT_ESTATE before the first frame launch */
int rt_tile_starts(rt_renderer *r, int32_t src, uint32_t *sets, int64_t cap, int32_t info[3]);
/* the tile lists of the last frame launch (with its tile mask; RT_TILE_LIST=0: none): the launch's 8 x 8 tiles
 * (row-major over its local rows, info[0] per row) that the frame kernel's queue handed out ('covered': a lane
 * of the tile lies in a block whose mask bit is set) and those its waves filled with the background at their
 * exit ('clear'), each in ascending order; tiles without a pixel on the image are in neither.  src 0: as the
 * device computed them; 1: recomputed on the host from the mask words read back.  info: tiles per row, tile
 * rows, covered tiles, clear tiles, 1 when the launch used lists (0: none, both counts 0).  tiles receives the
 * covered tiles, then the clear ones; it may be NULL (info only); cap: its size in words.  RT_ESTATE before the
 * first frame launch */
int rt_tile_lists(rt_renderer *r, int32_t src, int32_t *tiles, int64_t cap, int32_t info[5]);

/* ---- tp2/src/mat.cpp restated (host) ---- */
/* kind: 0 Translation(x,y,z) 1 RotationX(x deg) 2 RotationY 3 RotationZ 4 Scale(x,y,z) 5 Identity */
void rt_make_transform(int32_t kind, float x, float y, float z, float out[16]);
void rt_compose(const float a[16], const float b[16], float out[16]);                      /* a(b), mat.cpp:363-371 */
void rt_inverse(const float m[16], float out[16]);                                          /* mat.cpp:378-447 */
void rt_perspective(float fov, float aspect, float znear, float zfar, float out[16]);       /* mat.cpp:307-319 */
void rt_transform_points(const float m[16], const float *pts, int64_t n, float *out);       /* mat.cpp:83-100 */

/* ---- OBJ / MTL loading: read_meshio_data (tp2/src/mesh_io.cpp:426-591) +
 * MeshIOUtils::create_triangles(data, mat_offset, xform) (utils/meshIOUtils.cpp:4-30).
 * Two-step: rt_obj_open parses, rt_obj_fetch copies out (arrays sized from the counts). */
typedef struct rt_obj rt_obj;
rt_obj *rt_obj_open(const char *path, const float xform[16], int32_t mat_offset);
int rt_obj_counts(const rt_obj *o, int64_t *ntri, int32_t *nmat, int32_t *has_uv);
int rt_obj_fetch(const rt_obj *o, float *tri9, int32_t *mat, float *uv6, float *mats16);
void rt_obj_close(rt_obj *o);

/* Diagnostics (tile costs, per-wave records, the wide query and its risk words on the GPU, the host
 * octree digest and wide-BVH query) are declared in rt_mi355x_diag.h; the same library exports them. */

#ifdef __cplusplus
}
#endif
#endif
