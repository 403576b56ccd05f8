/* orbit_host_c.h — flat C surface of the C++ host mirror (orbit_host.hpp), for the
 * ctypes-driven test-suite.  The functions keep the reference's names
 * (src/passes/draw_gen.rs, src/passes/cluster.rs, src/math.rs, src/camera.rs). */
#ifndef ORBIT_HOST_C_H
#define ORBIT_HOST_C_H
#include "../../include/orbit_abi_ext.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ORBIT_HOST_PANIC (-100) /* the reference would have panicked; text in orbit_host_last_error() */

typedef struct OrbitHostProjection {
    uint32_t kind; /* 0 = Perspective{fov, near_clip}, 1 = Orthographic{half_width, near_clip, far_clip} */
    float fov, half_width, near_clip, far_clip;
} OrbitHostProjection;

/* CullInfo, draw_gen.rs:105-118 (+ OcclusionCullInfo :18-33) */
typedef struct OrbitHostCullInfo {
    float view_matrix[16];
    float view_space_cull_planes[16][4]; /* room for > 12 so that the assert can be exercised */
    uint32_t plane_count;
    OrbitHostProjection projection;
    uint32_t occlusion_kind; /* 0 None, 1 VisibilityRead, 2 VisibilityWrite */
    void *visibility_buffer;
    void *meshlet_visibility_buffer; /* NULL = Option::None */
    float *depth_pyramid;
    uint32_t depth_pyramid_size[2];
    uint32_t noskip_alphamode;
    float aspect_ratio;
    uint32_t alpha_mode_filter;
    uint32_t lod_range[2];
    float lod_base, lod_step;
    float lod_target_pos_view_space[3];
} OrbitHostCullInfo;

typedef struct OrbitHostAssets {
    void *meshlet_buffer, *mesh_info_buffer, *materials_buffer;
    uint32_t material_count;
} OrbitHostAssets;
typedef struct OrbitHostScene {
    uint64_t entity_draw_count;
    void *entity_draw_buffer, *entity_buffer, *light_data_buffer, *meshlet_visibility_buffer;
    uint64_t light_count;
} OrbitHostScene;
typedef struct OrbitHostBuffer {
    void *ptr;
    uint64_t size;
} OrbitHostBuffer;

typedef struct OrbitHostClusterSettings {
    uint32_t px_size_power, screen_resolution[2], z_slice_count;
    float far_plane, luminance_cutoff;
} OrbitHostClusterSettings;
typedef struct OrbitHostClusterDerived {
    uint64_t tile_counts[2], cluster_counts[3], linear_cluster_count, linear_max_allocated_cluster_count;
    uint32_t tile_px_size;
    float z_scale, z_bias;
} OrbitHostClusterDerived;
typedef struct OrbitHostClusterOut {
    OrbitHostBuffer tile_depth_slice_mask, depth_bounds, unique_cluster_buffer, light_offset_image, light_index_list;
    OrbitGpuClusterInfoBuffer info;
} OrbitHostClusterOut;

const char *orbit_host_last_error(void);

/* math.rs / camera.rs (host only) */
void orbit_host_perspective_infinite_reverse_rh(float fov_y, float aspect, float z_near, float out[16]);
void orbit_host_orthographic_rh(float l, float r, float b, float t, float n, float f, float out[16]);
void orbit_host_projection_compute_matrix(const OrbitHostProjection *p, float aspect, float out[16]);
void orbit_host_mat4_inverse(const float in[16], float out[16]);
void orbit_host_frustum_planes_from_matrix(const float m[16], float out[6][4], int32_t normalize);
uint32_t orbit_host_mip_levels_from_size(uint32_t max_size);
int32_t orbit_host_project_sphere_clip_space(const float sphere[4], float znear, float p00, float p11, float aabb[4]);
/* CullInfo::to_gpu */
int32_t orbit_host_cull_info_to_gpu(const OrbitHostCullInfo *ci, OrbitGpuCullInfo *out);
/* ShadowRenderer::render_cascaded_shadow, per-cascade CullInfo (shadow_renderer.rs:466-706).  direction and the
 * camera orientation are unit quaternions (x, y, z, w); the camera must be perspective {fov, near_clip}. */
typedef struct OrbitHostShadowCascadeIn {
    uint32_t shadow_resolution;
    float cascade_split_lambda, max_shadow_distance;
    uint32_t min_mesh_lod, max_mesh_lod;
    float lod_base, lod_step;
    float direction[4];
    float camera_position[3], camera_orientation[4];
    float camera_fov, camera_near_clip, camera_aspect_ratio;
    uint32_t cascade_index, frustum_culling;
} OrbitHostShadowCascadeIn;
int32_t orbit_host_shadow_cascade(const OrbitHostShadowCascadeIn *in, OrbitHostCullInfo *out_cull_info,
                                  float out_light_projection_matrix[16], float *out_world_size);
/* ClusterSettings methods */
void orbit_host_cluster_settings_derive(const OrbitHostClusterSettings *s, float z_near, OrbitHostClusterDerived *out);

/* compute_cluster_aabb, cluster.rs:150-184 (the reference's CPU twin of the cluster volume): out = min xyz, max xyz */
void orbit_host_compute_cluster_aabb(const float inverse_projection[16], const float screen_size[2], float tile_size_px,
                                     const float cluster_count[3], float z_near, float z_far, const float cluster_id[3],
                                     float out_min_max[6]);

/* graphics::Context slice + passes (need a GPU) */
void *orbit_host_context_create(int32_t device, void *stream, const OrbitCaps *caps);
void orbit_host_context_destroy(void *hctx);
/* Context::sync_meshlet_stream: derived meshlet streams of meshlets [first, first + count) re-derived and bound */
int32_t orbit_host_sync_meshlet_stream(void *hctx, void *meshlet_buffer, uint64_t first, uint64_t count,
                                       uint64_t capacity);
/* Context::sync_meshlet_stream_materials: the stream's alpha classes from the materials buffer */
int32_t orbit_host_sync_meshlet_stream_materials(void *hctx, void *materials_buffer, uint32_t material_count);
int32_t orbit_host_create_meshlet_dispatch_command(void *hctx, const char *name, const OrbitHostAssets *assets,
                                                   const OrbitHostScene *scene, const OrbitHostCullInfo *ci,
                                                   OrbitGpuCullInfo *out_cull_info, OrbitHostBuffer *out_dispatch);
int32_t orbit_host_create_meshlet_draw_commands(void *hctx, const char *name, const OrbitHostAssets *assets,
                                                const OrbitHostScene *scene, const OrbitHostCullInfo *ci,
                                                const OrbitHostBuffer *dispatch, OrbitHostBuffer *out_draws);
int32_t orbit_host_create_draw_commands(void *hctx, const char *name, const OrbitHostAssets *assets,
                                        const OrbitHostScene *scene, const OrbitHostCullInfo *ci,
                                        OrbitHostBuffer *out_draws);
/* DepthPyramid::new + update for a named pyramid; returns the image handle */
int32_t orbit_host_depth_pyramid_update(void *hctx, const char *name, const float *depth, uint32_t width,
                                        uint32_t height, float **out_pyramid, uint32_t out_size_mips[3]);
int32_t orbit_host_compute_clusters(void *hctx, const OrbitHostClusterSettings *settings, const float view_matrix[16],
                                    const OrbitHostProjection *projection, float aspect_ratio, const float *depth,
                                    uint32_t depth_size[2], uint32_t samples, const OrbitHostScene *scene,
                                    OrbitHostClusterOut *out);

/* ---- scene side (orbit_scene.hpp): collections::{Arena, FreeListAllocator}, scene::SceneData (host only) ---- */
typedef struct OrbitHostArenaIndex {
    uint32_t generation, slot;
} OrbitHostArenaIndex;
/* Arena<i64>: arena.rs:98-330 */
void *orbit_host_arena_create(void);
void orbit_host_arena_destroy(void *arena);
OrbitHostArenaIndex orbit_host_arena_insert(void *arena, int64_t value);
int32_t orbit_host_arena_get(const void *arena, OrbitHostArenaIndex index, int64_t *out);    /* 1 = Some */
int32_t orbit_host_arena_remove(void *arena, OrbitHostArenaIndex index, int64_t *out);       /* 1 = Some */
int32_t orbit_host_arena_has_index(const void *arena, OrbitHostArenaIndex index);
uint64_t orbit_host_arena_len(const void *arena);
/* occupied entries in iteration order; returns how many were written (<= capacity) */
uint64_t orbit_host_arena_iter(const void *arena, OrbitHostArenaIndex *indices, int64_t *values, uint64_t capacity);
/* FreeListAllocator: freelist_alloc.rs:22-121 */
void *orbit_host_freelist_create(uint64_t size);
void orbit_host_freelist_destroy(void *alloc);
int32_t orbit_host_freelist_allocate(void *alloc, uint64_t size, OrbitHostArenaIndex *out_index,
                                     uint64_t out_range[2]); /* 1 = Some, 0 = None */
void orbit_host_freelist_deallocate(void *alloc, OrbitHostArenaIndex index);
/* blocks in address order: ranges[2*i], ranges[2*i+1], is_free[i]; returns the block count */
uint64_t orbit_host_freelist_blocks(const void *alloc, uint64_t *ranges, int32_t *is_free, uint64_t capacity);

typedef struct OrbitHostLight {
    float color[3], intensity;
    uint32_t kind; /* 0 Sky, 1 Directional, 2 Point (scene.rs:136-141) */
    float param;   /* Directional: angular_size, Point: inner_radius */
    uint32_t irradiance_map_index, prefiltered_map_index; /* Sky */
    uint32_t cast_shadows;
} OrbitHostLight;
typedef struct OrbitHostEntity {
    float position[3], orientation[4], scale[3]; /* Transform, scene.rs:20-24; quaternion (x, y, z, w) */
    int32_t mesh;                                /* MeshHandle slot, -1 = None */
    int32_t has_light;
    OrbitHostLight light;
    const char *name; /* NULL = None */
} OrbitHostEntity;
/* SceneData (scene.rs:358-492); visibility_chunk_count 0 = MESHLET_VISIBILITY_BUFFER_CHUNK_COUNT */
void *orbit_host_scene_create(uint64_t visibility_chunk_count);
void orbit_host_scene_destroy(void *scene);
int64_t orbit_host_scene_add_entity(void *scene, const OrbitHostEntity *entity);
int32_t orbit_host_scene_set_transform(void *scene, uint64_t entity, const float position[3],
                                       const float orientation[4], const float scale[3]);
int32_t orbit_host_scene_update(void *scene, const OrbitMeshInfo *mesh_infos, uint64_t mesh_info_count,
                                float luminance_cutoff, uint64_t frame_index);
/* the caches update_scene filled: pointers stay valid until the next update / destroy */
const void *orbit_host_scene_entity_draws(const void *scene, uint64_t *count);   /* {instance, mesh, vis_offset}[] */
const OrbitEntityData *orbit_host_scene_entity_data(const void *scene, uint64_t *count);
const OrbitLightData *orbit_host_scene_light_data(const void *scene, uint64_t *count);
uint64_t orbit_host_scene_shadow_command_count(const void *scene);
/* update_scene with the EntityData rows left to orbit_scene_update_entities: draws, visibility words, light data and
 * shadow commands as orbit_host_scene_update makes them; the transforms of the drawn entities, in instance order, take
 * the place of the entity data (orbit_host_scene_entity_data is then empty) */
int32_t orbit_host_scene_update_deferred(void *scene, const OrbitMeshInfo *mesh_infos, uint64_t mesh_info_count,
                                         float luminance_cutoff, uint64_t frame_index);
const OrbitEntityTransform *orbit_host_scene_transforms(const void *scene, uint64_t *count);
/* the entity's instance index (its row of entity_data) from the latest update, -1 if it had none */
int64_t orbit_host_scene_instance_index(const void *scene, uint64_t entity);
/* `count` unnamed entities from one OrbitSceneEntity (visibility_offset is not read) and one transform each: the
 * inverse of orbit_host_scene_entity_table.  Returns the first one's index, -1 + orbit_host_last_error() on failure */
int64_t orbit_host_scene_add_entities(void *scene, const OrbitSceneEntity *table, const OrbitEntityTransform *transforms,
                                      uint64_t count);
/* another mesh for the entity, -1 = None; its visibility words stay its own */
int32_t orbit_host_scene_set_mesh(void *scene, uint64_t entity, int32_t mesh);
/* what stays on the host when orbit_scene_update builds draws, rows and lights on the device: allocates the visibility
 * words of mesh-bearing entities that have none and fills one OrbitSceneEntity and one transform per entity, in ENTITY
 * order (orbit_host_scene_transforms then returns every entity's); the caches of orbit_host_scene_update are untouched */
int32_t orbit_host_scene_update_device(void *scene, const OrbitMeshInfo *mesh_infos, uint64_t mesh_info_count);
const OrbitSceneEntity *orbit_host_scene_entity_table(const void *scene, uint64_t *count);
/* the shadow commands' orientations (x, y, z, w) of the latest update, at most `capacity` of them; returns their number */
uint64_t orbit_host_scene_shadow_orientations(const void *scene, float *orientations, uint64_t capacity);
/* the entity's row of light_data from the latest orbit_host_scene_update, -1 if it had none */
int64_t orbit_host_scene_light_index(const void *scene, uint64_t entity);

/* ---- asset side (orbit_assets.hpp): mesh -> Meshlet[] + meshlet data, mesh bounds (host only) ---- */
/* assets::mesh::compute_meshlets (mesh.rs:292-338).  Two-call protocol: with out_meshlets == NULL only the counts are
 * returned; then call again with buffers of those sizes.  positions: xyz per vertex. */
int32_t orbit_host_compute_meshlets(const float *positions, uint64_t vertex_count, const uint32_t *indices,
                                    uint64_t index_count, uint32_t material, uint32_t vertex_offset,
                                    uint32_t data_offset_base, OrbitMeshlet *out_meshlets, uint32_t *out_meshlet_data,
                                    uint64_t *meshlet_count, uint64_t *meshlet_data_words);
/* gltf_loader.rs:480-506 */
void orbit_host_compute_mesh_bounds(const float *positions, uint64_t vertex_count, float aabb_min[3], float aabb_max[3],
                                    float bounding_sphere[4]);

/* the reference of orbit_meshlet_bounds, on HOST copies of the same buffers: decodes each selected record as the device
 * does (global vertex = vertex_offset + meshlet_data[data_offset + local], in 64 bits; u8 corners from byte
 * (data_offset + vertex_count) * 4), applies the device's four range checks and calls compute_meshlet_bounds.
 * indices == NULL: the range [first, first + count).  out[i] = the i-th selected meshlet's bounds, all zero where a
 * range check failed; the records are not written.  A NaN float is returned as 0x7FC00000, as the device writes it.
 *  range_error (may be NULL): count flags, 1 where a check failed.
 * updates (may be NULL): count words, the growth updates of the meshlet's two Ritter spheres (corners + normals). */
int32_t orbit_host_meshlet_bounds(const OrbitMeshlet *meshlets, uint64_t meshlet_capacity, const uint32_t *indices,
                                  uint64_t first, uint64_t count, const uint32_t *meshlet_data, uint64_t meshlet_data_words,
                                  const void *vertices, uint64_t vertex_count, uint32_t vertex_stride,
                                  uint32_t position_offset, OrbitMeshletBoundsFull *out, int32_t *range_error,
                                  uint32_t *updates);

/* the reference of orbit_raster_depth (include/orbit_abi_ext.h R1-R9), on HOST copies of the same buffers, sequential:
 * the same depth bytes (cleared first with ORBIT_RASTER_CLEAR, else max-merged into what `depth` holds), the same
 * counters.  draw_commands = {u32 count; OrbitMeshletDrawCommand[]}, the count clamped by max_commands.
 * stats (may be NULL): overwritten.  command_error (may be NULL): min(count, max_commands) flags, 1 where the device
 * skips the command and latches ORBIT_E_RANGE.  ORBIT_HOST_PANIC for what the device call answers with ORBIT_E_INVALID. */
int32_t orbit_host_raster_depth(const void *draw_commands, uint32_t max_commands, const uint32_t *meshlet_data,
                                uint64_t meshlet_data_words, const void *vertices, uint64_t vertex_count,
                                uint32_t vertex_stride, uint32_t position_offset, const OrbitEntityData *entity_data,
                                uint32_t entity_count, const float view_proj[16], float *depth, uint32_t width,
                                uint32_t height, uint32_t flags, OrbitRasterStats *stats, int32_t *command_error);

/* the reference of orbit_raster_visibility (V1-V4): the arguments of orbit_host_raster_depth with the width * height u64
 * `visibility` in place of depth, and command_base.  command_error also flags a command with nt > 256 (V3). */
int32_t orbit_host_raster_visibility(const void *draw_commands, uint32_t max_commands, const uint32_t *meshlet_data,
                                     uint64_t meshlet_data_words, const void *vertices, uint64_t vertex_count,
                                     uint32_t vertex_stride, uint32_t position_offset, const OrbitEntityData *entity_data,
                                     uint32_t entity_count, const float view_proj[16], uint64_t *visibility, uint32_t width,
                                     uint32_t height, uint32_t flags, uint32_t command_base, OrbitRasterStats *stats,
                                     int32_t *command_error);
/* the reference of orbit_visibility_resolve: depth (width * height), command_pixels (max_commands) and stats may be NULL,
 * not all three. */
int32_t orbit_host_visibility_resolve(const uint64_t *visibility, uint32_t width, uint32_t height, uint32_t command_base,
                                      uint32_t max_commands, float *depth, uint32_t *command_pixels,
                                      OrbitVisibilityStats *stats);
/* the reference of orbit_visibility_compact (C1-C6): the device call's block with HOST pointers in it; workspace and
 * workspace_bytes are not read.  Every output holds the device's bytes.  *status (may be NULL): what the device latches,
 * ORBIT_E_RANGE before ORBIT_E_CAPACITY before ORBIT_OK.  ORBIT_HOST_PANIC for what the device answers with
 * ORBIT_E_INVALID (alignment and the workspace aside). */
int32_t orbit_host_visibility_compact(const OrbitVisibilityCompact *job, int32_t *status);
/* the reference of orbit_visibility_surface (S1-S7): the device call's block with HOST pointers in it.  Every output
 * holds the device's bytes.  *status (may be NULL): ORBIT_E_RANGE if a pixel was stale, else ORBIT_OK.  ORBIT_HOST_PANIC
 * for what the device answers with ORBIT_E_INVALID (alignment aside). */
int32_t orbit_host_visibility_surface(const OrbitVisibilitySurface *job, int32_t *status);
/* the reference of orbit_visibility_surface_drawn (S2d, S3c, S3w): as above, with the raster flags the buffer was drawn
 * with (ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD; any other bit is ORBIT_HOST_PANIC) */
int32_t orbit_host_visibility_surface_drawn(const OrbitVisibilitySurface *job, uint32_t raster_flags, int32_t *status);
/* the reference of orbit_surface_fragments (F1-F8): the device call's block with HOST pointers in it.  Every output holds
 * the device's bytes.  *status (may be NULL): ORBIT_E_RANGE if a pixel was stale, else ORBIT_OK.  ORBIT_HOST_PANIC for
 * what the device answers with ORBIT_E_INVALID (alignment and aliasing aside). */
int32_t orbit_host_surface_fragments(const OrbitSurfaceFragments *job, int32_t *status);

/* the reference of orbit_fragments_shade (L1-L9): the device call's block with HOST pointers in it.  color, lights_walked
 * and stats hold the device's bytes.  *status (may be NULL): ORBIT_E_RANGE if a pixel was stale, else ORBIT_OK.
 * ORBIT_HOST_PANIC for what the device answers with ORBIT_E_INVALID (alignment and aliasing aside). */
int32_t orbit_host_fragments_shade(const OrbitFragmentsShade *job, int32_t *status);
/* the reference of orbit_fragments_shade_shadowed (H1-H10): the device call's block with HOST pointers in it, as
 * orbit_host_fragments_shade; shadow_factor, cascade and shadow_stats hold the device's bytes too. */
int32_t orbit_host_fragments_shade_shadowed(const OrbitFragmentsShadeShadowed *job, int32_t *status);
/* the reference of orbit_fragments_shade_sky (K1-K10): the device call's block with HOST pointers in it, as
 * orbit_host_fragments_shade_shadowed; sky_stats holds the device's bytes too.  ORBIT_HOST_PANIC for everything the device
 * answers with ORBIT_E_INVALID, alignment and aliasing included: the two share one check.  census (may be NULL):
 * ORBIT_HOST_SKY_CENSUS counters — 0-63 the cube sampler's (ORBIT_HOST_ENV_CENSUS, over K4's, K5's and K9's samples), then
 * by index 64 / 65 SKY lights evaluated / skipped with the environment NULL; 66-70 evaluations with dot(N, V) negative, 0,
 * 1, NaN, any other value; 71 / 72 channels whose max(1 - roughness, f0) took 1 - roughness / f0; 73 / 74 evaluations whose
 * N / R was a bad direction; 75 / 76 / 77 table lookups with a tap clamped at 0 / at n - 1 / not clamped; 78 pixels shaded
 * with ao NULL, 79 with ao[p] < 1, 80 with 1.0f taken; 81 / 82 skybox pixels with a good / a bad direction; 83 second and
 * later SKY lights of one walk; 84-95 zero. */
#define ORBIT_HOST_SKY_CENSUS 96
int32_t orbit_host_fragments_shade_sky(const OrbitFragmentsShadeSky *job, int32_t *status, uint64_t *census);
/* K9's ray basis of the reference's perspective_infinite_reverse_rh camera: orientation (x, y, z, w) a unit quaternion,
 * fov_y in radians -> sky_x, sky_y, sky_z, three floats each */
int32_t orbit_host_skybox_basis(const float *orientation, float fov_y, float aspect, float *sky_x, float *sky_y, float *sky_z);
/* the reference of orbit_bloom (B1-B9): the device call's block with HOST pointers in it; mips and stats hold the
 * device's bytes.  ORBIT_HOST_PANIC for what the device answers with ORBIT_E_INVALID. */
int32_t orbit_host_bloom(const OrbitBloom *job);
/* the reference of orbit_post_process (T1-T5): as above; ldr, rgba8 and stats hold the device's bytes. */
int32_t orbit_host_post_process(const OrbitPostProcess *job);
/* tests: one downsample (B3-B5) / one upsample's added term (B6) on three floats per texel, nothing packed;
 * threshold_filter: B2's four floats (read with level0 != 0) */
void orbit_host_bloom_downsample_floats(const float *src, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, uint32_t level0,
                                        const float *threshold_filter, float *dst);
void orbit_host_bloom_upsample_floats(const float *src, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, float filter_radius,
                                      float *dst);
/* the reference of orbit_ssao (A1-A9): the device call's block with HOST pointers in it; raw, blurred, ao_pixel and stats
 * hold the device's bytes.  census (may be NULL): 19 counters over every pixel and sample — A2's four branches, samples in
 * range / out of range / occluded / not occluded, range_check strictly inside (0, 1) / 0 / 1 / NaN, samples with
 * sample_depth == proj.z, pixels with a horizontal and with a vertical tie of A2, in-range samples with a component
 * exactly 0 and exactly 1, rejected samples with a component one step below 0 and one above 1. */
int32_t orbit_host_ssao(const OrbitSsao *job, uint64_t *census);
/* the reference of orbit_env_map and orbit_env_sample (E0-E12): the device calls' blocks with HOST pointers in them; every
 * output holds the device's bytes.  census (may be NULL): ORBIT_HOST_ENV_CENSUS counters over every tap of the call — by
 * index 0-5 the sampled directions whose major axis is each layer; 6-29 the taps outside their face in one axis, by layer
 * * 4 + side (0 left, 1 right, 2 above, 3 below); 30-53 the taps outside in both, by layer * 4 + corner (bit 0 right, bit
 * 1 below); 54 / 55 prefilter texels whose abs(N.z) < 0.999 is true / false; 56 prefilter samples with dotNL <= 0; 57
 * prefilter texels at roughness 0; 58 prefilter texels with totalWeight == 0; 59 irradiance texels with a NaN frame; 60
 * sampled directions mixed from two levels; 61-63 zero. */
#define ORBIT_HOST_ENV_CENSUS 64
int32_t orbit_host_env_map(const OrbitEnvMap *job, uint64_t *census);
int32_t orbit_host_env_sample(const OrbitEnvSample *job, uint64_t *census);
/* tools: count texels (face * n * n + py * n + px) of level `level` of the job's prefiltered cube, from the job's sky cube
 * as it is; out: count 8-B texels.  What a full-size run is verified against where the whole mirror would take hours. */
int32_t orbit_host_env_prefilter_texels(const OrbitEnvMap *job, uint32_t level, const uint32_t *texels, uint32_t count, uint16_t *out);
/* tests: E1 of one texel (three floats); the routines over n values — which = 0: atan2c(a, b), 1: asinc(a), 2 / 3: the
 * sine / cosine of H6's routine at a, 4: E0's stored half of a read back as a float (NaN where a is not finite) */
void orbit_host_env_direction(uint32_t face, uint32_t px, uint32_t py, uint32_t n, float *out);
void orbit_host_env_routines(uint32_t which, const float *a, const float *b, uint64_t n, float *out);
/* tests: A4's table (sample_count x 4 floats: direction, radius), A5's range test of n (x, y, z) triples and its
 * range_check of n (min_radius, sample_depth, proj.w) triples */
void orbit_host_ssao_table(const uint8_t *samples, uint32_t samples_size, uint32_t sample_count, float min_radius, float max_radius, float *table);
void orbit_host_ssao_in_range(const float *proj, uint64_t n, uint8_t *out);
void orbit_host_ssao_range_check(const float *args, uint64_t n, float *out);
/* tests: B7 of n texels (clamped may be NULL: 1 per texel that counts in clamped_texels), and powc of B5 / T4 */
void orbit_host_bloom_pack(const float *rgb, uint64_t n, uint32_t *words, uint8_t *clamped);
void orbit_host_bloom_unpack(const uint32_t *words, uint64_t n, float *rgb);
void orbit_host_powc(const float *x, uint64_t n, float y, float *out);
/* tests: H6 of the pixels (x0 + x, y0 + y), x < width, y < height, row-major into three arrays of width * height floats:
 * theta and csrc/shadow_common.h's sine and cosine of it */
void orbit_host_shadow_rotation(uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, float *theta, float *sine, float *cosine);
/* tests: the host restatement of the canonical log2 (held to the oracle's) and L2's slice of a depth d */
float orbit_host_shade_log2(float x);
uint32_t orbit_host_shade_slice(float z_near, float d, float z_scale, float z_bias);

/* ---- asset ingestion (orbit_gltf.hpp): glTF 2.0 (.glb / .gltf) -> materials, meshes with their LOD chains, entities ----
 * load_gltf (gltf_loader.rs:511-676) + GpuAssets::add_mesh (assets/mod.rs:325-476).  NULL + orbit_host_last_error()
 * on failure.  The arrays stay valid until orbit_host_gltf_free. */
typedef struct OrbitHostGltfCounts {
    uint64_t meshes, meshlets, meshlet_data_words, materials, vertices, entities;
} OrbitHostGltfCounts;
typedef struct OrbitHostGltfEntity {
    int32_t mesh;                                /* MeshHandle slot, -1 = None */
    float position[3], orientation[4], scale[3]; /* Transform::from_mat4 of the node's world matrix */
} OrbitHostGltfEntity;
void *orbit_host_gltf_load(const char *path);
void orbit_host_gltf_free(void *scene);
void orbit_host_gltf_counts(const void *scene, OrbitHostGltfCounts *out);
const OrbitMeshInfo *orbit_host_gltf_mesh_infos(const void *scene);
const OrbitMeshlet *orbit_host_gltf_meshlets(const void *scene);
const uint32_t *orbit_host_gltf_meshlet_data(const void *scene);
const OrbitMaterialData *orbit_host_gltf_materials(const void *scene);
const float *orbit_host_gltf_vertex_positions(const void *scene);
/* copies the entities (capacity entries at most); returns their number */
uint64_t orbit_host_gltf_entities(const void *scene, OrbitHostGltfEntity *out, uint64_t capacity);
/* the LOD-chain pieces alone: meshopt::simplify's stand-in (vertex clustering); returns the indices written
 * (<= capacity, whole triangles), *needed = the full result's length */
uint64_t orbit_host_simplify_clustered(const float *positions, uint64_t vertex_count, const uint32_t *indices,
                                       uint64_t index_count, uint64_t target_index_count, uint32_t *out,
                                       uint64_t capacity, uint64_t *needed);
/* Transform::from_mat4 (scene.rs:41-48) of a column-major matrix -> position[3], orientation[4] (x, y, z, w), scale[3] */
void orbit_host_transform_from_mat4(const float matrix[16], float position[3], float orientation[4], float scale[3]);
/* The per-block pre-test of the pass-0 evaluation (orbit_amd/csrc/block_pretest.h: the same functions the device runs),
 * for tests of its certification on the host.
 * orbit_host_block_bounds: the bounds of the ceil(count / 32) blocks of `count` spheres {x, y, z, radius} (block b =
 * spheres [32 b, 32 b + 32)), as orbit_meshlet_stream_update derives them; out: 32 B per block
 * (include/orbit_abi_ext.h orbit_meshlet_stream_block_bounds).
 * orbit_host_block_pretest: one dispatch record — view x model `m` (column-major), `affine` and `scale` as the wave tile's
 * slab holds them, its block's 32-B bound (read the way the evaluation reads it), n_planes cull planes {nx, ny, nz, w} —
 * against `count` cone words.  verdicts[i]: 0 = the record is dense or the meshlet's verdict open (the literal evaluation
 * decides), 1 = certainly culled by the cone, 2 = certainly kept by the cone, 2 | 4 = ... and certainly inside every plane.
 * ratio: the record is sparse only if its block is further than ratio x its view-space radius (< 0: the evaluation's).
 * Returns the record's flags (1: sparse, 2: inside).
 * orbit_host_block_record: the record's 32-B BlockRecord itself, from block_record_setup (quad = 0) or from the form the
 * evaluation runs on four lanes per record (quad != 0: block_record_setup_quad, plane norms from block_plane_norm) — the
 * two must agree in every bit.  orbit_host_block_plane_norm: block_plane_norm of one plane's normal. */
void orbit_host_block_bounds(const float *spheres, uint64_t count, void *out);
uint32_t orbit_host_block_pretest(const float m[16], int32_t affine, float scale, const void *bound, const float *planes,
                                  uint32_t n_planes, float ratio, const uint32_t *cones, uint64_t count, uint8_t *verdicts);
void orbit_host_block_record(const float m[16], int32_t affine, float scale, const void *bound, const float *planes,
                             uint32_t n_planes, float ratio, int32_t quad, void *out);
float orbit_host_block_plane_norm(float nx, float ny, float nz);
#ifdef __cplusplus
}
#endif
#endif
