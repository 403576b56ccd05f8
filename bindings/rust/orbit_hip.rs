//! Reference-side binding of the MI355X cull engine (`include/orbit_abi.h`).
//!
//! This is the file a maintainer of Thefefe/orbit adds as `src/passes/orbit_hip.rs`; it is NOT
//! compiled in this repository (no Rust toolchain in the build image) and contains no logic:
//! `extern "C"` declarations mirroring the header, `#[repr(C)]` structs that are byte-identical to
//! the existing `GpuCullInfo` / `ClusterCullInfo`, and the two-line bodies that replace the
//! Vulkan recording in `src/passes/draw_gen.rs` and `src/passes/cluster.rs`.
#![allow(non_camel_case_types, dead_code)]
use std::ffi::{c_char, c_void};

#[repr(C)]
pub struct OrbitCtx { _private: [u8; 0] }
#[repr(C)]
pub struct OrbitMeshletStream { _private: [u8; 0] }
/// orbit_meshlet_stream_read_arrays' HOST arrays (tests): every one must be given
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitMeshletStreamArrays {
    pub sphere: *mut c_void, pub cone: *mut c_void, pub mat: *mut c_void, pub cmd: *mut c_void, pub cnt: *mut c_void,
    pub link: *mut c_void, pub cls0: *mut c_void, pub cls1: *mut c_void, pub base32: *mut c_void,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitCaps {
    pub max_entities: u32, pub max_dispatches: u32, pub max_draws: u32, pub max_lights: u32,
    pub max_clusters: u32, pub dispatch_size: u32, pub max_views: u32, pub validate_streams: u32, pub cull_path: u32,
    pub arith_profile: u32,
}

/// orbit_compute_clusters' arguments as a block (orbit_frame_late)
#[repr(C)]
pub struct OrbitClusterFrame {
    pub push: *const c_void, pub info: *const c_void, pub depth: *const f32, pub lights: *const c_void,
    pub tile_depth_slice_mask: *mut u32, pub depth_bounds: *mut c_void, pub unique_cluster_buffer: *mut c_void,
    pub light_index_buffer: *mut c_void, pub cluster_offset_image: *mut u32,
    pub index_capacity: u32, pub light_index_capacity: u32,
}
#[repr(C)]
pub struct OrbitFrameLate {
    pub pyramids: *const c_void, pub late_views: *const c_void, pub cascade_views: *const c_void,
    pub clusters: *const OrbitClusterFrame,
    pub pyramid_count: u32, pub late_view_count: u32, pub cascade_view_count: u32, pub _pad: u32,
}

/// scene.rs Transform as orbit_scene_update_entities reads it (40 B; quaternion x, y, z, w)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitEntityTransform { pub position: [f32; 3], pub orientation: [f32; 4], pub scale: [f32; 3] }

pub const ORBIT_SCENE_NONE: u32 = 0xFFFF_FFFF;

/// One entity as orbit_scene_update reads it (48 B, entity order): mesh slot and visibility offset, light kind
/// (0 Sky, 1 Directional, 2 Point) and its parameters; ORBIT_SCENE_NONE in mesh_index / light_kind = none
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitSceneEntity {
    pub mesh_index: u32, pub visibility_offset: u32, pub light_kind: u32, pub light_flags: u32,
    pub light_color: [f32; 3], pub light_intensity: f32, pub light_param: f32,
    pub irradiance_map_index: u32, pub prefiltered_map_index: u32, pub _pad: u32,
}

/// The uncapped totals orbit_scene_update leaves on the device
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitSceneCounts { pub draws: u32, pub lights: u32, pub shadows: u32, pub entities: u32 }

/// orbit_scene_update's argument block (96 B): DEVICE pointers; the last four may be null
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitSceneUpdate {
    pub entities: *const OrbitSceneEntity, pub transforms: *const OrbitEntityTransform,
    pub entity_data: *mut c_void, pub entity_draw_buffer: *mut c_void, pub light_data: *mut c_void,
    pub shadow_orientations: *mut f32, pub instance_of_entity: *mut u32, pub light_of_entity: *mut u32,
    pub counts: *mut OrbitSceneCounts,
    pub entity_count: u32, pub instance_capacity: u32, pub light_capacity: u32, pub shadow_capacity: u32,
    pub luminance_cutoff: f32, pub shadow_index_base: u32,
}

/// orbit_cull_stats' 256-B block of u64 counters (include/orbit_abi_ext.h OrbitCullStats)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitCullStats {
    pub entities: u64, pub entity_skipped_prev_invisible: u64, pub entity_frustum_culled: u64,
    pub entity_occlusion_culled: u64, pub entity_drawn_in_early_pass: u64, pub entity_drawn: u64, pub records: u64,
    pub reserved0: u64, pub lod_drawn: [u64; 8],
    pub meshlets: u64, pub meshlet_skipped_prev_invisible: u64, pub meshlet_frustum_culled: u64,
    pub meshlet_cone_culled: u64, pub meshlet_occlusion_culled: u64, pub meshlet_alpha_filtered: u64,
    pub meshlet_drawn_in_early_pass: u64, pub meshlet_drawn: u64, pub reserved1: [u64; 8],
}

/// orbit_cluster_stats' 256-B block of u64 counters (include/orbit_abi_ext.h OrbitClusterStats); the classes of a
/// cluster's uncapped light count: 0, 1-16, 17-64, 65-256, > 256
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitClusterStats {
    pub samples: u64, pub samples_outside_grid: u64, pub active_clusters: u64, pub light_refs: u64,
    pub light_indices: u64, pub max_cluster_lights: u64, pub sample_light_refs: u64, pub reserved0: u64,
    pub clusters_by_lights: [u64; 5], pub reserved1: [u64; 3], pub samples_by_lights: [u64; 5], pub reserved2: [u64; 11],
}

/// meshopt::Bounds as orbit_meshlet_bounds writes it (48 B)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitMeshletBoundsFull {
    pub center: [f32; 3], pub radius: f32, pub cone_apex: [f32; 3], pub cone_cutoff: f32, pub cone_axis: [f32; 3],
    pub cone_axis_s8: [i8; 3], pub cone_cutoff_s8: i8,
}

pub const ORBIT_BOUNDS_KEEP_RECORDS: u32 = 1;

/// orbit_meshlet_bounds' argument block (96 B, HOST): DEVICE pointers; meshlet_indices and full may be null
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitMeshletBoundsJob {
    pub meshlets: *mut c_void, pub meshlet_data: *const u32, pub vertices: *const c_void,
    pub meshlet_indices: *const u32, pub full: *mut OrbitMeshletBoundsFull,
    pub first_meshlet: u64, pub meshlet_count: u64, pub meshlet_capacity: u64, pub meshlet_data_words: u64,
    pub vertex_count: u64,
    pub vertex_stride: u32, pub position_offset: u32, pub flags: u32, pub _pad: u32,
}

/// One mesh of orbit_mesh_bounds (12 B, DEVICE): the vertices [first_vertex, first_vertex + vertex_count)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitMeshBoundsRange { pub mesh_index: u32, pub first_vertex: u32, pub vertex_count: u32 }

/// The counters of orbit_raster_depth (32 B, DEVICE)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitRasterStats {
    pub commands: u32, pub triangles: u32, pub clip_skipped: u32, pub guard_skipped: u32, pub back_facing: u32,
    pub no_coverage: u32, pub fragments: u32, pub range_errors: u32,
}

pub const ORBIT_RASTER_CLEAR: u32 = 1;
pub const ORBIT_RASTER_CULL_NONE: u32 = 2;
pub const ORBIT_RASTER_CLIP_NEAR: u32 = 8; // (4 is no flag)
pub const ORBIT_RASTER_WIDE_GUARD: u32 = 32; // (16 is no flag)
pub const ORBIT_RASTER_MAX_DIM: u32 = 32768;

/// orbit_raster_depth's argument block (160 B, HOST): DEVICE pointers; stats may be null
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitRasterDepth {
    pub draw_commands: *const c_void, pub meshlet_data: *const u32, pub vertices: *const c_void,
    pub entity_data: *const c_void, pub depth: *mut f32, pub stats: *mut OrbitRasterStats,
    pub meshlet_data_words: u64, pub vertex_count: u64,
    pub max_commands: u32, pub entity_count: u32, pub vertex_stride: u32, pub position_offset: u32,
    pub width: u32, pub height: u32, pub flags: u32, pub _pad: u32,
    pub view_proj: [f32; 16],
}

pub const ORBIT_VIS_MAX_COMMANDS: u32 = 1 << 24;

/// orbit_raster_visibility's argument block (160 B, HOST): OrbitRasterDepth with the u64 buffer and command_base
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitRasterVisibility {
    pub draw_commands: *const c_void, pub meshlet_data: *const u32, pub vertices: *const c_void,
    pub entity_data: *const c_void, pub visibility: *mut u64, pub stats: *mut OrbitRasterStats,
    pub meshlet_data_words: u64, pub vertex_count: u64,
    pub max_commands: u32, pub entity_count: u32, pub vertex_stride: u32, pub position_offset: u32,
    pub width: u32, pub height: u32, pub flags: u32, pub command_base: u32,
    pub view_proj: [f32; 16],
}

/// The counters of orbit_visibility_resolve (16 B, DEVICE)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitVisibilityStats { pub covered_pixels: u32, pub visible_commands: u32, pub foreign_pixels: u32, pub _pad: u32 }

pub const ORBIT_COMPACT_TRIANGLES: u32 = 1;

/// The counters of orbit_visibility_compact (32 B, DEVICE, cleared by the call)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitVisibilityCompactStats {
    pub covered_pixels: u32, pub foreign_pixels: u32, pub visible_commands: u32, pub visible_triangles: u32,
    pub written_commands: u32, pub dropped_commands: u32, pub data_words_needed: u32, pub range_errors: u32,
}

/// orbit_visibility_compact's argument block (120 B, HOST): DEVICE pointers; visible_ids and stats may be null,
/// meshlet_data and visible_data only without ORBIT_COMPACT_TRIANGLES
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitVisibilityCompact {
    pub visibility: *const u64, pub draw_commands: *const c_void, pub meshlet_data: *const u32,
    pub triangle_masks: *mut u32, pub visible_commands: *mut c_void, pub visible_ids: *mut u32,
    pub visible_data: *mut u32, pub stats: *mut OrbitVisibilityCompactStats, pub workspace: *mut c_void,
    pub meshlet_data_words: u64, pub workspace_bytes: u64,
    pub width: u32, pub height: u32, pub command_base: u32, pub max_commands: u32,
    pub visible_capacity: u32, pub visible_data_words: u32, pub flags: u32, pub _pad: u32,
}

pub const ORBIT_SURFACE_CLEAR: u32 = 1;

/// The counters of orbit_visibility_surface (32 B, DEVICE, cleared by the call): covered = written + foreign +
/// unsupported + stale.  cut_pixels and wide_pixels are orbit_visibility_surface_drawn's (written from a piece of a
/// near-cut triangle, from a wide setup); orbit_visibility_surface leaves them 0
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitSurfaceStats {
    pub covered_pixels: u32, pub written_pixels: u32, pub foreign_pixels: u32, pub unsupported_pixels: u32,
    pub stale_pixels: u32, pub degenerate_pixels: u32, pub cut_pixels: u32, pub wide_pixels: u32,
}

/// orbit_visibility_surface's argument block (184 B, HOST): DEVICE pointers; bary (2 f32 per pixel), grad (4 f32),
/// triangle (4 u32) and stats may be null, not all three outputs
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitVisibilitySurface {
    pub visibility: *const u64, pub draw_commands: *const c_void, pub meshlet_data: *const u32,
    pub vertices: *const c_void, pub entity_data: *const c_void,
    pub bary: *mut f32, pub grad: *mut f32, pub triangle: *mut u32, pub stats: *mut OrbitSurfaceStats,
    pub meshlet_data_words: u64, pub vertex_count: u64,
    pub max_commands: u32, pub entity_count: u32, pub vertex_stride: u32, pub position_offset: u32,
    pub width: u32, pub height: u32, pub flags: u32, pub command_base: u32,
    pub view_proj: [f32; 16],
}

pub const ORBIT_FRAGMENTS_CLEAR: u32 = 1;

/// The counters of orbit_surface_fragments (32 B, DEVICE, cleared by the call): covered = written + foreign + unshaded +
/// stale
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitFragmentStats {
    pub covered_pixels: u32, pub written_pixels: u32, pub foreign_pixels: u32, pub unshaded_pixels: u32,
    pub stale_pixels: u32, pub degenerate_pixels: u32, pub _pad: [u32; 2],
}

/// orbit_surface_fragments' argument block (176 B, HOST): DEVICE pointers; bary, grad and triangle as a surface call left
/// them (grad may be null, then uv_grad is); the six outputs and stats may be null, not all six.  MeshVertex (mesh.rs:14-20)
/// is vertex_stride 32 with position / normal / uv / tangent at 0 / 12 / 16 / 24
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitSurfaceFragments {
    pub visibility: *const u64, pub draw_commands: *const c_void, pub meshlets: *const c_void,
    pub bary: *const f32, pub grad: *const f32, pub triangle: *const u32,
    pub vertices: *const c_void, pub entity_data: *const c_void,
    pub world_pos: *mut f32, pub normal: *mut f32, pub tangent: *mut f32, pub uv: *mut f32, pub uv_grad: *mut f32,
    pub material: *mut u32, pub stats: *mut OrbitFragmentStats,
    pub vertex_count: u64,
    pub meshlet_count: u32, pub max_commands: u32, pub entity_count: u32, pub vertex_stride: u32,
    pub position_offset: u32, pub normal_offset: u32, pub uv_offset: u32, pub tangent_offset: u32,
    pub width: u32, pub height: u32, pub flags: u32, pub command_base: u32,
}

pub const ORBIT_SHADE_CLEAR: u32 = 1;
pub const ORBIT_SHADE_FORCE_PER_LANE: u32 = 2;
pub const ORBIT_SHADE_FORCE_STAGED: u32 = 4;

/// The counters of orbit_fragments_shade (32 B, DEVICE, cleared by the call): covered = written + unshaded + stale; the
/// other five count written pixels
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitShadeStats {
    pub covered_pixels: u32, pub written_pixels: u32, pub unshaded_pixels: u32, pub stale_pixels: u32,
    pub outside_pixels: u32, pub degenerate_pixels: u32, pub textured_pixels: u32, pub unserved_pixels: u32,
}

/// orbit_fragments_shade's argument block (160 B, HOST): DEVICE pointers; world_pos, normal and material as
/// orbit_surface_fragments left them under ORBIT_FRAGMENTS_CLEAR; cluster_offset_image and light_index_buffer
/// (ClusterLightIndices, index_capacity indices behind its 4-byte header) as orbit_compute_clusters left them; cluster_count,
/// tile_size_px, z_scale, z_bias, luminance_cutoff: the fields of GpuClusterInfoBuffer (cluster.rs:322-335); z_near and
/// view_pos: PerFrameBuffer's; render_mode 0 or 8; lights_walked and stats may be null
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitFragmentsShade {
    pub visibility: *const u64, pub world_pos: *const f32, pub normal: *const f32, pub material: *const u32,
    pub materials: *const c_void, pub lights: *const c_void, pub cluster_offset_image: *const u32,
    pub light_index_buffer: *const c_void,
    pub color: *mut f32, pub lights_walked: *mut u32, pub stats: *mut OrbitShadeStats,
    pub material_count: u32, pub light_count: u32, pub index_capacity: u32,
    pub cluster_count: [u32; 3], pub tile_size_px: u32,
    pub z_scale: f32, pub z_bias: f32, pub luminance_cutoff: f32,
    pub z_near: f32, pub view_pos: [f32; 3],
    pub render_mode: u32, pub width: u32, pub height: u32, pub flags: u32,
}

/// One row of ShadowDataBuffer (288 B, DEVICE; types.glsl:29-33 in std430): four column-major light_projection_matrices,
/// their shadow_map_world_sizes, and shadow_map_indices into orbit_fragments_shade_shadowed's shadow_maps array (the
/// caller maps its bindless indices onto it)
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitShadowData {
    pub light_projection_matrices: [[f32; 16]; 4], pub shadow_map_world_sizes: [f32; 4], pub shadow_map_indices: [u32; 4],
}

/// The counters orbit_fragments_shade_shadowed adds (16 B, DEVICE, cleared by the call), over written pixels
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitShadowStats {
    pub shadowed_pixels: u32, pub no_cascade_pixels: u32, pub early_out_pixels: u32, pub shadow_evaluations: u32,
}

/// orbit_fragments_shade_shadowed's argument block (232 B, HOST): an OrbitFragmentsShade, then the shadow rows
/// (shadow_count of them, 16-B aligned), the maps (shadow_map_count squares of shadow_resolution^2 f32, reversed z, as
/// orbit_raster_depth leaves them under a cascade's matrix with ORBIT_RASTER_CLEAR), the optional outputs shadow_factor,
/// cascade and shadow_stats (may be null), shadow_index_base = MAX_SHADOW_COMMANDS * frame_index, and ShadowSettings'
/// blocker_search_radius, normal_bias_scale and oriented_bias (as shadow_renderer.rs:129 sends it: negated)
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitFragmentsShadeShadowed {
    pub shade: OrbitFragmentsShade,
    pub shadows: *const OrbitShadowData, pub shadow_maps: *const f32,
    pub shadow_factor: *mut f32, pub cascade: *mut u32, pub shadow_stats: *mut OrbitShadowStats,
    pub shadow_count: u32, pub shadow_index_base: u32, pub shadow_map_count: u32, pub shadow_resolution: u32,
    pub blocker_search_radius: f32, pub normal_bias_scale: f32, pub oriented_bias: f32, pub _pad: u32,
}

/// orbit_bloom_layout's result (88 B, HOST): max_levels is read (1..6, 0 = 6); level k is level_width[k] x level_height[k]
/// packed texels starting at texel level_offset[k] of mips (bloom.rs:60-80: level 0 is the full size, at most six levels)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitBloomLayout {
    pub max_levels: u32, pub levels: u32, pub total_texels: u32, pub _pad: u32,
    pub level_width: [u32; 6], pub level_height: [u32; 6], pub level_offset: [u32; 6],
}

/// The counters of orbit_bloom (16 B, DEVICE, cleared by the call)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitBloomStats {
    pub levels: u32, pub texels_written: u32, pub nonfinite_inputs: u32, pub clamped_texels: u32,
}

pub const ORBIT_BLOOM_FORCE_PER_LEVEL: u32 = 1;
pub const ORBIT_BLOOM_FORCE_DIRECT: u32 = 4;
pub const ORBIT_POST_BGRA: u32 = 1;

/// orbit_bloom's argument block (56 B, HOST): the shade calls' colour plane (4 f32 per pixel, 16-B aligned), the packed
/// B10G11R11 mip chain in OrbitBloomLayout's layout (total_texels u32), the optional counters, and BloomSettings'
/// threshold, soft_threshold and filter_radius (bloom.rs:12-17); compute_bloom (bloom.rs:54-174) by rules B1-B9
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitBloom {
    pub color: *const f32, pub mips: *mut u32, pub stats: *mut OrbitBloomStats,
    pub width: u32, pub height: u32,
    pub threshold: f32, pub soft_threshold: f32, pub filter_radius: f32,
    pub max_levels: u32, pub flags: u32, pub _pad: u32,
}

/// The counters of orbit_post_process (16 B, DEVICE, cleared by the call)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitPostStats {
    pub pixels: u32, pub nonfinite_pixels: u32, pub bloom_pixels: u32, pub _pad: u32,
}

/// orbit_post_process's argument block (64 B, HOST): colour, level 0 of the bloom chain (or null), the outputs ldr (4 f32
/// per pixel) and rgba8 (4 bytes per pixel; at least one of the two), the optional counters, and the push constants of
/// post_process.frag:47-56 that are served: exposure, bloom_intensity, render_mode (0 or 8); rules T1-T5
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitPostProcess {
    pub color: *const f32, pub bloom: *const u32, pub ldr: *mut f32, pub rgba8: *mut u8, pub stats: *mut OrbitPostStats,
    pub exposure: f32, pub bloom_intensity: f32, pub render_mode: u32, pub width: u32, pub height: u32, pub flags: u32,
}

/// The counters of orbit_ssao (24 B, DEVICE, 8-B aligned, cleared by the call)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitSsaoStats {
    pub pixels: u32, pub nonfinite_pixels: u32, pub unoccluded_pixels: u32, pub _pad: u32,
    pub samples_in_range: u64,
}

/// orbit_ssao's argument block (224 B, HOST): the depth plane (f32, reverse-z), SsaoRenderer's noise (R8G8_SNORM) and
/// samples (R8G8B8A8_UNORM) textures as bytes, the outputs raw and blurred (R8, ssao_w x ssao_h; ssao.rs:99-127) and
/// ao_pixel (f32 per screen pixel: forward.frag:336-337's sample), the optional counters, and GpuSSAOInfo's matrices,
/// sizes and settings (ssao.rs:50-67); rules A1-A9
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitSsao {
    pub depth: *const f32, pub noise: *const i8, pub samples: *const u8,
    pub raw: *mut u8, pub blurred: *mut u8, pub ao_pixel: *mut f32, pub stats: *mut OrbitSsaoStats,
    pub projection: [f32; 16], pub inverse_projection: [f32; 16],
    pub screen_w: u32, pub screen_h: u32, pub ssao_w: u32, pub ssao_h: u32,
    pub noise_size: u32, pub samples_size: u32, pub sample_count: u32,
    pub min_radius: f32, pub max_radius: f32, pub flags: u32,
}

/// The counters orbit_fragments_shade_sky adds (32 B, DEVICE, 8-B aligned, cleared by the call; rule K10): SKY lights
/// evaluated over written pixels, written pixels with at least one, pixels the skybox wrote, E4's bad directions over every
/// cube sample of the call
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitSkyStats {
    pub sky_evaluations: u32, pub sky_lit_pixels: u32, pub skybox_pixels: u32, pub _pad: u32,
    pub bad_directions: u64, pub _pad2: u64,
}

/// orbit_fragments_shade_sky's argument block (344 B, HOST): an OrbitFragmentsShadeShadowed, then the environment
/// (irradiance, prefiltered and brdf as orbit_env_map writes them: all three or none), the sky cube (null: no skybox),
/// the ao plane (null, or orbit_ssao's ao_pixel), the counters (may be null), the images' sizes and level counts, the
/// skybox's constant lod and K9's ray basis (orbit_host_skybox_basis)
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitFragmentsShadeSky {
    pub shadowed: OrbitFragmentsShadeShadowed,
    pub irradiance: *const u16, pub prefiltered: *const u16, pub brdf: *const u16, pub sky: *const u16,
    pub ao: *const f32, pub sky_stats: *mut OrbitSkyStats,
    pub irradiance_size: u32, pub prefiltered_size: u32, pub prefiltered_levels: u32, pub brdf_size: u32,
    pub sky_size: u32, pub sky_levels: u32, pub skybox_lod: f32,
    pub sky_x: [f32; 3], pub sky_y: [f32; 3], pub sky_z: [f32; 3],
}

/// orbit_env_map_layout's answer (264 B, HOST): sizes and offsets in texels of the sky cube's full chain and the
/// prefiltered cube's levels (8-B texels), the irradiance cube and the BRDF table (4-B texels); rule E0
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitEnvMapLayout {
    pub sky_size: u32, pub sky_levels: u32, pub irradiance_size: u32, pub prefiltered_size: u32, pub prefiltered_levels: u32, pub brdf_size: u32,
    pub sky_level_size: [u32; 13], pub sky_level_offset: [u32; 13],
    pub prefiltered_level_size: [u32; 13], pub prefiltered_level_offset: [u32; 13],
    pub sky_texels: u64, pub irradiance_texels: u64, pub prefiltered_texels: u64, pub brdf_texels: u64,
}

/// The counters of orbit_env_map (48 B, DEVICE, 8-B aligned, cleared by the call; rule E8)
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct OrbitEnvMapStats {
    pub sky_nonfinite: u64, pub irradiance_nonfinite: u64, pub prefiltered_nonfinite: u64, pub brdf_nonfinite: u64,
    pub bad_directions: u64, pub _pad: u64,
}

/// orbit_env_map's argument block (96 B, HOST): the panorama (f32 RGBA; null: `sky` is the caller's), the four products
/// (R16G16B16A16_SFLOAT cubes in E0's layout, the R16G16_SFLOAT table; null: not made), the optional counters, the sizes
/// of orbit_env_map_layout and env_map_loader.rs' constants (sample_count 4096, sample_delta 0.025, brdf_sample_count
/// 1024); rules E0-E12
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitEnvMap {
    pub equirect: *const f32, pub sky: *mut u16, pub irradiance: *mut u16, pub prefiltered: *mut u16, pub brdf: *mut u16,
    pub stats: *mut OrbitEnvMapStats,
    pub equirect_w: u32, pub equirect_h: u32,
    pub sky_size: u32, pub irradiance_size: u32, pub prefiltered_size: u32, pub prefiltered_levels: u32, pub brdf_size: u32,
    pub sample_count: u32, pub sample_delta: f32, pub brdf_sample_count: u32, pub flags: u32, pub _pad: u32,
}

/// orbit_env_sample's argument block (56 B, HOST): a cube in E0's layout, n directions and lods, n rgb results and the
/// optional counter of bad directions; rule E4
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitEnvSample {
    pub cube: *const u16, pub directions: *const f32, pub lods: *const f32, pub rgb: *mut f32, pub bad_directions: *mut u64,
    pub size: u32, pub levels: u32, pub n: u32, pub flags: u32,
}

/// orbit_visibility_resolve's argument block (48 B, HOST): DEVICE pointers; each output may be null, not all
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitVisibilityResolve {
    pub visibility: *const u64, pub depth: *mut f32, pub command_pixels: *mut u32, pub stats: *mut OrbitVisibilityStats,
    pub width: u32, pub height: u32, pub command_base: u32, pub max_commands: u32,
}

/// push-constant order of shaders/entity_cull.comp:17-23 (== draw_gen.rs:372-376)
#[repr(C)]
pub struct OrbitEntityCullBufs {
    pub entity_draw_buffer: *const c_void, pub mesh_info_buffer: *const c_void,
    pub meshlet_dispatch_buffer: *mut c_void, pub entity_buffer: *const c_void,
    pub visibility_buffer: *mut u32, pub depth_pyramid: *const f32,
    pub depth_pyramid_size: [u32; 2], pub dispatch_capacity: u32, pub _pad: u32,
    /// null: `depth_pyramid` is the packed chain; else a DEVICE array of mip levels (separate per-mip images)
    pub depth_pyramid_levels: *const OrbitDepthPyramidLevel,
}

/// One view of orbit_cull_views (the frame's early pass and shadow cascades culled side by side)
#[repr(C)]
pub struct OrbitCullView {
    pub cull_info: *const c_void, pub entity: OrbitEntityCullBufs, pub meshlet: OrbitMeshletCullBufs,
    pub entity_draw_count: u32, pub skip_meshlet_stage: u32,
}

/// One mip of a pyramid that is not one packed buffer (linear-tiled image per level: INTEGRATION.md)
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitDepthPyramidLevel { pub texels: *mut f32, pub row_pitch: u32, pub _pad: u32 }

/// One pyramid of orbit_depth_reduce_multi; exactly one of `pyramid` / `levels` (HOST array) is non-null
#[repr(C)]
pub struct OrbitDepthReduceItem {
    pub depth: *const f32, pub screen_width: u32, pub screen_height: u32, pub depth_row_pitch: u32, pub _pad: u32,
    pub pyramid: *mut f32, pub levels: *const OrbitDepthPyramidLevel,
}

/// push-constant order of shaders/meshlet_cull.comp:16-23 (== draw_gen.rs:426-431)
#[repr(C)]
pub struct OrbitMeshletCullBufs {
    pub meshlet_dispatch_buffer: *const c_void, pub meshlet_buffer: *const c_void,
    pub draw_commands_buffer: *mut c_void, pub entity_buffer: *const c_void,
    pub material_buffer: *const c_void, pub meshlet_visibility_buffer: *mut u32,
    pub depth_pyramid: *const f32, pub depth_pyramid_size: [u32; 2],
    pub dispatch_capacity: u32, pub draw_capacity: u32, pub material_count: u32, pub _pad: u32,
    pub depth_pyramid_levels: *const OrbitDepthPyramidLevel,
}

pub const ORBIT_MAX_PYRAMID_MIPS: usize = 16;
/// Geometry of the R32F mip chain `DepthPyramid::new` allocates (draw_gen.rs:456-494); buffer = 4 * total_texels bytes.
#[repr(C)] #[derive(Clone, Copy)]
pub struct OrbitDepthPyramidDesc {
    pub width: u32, pub height: u32, pub mip_levels: u32, pub total_texels: u32,
    pub mip_offset: [u32; ORBIT_MAX_PYRAMID_MIPS], pub mip_width: [u32; ORBIT_MAX_PYRAMID_MIPS],
    pub mip_height: [u32; ORBIT_MAX_PYRAMID_MIPS],
}

#[link(name = "orbit_cull")]
extern "C" {
    pub fn orbit_abi_version() -> u32;
    pub fn orbit_default_caps(caps: *mut OrbitCaps);
    pub fn orbit_ctx_create(device_id: i32, caps: *const OrbitCaps, out: *mut *mut OrbitCtx) -> i32;
    pub fn orbit_ctx_destroy(ctx: *mut OrbitCtx) -> i32;
    pub fn orbit_last_error(ctx: *const OrbitCtx) -> *const c_char;
    pub fn orbit_ctx_status(ctx: *mut OrbitCtx, stream: *mut c_void, sync: i32) -> i32;
    /// `cull_info` = `bytemuck::bytes_of(&GpuCullInfo)` (400 B, draw_gen.rs:208-237), a HOST pointer
    pub fn orbit_entity_cull(ctx: *mut OrbitCtx, cull_info: *const c_void, bufs: *const OrbitEntityCullBufs,
                             entity_draw_count: u32, stream: *mut c_void) -> i32;
    pub fn orbit_entity_cull_range(ctx: *mut OrbitCtx, cull_info: *const c_void, bufs: *const OrbitEntityCullBufs,
                                   draw_first: u32, draw_count: u32, stream: *mut c_void) -> i32;
    pub fn orbit_meshlet_cull(ctx: *mut OrbitCtx, cull_info: *const c_void, bufs: *const OrbitMeshletCullBufs,
                              stream: *mut c_void) -> i32;
    /// Host only: pyramid geometry for a screen size / from the mip-0 size the cull kernels see.
    pub fn orbit_depth_pyramid_desc(screen_w: u32, screen_h: u32, desc: *mut OrbitDepthPyramidDesc) -> i32;
    pub fn orbit_depth_pyramid_desc_from_mip0(mip0_w: u32, mip0_h: u32, desc: *mut OrbitDepthPyramidDesc) -> i32;
    /// Measurement hooks: HIP events around the dominant kernel on the launch stream.
    pub fn orbit_ctx_profile(ctx: *mut OrbitCtx, enable: i32) -> i32;
    pub fn orbit_ctx_profile_reserve(ctx: *mut OrbitCtx, pairs: u32, stream: *mut c_void) -> i32;
    pub fn orbit_ctx_profile_read(ctx: *mut OrbitCtx, avg_ms: *mut f32, launches: *mut u32) -> i32;
    pub fn orbit_cull_views(ctx: *mut OrbitCtx, views: *const OrbitCullView, count: u32, stream: *mut c_void) -> i32;
    pub fn orbit_depth_reduce(ctx: *mut OrbitCtx, depth: *const f32, screen_w: u32, screen_h: u32,
                              pyramid: *mut f32, stream: *mut c_void) -> i32;
    /// update_multiple_depth_pyramids::<C> (draw_gen.rs:569-628): up to 8 pyramids in one launch
    pub fn orbit_depth_reduce_multi(ctx: *mut OrbitCtx, items: *const OrbitDepthReduceItem, count: u32,
                                    stream: *mut c_void) -> i32;
    pub fn orbit_cluster_mark(ctx: *mut OrbitCtx, push: *const c_void, depth: *const f32, masks: *mut u32,
                              bounds: *mut c_void, stream: *mut c_void) -> i32;
    pub fn orbit_cluster_compact(ctx: *mut OrbitCtx, cluster_count: *const [u32; 3], masks: *const u32,
                                 unique: *mut c_void, index_capacity: u32, stream: *mut c_void) -> i32;
    pub fn orbit_cluster_assign(ctx: *mut OrbitCtx, info: *const c_void, unique: *const c_void, bounds: *const c_void,
                                lights: *const c_void, light_index_buffer: *mut c_void, light_index_capacity: u32,
                                cluster_offset_image: *mut u32, stream: *mut c_void) -> i32;
    /// Mesh-shading path: per dispatch record the EmitMeshTasksEXT count + MeshTaskPayload (44 B) that the task
    /// shaders (forward_depth_prepass.task, forward.task) compute; a task shader then only loads its record.
    pub fn orbit_meshlet_task_cull(ctx: *mut OrbitCtx, cull_info: *const c_void, bufs: *const c_void,
                                   task_records: *mut c_void, stream: *mut c_void) -> i32;
    /// compute_clusters (cluster.rs:368-397): the three stages in one call.
    pub fn orbit_compute_clusters(ctx: *mut OrbitCtx, push: *const c_void, info: *const c_void, depth: *const f32,
                                  lights: *const c_void, masks: *mut u32, bounds: *mut c_void, unique: *mut c_void,
                                  index_capacity: u32, light_index_buffer: *mut c_void, light_index_capacity: u32,
                                  cluster_offset_image: *mut u32, stream: *mut c_void) -> i32;
    /// Sharded engine: the shard range; SURVEY §8b's gather of 28-B command lists over the caller's ncclComm_t (one host sync).
    pub fn orbit_shard_range(entity_draw_count: u32, rank: u32, world: u32, begin: *mut u32, end: *mut u32);
    pub fn orbit_gather_visible(ctx: *mut OrbitCtx, nccl_comm: *mut c_void, rank: u32, world: u32,
                                local_draw_buffer: *const c_void, out_draw_buffer: *mut c_void, out_capacity: u32,
                                stream: *mut c_void) -> i32;
    /// The sharded engine's visible list: 12 B {entity_index, meshlet_offset, mask} per dispatch record, written by the
    /// evaluation launch itself; expanded on the receiving side.
    pub fn orbit_meshlet_cull_visible_records(ctx: *mut OrbitCtx, cull_info: *const c_void, bufs: *const c_void,
                                              record_buffer: *mut c_void, record_capacity: u32,
                                              stream: *mut c_void) -> i32;
    pub fn orbit_expand_visible_records(ctx: *mut OrbitCtx, record_buffer: *const c_void, meshlet_buffer: *const c_void,
                                        draw_commands_buffer: *mut c_void, draw_capacity: u32,
                                        stream: *mut c_void) -> i32;
    // derived meshlet streams: GpuAssets::add_mesh calls `update` for the range it wrote (assets/mod.rs:441-445),
    // every cull context binds the stream once
    pub fn orbit_meshlet_stream_create(ctx: *mut OrbitCtx, first_meshlet: u64, capacity: u64,
                                       out_stream: *mut *mut OrbitMeshletStream) -> i32;
    pub fn orbit_meshlet_stream_update(ctx: *mut OrbitCtx, ms: *mut OrbitMeshletStream, meshlet_buffer: *const c_void,
                                       first: u64, count: u64, stream: *mut c_void) -> i32;
    // GpuAssets::add_material calls `set_materials` after the upload (assets/mod.rs:520): the alpha classes
    pub fn orbit_meshlet_stream_set_materials(ctx: *mut OrbitCtx, ms: *mut OrbitMeshletStream, material_buffer: *const c_void,
                                              material_count: u32, stream: *mut c_void) -> i32;
    pub fn orbit_meshlet_stream_validate(ctx: *mut OrbitCtx, ms: *mut OrbitMeshletStream, meshlet_buffer: *const c_void,
                                         material_buffer: *const c_void, stream: *mut c_void) -> i32;
    pub fn orbit_meshlet_stream_destroy(ms: *mut OrbitMeshletStream) -> i32;
    // GpuAssets::add_mesh calls `update_meshes` for the MeshInfo it wrote (assets/mod.rs:18-28): the entity stage then
    // reads a 32-B side entry per mesh instead of the 128-B MeshInfo line
    pub fn orbit_meshlet_stream_update_meshes(ctx: *mut OrbitCtx, ms: *mut OrbitMeshletStream, mesh_info_buffer: *const c_void,
                                              first_mesh: u32, count: u32, stream: *mut c_void) -> i32;
    pub fn orbit_ctx_mesh_side_culls(ctx: *const OrbitCtx) -> u64;
    pub fn orbit_ctx_bind_meshlet_stream(ctx: *mut OrbitCtx, ms: *mut OrbitMeshletStream) -> i32;
    pub fn orbit_ctx_fused_culls(ctx: *const OrbitCtx) -> u64;
    /// The late half of a frame (app.rs:1151-1212) with its independent chains side by side: {pyramids -> late culls} on
    /// `stream`, {cascade culls} and {compute_clusters} on two streams of the context, forked and joined by events.
    pub fn orbit_frame_late(ctx: *mut OrbitCtx, frame: *const OrbitFrameLate, stream: *mut c_void) -> i32;
    pub fn orbit_ctx_meshlet_stream_culls(ctx: *const OrbitCtx) -> u64;
    pub fn orbit_ctx_meshlet_class_culls(ctx: *const OrbitCtx) -> u64;
    /// Pass-0 culls decided per block of 32 meshlets from the stream's block bounds (on by default; same outputs).
    pub fn orbit_ctx_block_culls(ctx: *const OrbitCtx) -> u64;
    pub fn orbit_ctx_set_block_cull(ctx: *mut OrbitCtx, enable: u32) -> i32;
    pub fn orbit_ctx_set_block_cull_grid(ctx: *mut OrbitCtx, max_workgroups: u32) -> i32;
    pub fn orbit_ctx_set_raster_grid(ctx: *mut OrbitCtx, max_workgroups: u32) -> i32;
    pub fn orbit_ctx_set_visibility_grid(ctx: *mut OrbitCtx, max_workgroups: u32) -> i32;
    pub fn orbit_ctx_set_fused_grid(ctx: *mut OrbitCtx, max_workgroups: u32) -> i32;
    pub fn orbit_meshlet_stream_block_bounds(ctx: *mut OrbitCtx, ms: *mut OrbitMeshletStream, first_block: u64, count: u64,
                                             out: *mut c_void, stream: *mut c_void) -> i32;
    /// Tests: the stream's derived arrays of meshlets [first, first + count) into host arrays.
    pub fn orbit_meshlet_stream_read_arrays(ctx: *mut OrbitCtx, ms: *mut OrbitMeshletStream, first: u64, count: u64,
                                            out: *const OrbitMeshletStreamArrays, stream: *mut c_void) -> i32;
    // exchange without a host in the step: IPC-mapped peer buffers + a device-signalled rank-ordered scatter (orbit_exchange_list)
    pub fn orbit_p2p_alloc(ctx: *mut OrbitCtx, bytes: u64, out_ptr: *mut *mut c_void, out_handle: *mut [u8; 64]) -> i32;
    pub fn orbit_p2p_free(ctx: *mut OrbitCtx, ptr: *mut c_void) -> i32;
    pub fn orbit_p2p_open(ctx: *mut OrbitCtx, handle: *const [u8; 64], out_peer_ptr: *mut *mut c_void) -> i32;
    pub fn orbit_p2p_close(ctx: *mut OrbitCtx, peer_ptr: *mut c_void) -> i32;
    pub fn orbit_meshlet_cull_records_and_commands(ctx: *mut OrbitCtx, cull_info: *const c_void,
                                                   bufs: *const OrbitMeshletCullBufs, record_buffer: *mut c_void,
                                                   record_capacity: u32, stream: *mut c_void) -> i32;
    pub fn orbit_exchange_list(ctx: *mut OrbitCtx, local_list: *const c_void, rank: u32, world: u32,
                               out_buffers: *const *mut c_void, ctrl_buffers: *const *mut c_void, out_capacity: u32,
                               header_bytes: u32, stride: u32, stream: *mut c_void) -> i32;
    /// A rank's whole cull (entity range + meshlet stage into the record list [+ its own commands]) as one call — one
    /// launch for pass 0 and up to 65 536 entity-draws.
    pub fn orbit_cull_shard(ctx: *mut OrbitCtx, cull_info: *const c_void, entity_bufs: *const OrbitEntityCullBufs,
                            draw_first: u32, draw_count: u32, meshlet_bufs: *const OrbitMeshletCullBufs,
                            record_buffer: *mut c_void, record_capacity: u32, with_commands: u32,
                            stream: *mut c_void) -> i32;
    pub fn orbit_ctx_shard_culls(ctx: *const OrbitCtx) -> u64;
    /// north_star's transport, device-only: ONE ncclAllGather of the ranks' fixed-capacity list segments, then one
    /// launch that compacts them into the contiguous rank-ordered list (no count on the host, no stream wait).
    pub fn orbit_allgather_list(ctx: *mut OrbitCtx, nccl_comm: *mut c_void, rank: u32, world: u32,
                                local_list: *const c_void, segment_capacity: u32, segments: *mut c_void,
                                out_list: *mut c_void, out_capacity: u32, header_bytes: u32, stride: u32,
                                stream: *mut c_void) -> i32;
    pub fn orbit_compact_segments(ctx: *mut OrbitCtx, segments: *const c_void, world: u32, segment_capacity: u32,
                                  out_list: *mut c_void, out_capacity: u32, header_bytes: u32, stride: u32,
                                  stream: *mut c_void) -> i32;
    /// SceneData::update_scene's EntityData rows computed on the device from the entities' transforms: all of them
    /// (instance_indices null, count <= entity_capacity) or only the rows named by a DEVICE list of instance indices.
    pub fn orbit_scene_update_entities(ctx: *mut OrbitCtx, transforms: *const OrbitEntityTransform,
                                       instance_indices: *const u32, count: u32, entity_data: *mut c_void,
                                       entity_capacity: u32, stream: *mut c_void) -> i32;
    /// All of SceneData::update_scene on the device, from one OrbitSceneEntity and one transform per entity in entity
    /// order: EntityData rows, the EntityDrawBuffer, LightData rows with shadow indices, shadow orientations, maps.
    pub fn orbit_scene_update(ctx: *mut OrbitCtx, update: *const OrbitSceneUpdate, stream: *mut c_void) -> i32;
    /// What orbit_entity_cull + orbit_meshlet_cull with these arguments would do, counted per test into a DEVICE
    /// OrbitCullStats (overwritten).  Call it BEFORE the cull: passes 1 and 2 rewrite the visibility words it reads.
    pub fn orbit_cull_stats(ctx: *mut OrbitCtx, cull_info: *const c_void, ebufs: *const OrbitEntityCullBufs,
                            entity_draw_count: u32, mbufs: *const OrbitMeshletCullBufs, stats: *mut OrbitCullStats,
                            stream: *mut c_void) -> i32;
    /// The uncapped counts of orbit_compute_clusters for these inputs into a DEVICE OrbitClusterStats (overwritten).
    /// Writes nothing else, uses no context scratch: before, after or beside the chain.
    pub fn orbit_cluster_stats(ctx: *mut OrbitCtx, push: *const c_void, info: *const c_void, depth: *const f32,
                               lights: *const c_void, stats: *mut OrbitClusterStats, stream: *mut c_void) -> i32;
    /// Bounding sphere, snorm8 cone axis and cutoff (bytes 0..19) of the selected Meshlet records recomputed on the
    /// device from the vertex buffer, bit-equal to meshopt's bounds as the host mirror restates them.  Call it after a
    /// vertex write and before orbit_meshlet_stream_update of the same range.
    pub fn orbit_meshlet_bounds(ctx: *mut OrbitCtx, job: *const OrbitMeshletBoundsJob, stream: *mut c_void) -> i32;
    /// Sphere and AABB of mesh_infos[mesh_index] per DEVICE range of vertices (gltf_loader.rs:480-506); then
    /// orbit_meshlet_stream_update_meshes if a mesh side table is bound.
    pub fn orbit_mesh_bounds(ctx: *mut OrbitCtx, ranges: *const OrbitMeshBoundsRange, range_count: u32,
                             vertices: *const c_void, vertex_count: u64, vertex_stride: u32, position_offset: u32,
                             mesh_infos: *mut c_void, mesh_capacity: u32, stream: *mut c_void) -> i32;
    /// The depth prepass (forward.rs:300-356) in compute: rasterises the MeshletDrawCommandBuffer the meshlet cull wrote
    /// (count read on the device) into width * height reversed-z floats by atomic max; ORBIT_RASTER_CLEAR clears first.
    /// Byte-equal to the host mirror.  Near-plane clipping is out of scope: a triangle with a vertex outside w > 0,
    /// 0 <= z <= w is not drawn.  Cull occluders with alpha_mode_flag = OPAQUE: masked materials are not alpha-tested.
    pub fn orbit_raster_depth(ctx: *mut OrbitCtx, job: *const OrbitRasterDepth, stream: *mut c_void) -> i32;
    /// orbit_raster_depth keeping the winner: per pixel float_bits(d) << 32 | (command_base + i) << 8 | t, merged by a
    /// 64-bit atomic max; 0 is an uncovered pixel.  A command with more than 256 triangles is a range error.
    pub fn orbit_raster_visibility(ctx: *mut OrbitCtx, job: *const OrbitRasterVisibility, stream: *mut c_void) -> i32;
    /// One read of the visibility buffer: depth (the high halves), pixels per command, covered / visible / foreign counts.
    pub fn orbit_visibility_resolve(ctx: *mut OrbitCtx, job: *const OrbitVisibilityResolve, stream: *mut c_void) -> i32;
    /// The bytes of scratch orbit_visibility_compact needs for a list of max_commands.
    pub fn orbit_visibility_compact_workspace(max_commands: u32) -> u64;
    /// The exact visible draw list of a visibility buffer, optionally cut down to the visible triangles (C1-C6).
    pub fn orbit_visibility_compact(ctx: *mut OrbitCtx, job: *const OrbitVisibilityCompact, stream: *mut c_void) -> i32;
    /// Perspective-correct barycentrics, their one-pixel differences and the triangle's ids of every pixel the list owns
    /// (S1-S7): what a renderer shades from, by the raster's own rules.
    pub fn orbit_visibility_surface(ctx: *mut OrbitCtx, job: *const OrbitVisibilitySurface, stream: *mut c_void) -> i32;
    pub fn orbit_visibility_surface_drawn(ctx: *mut OrbitCtx, job: *const OrbitVisibilitySurface, raster_flags: u32, stream: *mut c_void) -> i32;
    pub fn orbit_surface_fragments(ctx: *mut OrbitCtx, job: *const OrbitSurfaceFragments, stream: *mut c_void) -> i32;
    /// forward.frag's clustered lighting of every visible pixel (L1-L9): the texture-free part of render_mode 0, and
    /// render_mode 8, from the fragments call's planes and the cluster chain's light lists.
    pub fn orbit_fragments_shade(ctx: *mut OrbitCtx, job: *const OrbitFragmentsShade, stream: *mut c_void) -> i32;
    /// The same with forward.frag's cascaded PCSS shadow term on the shadowed directional lights (H1-H10).
    pub fn orbit_fragments_shade_shadowed(ctx: *mut OrbitCtx, job: *const OrbitFragmentsShadeShadowed, stream: *mut c_void) -> i32;
    /// The shape of the bloom chain of a width x height target (host only; out.max_levels is read).
    pub fn orbit_bloom_layout(width: u32, height: u32, out: *mut OrbitBloomLayout) -> i32;
    /// compute_bloom of the colour plane the shade calls leave (B1-B9): afterwards level 0 of mips is the bloom image.
    pub fn orbit_bloom(ctx: *mut OrbitCtx, job: *const OrbitBloom, stream: *mut c_void) -> i32;
    /// post_process.frag of that plane and the bloom image (T1-T5): the ACES fit and the swapchain's sRGB bytes.
    pub fn orbit_post_process(ctx: *mut OrbitCtx, job: *const OrbitPostProcess, stream: *mut c_void) -> i32;
    /// compute_ssao of the depth plane (A1-A9): raw, its blur, and what forward.frag reads of the blur per pixel.
    pub fn orbit_ssao(ctx: *mut OrbitCtx, job: *const OrbitSsao, stream: *mut c_void) -> i32;
    /// The shape of the sky, irradiance and prefiltered cubes and the BRDF table (host only; E0).
    /// forward.frag's clustered lighting with shadows, the sky light's term and the skybox (rules K1-K10)
    pub fn orbit_fragments_shade_sky(ctx: *mut OrbitCtx, job: *const OrbitFragmentsShadeSky, stream: *mut c_void) -> i32;
    pub fn orbit_env_map_layout(sky_size: u32, irradiance_size: u32, prefiltered_size: u32, prefiltered_levels: u32, brdf_size: u32,
                                out: *mut OrbitEnvMapLayout) -> i32;
    /// EnvironmentMap::new and the BRDF table of forward.rs:113-205 (E0-E12): every product that is not null.
    pub fn orbit_env_map(ctx: *mut OrbitCtx, job: *const OrbitEnvMap, stream: *mut c_void) -> i32;
    /// textureLod of a cube in E0's layout at n directions (E4).
    pub fn orbit_env_sample(ctx: *mut OrbitCtx, job: *const OrbitEnvSample, stream: *mut c_void) -> i32;
}

/// Turns a non-zero status into the panic the Vulkan path produced (assert!/unwrap, draw_gen.rs:247).
pub fn check(ctx: *const OrbitCtx, rc: i32) {
    if rc != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(orbit_last_error(ctx)) }.to_string_lossy().into_owned();
        panic!("orbit_hip error {rc}: {msg}");
    }
}

// --- body swap in src/passes/draw_gen.rs::create_meshlet_dispatch_command (lines 354-377) -----------------
//
//     let gpu_cull_info_data = cull_info.to_gpu(context);                       // unchanged (draw_gen.rs:347)
//     context.add_pass(format!("{draw_commands_name}_entity_culling_hip"))
//         .with_dependency(meshlet_dispatch_buffer, AccessKind::ComputeShaderWrite)
//         .record_custom(move |_cmd, graph| {
//             let bufs = OrbitEntityCullBufs {
//                 entity_draw_buffer: graph.hip_ptr(scene.entity_draw_buffer),   // VK_KHR_external_memory_fd
//                 mesh_info_buffer: graph.hip_ptr(assets.mesh_info_buffer),      //   import, SURVEY.md §8f rank 1
//                 meshlet_dispatch_buffer: graph.hip_ptr_mut(meshlet_dispatch_buffer),
//                 entity_buffer: graph.hip_ptr(scene.entity_buffer),
//                 visibility_buffer: visibility.map_or(null_mut(), |b| graph.hip_ptr_mut(b) as *mut u32),
//                 depth_pyramid: pyramid.map_or(null(), |i| graph.hip_image_ptr(i)),
//                 depth_pyramid_size: pyramid_size, dispatch_capacity: MAX_MESHLET_DISPATCH_COUNT as u32, _pad: 0 };
//             check(ctx, unsafe { orbit_entity_cull(ctx, bytes_of(&gpu_cull_info_data).as_ptr() as _, &bufs,
//                                                   scene.entity_draw_count as u32, hip_stream) });
//         });
//     // the fill_buffer clears (draw_gen.rs:356-363) disappear: the library writes the {n,1,1} header itself.

// --- body swap in src/passes/draw_gen.rs::create_draw_commands (lines 239-325: both stages) -----------------------
//
// ONE pass, ONE library call; the library runs a scene of the renderer's size (<= 16 384 entity-draws per view) as ONE
// launch and a larger one as the launch chain, with the same buffers either way:
//
//     context.add_pass(format!("{draw_commands_name}_culling_hip"))
//         .with_dependency(meshlet_dispatch_buffer, AccessKind::ComputeShaderWrite)
//         .with_dependency(draw_commands_buffer, AccessKind::ComputeShaderWrite)
//         .record_custom(move |_cmd, graph| {
//             let view = OrbitCullView { cull_info: bytes_of(&gpu_cull_info_data).as_ptr() as _,
//                                        entity: entity_bufs(graph), meshlet: meshlet_bufs(graph),  // as above / below
//                                        entity_draw_count: scene.entity_draw_count as u32, skip_meshlet_stage: 0 };
//             check(ctx, unsafe { orbit_cull_views(ctx, &view, 1, hip_stream) });
//         });
//
// The frame's five independent culls (forward.rs:286-298 + shadow_renderer.rs:391-403) become one pass the same way:
// an array of five OrbitCullView and count = 5 — one launch for all of them.

// --- optional: derived meshlet streams, in src/assets/mod.rs ---------------------------------------------------
//
// GpuAssets::new (after meshlet_buffer is created, assets/mod.rs:272-276):
//     let mut ms = std::ptr::null_mut();
//     check(ctx, unsafe { orbit_meshlet_stream_create(ctx, 0, MAX_MESHLET_COUNT as u64, &mut ms) });
//     // once per cull context (frame slot): orbit_ctx_bind_meshlet_stream(slot_ctx, ms)
//
// GpuAssets::add_mesh, right after the upload (assets/mod.rs:441-445):
//     context.queue_write_buffer(&self.meshlet_buffer, meshlet_range.start * size_of::<GpuMeshlet>(), meshlet_bytes);
//     // ordered behind that write like any reader of the buffer (same HIP stream / the imported semaphore):
//     check(ctx, unsafe { orbit_meshlet_stream_update(ctx, ms, hip_ptr(&self.meshlet_buffer),
//                                                     meshlet_range.start as u64, meshlets.len() as u64, hip_stream) });
//
// GpuAssets::add_material, right after the upload (assets/mod.rs:520-526):
//     check(ctx, unsafe { orbit_meshlet_stream_set_materials(ctx, ms, hip_ptr(&self.materials_buffer),
//                                                            self.material_indices.len() as u32, hip_stream) });
//
// Nothing else changes: orbit_meshlet_cull keeps taking bufs.meshlet_buffer; when it is the pointer the stream was
// updated from, passes 0 and 2 read the stream (22 B per meshlet instead of 32 — 20.25 when bufs.material_buffer is
// the pointer of set_materials — no survivor payload, commands derived from the 2-B count chain).  A meshlet the
// stream does not cover latches ORBIT_E_RANGE (orbit_ctx_status) instead of being read out of range; a debug build of
// the renderer creates its contexts with caps.validate_streams = 1 and gets ORBIT_E_STALE where an update is missing.
