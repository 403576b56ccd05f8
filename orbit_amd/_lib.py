"""ctypes binding of ``liborbit_cull.so`` (the C ABI of ``include/orbit_abi.h``).

There is exactly one compute path: the HIP library.  If it is missing or no
gfx950 device is usable, loading / context creation raises — nothing here falls
back to a host implementation.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liborbit_cull.so")

OK, E_INVALID, E_PLANES, E_CAPACITY, E_HIP, E_NO_DEVICE, E_TIMEOUT, E_MISSING, E_COMM, E_RANGE, E_STALE = (
    0, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10)
ERROR_NAMES = {
    E_INVALID: "ORBIT_E_INVALID", E_PLANES: "ORBIT_E_PLANES", E_CAPACITY: "ORBIT_E_CAPACITY", E_HIP: "ORBIT_E_HIP",
    E_NO_DEVICE: "ORBIT_E_NO_DEVICE", E_TIMEOUT: "ORBIT_E_TIMEOUT", E_MISSING: "ORBIT_E_MISSING",
    E_COMM: "ORBIT_E_COMM", E_RANGE: "ORBIT_E_RANGE", E_STALE: "ORBIT_E_STALE",
}

MAX_PYRAMID_MIPS = 16


class OrbitError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


class Caps(C.Structure):
    _fields_ = [("max_entities", C.c_uint32), ("max_dispatches", C.c_uint32), ("max_draws", C.c_uint32),
                ("max_lights", C.c_uint32), ("max_clusters", C.c_uint32), ("dispatch_size", C.c_uint32),
                ("max_views", C.c_uint32), ("validate_streams", C.c_uint32), ("cull_path", C.c_uint32),
                ("arith_profile", C.c_uint32)]


class EntityCullBufs(C.Structure):
    _fields_ = [("entity_draw_buffer", C.c_void_p), ("mesh_info_buffer", C.c_void_p),
                ("meshlet_dispatch_buffer", C.c_void_p), ("entity_buffer", C.c_void_p),
                ("visibility_buffer", C.c_void_p), ("depth_pyramid", C.c_void_p),
                ("depth_pyramid_size", C.c_uint32 * 2), ("dispatch_capacity", C.c_uint32), ("_pad", C.c_uint32),
                ("depth_pyramid_levels", C.c_void_p)]


class MeshletCullBufs(C.Structure):
    _fields_ = [("meshlet_dispatch_buffer", C.c_void_p), ("meshlet_buffer", C.c_void_p),
                ("draw_commands_buffer", C.c_void_p), ("entity_buffer", C.c_void_p), ("material_buffer", C.c_void_p),
                ("meshlet_visibility_buffer", C.c_void_p), ("depth_pyramid", C.c_void_p),
                ("depth_pyramid_size", C.c_uint32 * 2), ("dispatch_capacity", C.c_uint32),
                ("draw_capacity", C.c_uint32), ("material_count", C.c_uint32), ("_pad", C.c_uint32),
                ("depth_pyramid_levels", C.c_void_p)]


class CullView(C.Structure):  # OrbitCullView
    _fields_ = [("cull_info", C.c_void_p), ("entity", EntityCullBufs), ("meshlet", MeshletCullBufs),
                ("entity_draw_count", C.c_uint32), ("skip_meshlet_stage", C.c_uint32)]


class DepthPyramidLevel(C.Structure):  # OrbitDepthPyramidLevel: one mip of a pyramid made of separate images
    _fields_ = [("texels", C.c_void_p), ("row_pitch", C.c_uint32), ("_pad", C.c_uint32)]


class DepthReduceItem(C.Structure):  # OrbitDepthReduceItem
    _fields_ = [("depth", C.c_void_p), ("screen_width", C.c_uint32), ("screen_height", C.c_uint32),
                ("depth_row_pitch", C.c_uint32), ("_pad", C.c_uint32), ("pyramid", C.c_void_p),
                ("levels", C.POINTER(DepthPyramidLevel))]


class DepthPyramidDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("mip_levels", C.c_uint32),
                ("total_texels", C.c_uint32), ("mip_offset", C.c_uint32 * MAX_PYRAMID_MIPS),
                ("mip_width", C.c_uint32 * MAX_PYRAMID_MIPS), ("mip_height", C.c_uint32 * MAX_PYRAMID_MIPS)]


class MeshletStreamArrays(C.Structure):  # OrbitMeshletStreamArrays: host arrays of orbit_meshlet_stream_read_arrays
    _fields_ = [(name, C.c_void_p) for name in ("sphere", "cone", "mat", "cmd", "cnt", "link", "cls0", "cls1", "base32")]


class SceneUpdate(C.Structure):  # OrbitSceneUpdate
    _fields_ = [("entities", C.c_void_p), ("transforms", C.c_void_p), ("entity_data", C.c_void_p),
                ("entity_draw_buffer", C.c_void_p), ("light_data", C.c_void_p), ("shadow_orientations", C.c_void_p),
                ("instance_of_entity", C.c_void_p), ("light_of_entity", C.c_void_p), ("counts", C.c_void_p),
                ("entity_count", C.c_uint32), ("instance_capacity", C.c_uint32), ("light_capacity", C.c_uint32),
                ("shadow_capacity", C.c_uint32), ("luminance_cutoff", C.c_float), ("shadow_index_base", C.c_uint32)]


class MeshletBoundsJob(C.Structure):  # OrbitMeshletBoundsJob
    _fields_ = [("meshlets", C.c_void_p), ("meshlet_data", C.c_void_p), ("vertices", C.c_void_p),
                ("meshlet_indices", C.c_void_p), ("full", C.c_void_p), ("first_meshlet", C.c_uint64),
                ("meshlet_count", C.c_uint64), ("meshlet_capacity", C.c_uint64), ("meshlet_data_words", C.c_uint64),
                ("vertex_count", C.c_uint64), ("vertex_stride", C.c_uint32), ("position_offset", C.c_uint32),
                ("flags", C.c_uint32), ("_pad", C.c_uint32)]


BOUNDS_KEEP_RECORDS = 1  # ORBIT_BOUNDS_KEEP_RECORDS


class RasterDepth(C.Structure):  # OrbitRasterDepth
    _fields_ = [("draw_commands", C.c_void_p), ("meshlet_data", C.c_void_p), ("vertices", C.c_void_p),
                ("entity_data", C.c_void_p), ("depth", C.c_void_p), ("stats", C.c_void_p),
                ("meshlet_data_words", C.c_uint64), ("vertex_count", C.c_uint64), ("max_commands", C.c_uint32),
                ("entity_count", C.c_uint32), ("vertex_stride", C.c_uint32), ("position_offset", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32),
                ("view_proj", C.c_float * 16)]


RASTER_CLEAR, RASTER_CULL_NONE = 1, 2  # ORBIT_RASTER_CLEAR, ORBIT_RASTER_CULL_NONE
RASTER_CLIP_NEAR = 8                   # ORBIT_RASTER_CLIP_NEAR (4 is no flag)
RASTER_WIDE_GUARD = 32                 # ORBIT_RASTER_WIDE_GUARD (16 is no flag)
RASTER_MAX_DIM = 32768                 # ORBIT_RASTER_MAX_DIM
VIS_MAX_COMMANDS = 1 << 24             # ORBIT_VIS_MAX_COMMANDS


class RasterVisibility(C.Structure):  # OrbitRasterVisibility: RasterDepth with visibility for depth, command_base for _pad
    _fields_ = [({"depth": "visibility", "_pad": "command_base"}.get(name, name), kind) for name, kind in RasterDepth._fields_]


class VisibilityResolve(C.Structure):  # OrbitVisibilityResolve
    _fields_ = [("visibility", C.c_void_p), ("depth", C.c_void_p), ("command_pixels", C.c_void_p), ("stats", C.c_void_p),
                ("width", C.c_uint32), ("height", C.c_uint32), ("command_base", C.c_uint32), ("max_commands", C.c_uint32)]


class VisibilityCompact(C.Structure):  # OrbitVisibilityCompact (120 B)
    _fields_ = [("visibility", C.c_void_p), ("draw_commands", C.c_void_p), ("meshlet_data", C.c_void_p),
                ("triangle_masks", C.c_void_p), ("visible_commands", C.c_void_p), ("visible_ids", C.c_void_p),
                ("visible_data", C.c_void_p), ("stats", C.c_void_p), ("workspace", C.c_void_p),
                ("meshlet_data_words", C.c_uint64), ("workspace_bytes", C.c_uint64), ("width", C.c_uint32),
                ("height", C.c_uint32), ("command_base", C.c_uint32), ("max_commands", C.c_uint32),
                ("visible_capacity", C.c_uint32), ("visible_data_words", C.c_uint32), ("flags", C.c_uint32),
                ("_pad", C.c_uint32)]


COMPACT_TRIANGLES = 1  # ORBIT_COMPACT_TRIANGLES


class VisibilitySurface(C.Structure):  # OrbitVisibilitySurface (184 B)
    _fields_ = [("visibility", C.c_void_p), ("draw_commands", C.c_void_p), ("meshlet_data", C.c_void_p),
                ("vertices", C.c_void_p), ("entity_data", C.c_void_p), ("bary", C.c_void_p), ("grad", C.c_void_p),
                ("triangle", C.c_void_p), ("stats", C.c_void_p), ("meshlet_data_words", C.c_uint64),
                ("vertex_count", C.c_uint64), ("max_commands", C.c_uint32), ("entity_count", C.c_uint32),
                ("vertex_stride", C.c_uint32), ("position_offset", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("flags", C.c_uint32), ("command_base", C.c_uint32),
                ("view_proj", C.c_float * 16)]


SURFACE_CLEAR = 1  # ORBIT_SURFACE_CLEAR


class SurfaceFragments(C.Structure):  # OrbitSurfaceFragments (176 B)
    _fields_ = [("visibility", C.c_void_p), ("draw_commands", C.c_void_p), ("meshlets", C.c_void_p), ("bary", C.c_void_p),
                ("grad", C.c_void_p), ("triangle", C.c_void_p), ("vertices", C.c_void_p), ("entity_data", C.c_void_p),
                ("world_pos", C.c_void_p), ("normal", C.c_void_p), ("tangent", C.c_void_p), ("uv", C.c_void_p),
                ("uv_grad", C.c_void_p), ("material", C.c_void_p), ("stats", C.c_void_p), ("vertex_count", C.c_uint64),
                ("meshlet_count", C.c_uint32), ("max_commands", C.c_uint32), ("entity_count", C.c_uint32),
                ("vertex_stride", C.c_uint32), ("position_offset", C.c_uint32), ("normal_offset", C.c_uint32),
                ("uv_offset", C.c_uint32), ("tangent_offset", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("flags", C.c_uint32), ("command_base", C.c_uint32)]


FRAGMENTS_CLEAR = 1  # ORBIT_FRAGMENTS_CLEAR


class FragmentsShade(C.Structure):  # OrbitFragmentsShade (160 B)
    _fields_ = [("visibility", C.c_void_p), ("world_pos", C.c_void_p), ("normal", C.c_void_p), ("material", C.c_void_p),
                ("materials", C.c_void_p), ("lights", C.c_void_p), ("cluster_offset_image", C.c_void_p),
                ("light_index_buffer", C.c_void_p), ("color", C.c_void_p), ("lights_walked", C.c_void_p), ("stats", C.c_void_p),
                ("material_count", C.c_uint32), ("light_count", C.c_uint32), ("index_capacity", C.c_uint32),
                ("cluster_count", C.c_uint32 * 3), ("tile_size_px", C.c_uint32), ("z_scale", C.c_float), ("z_bias", C.c_float),
                ("luminance_cutoff", C.c_float), ("z_near", C.c_float), ("view_pos", C.c_float * 3), ("render_mode", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32)]


SHADE_CLEAR, SHADE_FORCE_PER_LANE, SHADE_FORCE_STAGED = 1, 2, 4  # ORBIT_SHADE_*


def fill_fragments_shade(j, cluster_count, tile_size_px, z_scale, z_bias, luminance_cutoff, z_near, view_pos, render_mode, width,
                         height, clear, form):
    """The by-value fields of an OrbitFragmentsShade; form: None (the library chooses), "per_lane", "staged" or raw
    flag bits."""
    j.cluster_count[:] = [int(c) for c in cluster_count]
    j.tile_size_px, j.z_scale, j.z_bias, j.luminance_cutoff = int(tile_size_px), float(z_scale), float(z_bias), float(luminance_cutoff)
    j.z_near, j.render_mode, j.width, j.height = float(z_near), int(render_mode), int(width), int(height)
    j.view_pos[:] = [float(v) for v in view_pos]
    forms = {None: 0, "per_lane": SHADE_FORCE_PER_LANE, "staged": SHADE_FORCE_STAGED}
    j.flags = (SHADE_CLEAR if clear else 0) | (form if isinstance(form, int) else forms[form])  # an int: raw flag bits


class FragmentsShadeShadowed(C.Structure):  # OrbitFragmentsShadeShadowed (232 B)
    _fields_ = [("shade", FragmentsShade), ("shadows", C.c_void_p), ("shadow_maps", C.c_void_p), ("shadow_factor", C.c_void_p),
                ("cascade", C.c_void_p), ("shadow_stats", C.c_void_p), ("shadow_count", C.c_uint32), ("shadow_index_base", C.c_uint32),
                ("shadow_map_count", C.c_uint32), ("shadow_resolution", C.c_uint32), ("blocker_search_radius", C.c_float),
                ("normal_bias_scale", C.c_float), ("oriented_bias", C.c_float), ("_pad", C.c_uint32)]


def fill_shadow_fields(j, shadow_count, shadow_index_base, shadow_map_count, shadow_resolution, blocker_search_radius, normal_bias_scale,
                       oriented_bias):
    """The by-value shadow fields of an OrbitFragmentsShadeShadowed; oriented_bias as the reference sends it (negated)."""
    j.shadow_count, j.shadow_index_base = int(shadow_count), int(shadow_index_base)
    j.shadow_map_count, j.shadow_resolution = int(shadow_map_count), int(shadow_resolution)
    j.blocker_search_radius, j.normal_bias_scale, j.oriented_bias = float(blocker_search_radius), float(normal_bias_scale), float(oriented_bias)


class FragmentsShadeSky(C.Structure):  # OrbitFragmentsShadeSky (344 B)
    _fields_ = [("shadowed", FragmentsShadeShadowed), ("irradiance", C.c_void_p), ("prefiltered", C.c_void_p), ("brdf", C.c_void_p),
                ("sky", C.c_void_p), ("ao", C.c_void_p), ("sky_stats", C.c_void_p), ("irradiance_size", C.c_uint32),
                ("prefiltered_size", C.c_uint32), ("prefiltered_levels", C.c_uint32), ("brdf_size", C.c_uint32), ("sky_size", C.c_uint32),
                ("sky_levels", C.c_uint32), ("skybox_lod", C.c_float), ("sky_x", C.c_float * 3), ("sky_y", C.c_float * 3),
                ("sky_z", C.c_float * 3)]


def fill_sky_fields(j, irradiance_size=0, prefiltered_size=0, prefiltered_levels=0, brdf_size=0, sky_size=0, sky_levels=0, skybox_lod=0.0,
                    basis=None):
    """The by-value sky fields of an OrbitFragmentsShadeSky; basis: K9's (sky_x, sky_y, sky_z), three floats each, or None
    (zeros)."""
    j.irradiance_size, j.prefiltered_size, j.prefiltered_levels = int(irradiance_size), int(prefiltered_size), int(prefiltered_levels)
    j.brdf_size, j.sky_size, j.sky_levels, j.skybox_lod = int(brdf_size), int(sky_size), int(sky_levels), float(skybox_lod)
    if basis is not None:
        for field, v in zip((j.sky_x, j.sky_y, j.sky_z), basis):
            field[:] = [float(c) for c in v]


BLOOM_MAX_LEVELS = 6                                # ORBIT_BLOOM_MAX_LEVELS
BLOOM_FORCE_PER_LEVEL, BLOOM_FORCE_DIRECT = 1, 4    # ORBIT_BLOOM_FORCE_PER_LEVEL, ORBIT_BLOOM_FORCE_DIRECT (2 is no flag)
POST_BGRA = 1                                       # ORBIT_POST_BGRA


class BloomLayout(C.Structure):  # OrbitBloomLayout (88 B)
    _fields_ = [("max_levels", C.c_uint32), ("levels", C.c_uint32), ("total_texels", C.c_uint32), ("_pad", C.c_uint32),
                ("level_width", C.c_uint32 * BLOOM_MAX_LEVELS), ("level_height", C.c_uint32 * BLOOM_MAX_LEVELS),
                ("level_offset", C.c_uint32 * BLOOM_MAX_LEVELS)]


class Bloom(C.Structure):  # OrbitBloom (56 B)
    _fields_ = [("color", C.c_void_p), ("mips", C.c_void_p), ("stats", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32),
                ("threshold", C.c_float), ("soft_threshold", C.c_float), ("filter_radius", C.c_float), ("max_levels", C.c_uint32),
                ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class PostProcess(C.Structure):  # OrbitPostProcess (64 B)
    _fields_ = [("color", C.c_void_p), ("bloom", C.c_void_p), ("ldr", C.c_void_p), ("rgba8", C.c_void_p), ("stats", C.c_void_p),
                ("exposure", C.c_float), ("bloom_intensity", C.c_float), ("render_mode", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("flags", C.c_uint32)]


def fill_bloom(j, width, height, threshold, soft_threshold, filter_radius, max_levels, form):
    """The by-value fields of an OrbitBloom; form: None (the library chooses), "per_level", "direct" or raw flag bits."""
    j.width, j.height, j.max_levels = int(width), int(height), int(max_levels)
    j.threshold, j.soft_threshold, j.filter_radius = float(threshold), float(soft_threshold), float(filter_radius)
    forms = {None: 0, "per_level": BLOOM_FORCE_PER_LEVEL, "direct": BLOOM_FORCE_DIRECT}
    j.flags = form if isinstance(form, int) else forms[form]


def fill_post_process(j, width, height, exposure, bloom_intensity, render_mode, bgra):
    """The by-value fields of an OrbitPostProcess; bgra: True, False or raw flag bits."""
    j.width, j.height, j.render_mode = int(width), int(height), int(render_mode)
    j.exposure, j.bloom_intensity = float(exposure), float(bloom_intensity)
    j.flags = POST_BGRA if bgra is True else int(bgra)


SSAO_MAX_SAMPLES, SSAO_MAX_NOISE_SIZE, SSAO_MAX_SAMPLES_SIZE = 64, 64, 256  # ORBIT_SSAO_MAX_*


class Ssao(C.Structure):  # OrbitSsao (224 B)
    _fields_ = [("depth", C.c_void_p), ("noise", C.c_void_p), ("samples", C.c_void_p), ("raw", C.c_void_p), ("blurred", C.c_void_p),
                ("ao_pixel", C.c_void_p), ("stats", C.c_void_p), ("projection", C.c_float * 16), ("inverse_projection", C.c_float * 16),
                ("screen_w", C.c_uint32), ("screen_h", C.c_uint32), ("ssao_w", C.c_uint32), ("ssao_h", C.c_uint32),
                ("noise_size", C.c_uint32), ("samples_size", C.c_uint32), ("sample_count", C.c_uint32), ("min_radius", C.c_float),
                ("max_radius", C.c_float), ("flags", C.c_uint32)]


def fill_ssao(j, projection, inverse_projection, screen_w, screen_h, ssao_w, ssao_h, noise_size, samples_size, sample_count, min_radius,
              max_radius, flags=0):
    """The by-value fields of an OrbitSsao; the matrices column-major, 16 floats each."""
    import numpy as np

    j.projection = (C.c_float * 16)(*np.asarray(projection, dtype=np.float32).reshape(16))
    j.inverse_projection = (C.c_float * 16)(*np.asarray(inverse_projection, dtype=np.float32).reshape(16))
    j.screen_w, j.screen_h, j.ssao_w, j.ssao_h = int(screen_w), int(screen_h), int(ssao_w), int(ssao_h)
    j.noise_size, j.samples_size, j.sample_count = int(noise_size), int(samples_size), int(sample_count)
    j.min_radius, j.max_radius, j.flags = float(min_radius), float(max_radius), int(flags)


ENV_MAX_SIZE, ENV_MAX_LEVELS, ENV_MAX_SAMPLES = 4096, 13, 65536  # ORBIT_ENV_MAX_*


class EnvMapLayout(C.Structure):  # OrbitEnvMapLayout (264 B)
    _fields_ = [("sky_size", C.c_uint32), ("sky_levels", C.c_uint32), ("irradiance_size", C.c_uint32), ("prefiltered_size", C.c_uint32),
                ("prefiltered_levels", C.c_uint32), ("brdf_size", C.c_uint32), ("sky_level_size", C.c_uint32 * ENV_MAX_LEVELS),
                ("sky_level_offset", C.c_uint32 * ENV_MAX_LEVELS), ("prefiltered_level_size", C.c_uint32 * ENV_MAX_LEVELS),
                ("prefiltered_level_offset", C.c_uint32 * ENV_MAX_LEVELS), ("sky_texels", C.c_uint64), ("irradiance_texels", C.c_uint64),
                ("prefiltered_texels", C.c_uint64), ("brdf_texels", C.c_uint64)]


class EnvMap(C.Structure):  # OrbitEnvMap (96 B)
    _fields_ = [("equirect", C.c_void_p), ("sky", C.c_void_p), ("irradiance", C.c_void_p), ("prefiltered", C.c_void_p), ("brdf", C.c_void_p),
                ("stats", C.c_void_p), ("equirect_w", C.c_uint32), ("equirect_h", C.c_uint32), ("sky_size", C.c_uint32),
                ("irradiance_size", C.c_uint32), ("prefiltered_size", C.c_uint32), ("prefiltered_levels", C.c_uint32), ("brdf_size", C.c_uint32),
                ("sample_count", C.c_uint32), ("sample_delta", C.c_float), ("brdf_sample_count", C.c_uint32), ("flags", C.c_uint32),
                ("_pad", C.c_uint32)]


class EnvSample(C.Structure):  # OrbitEnvSample (56 B)
    _fields_ = [("cube", C.c_void_p), ("directions", C.c_void_p), ("lods", C.c_void_p), ("rgb", C.c_void_p), ("bad_directions", C.c_void_p),
                ("size", C.c_uint32), ("levels", C.c_uint32), ("n", C.c_uint32), ("flags", C.c_uint32)]


def fill_env_map(j, equirect_w, equirect_h, sky_size, irradiance_size, prefiltered_size, prefiltered_levels, brdf_size, sample_count,
                 sample_delta, brdf_sample_count, flags=0):
    """The by-value fields of an OrbitEnvMap."""
    j.equirect_w, j.equirect_h, j.sky_size, j.irradiance_size = int(equirect_w), int(equirect_h), int(sky_size), int(irradiance_size)
    j.prefiltered_size, j.prefiltered_levels, j.brdf_size = int(prefiltered_size), int(prefiltered_levels), int(brdf_size)
    j.sample_count, j.sample_delta, j.brdf_sample_count, j.flags = int(sample_count), float(sample_delta), int(brdf_sample_count), int(flags)


class ClusterFrame(C.Structure):  # OrbitClusterFrame
    _fields_ = [("push", C.c_void_p), ("info", C.c_void_p), ("depth", C.c_void_p), ("lights", C.c_void_p),
                ("tile_depth_slice_mask", C.c_void_p), ("depth_bounds", C.c_void_p), ("unique_cluster_buffer", C.c_void_p),
                ("light_index_buffer", C.c_void_p), ("cluster_offset_image", C.c_void_p), ("index_capacity", C.c_uint32),
                ("light_index_capacity", C.c_uint32)]


class FrameLate(C.Structure):  # OrbitFrameLate
    _fields_ = [("pyramids", C.POINTER(DepthReduceItem)), ("late_views", C.POINTER(CullView)),
                ("cascade_views", C.POINTER(CullView)), ("clusters", C.POINTER(ClusterFrame)),
                ("pyramid_count", C.c_uint32), ("late_view_count", C.c_uint32), ("cascade_view_count", C.c_uint32),
                ("_pad", C.c_uint32)]


# every symbol include/orbit_abi.h and orbit_abi_ext.h declare: (restype, argtypes)
SYMBOLS = {
    "orbit_abi_version": (C.c_uint32, []),
    "orbit_meshlet_cull_records_and_commands": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(MeshletCullBufs),
                                                            C.c_void_p, C.c_uint32, C.c_void_p]),
    "orbit_exchange_list": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "orbit_ctx_fused_culls": (C.c_uint64, [C.c_void_p]),
    "orbit_frame_late": (C.c_int32, [C.c_void_p, C.POINTER(FrameLate), C.c_void_p]),
    "orbit_default_caps": (None, [C.POINTER(Caps)]),
    "orbit_ctx_create": (C.c_int32, [C.c_int32, C.POINTER(Caps), C.POINTER(C.c_void_p)]),
    "orbit_ctx_destroy": (C.c_int32, [C.c_void_p]),
    "orbit_last_error": (C.c_char_p, [C.c_void_p]),
    "orbit_ctx_status": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32]),
    "orbit_entity_cull": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(EntityCullBufs), C.c_uint32, C.c_void_p]),
    "orbit_entity_cull_range": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(EntityCullBufs), C.c_uint32,
                                            C.c_uint32, C.c_void_p]),
    "orbit_meshlet_cull": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(MeshletCullBufs), C.c_void_p]),
    "orbit_meshlet_task_cull": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(MeshletCullBufs), C.c_void_p, C.c_void_p]),
    "orbit_depth_pyramid_desc": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(DepthPyramidDesc)]),
    "orbit_cull_views": (C.c_int32, [C.c_void_p, C.POINTER(CullView), C.c_uint32, C.c_void_p]),
    "orbit_depth_reduce_multi": (C.c_int32, [C.c_void_p, C.POINTER(DepthReduceItem), C.c_uint32, C.c_void_p]),
    "orbit_depth_pyramid_desc_from_mip0": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(DepthPyramidDesc)]),
    "orbit_depth_reduce": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "orbit_cluster_mark": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "orbit_cluster_compact": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32 * 3), C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.c_void_p]),
    "orbit_cluster_assign": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_uint32, C.c_void_p, C.c_void_p]),
    "orbit_compute_clusters": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                           C.c_void_p]),
    "orbit_ctx_profile": (C.c_int32, [C.c_void_p, C.c_int32]),
    "orbit_ctx_profile_reserve": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "orbit_ctx_profile_read": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "orbit_shard_range": (None, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "orbit_gather_visible": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_uint32, C.c_void_p]),
    "orbit_meshlet_cull_visible_records": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(MeshletCullBufs), C.c_void_p,
                                                       C.c_uint32, C.c_void_p]),
    "orbit_expand_visible_records": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                 C.c_void_p]),
    "orbit_p2p_alloc": (C.c_int32, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.c_void_p]),
    "orbit_p2p_free": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "orbit_p2p_open": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "orbit_p2p_close": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "orbit_meshlet_stream_create": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]),
    "orbit_meshlet_stream_update": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                                C.c_void_p]),
    "orbit_meshlet_stream_set_materials": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "orbit_meshlet_stream_validate": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "orbit_meshlet_stream_destroy": (C.c_int32, [C.c_void_p]),
    "orbit_meshlet_stream_update_meshes": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "orbit_ctx_mesh_side_culls": (C.c_uint64, [C.c_void_p]),
    "orbit_ctx_bind_meshlet_stream": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "orbit_ctx_meshlet_stream_culls": (C.c_uint64, [C.c_void_p]),
    "orbit_ctx_meshlet_class_culls": (C.c_uint64, [C.c_void_p]),
    "orbit_ctx_block_culls": (C.c_uint64, [C.c_void_p]),
    "orbit_ctx_set_block_cull": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "orbit_ctx_set_block_cull_grid": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "orbit_ctx_set_raster_grid": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "orbit_ctx_set_visibility_grid": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "orbit_ctx_set_fused_grid": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "orbit_meshlet_stream_block_bounds": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                                      C.c_void_p]),
    "orbit_meshlet_stream_read_arrays": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                                     C.POINTER(MeshletStreamArrays), C.c_void_p]),
    "orbit_cull_shard": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(EntityCullBufs), C.c_uint32, C.c_uint32,
                                     C.POINTER(MeshletCullBufs), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "orbit_ctx_shard_culls": (C.c_uint64, [C.c_void_p]),
    "orbit_allgather_list": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "orbit_compact_segments": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                           C.c_uint32, C.c_uint32, C.c_void_p]),
    "orbit_scene_update_entities": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                C.c_void_p]),
    "orbit_scene_update": (C.c_int32, [C.c_void_p, C.POINTER(SceneUpdate), C.c_void_p]),
    "orbit_cull_stats": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(EntityCullBufs), C.c_uint32,
                                     C.POINTER(MeshletCullBufs), C.c_void_p, C.c_void_p]),
    "orbit_cluster_stats": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "orbit_meshlet_bounds": (C.c_int32, [C.c_void_p, C.POINTER(MeshletBoundsJob), C.c_void_p]),
    "orbit_mesh_bounds": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_uint32, C.c_void_p]),
    "orbit_raster_depth": (C.c_int32, [C.c_void_p, C.POINTER(RasterDepth), C.c_void_p]),
    "orbit_raster_visibility": (C.c_int32, [C.c_void_p, C.POINTER(RasterVisibility), C.c_void_p]),
    "orbit_visibility_resolve": (C.c_int32, [C.c_void_p, C.POINTER(VisibilityResolve), C.c_void_p]),
    "orbit_visibility_compact_workspace": (C.c_uint64, [C.c_uint32]),
    "orbit_visibility_compact": (C.c_int32, [C.c_void_p, C.POINTER(VisibilityCompact), C.c_void_p]),
    "orbit_visibility_surface": (C.c_int32, [C.c_void_p, C.POINTER(VisibilitySurface), C.c_void_p]),
    "orbit_visibility_surface_drawn": (C.c_int32, [C.c_void_p, C.POINTER(VisibilitySurface), C.c_uint32, C.c_void_p]),
    "orbit_surface_fragments": (C.c_int32, [C.c_void_p, C.POINTER(SurfaceFragments), C.c_void_p]),
    "orbit_fragments_shade": (C.c_int32, [C.c_void_p, C.POINTER(FragmentsShade), C.c_void_p]),
    "orbit_fragments_shade_shadowed": (C.c_int32, [C.c_void_p, C.POINTER(FragmentsShadeShadowed), C.c_void_p]),
    "orbit_fragments_shade_sky": (C.c_int32, [C.c_void_p, C.POINTER(FragmentsShadeSky), C.c_void_p]),
    "orbit_bloom_layout": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(BloomLayout)]),
    "orbit_bloom": (C.c_int32, [C.c_void_p, C.POINTER(Bloom), C.c_void_p]),
    "orbit_post_process": (C.c_int32, [C.c_void_p, C.POINTER(PostProcess), C.c_void_p]),
    "orbit_ssao": (C.c_int32, [C.c_void_p, C.POINTER(Ssao), C.c_void_p]),
    "orbit_env_map_layout": (C.c_int32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(EnvMapLayout)]),
    "orbit_env_map": (C.c_int32, [C.c_void_p, C.POINTER(EnvMap), C.c_void_p]),
    "orbit_env_sample": (C.c_int32, [C.c_void_p, C.POINTER(EnvSample), C.c_void_p]),
}

_lib = None


def load_variant(path):
    """A second build of the library under another path (A/B tools: tools/ab_libs.py); not cached."""
    import torch  # noqa: F401  (same HIP runtime as the main copy)

    lib = C.CDLL(path)
    for name, (restype, argtypes) in SYMBOLS.items():
        if hasattr(lib, name):  # an older build may lack the newest entry points
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
    return lib


def load():
    """Loads the shared library once; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} is missing: build it with `make -C orbit_amd/csrc` or "
                      "`python -c 'import __graft_entry__ as g; g.build()'` (there is no fallback path)")
    try:
        # torch ships its own libamdhip64; if it is going to be used in this process it has to be the copy the
        # library binds to as well (two HIP runtimes in one process: the second one finds no device)
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc, ctx=None):
    if rc != OK:
        msg = load().orbit_last_error(ctx)
        raise OrbitError(rc, msg.decode() if msg else "")
