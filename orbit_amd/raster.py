"""ctypes binding of the host mirror of ``orbit_raster_depth``, ``orbit_raster_visibility`` and
``orbit_visibility_resolve`` (``orbit_amd/host/orbit_raster.hpp``): the depth prepass of a MeshletDrawCommandBuffer on
host arrays, the same pass keeping the winner's identity and its resolve — the references of ``Engine.raster_depth``,
``Engine.raster_visibility`` and ``Engine.visibility_resolve`` — and of ``orbit_visibility_compact``, the visible draw
list of such a buffer, the reference of ``Engine.visibility_compact``, and of ``orbit_visibility_surface``, the
barycentrics and ids per pixel of such a buffer, the reference of ``Engine.visibility_surface``, and of
``orbit_surface_fragments``, the fragment shader's inputs per pixel from those, the reference of
``Engine.surface_fragments``, and of ``orbit_fragments_shade``, the clustered lighting of those pixels, the reference of
``Engine.fragments_shade``, and of ``orbit_fragments_shade_shadowed``, the same with cascaded shadows, the reference of
``Engine.fragments_shade_shadowed``, with the two helpers that draw the cascades' maps into one atlas (``host_shadow_atlas``
on the host, ``shadow_atlas`` through an Engine).  Python adds nothing."""
import ctypes as C

import numpy as np

from . import _lib
from . import layouts as L
from .passes import _check, lib

CLEAR, CULL_NONE, CLIP_NEAR = _lib.RASTER_CLEAR, _lib.RASTER_CULL_NONE, _lib.RASTER_CLIP_NEAR
WIDE_GUARD = _lib.RASTER_WIDE_GUARD


def command_buffer(commands, capacity=None, count=None):
    """{u32 count; 28-B commands} as np.uint32 words from np[layouts.DRAW_COMMAND] rows; `count` overrides the header."""
    cmds = np.ascontiguousarray(commands, dtype=L.MESHLET_DRAW_COMMAND)
    capacity = len(cmds) if capacity is None else capacity
    buf = np.zeros(1 + 7 * capacity, np.uint32)
    buf[0] = len(cmds) if count is None else count
    buf[1:1 + 7 * len(cmds)] = cmds.view(np.uint32).reshape(-1)
    return buf


def _host_raster(call, dtype, draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj,
                 width, height, target, no_target, clear, cull_none, vertex_stride, position_offset, entity_count,
                 meshlet_data_words, clip_near, wide_guard, *extra):
    """What the two raster calls of the host mirror share: the arguments as the C call takes them (`extra` goes between
    the flags and the stats), the target loaded (copied) or cleared, -> (target, stats row, command_error)."""
    buf = np.ascontiguousarray(draw_commands).view(np.uint8).reshape(-1)
    if buf.nbytes < 4 + 28 * int(max_commands):
        raise ValueError("max_commands reaches beyond the command array")
    data = np.ascontiguousarray(meshlet_data, dtype=np.uint32).reshape(-1)
    vb = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1)
    if int(vertex_count) and (int(vertex_count) - 1) * int(vertex_stride) + int(position_offset) + 12 > vb.nbytes:
        raise ValueError("vertex_count reaches beyond the vertex array")
    ent = np.ascontiguousarray(entity_data).view(np.uint8).reshape(-1)
    entity_count = ent.nbytes // 128 if entity_count is None else int(entity_count)
    words = len(data) if meshlet_data_words is None else int(meshlet_data_words)
    if target is None:
        if not clear:
            raise ValueError(no_target)
        out = np.zeros((height, width), dtype)
    else:
        out = np.array(target, dtype=dtype, order="C").reshape(height, width)
    n = min(int(buf[:4].view(np.uint32)[0]), int(max_commands))
    stats, err = np.zeros(1, L.RASTER_STATS), np.zeros(n, np.int32)
    vp = (C.c_float * 16)(*np.asarray(view_proj, dtype=np.float32).reshape(16))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    flags = ((CLEAR if clear else 0) | (CULL_NONE if cull_none else 0) | (CLIP_NEAR if clip_near else 0)
             | (WIDE_GUARD if wide_guard else 0))
    _check(call(p(buf), C.c_uint32(max_commands), p(data), C.c_uint64(words), p(vb), C.c_uint64(vertex_count),
                C.c_uint32(vertex_stride), C.c_uint32(position_offset), p(ent), C.c_uint32(entity_count), vp, p(out),
                C.c_uint32(width), C.c_uint32(height), C.c_uint32(flags),
                *extra, p(stats), p(err)))
    return out, stats[0], err


def host_raster_depth(draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj, width,
                      height, depth=None, clear=True, cull_none=False, vertex_stride=12, position_offset=0,
                      entity_count=None, meshlet_data_words=None, clip_near=False, wide_guard=False):
    """orbit_host_raster_depth on host arrays -> (depth: np.float32 (height, width), stats: np[layouts.RASTER_STATS]
    scalar row, command_error: np.int32 per processed command).  `draw_commands`: the {count; commands} words (any
    contiguous array, read as bytes).  `depth`: the buffer to load (copied); None needs clear=True.  clip_near:
    ORBIT_RASTER_CLIP_NEAR; wide_guard: ORBIT_RASTER_WIDE_GUARD."""
    return _host_raster(lib().orbit_host_raster_depth, np.float32, draw_commands, max_commands, meshlet_data, vertices,
                        vertex_count, entity_data, view_proj, width, height, depth, "no depth to load", clear, cull_none,
                        vertex_stride, position_offset, entity_count, meshlet_data_words, clip_near, wide_guard)


def host_raster_visibility(draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj,
                           width, height, visibility=None, command_base=0, clear=True, cull_none=False, vertex_stride=12,
                           position_offset=0, entity_count=None, meshlet_data_words=None, clip_near=False,
                           wide_guard=False):
    """orbit_host_raster_visibility on host arrays -> (visibility: np.uint64 (height, width), stats:
    np[layouts.RASTER_STATS] scalar row, command_error: np.int32 per processed command).  The arguments are
    host_raster_depth's; `visibility`: the buffer to merge into (copied); None needs clear=True."""
    return _host_raster(lib().orbit_host_raster_visibility, np.uint64, draw_commands, max_commands, meshlet_data, vertices,
                        vertex_count, entity_data, view_proj, width, height, visibility, "no buffer to merge into", clear,
                        cull_none, vertex_stride, position_offset, entity_count, meshlet_data_words, clip_near,
                        wide_guard, C.c_uint32(command_base))


def host_visibility_resolve(visibility, command_base=0, max_commands=0, want_command_pixels=True):
    """orbit_host_visibility_resolve on a (height, width) np.uint64 buffer -> (depth: np.float32 (height, width),
    command_pixels: np.uint32[max_commands] or None, stats: np[layouts.VIS_STATS] scalar row)."""
    vis = np.ascontiguousarray(visibility, dtype=np.uint64)
    height, width = vis.shape
    depth = np.zeros((height, width), np.float32)
    pixels = np.zeros(max(int(max_commands), 1), np.uint32) if want_command_pixels else None
    stats = np.zeros(1, L.VIS_STATS)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _check(lib().orbit_host_visibility_resolve(p(vis), C.c_uint32(width), C.c_uint32(height), C.c_uint32(command_base),
                                               C.c_uint32(max_commands), p(depth), p(pixels), p(stats)))
    return depth, None if pixels is None else pixels[:int(max_commands)], stats[0]


def host_visibility_compact(visibility, draw_commands, max_commands, command_base=0, meshlet_data=None, triangles=False,
                            visible_capacity=None, visible_data_words=None, meshlet_data_words=None, fill=0,
                            want_ids=True):
    """orbit_host_visibility_compact on a (height, width) np.uint64 buffer and the {count; commands} words that were
    rasterised into it -> dict(masks: np.uint32[8 * max_commands], commands: np.uint32[1 + 7 * visible_capacity] (the
    output list), ids: np.uint32[visible_capacity] or None, data: np.uint32[visible_data_words] or None (only with
    triangles=True, ORBIT_COMPACT_TRIANGLES), stats: np[layouts.VIS_COMPACT_STATS] scalar row, status: what the device
    call latches).  The capacities default to max_commands commands and, with triangles, the words of meshlet_data.
    Every output is filled with `fill` (a u32) first: what the call does not write keeps it."""
    vis = np.ascontiguousarray(visibility, dtype=np.uint64)
    height, width = vis.shape
    buf = np.ascontiguousarray(draw_commands).view(np.uint8).reshape(-1)
    if buf.nbytes < 4 + 28 * int(max_commands):
        raise ValueError("max_commands reaches beyond the command array")
    data = None if meshlet_data is None else np.ascontiguousarray(meshlet_data, dtype=np.uint32).reshape(-1)
    if triangles and data is None:
        raise ValueError("triangles=True needs meshlet_data")
    cap = int(max_commands) if visible_capacity is None else int(visible_capacity)
    words = (len(data) if triangles else 0) if visible_data_words is None else int(visible_data_words)
    new = lambda n: np.full(max(int(n), 1), fill, np.uint32)  # noqa: E731
    masks, out, ids, stats = new(8 * max_commands), new(1 + 7 * cap), new(cap) if want_ids else None, np.zeros(1, L.VIS_COMPACT_STATS)
    vdata = new(words) if triangles else None
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    j = _lib.VisibilityCompact()
    j.visibility, j.draw_commands, j.meshlet_data, j.triangle_masks = p(vis), p(buf), p(data), p(masks)
    j.visible_commands, j.visible_ids, j.visible_data, j.stats = p(out), p(ids), p(vdata), p(stats)
    j.meshlet_data_words = (0 if data is None else len(data)) if meshlet_data_words is None else int(meshlet_data_words)
    j.width, j.height, j.command_base, j.max_commands = width, height, int(command_base), int(max_commands)
    j.visible_capacity, j.visible_data_words, j.flags = cap, words, _lib.COMPACT_TRIANGLES if triangles else 0
    status = C.c_int32(0)
    _check(lib().orbit_host_visibility_compact(C.byref(j), C.byref(status)))
    return dict(masks=masks[:8 * int(max_commands)], commands=out[:1 + 7 * cap], ids=None if ids is None else ids[:cap],
                data=None if vdata is None else vdata[:words], stats=stats[0], status=status.value)


def host_visibility_surface(visibility, draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data,
                            view_proj, command_base=0, clear=True, into=None, want=("bary", "grad", "triangle"),
                            vertex_stride=12, position_offset=0, entity_count=None, meshlet_data_words=None, fill=0,
                            want_stats=True, _drawn=None):
    """orbit_host_visibility_surface on a (height, width) np.uint64 buffer and the arguments of host_raster_visibility
    that made it -> dict(bary: np.float32 (height, width, 2), grad: np.float32 (height, width, 4), triangle: np.uint32
    (height, width, 4), each None unless named in `want`; stats: np[layouts.SURFACE_STATS] scalar row or None; status:
    what the device call latches).  `into`: the dict of an earlier call to write into (copied): a frame's second list,
    clear=False.  Otherwise every output starts filled with the u32 `fill`: what the call does not write keeps it."""
    vis = np.ascontiguousarray(visibility, dtype=np.uint64)
    height, width = vis.shape
    buf = np.ascontiguousarray(draw_commands).view(np.uint8).reshape(-1)
    if buf.nbytes < 4 + 28 * int(max_commands):
        raise ValueError("max_commands reaches beyond the command array")
    data = np.ascontiguousarray(meshlet_data, dtype=np.uint32).reshape(-1)
    vb = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1)
    if int(vertex_count) and (int(vertex_count) - 1) * int(vertex_stride) + int(position_offset) + 12 > vb.nbytes:
        raise ValueError("vertex_count reaches beyond the vertex array")
    ent = np.ascontiguousarray(entity_data).view(np.uint8).reshape(-1)
    outs = {}
    for name, per_pixel, dtype in (("bary", 2, np.float32), ("grad", 4, np.float32), ("triangle", 4, np.uint32)):
        if name not in want:
            outs[name] = None
        elif into is not None:
            outs[name] = np.array(into[name], dtype=dtype, order="C").reshape(height, width, per_pixel)
        else:
            outs[name] = np.full((height, width, per_pixel), fill, np.uint32).view(dtype)
    stats = np.zeros(1, L.SURFACE_STATS if _drawn is None else L.SURFACE_DRAWN_STATS) if want_stats else None
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    j = _lib.VisibilitySurface()
    j.visibility, j.draw_commands, j.meshlet_data, j.vertices, j.entity_data = p(vis), p(buf), p(data), p(vb), p(ent)
    j.bary, j.grad, j.triangle, j.stats = p(outs["bary"]), p(outs["grad"]), p(outs["triangle"]), p(stats)
    j.meshlet_data_words = len(data) if meshlet_data_words is None else int(meshlet_data_words)
    j.vertex_count, j.max_commands = int(vertex_count), int(max_commands)
    j.entity_count = ent.nbytes // 128 if entity_count is None else int(entity_count)
    j.vertex_stride, j.position_offset, j.width, j.height = int(vertex_stride), int(position_offset), width, height
    j.flags, j.command_base = _lib.SURFACE_CLEAR if clear else 0, int(command_base)
    j.view_proj = (C.c_float * 16)(*np.asarray(view_proj, dtype=np.float32).reshape(16))
    status = C.c_int32(0)
    if _drawn is None:
        _check(lib().orbit_host_visibility_surface(C.byref(j), C.byref(status)))
    else:
        _check(lib().orbit_host_visibility_surface_drawn(C.byref(j), C.c_uint32(_drawn), C.byref(status)))
    return dict(outs, stats=None if stats is None else stats[0], status=status.value)


def host_visibility_surface_drawn(*args, clip_near=False, wide_guard=False, raster_flags=None, **kwargs):
    """orbit_host_visibility_surface_drawn: host_visibility_surface's arguments and result for a buffer drawn with
    clip_near (ORBIT_RASTER_CLIP_NEAR) and / or wide_guard (ORBIT_RASTER_WIDE_GUARD); `raster_flags` gives the word
    itself.  stats: np[layouts.SURFACE_DRAWN_STATS].  Neither flag: host_visibility_surface's bytes."""
    flags = (CLIP_NEAR if clip_near else 0) | (WIDE_GUARD if wide_guard else 0) if raster_flags is None else int(raster_flags)
    return host_visibility_surface(*args, _drawn=flags, **kwargs)


FRAGMENT_OUTPUTS = (("world_pos", 4, np.float32), ("normal", 3, np.float32), ("tangent", 4, np.float32), ("uv", 2, np.float32),
                    ("uv_grad", 4, np.float32), ("material", 1, np.uint32))


def host_surface_fragments(visibility, draw_commands, max_commands, meshlets, surface, vertices, vertex_count, entity_data,
                           command_base=0, clear=True, into=None, want=tuple(n for n, _, _ in FRAGMENT_OUTPUTS),
                           vertex_stride=32, position_offset=0, normal_offset=12, uv_offset=16, tangent_offset=24,
                           entity_count=None, meshlet_count=None, fill=0, want_stats=True):
    """orbit_host_surface_fragments on a (height, width) np.uint64 buffer, the {count; commands} words that were
    rasterised into it, the 32-B meshlet records, `surface` (the dict of host_visibility_surface[_drawn]: bary, triangle
    and, may be None, grad) and the vertex rows -> dict(world_pos (height, width, 4), normal (.., 3), tangent (.., 4), uv
    (.., 2), uv_grad (.., 4) np.float32, material (.., 1) np.uint32, each None unless named in `want`; stats:
    np[layouts.SURFACE_FRAGMENT_STATS] scalar row or None; status: what the device call latches).  `into`: the dict of an
    earlier call to write into (copied): a frame's second list, clear=False.  Otherwise every output starts filled with
    the u32 `fill`: what the call does not write keeps it."""
    vis = np.ascontiguousarray(visibility, dtype=np.uint64)
    height, width = vis.shape
    buf = np.ascontiguousarray(draw_commands).view(np.uint8).reshape(-1)
    if buf.nbytes < 4 + 28 * int(max_commands):
        raise ValueError("max_commands reaches beyond the command array")
    mlt = np.ascontiguousarray(meshlets).view(np.uint8).reshape(-1)
    meshlet_count = mlt.nbytes // 32 if meshlet_count is None else int(meshlet_count)
    if meshlet_count and (meshlet_count - 1) * 32 + 30 > mlt.nbytes:
        raise ValueError("meshlet_count reaches beyond the meshlet array")
    vb = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1)
    ends = (int(position_offset) + 12, int(normal_offset) + 4, int(uv_offset) + 8, int(tangent_offset) + 4)
    if int(vertex_count) and (int(vertex_count) - 1) * int(vertex_stride) + max(ends) > vb.nbytes:
        raise ValueError("vertex_count reaches beyond the vertex array")
    ent = np.ascontiguousarray(entity_data).view(np.uint8).reshape(-1)
    shaped = lambda a, per, dtype: None if a is None else np.ascontiguousarray(a, dtype=dtype).reshape(height, width, per)  # noqa: E731
    bary, grad, tri = shaped(surface["bary"], 2, np.float32), shaped(surface.get("grad"), 4, np.float32), shaped(surface["triangle"], 4, np.uint32)
    if bary is None or tri is None:
        raise ValueError("surface needs bary and triangle")
    outs = {}
    for name, per_pixel, dtype in FRAGMENT_OUTPUTS:
        if name not in want:
            outs[name] = None
        elif into is not None:
            outs[name] = np.array(into[name], dtype=dtype, order="C").reshape(height, width, per_pixel)
        else:
            outs[name] = np.full((height, width, per_pixel), fill, np.uint32).view(dtype)
    stats = np.zeros(1, L.SURFACE_FRAGMENT_STATS) if want_stats else None
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    j = _lib.SurfaceFragments()
    j.visibility, j.draw_commands, j.meshlets, j.vertices, j.entity_data = p(vis), p(buf), p(mlt), p(vb), p(ent)
    j.bary, j.grad, j.triangle, j.stats = p(bary), p(grad), p(tri), p(stats)
    for name, _, _ in FRAGMENT_OUTPUTS:
        setattr(j, name, p(outs[name]))
    j.vertex_count, j.meshlet_count, j.max_commands = int(vertex_count), meshlet_count, int(max_commands)
    j.entity_count = ent.nbytes // 128 if entity_count is None else int(entity_count)
    j.vertex_stride, j.position_offset, j.normal_offset = int(vertex_stride), int(position_offset), int(normal_offset)
    j.uv_offset, j.tangent_offset, j.width, j.height = int(uv_offset), int(tangent_offset), width, height
    j.flags, j.command_base = _lib.FRAGMENTS_CLEAR if clear else 0, int(command_base)
    status = C.c_int32(0)
    _check(lib().orbit_host_surface_fragments(C.byref(j), C.byref(status)))
    return dict(outs, stats=None if stats is None else stats[0], status=status.value)


def host_fragments_shade(visibility, world_pos, normal, material, materials, lights, cluster_offset_image, light_index_buffer,
                         cluster_count, tile_size_px, z_scale, z_bias, luminance_cutoff, z_near, view_pos, render_mode=0,
                         clear=True, into=None, form=None, material_count=None, light_count=None, index_capacity=None, fill=0,
                         want_walked=True, want_stats=True):
    """orbit_host_fragments_shade on a (height, width) np.uint64 buffer, the planes of host_surface_fragments (world_pos
    (.., 4), normal (.., 3) np.float32, material (.., 1) np.uint32), np[layouts.MATERIAL] and np[layouts.LIGHT] rows, the
    (offset, count) image (cx * cy * cz pairs of u32) and the ClusterLightIndices bytes (indices at byte 4) -> dict(color
    (height, width, 4) np.float32, lights_walked (height, width) np.uint32 or None, stats: np[layouts.SHADE_STATS] scalar
    row or None, status: what the device call latches).  `into`: the dict of an earlier call to write into (copied),
    clear=False.  Otherwise color and lights_walked start filled with the u32 `fill`: what the call does not write keeps
    it.  The counts default to what the arrays hold."""
    vis = np.ascontiguousarray(visibility, dtype=np.uint64)
    height, width = vis.shape
    wp = np.ascontiguousarray(world_pos, dtype=np.float32).reshape(height, width, 4)
    nrm = np.ascontiguousarray(normal, dtype=np.float32).reshape(height, width, 3)
    mat = np.ascontiguousarray(material, dtype=np.uint32).reshape(height, width)
    mats = np.ascontiguousarray(materials).view(np.uint8).reshape(-1)
    lts = np.ascontiguousarray(lights).view(np.uint8).reshape(-1)
    img = np.ascontiguousarray(cluster_offset_image).view(np.uint32).reshape(-1)
    lib_ = np.ascontiguousarray(light_index_buffer).view(np.uint8).reshape(-1)
    cx, cy, cz = (int(c) for c in cluster_count)
    if img.size < 2 * cx * cy * cz:
        raise ValueError("cluster_count reaches beyond the offset image")
    material_count = mats.nbytes // 80 if material_count is None else int(material_count)
    light_count = lts.nbytes // 64 if light_count is None else int(light_count)
    index_capacity = max(lib_.nbytes - 4, 0) // 4 if index_capacity is None else int(index_capacity)
    if material_count * 80 > mats.nbytes or light_count * 64 > lts.nbytes or 4 + 4 * index_capacity > max(lib_.nbytes, 4):
        raise ValueError("a count reaches beyond its array")
    if into is not None:
        color = np.array(into["color"], dtype=np.float32, order="C").reshape(height, width, 4)
        walked = None if not want_walked else np.array(into["lights_walked"], dtype=np.uint32, order="C").reshape(height, width)
    else:
        color = np.full((height, width, 4), fill, np.uint32).view(np.float32)
        walked = np.full((height, width), fill, np.uint32) if want_walked else None
    stats = np.zeros(1, L.SHADE_STATS) if want_stats else None
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    j = _lib.FragmentsShade()
    j.visibility, j.world_pos, j.normal, j.material, j.materials, j.lights = p(vis), p(wp), p(nrm), p(mat), p(mats), p(lts)
    j.cluster_offset_image, j.light_index_buffer, j.color, j.lights_walked, j.stats = p(img), p(lib_), p(color), p(walked), p(stats)
    j.material_count, j.light_count, j.index_capacity = material_count, light_count, index_capacity
    _lib.fill_fragments_shade(j, (cx, cy, cz), tile_size_px, z_scale, z_bias, luminance_cutoff, z_near, view_pos, render_mode, width,
                              height, clear, form)
    status = C.c_int32(0)
    _check(lib().orbit_host_fragments_shade(C.byref(j), C.byref(status)))
    return dict(color=color, lights_walked=walked, stats=None if stats is None else stats[0], status=status.value)


def host_fragments_shade_shadowed(visibility, world_pos, normal, material, materials, lights, cluster_offset_image, light_index_buffer,
                                  cluster_count, tile_size_px, z_scale, z_bias, luminance_cutoff, z_near, view_pos, shadows, shadow_maps,
                                  shadow_resolution, blocker_search_radius, normal_bias_scale, oriented_bias, shadow_index_base=0,
                                  shadow_count=None, shadow_map_count=None, render_mode=0, clear=True, into=None, form=None,
                                  material_count=None, light_count=None, index_capacity=None, fill=0, want_walked=True, want_stats=True,
                                  want_factor=True, want_cascade=True, want_shadow_stats=True):
    """orbit_host_fragments_shade_shadowed: host_fragments_shade's arguments, then np[layouts.SHADOW_DATA] rows (or None),
    the maps as float32 (map k at float k * res * res; or None) and the ShadowSettings -> host_fragments_shade's dict with
    shadow_factor (height, width) np.float32, cascade (height, width) np.uint32 and shadow_stats:
    np[layouts.SHADOW_STATS] scalar row, each None if not wanted.  With `into` the two planes are taken from it; otherwise
    they start filled with the u32 `fill`.  The counts default to what the arrays hold."""
    vis = np.ascontiguousarray(visibility, dtype=np.uint64)
    height, width = vis.shape
    wp = np.ascontiguousarray(world_pos, dtype=np.float32).reshape(height, width, 4)
    nrm = np.ascontiguousarray(normal, dtype=np.float32).reshape(height, width, 3)
    mat = np.ascontiguousarray(material, dtype=np.uint32).reshape(height, width)
    mats = np.ascontiguousarray(materials).view(np.uint8).reshape(-1)
    lts = np.ascontiguousarray(lights).view(np.uint8).reshape(-1)
    img = np.ascontiguousarray(cluster_offset_image).view(np.uint32).reshape(-1)
    lib_ = np.ascontiguousarray(light_index_buffer).view(np.uint8).reshape(-1)
    rows = None if shadows is None else np.ascontiguousarray(shadows).view(np.uint8).reshape(-1)
    maps = None if shadow_maps is None else np.ascontiguousarray(shadow_maps, dtype=np.float32).reshape(-1)
    cx, cy, cz = (int(c) for c in cluster_count)
    if img.size < 2 * cx * cy * cz:
        raise ValueError("cluster_count reaches beyond the offset image")
    material_count = mats.nbytes // 80 if material_count is None else int(material_count)
    light_count = lts.nbytes // 64 if light_count is None else int(light_count)
    index_capacity = max(lib_.nbytes - 4, 0) // 4 if index_capacity is None else int(index_capacity)
    res = int(shadow_resolution)
    shadow_count = (0 if rows is None else rows.nbytes // 288) if shadow_count is None else int(shadow_count)
    shadow_map_count = (0 if maps is None or res == 0 else maps.size // (res * res)) if shadow_map_count is None else int(shadow_map_count)
    if material_count * 80 > mats.nbytes or light_count * 64 > lts.nbytes or 4 + 4 * index_capacity > max(lib_.nbytes, 4):
        raise ValueError("a count reaches beyond its array")
    if shadow_count * 288 > (0 if rows is None else rows.nbytes) or shadow_map_count * res * res > (0 if maps is None else maps.size):
        raise ValueError("a shadow count reaches beyond its array")
    if into is not None:
        color = np.array(into["color"], dtype=np.float32, order="C").reshape(height, width, 4)
        walked = None if not want_walked else np.array(into["lights_walked"], dtype=np.uint32, order="C").reshape(height, width)
        factor = None if not want_factor else np.array(into["shadow_factor"], dtype=np.float32, order="C").reshape(height, width)
        cascade = None if not want_cascade else np.array(into["cascade"], dtype=np.uint32, order="C").reshape(height, width)
    else:
        color = np.full((height, width, 4), fill, np.uint32).view(np.float32)
        walked = np.full((height, width), fill, np.uint32) if want_walked else None
        factor = np.full((height, width), fill, np.uint32).view(np.float32) if want_factor else None
        cascade = np.full((height, width), fill, np.uint32) if want_cascade else None
    stats = np.zeros(1, L.SHADE_STATS) if want_stats else None
    shadow_stats = np.zeros(1, L.SHADOW_STATS) if want_shadow_stats else None
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    js = _lib.FragmentsShadeShadowed()
    j = js.shade
    j.visibility, j.world_pos, j.normal, j.material, j.materials, j.lights = p(vis), p(wp), p(nrm), p(mat), p(mats), p(lts)
    j.cluster_offset_image, j.light_index_buffer, j.color, j.lights_walked, j.stats = p(img), p(lib_), p(color), p(walked), p(stats)
    j.material_count, j.light_count, j.index_capacity = material_count, light_count, index_capacity
    _lib.fill_fragments_shade(j, (cx, cy, cz), tile_size_px, z_scale, z_bias, luminance_cutoff, z_near, view_pos, render_mode, width,
                              height, clear, form)
    js.shadows, js.shadow_maps, js.shadow_factor, js.cascade, js.shadow_stats = p(rows), p(maps), p(factor), p(cascade), p(shadow_stats)
    _lib.fill_shadow_fields(js, shadow_count, shadow_index_base, shadow_map_count, res, blocker_search_radius, normal_bias_scale, oriented_bias)
    status = C.c_int32(0)
    _check(lib().orbit_host_fragments_shade_shadowed(C.byref(js), C.byref(status)))
    return dict(color=color, lights_walked=walked, stats=None if stats is None else stats[0], status=status.value, shadow_factor=factor,
                cascade=cascade, shadow_stats=None if shadow_stats is None else shadow_stats[0])

SKY_CENSUS_SIZE = 96  # ORBIT_HOST_SKY_CENSUS
SKY_CENSUS = dict(evaluated=64, skipped=65, ndv_negative=66, ndv_zero=67, ndv_one=68, ndv_nan=69, ndv_other=70, took_roughness=71,
                  took_f0=72, bad_normal=73, bad_reflection=74, table_low=75, table_high=76, table_inside=77, ao_null=78,
                  ao_below_one=79, ao_one=80, skybox=81, skybox_bad=82, second_sky_light=83)


def host_fragments_shade_sky(visibility, world_pos, normal, material, materials, lights, cluster_offset_image, light_index_buffer,
                             cluster_count, tile_size_px, z_scale, z_bias, luminance_cutoff, z_near, view_pos, shadows, shadow_maps,
                             shadow_resolution, blocker_search_radius, normal_bias_scale, oriented_bias, env=None, sky=None,
                             skybox_lod=0.0, basis=None, ao=None, shadow_index_base=0, shadow_count=None, shadow_map_count=None,
                             render_mode=0, clear=True, into=None, form=None, material_count=None, light_count=None, index_capacity=None,
                             fill=0, want_walked=True, want_stats=True, want_factor=True, want_cascade=True, want_shadow_stats=True,
                             want_sky_stats=True, want_census=False, over=None, return_job=False):
    """orbit_host_fragments_shade_sky: host_fragments_shade_shadowed's arguments, then env: None or dict(irradiance,
    prefiltered, brdf: np.uint16 arrays in E0's layout as orbit_amd.env_map.host_env_map returns them; irradiance_size,
    prefiltered_size, prefiltered_levels, brdf_size), sky: None or dict(cube, size, levels), K9's skybox_lod and basis
    (orbit_amd.camera.skybox_basis), ao: None or (height, width) float32 -> host_fragments_shade_shadowed's dict with
    sky_stats: np[layouts.SKY_STATS] scalar row and census: np.uint64 (SKY_CENSUS_SIZE,), each None if not wanted.
    `over`: fields of the OrbitFragmentsShadeSky block set last, as they are; return_job: nothing is run, the block and the
    arrays it points into are returned (both for the tests of the argument errors)."""
    vis = np.ascontiguousarray(visibility, dtype=np.uint64)
    height, width = vis.shape
    wp = np.ascontiguousarray(world_pos, dtype=np.float32).reshape(height, width, 4)
    nrm = np.ascontiguousarray(normal, dtype=np.float32).reshape(height, width, 3)
    mat = np.ascontiguousarray(material, dtype=np.uint32).reshape(height, width)
    mats = np.ascontiguousarray(materials).view(np.uint8).reshape(-1)
    lts = np.ascontiguousarray(lights).view(np.uint8).reshape(-1)
    img = np.ascontiguousarray(cluster_offset_image).view(np.uint32).reshape(-1)
    lib_ = np.ascontiguousarray(light_index_buffer).view(np.uint8).reshape(-1)
    rows = None if shadows is None else np.ascontiguousarray(shadows).view(np.uint8).reshape(-1)
    maps = None if shadow_maps is None else np.ascontiguousarray(shadow_maps, dtype=np.float32).reshape(-1)
    cx, cy, cz = (int(c) for c in cluster_count)
    if img.size < 2 * cx * cy * cz:
        raise ValueError("cluster_count reaches beyond the offset image")
    material_count = mats.nbytes // 80 if material_count is None else int(material_count)
    light_count = lts.nbytes // 64 if light_count is None else int(light_count)
    index_capacity = max(lib_.nbytes - 4, 0) // 4 if index_capacity is None else int(index_capacity)
    res = int(shadow_resolution)
    shadow_count = (0 if rows is None else rows.nbytes // 288) if shadow_count is None else int(shadow_count)
    shadow_map_count = (0 if maps is None or res == 0 else maps.size // (res * res)) if shadow_map_count is None else int(shadow_map_count)
    if material_count * 80 > mats.nbytes or light_count * 64 > lts.nbytes or 4 + 4 * index_capacity > max(lib_.nbytes, 4):
        raise ValueError("a count reaches beyond its array")
    if shadow_count * 288 > (0 if rows is None else rows.nbytes) or shadow_map_count * res * res > (0 if maps is None else maps.size):
        raise ValueError("a shadow count reaches beyond its array")
    cubes = {}
    if env is not None:
        cubes = {k: np.ascontiguousarray(env[k], dtype=np.uint16).reshape(-1) for k in ("irradiance", "prefiltered", "brdf")}
        n, m, levels, t = (int(env[k]) for k in ("irradiance_size", "prefiltered_size", "prefiltered_levels", "brdf_size"))
        need = dict(irradiance=24 * n * n, prefiltered=24 * sum(max(1, m >> k) ** 2 for k in range(levels)), brdf=2 * t * t)
        if any(cubes[k].size < need[k] for k in need):
            raise ValueError("an environment size reaches beyond its array")
    if sky is not None:
        cubes["sky"] = np.ascontiguousarray(sky["cube"], dtype=np.uint16).reshape(-1)
        if cubes["sky"].size < 24 * sum(max(1, int(sky["size"]) >> k) ** 2 for k in range(int(sky["levels"]))):
            raise ValueError("the sky cube's size and levels reach beyond its array")
    ao_ = None if ao is None else np.ascontiguousarray(ao, dtype=np.float32).reshape(height, width)
    if into is not None:
        color = np.array(into["color"], dtype=np.float32, order="C").reshape(height, width, 4)
        walked = None if not want_walked else np.array(into["lights_walked"], dtype=np.uint32, order="C").reshape(height, width)
        factor = None if not want_factor else np.array(into["shadow_factor"], dtype=np.float32, order="C").reshape(height, width)
        cascade = None if not want_cascade else np.array(into["cascade"], dtype=np.uint32, order="C").reshape(height, width)
    else:
        color = np.full((height, width, 4), fill, np.uint32).view(np.float32)
        walked = np.full((height, width), fill, np.uint32) if want_walked else None
        factor = np.full((height, width), fill, np.uint32).view(np.float32) if want_factor else None
        cascade = np.full((height, width), fill, np.uint32) if want_cascade else None
    stats = np.zeros(1, L.SHADE_STATS) if want_stats else None
    shadow_stats = np.zeros(1, L.SHADOW_STATS) if want_shadow_stats else None
    sky_stats = np.zeros(1, L.SKY_STATS) if want_sky_stats else None
    census = np.zeros(SKY_CENSUS_SIZE, np.uint64) if want_census else None
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    jk = _lib.FragmentsShadeSky()
    js = jk.shadowed
    j = js.shade
    j.visibility, j.world_pos, j.normal, j.material, j.materials, j.lights = p(vis), p(wp), p(nrm), p(mat), p(mats), p(lts)
    j.cluster_offset_image, j.light_index_buffer, j.color, j.lights_walked, j.stats = p(img), p(lib_), p(color), p(walked), p(stats)
    j.material_count, j.light_count, j.index_capacity = material_count, light_count, index_capacity
    _lib.fill_fragments_shade(j, (cx, cy, cz), tile_size_px, z_scale, z_bias, luminance_cutoff, z_near, view_pos, render_mode, width,
                              height, clear, form)
    js.shadows, js.shadow_maps, js.shadow_factor, js.cascade, js.shadow_stats = p(rows), p(maps), p(factor), p(cascade), p(shadow_stats)
    _lib.fill_shadow_fields(js, shadow_count, shadow_index_base, shadow_map_count, res, blocker_search_radius, normal_bias_scale, oriented_bias)
    jk.irradiance, jk.prefiltered, jk.brdf, jk.sky = (p(cubes.get(k)) for k in ("irradiance", "prefiltered", "brdf", "sky"))
    jk.ao, jk.sky_stats = p(ao_), p(sky_stats)
    e, s = env or {}, sky or {}
    _lib.fill_sky_fields(jk, e.get("irradiance_size", 0), e.get("prefiltered_size", 0), e.get("prefiltered_levels", 0), e.get("brdf_size", 0),
                         s.get("size", 0), s.get("levels", 0), skybox_lod, basis)
    for name, value in (over or {}).items():
        target = jk if hasattr(jk, name) else js if hasattr(js, name) else j
        setattr(target, name, value)
    if return_job:
        return jk, (vis, wp, nrm, mat, mats, lts, img, lib_, rows, maps, cubes, ao_, color, walked, factor, cascade, stats, shadow_stats, sky_stats)
    status = C.c_int32(0)
    fn = lib().orbit_host_fragments_shade_sky
    fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]
    _check(fn(C.byref(jk), C.byref(status), p(census)))
    return dict(color=color, lights_walked=walked, stats=None if stats is None else stats[0], status=status.value, shadow_factor=factor,
                cascade=cascade, shadow_stats=None if shadow_stats is None else shadow_stats[0],
                sky_stats=None if sky_stats is None else sky_stats[0], census=census)


def host_shadow_rotation(x0, y0, width, height):
    """H6 of the pixels (x0 + x, y0 + y), x < width, y < height -> (theta, sine, cosine), each (height, width) np.float32:
    the mirror's noise angle and csrc/shadow_common.h's sine and cosine of it."""
    out = [np.empty((height, width), np.float32) for _ in range(3)]
    fn = lib().orbit_host_shadow_rotation
    fn.restype, fn.argtypes = None, [C.c_uint32] * 4 + [C.c_void_p] * 3
    fn(int(x0), int(y0), int(width), int(height), *(a.ctypes.data for a in out))
    return tuple(out)


def shadow_rows(matrices, world_sizes, map_indices=(0, 1, 2, 3)):
    """One np[layouts.SHADOW_DATA] row from four column-major 16-float matrices, four world sizes and four map indices."""
    row = np.zeros(1, L.SHADOW_DATA)
    row["light_projection_matrices"][0] = np.asarray(matrices, np.float32).reshape(4, 16)
    row["shadow_map_world_sizes"][0], row["shadow_map_indices"][0] = world_sizes, map_indices
    return row


def host_shadow_atlas(draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data, matrices, resolution, **kw):
    """The cascades' maps on the host: one host_raster_depth call per matrix (column-major 16 floats) with the clear, into
    one (len(matrices), resolution, resolution) np.float32 atlas — what Engine.shadow_atlas leaves on the device."""
    atlas = np.zeros((len(matrices), resolution, resolution), np.float32)
    for k, m in enumerate(matrices):
        atlas[k] = host_raster_depth(draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data, m, resolution,
                                     resolution, **kw)[0]
    return atlas


def shadow_atlas(engine, atlas, draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data, entity_count, matrices,
                 resolution, **kw):
    """The cascades' maps on the device: one Engine.raster_depth call per matrix (column-major 16 floats) with the clear,
    map k into atlas[k] of the (len(matrices), resolution, resolution) float32 device tensor `atlas` — the shadow_maps of
    Engine.fragments_shade_shadowed, shadow_map_indices[c] = k.  No kernel of its own; kw: raster_depth's keywords."""
    for k, m in enumerate(matrices):
        engine.raster_depth(draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data, entity_count, m, atlas[k],
                            resolution, resolution, clear=True, **kw)
    return atlas


def host_shade_log2(x):
    """The host restatement of the canonical log2 (csrc/shade_common.h shade_log2c) of a float32 -> np.float32."""
    fn = lib().orbit_host_shade_log2
    fn.restype, fn.argtypes = C.c_float, [C.c_float]
    return np.float32(fn(float(x)))


def host_shade_slice(z_near, d, z_scale, z_bias):
    """L2's slice of a depth d: uint(fma(log2c(z_near / d), z_scale, z_bias)) as the host mirror takes it."""
    fn = lib().orbit_host_shade_slice
    fn.restype, fn.argtypes = C.c_uint32, [C.c_float] * 4
    return int(fn(float(z_near), float(d), float(z_scale), float(z_bias)))
