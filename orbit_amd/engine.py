"""Thin object wrapper over the C ABI for callers that hold torch tensors.

torch is plumbing here (device memory + streams); every method forwards raw
device pointers to ``liborbit_cull.so`` and enqueues on the current HIP stream.
Argument order follows the push-constant order of the reference shaders, as in
``include/orbit_abi.h``.
"""
import ctypes as C

import numpy as np

from . import _lib, layouts


def _ptr(t):
    """Device pointer of a torch tensor, or a raw integer address (used to pass a
    shard of a large buffer under its global indices: base = shard_ptr - first * stride)."""
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    return C.c_void_p(t.data_ptr())


def _stream(stream):
    import torch

    s = torch.cuda.current_stream() if stream is None else stream
    return C.c_void_p(s.cuda_stream)


def _host_bytes(x, nbytes):
    a = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    if a.nbytes != nbytes:
        raise ValueError(f"expected a {nbytes}-byte host block, got {a.nbytes}")
    return a


def _raster_job(j, draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data, entity_count, view_proj,
                width, height, clear, cull_none, stats, vertex_stride, position_offset, meshlet_data_words, clip_near=False,
                wide_guard=False):
    """The fields that _lib.RasterDepth and _lib.RasterVisibility share, filled into `j` -> j."""
    nbytes = lambda t: 0 if t is None or isinstance(t, int) else t.numel() * t.element_size()  # noqa: E731
    j.draw_commands, j.meshlet_data, j.vertices = _ptr(draw_commands), _ptr(meshlet_data), _ptr(vertices)
    j.entity_data, j.stats = _ptr(entity_data), _ptr(stats)
    j.meshlet_data_words = nbytes(meshlet_data) // 4 if meshlet_data_words is None else int(meshlet_data_words)
    j.vertex_count, j.max_commands, j.entity_count = int(vertex_count), int(max_commands), int(entity_count)
    j.vertex_stride, j.position_offset, j.width, j.height = int(vertex_stride), int(position_offset), int(width), int(height)
    j.flags = ((_lib.RASTER_CLEAR if clear else 0) | (_lib.RASTER_CULL_NONE if cull_none else 0)
               | (_lib.RASTER_CLIP_NEAR if clip_near else 0) | (_lib.RASTER_WIDE_GUARD if wide_guard else 0))
    j.view_proj = (C.c_float * 16)(*np.asarray(view_proj, dtype=np.float32).reshape(16))
    return j


def depth_pyramid_desc(screen_width, screen_height):
    """DepthPyramid::new geometry (src/passes/draw_gen.rs:457-459)."""
    d = _lib.DepthPyramidDesc()
    _lib.check(_lib.load().orbit_depth_pyramid_desc(screen_width, screen_height, C.byref(d)))
    return d


def visibility_compact_workspace(max_commands):
    """The bytes of scratch Engine.visibility_compact needs for a list of max_commands (orbit_visibility_compact_workspace)."""
    return int(_lib.load().orbit_visibility_compact_workspace(int(max_commands)))


def shard_range(entity_draw_count, rank, world):
    b, e = C.c_uint32(), C.c_uint32()
    _lib.load().orbit_shard_range(entity_draw_count, rank, world, C.byref(b), C.byref(e))
    return b.value, e.value


def cull_stats_dict(stats):
    """The 256 bytes of an OrbitCullStats (a torch tensor or anything numpy can view as bytes) as {counter: int};
    lod_drawn is a list of 8 and the reserved words are left out."""
    if hasattr(stats, "detach"):
        stats = stats.detach().cpu().numpy()
    raw = np.ascontiguousarray(stats).reshape(-1).view(np.uint8)[:layouts.CULL_STATS.itemsize]
    rec = raw.view(layouts.CULL_STATS)[0]
    return {n: [int(v) for v in rec[n]] if n == "lod_drawn" else int(rec[n])
            for n in layouts.CULL_STATS.names if not n.startswith("reserved")}


def cluster_stats_dict(stats):
    """The 256 bytes of an OrbitClusterStats (a torch tensor or anything numpy can view as bytes) as {counter: int};
    clusters_by_lights and samples_by_lights are lists of 5 and the reserved words are left out."""
    if hasattr(stats, "detach"):
        stats = stats.detach().cpu().numpy()
    raw = np.ascontiguousarray(stats).reshape(-1).view(np.uint8)[:layouts.CLUSTER_STATS.itemsize]
    rec = raw.view(layouts.CLUSTER_STATS)[0]
    return {n: [int(v) for v in rec[n]] if n.endswith("_by_lights") else int(rec[n])
            for n in layouts.CLUSTER_STATS.names if not n.startswith("reserved")}


class MeshletStream:
    """Handle of an OrbitMeshletStream (include/orbit_abi.h, "Derived meshlet streams"): created over [first, first +
    count) and updated from `meshlet_buffer` over all of it (initial_update=False: created only, nothing readable yet)."""

    def __init__(self, engine, meshlet_buffer, first, count, stream=None, initial_update=True):
        self._engine, self._lib = engine, engine._lib
        self._h = C.c_void_p()
        self.first, self.capacity = int(first), int(count)
        _lib.check(self._lib.orbit_meshlet_stream_create(engine._ctx, self.first, self.capacity, C.byref(self._h)),
                   engine._ctx)
        if initial_update:
            self.update(meshlet_buffer, first, count, stream)

    def update(self, meshlet_buffer, first=None, count=None, stream=None):
        first = self.first if first is None else int(first)
        count = self.capacity if count is None else int(count)
        _lib.check(self._lib.orbit_meshlet_stream_update(self._engine._ctx, self._h, _ptr(meshlet_buffer), first, count,
                                                         _stream(stream)), self._engine._ctx)

    def set_materials(self, material_buffer, material_count, stream=None):
        """orbit_meshlet_stream_set_materials: alpha classes from material_buffer[material_index].alpha_mode
        (None forgets them).  Culls whose material buffer is this one then read no material index."""
        _lib.check(self._lib.orbit_meshlet_stream_set_materials(self._engine._ctx, self._h, _ptr(material_buffer),
                                                                int(material_count), _stream(stream)), self._engine._ctx)

    def update_meshes(self, mesh_info_buffer, first_mesh, count, stream=None):
        """orbit_meshlet_stream_update_meshes: 32-B side entries of meshes [first_mesh, first_mesh + count) of
        `mesh_info_buffer` (None forgets the table); entity culls of that buffer then read them instead of the MeshInfos."""
        _lib.check(self._lib.orbit_meshlet_stream_update_meshes(self._engine._ctx, self._h, _ptr(mesh_info_buffer),
                                                                int(first_mesh), int(count), _stream(stream)),
                   self._engine._ctx)

    def validate(self, meshlet_buffer, material_buffer=None, stream=None):
        """orbit_meshlet_stream_validate: ORBIT_E_STALE is latched (Engine.status raises) if the stream differs."""
        _lib.check(self._lib.orbit_meshlet_stream_validate(self._engine._ctx, self._h, _ptr(meshlet_buffer),
                                                           _ptr(material_buffer), _stream(stream)), self._engine._ctx)

    def read_arrays(self, first=None, count=None, stream=None):
        """orbit_meshlet_stream_read_arrays (tests): the derived arrays of meshlets [first, first + count) — by default
        the whole stream — as a dict of numpy arrays: sphere u32[n, 4], cone u32[n], mat u16[n], cmd u32[n, 3], cnt
        u16[n], and link / cls0 / cls1 u32[words], base32 u32[words, 2] for words first // 32 .. (first + count - 1) // 32
        of global meshlet indices."""
        first = self.first if first is None else int(first)
        count = self.capacity if count is None else int(count)
        words = ((first + count - 1) >> 5) - (first >> 5) + 1 if count else 0
        out = dict(sphere=np.zeros((count, 4), np.uint32), cone=np.zeros(count, np.uint32), mat=np.zeros(count, np.uint16),
                   cmd=np.zeros((count, 3), np.uint32), cnt=np.zeros(count, np.uint16), link=np.zeros(words, np.uint32),
                   cls0=np.zeros(words, np.uint32), cls1=np.zeros(words, np.uint32), base32=np.zeros((words, 2), np.uint32))
        block = _lib.MeshletStreamArrays(**{k: v.ctypes.data for k, v in out.items()})
        _lib.check(self._lib.orbit_meshlet_stream_read_arrays(self._engine._ctx, self._h, first, count, C.byref(block),
                                                              _stream(stream)), self._engine._ctx)
        return out

    def close(self):
        """orbit_meshlet_stream_destroy.  The library refuses while a context still has the stream bound; the engine
        this handle came from is unbound here, other engines are the caller's to unbind first."""
        if getattr(self, "_h", None) is not None and self._h.value:
            if getattr(self._engine, "_meshlet_stream", None) is self and getattr(self._engine, "_ctx", None):
                self._engine.bind_meshlet_stream(None)
            _lib.check(self._lib.orbit_meshlet_stream_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreparedShardCull:
    """Engine.prepare_cull_shard: orbit_cull_shard's argument blocks, kept alive and reusable frame after frame."""

    def __init__(self, engine, cull_info, entity_draw_buffer, mesh_info_buffer, meshlet_dispatch_buffer, entity_buffer,
                 draw_first, draw_count, dispatch_capacity, meshlet_buffer, material_buffer, record_buffer, record_capacity,
                 draw_commands_buffer, draw_capacity, material_count, visibility_buffer, meshlet_visibility_buffer,
                 depth_pyramid, depth_pyramid_size, stream):
        self.cull_info = _host_bytes(cull_info, 400).copy()  # the call reads THIS buffer: update it in place per frame
        e, m = _lib.EntityCullBufs(), _lib.MeshletCullBufs()
        e.entity_draw_buffer = _ptr(entity_draw_buffer)
        e.mesh_info_buffer = _ptr(mesh_info_buffer)
        e.meshlet_dispatch_buffer = m.meshlet_dispatch_buffer = _ptr(meshlet_dispatch_buffer)
        e.entity_buffer = m.entity_buffer = _ptr(entity_buffer)
        e.visibility_buffer = _ptr(visibility_buffer)
        e.depth_pyramid = m.depth_pyramid = _ptr(depth_pyramid)
        e.depth_pyramid_size[0], e.depth_pyramid_size[1] = depth_pyramid_size
        m.depth_pyramid_size[0], m.depth_pyramid_size[1] = depth_pyramid_size
        e.dispatch_capacity = m.dispatch_capacity = dispatch_capacity
        m.meshlet_buffer = _ptr(meshlet_buffer)
        m.draw_commands_buffer = _ptr(draw_commands_buffer)
        m.material_buffer = _ptr(material_buffer)
        m.meshlet_visibility_buffer = _ptr(meshlet_visibility_buffer)
        m.draw_capacity = draw_capacity
        m.material_count = material_count
        self._fn, self._ctx = engine._lib.orbit_cull_shard, engine._ctx
        self._cip, self._ep, self._mp = self.cull_info.ctypes.data_as(C.c_void_p), C.byref(e), C.byref(m)
        self._rec, self._st = _ptr(record_buffer), _stream(stream)
        self._args = (int(draw_first), int(draw_count), int(record_capacity), 1 if draw_commands_buffer is not None else 0)
        self._keep = (e, m, stream, engine)  # the blocks (and the stream object) live as long as the call does

    def set_cull_info(self, cull_info):
        self.cull_info[:] = _host_bytes(cull_info, 400)

    def __call__(self):
        first, count, cap, with_cmds = self._args
        rc = self._fn(self._ctx, self._cip, self._ep, first, count, self._mp, self._rec, cap, with_cmds, self._st)
        if rc != _lib.OK:
            _lib.check(rc, self._ctx)


class Engine:
    """One ``OrbitCtx``: scan scratch sized from ``caps`` on one gfx950 device."""

    def __init__(self, device_index=0, _library=None, **caps):
        lib = _lib.load() if _library is None else _library  # _library: a variant build (tools/ab_libs.py)
        c = _lib.Caps()
        lib.orbit_default_caps(C.byref(c))
        for k, v in caps.items():
            if not hasattr(c, k):
                raise TypeError(f"unknown capacity {k}")
            setattr(c, k, int(v))
        self.caps = c
        self._ctx = C.c_void_p()
        _lib.check(lib.orbit_ctx_create(device_index, C.byref(c), C.byref(self._ctx)))
        self._lib = lib

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.orbit_ctx_destroy(self._ctx)  # unbinds its meshlet stream
            self._ctx = C.c_void_p()
            self._meshlet_stream = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def status(self, stream=None, sync=True):
        """Raises OrbitError for a device-latched condition (capacity overflow, timeout)."""
        _lib.check(self._lib.orbit_ctx_status(self._ctx, _stream(stream), 1 if sync else 0), self._ctx)

    def profile(self, enable=True, every=1):
        """HIP-event timing of the dominant kernel of meshlet_cull (measurement hook); every n-th call is timed."""
        _lib.check(self._lib.orbit_ctx_profile(self._ctx, int(every) if enable else 0), self._ctx)

    def profile_reserve(self, pairs, stream=None):
        """orbit_ctx_profile_reserve: the hook's event pairs created (and recorded once on `stream`) before a timed region."""
        _lib.check(self._lib.orbit_ctx_profile_reserve(self._ctx, int(pairs), _stream(stream)), self._ctx)

    def profile_read(self):
        ms, n = C.c_float(), C.c_uint32()
        _lib.check(self._lib.orbit_ctx_profile_read(self._ctx, C.byref(ms), C.byref(n)), self._ctx)
        return ms.value, n.value

    # -- entity_cull: create_meshlet_dispatch_command body (draw_gen.rs:327-380)
    def entity_cull(self, cull_info, entity_draw_buffer, mesh_info_buffer, meshlet_dispatch_buffer, entity_buffer,
                    entity_draw_count, dispatch_capacity, visibility_buffer=None, depth_pyramid=None,
                    depth_pyramid_size=(0, 0), draw_first=None, stream=None, depth_pyramid_levels=None):
        ci = _host_bytes(cull_info, 400)
        b = _lib.EntityCullBufs()
        b.entity_draw_buffer = _ptr(entity_draw_buffer)
        b.mesh_info_buffer = _ptr(mesh_info_buffer)
        b.meshlet_dispatch_buffer = _ptr(meshlet_dispatch_buffer)
        b.entity_buffer = _ptr(entity_buffer)
        b.visibility_buffer = _ptr(visibility_buffer)
        b.depth_pyramid = _ptr(depth_pyramid)
        b.depth_pyramid_size[0], b.depth_pyramid_size[1] = depth_pyramid_size
        b.dispatch_capacity = dispatch_capacity
        b.depth_pyramid_levels = _ptr(depth_pyramid_levels)  # DEVICE array of OrbitDepthPyramidLevel, or None
        if draw_first is None:
            rc = self._lib.orbit_entity_cull(self._ctx, ci.ctypes.data_as(C.c_void_p), C.byref(b), entity_draw_count,
                                             _stream(stream))
        else:
            rc = self._lib.orbit_entity_cull_range(self._ctx, ci.ctypes.data_as(C.c_void_p), C.byref(b), draw_first,
                                                   entity_draw_count, _stream(stream))
        _lib.check(rc, self._ctx)

    # -- the scene update: EntityData rows from transforms on the device (orbit_scene_update_entities)
    def scene_update_entities(self, transforms, entity_data, count=None, instance_indices=None, entity_capacity=None,
                              stream=None):
        """entity_data[i] (or entity_data[instance_indices[i]]) = EntityData::entity_gpu_data of transforms[i], i < count.
        transforms: device tensor holding layouts.ENTITY_TRANSFORM rows (40 B each); instance_indices: device tensor
        holding u32 indices (any dtype: its bytes are read), or None for the dense form.  count defaults to the 4-B
        entries of instance_indices (sparse) or the 40-B rows of transforms (dense), entity_capacity to the 128-B rows
        entity_data holds.  Enqueued on `stream`; an index past the capacity is reported by status() (ORBIT_E_RANGE)."""
        nbytes = lambda t: t.numel() * t.element_size()  # noqa: E731
        if count is None:
            count = nbytes(instance_indices) // 4 if instance_indices is not None else nbytes(transforms) // 40
        if entity_capacity is None:
            entity_capacity = nbytes(entity_data) // 128
        _lib.check(self._lib.orbit_scene_update_entities(self._ctx, _ptr(transforms), _ptr(instance_indices), int(count),
                                                         _ptr(entity_data), int(entity_capacity), _stream(stream)),
                   self._ctx)

    # -- the whole scene update on the device: draws, rows, lights and shadow indices (orbit_scene_update)
    def scene_update(self, entities, transforms, entity_data, entity_draw_buffer, light_data, entity_count=None,
                     shadow_orientations=None, instance_of_entity=None, light_of_entity=None, counts=None,
                     instance_capacity=None, light_capacity=None, shadow_capacity=None, luminance_cutoff=0.25,
                     shadow_index_base=0, stream=None):
        """SceneData::update_scene on the device.  entities / transforms: device tensors holding one
        layouts.SCENE_ENTITY (48 B) and one layouts.ENTITY_TRANSFORM (40 B) per entity, in entity order
        (SceneData.update_scene_device makes them).  Written: entity_data (128-B rows in instance order),
        entity_draw_buffer ({u32 count; draws}), light_data (64-B rows) and, where given, shadow_orientations (16 B per
        shadow command), the two u32 maps entity -> instance / light (layouts.NONE where none) and counts
        (layouts.SCENE_COUNTS, uncapped).  entity_count defaults to the 48-B entries of `entities`, the capacities to
        what the output tensors hold.  Enqueued on `stream`; rows past a capacity and light kinds above 2 are reported
        by status() (ORBIT_E_CAPACITY, ORBIT_E_RANGE).  The entity cull takes the draw count from the buffer: pass it
        entity_draw_count = entity_count (an upper bound) and nothing is read back."""
        nbytes = lambda t: 0 if t is None or isinstance(t, int) else t.numel() * t.element_size()  # noqa: E731
        u = _lib.SceneUpdate()
        u.entities, u.transforms, u.entity_data = _ptr(entities), _ptr(transforms), _ptr(entity_data)
        u.entity_draw_buffer, u.light_data = _ptr(entity_draw_buffer), _ptr(light_data)
        u.shadow_orientations = _ptr(shadow_orientations)
        u.instance_of_entity, u.light_of_entity, u.counts = _ptr(instance_of_entity), _ptr(light_of_entity), _ptr(counts)
        u.entity_count = nbytes(entities) // 48 if entity_count is None else int(entity_count)
        u.instance_capacity = (min(nbytes(entity_data) // 128, max(nbytes(entity_draw_buffer) - 4, 0) // 12)
                               if instance_capacity is None else int(instance_capacity))
        u.light_capacity = nbytes(light_data) // 64 if light_capacity is None else int(light_capacity)
        u.shadow_capacity = nbytes(shadow_orientations) // 16 if shadow_capacity is None else int(shadow_capacity)
        u.luminance_cutoff = float(luminance_cutoff)
        u.shadow_index_base = int(shadow_index_base) & 0xFFFFFFFF
        _lib.check(self._lib.orbit_scene_update(self._ctx, C.byref(u), _stream(stream)), self._ctx)

    # -- geometry bounds from the vertex buffer on the device (orbit_meshlet_bounds, orbit_mesh_bounds)
    def meshlet_bounds(self, meshlets, meshlet_data, vertices, vertex_count, vertex_stride=12, position_offset=0,
                       first_meshlet=0, meshlet_count=None, meshlet_indices=None, full=None, keep_records=False,
                       meshlet_capacity=None, meshlet_data_words=None, stream=None):
        """Bytes 0..19 (sphere, snorm8 cone axis and cutoff) of the selected 32-B records of `meshlets` recomputed from
        `vertices` (position i = 3 floats at byte i * vertex_stride + position_offset), bit-equal to the host mirror's
        compute_meshlet_bounds.  The selection is the range [first_meshlet, first_meshlet + meshlet_count) or, if given,
        the u32 global indices in the device tensor `meshlet_indices` (any dtype: its bytes are read).  full: device
        tensor of 48-B layouts.MESHLET_BOUNDS_FULL rows, one per selected meshlet; keep_records: write `full` only.
        The capacities default to what the tensors hold.  Enqueued on `stream`; a meshlet that points out of range is
        left unwritten and reported by status() (ORBIT_E_RANGE).  A derived stream of these records needs
        MeshletStream.update of the same range afterwards."""
        nbytes = lambda t: 0 if t is None or isinstance(t, int) else t.numel() * t.element_size()  # noqa: E731
        j = _lib.MeshletBoundsJob()
        j.meshlets, j.meshlet_data, j.vertices = _ptr(meshlets), _ptr(meshlet_data), _ptr(vertices)
        j.meshlet_indices, j.full = _ptr(meshlet_indices), _ptr(full)
        j.meshlet_capacity = nbytes(meshlets) // 32 if meshlet_capacity is None else int(meshlet_capacity)
        j.meshlet_data_words = nbytes(meshlet_data) // 4 if meshlet_data_words is None else int(meshlet_data_words)
        if meshlet_count is None:
            meshlet_count = nbytes(meshlet_indices) // 4 if meshlet_indices is not None else j.meshlet_capacity - first_meshlet
        j.first_meshlet, j.meshlet_count, j.vertex_count = int(first_meshlet), int(meshlet_count), int(vertex_count)
        j.vertex_stride, j.position_offset = int(vertex_stride), int(position_offset)
        j.flags = _lib.BOUNDS_KEEP_RECORDS if keep_records else 0
        _lib.check(self._lib.orbit_meshlet_bounds(self._ctx, C.byref(j), _stream(stream)), self._ctx)

    def mesh_bounds(self, ranges, vertices, vertex_count, mesh_infos, vertex_stride=12, position_offset=0,
                    range_count=None, mesh_capacity=None, stream=None):
        """bounding_sphere, aabb_min.xyz and aabb_max.xyz of mesh_infos[mesh_index] for every {mesh_index, first_vertex,
        vertex_count} (3 u32) of the device tensor `ranges`, as gltf_loader.rs:480-506 computes them; nothing else of
        the 128-B MeshInfos is written.  range_count and mesh_capacity default to what the tensors hold.  Enqueued on
        `stream`; a range beyond vertex_count or a mesh beyond the capacity is reported by status() (ORBIT_E_RANGE).
        A bound mesh side table needs MeshletStream.update_meshes afterwards."""
        nbytes = lambda t: 0 if t is None or isinstance(t, int) else t.numel() * t.element_size()  # noqa: E731
        range_count = nbytes(ranges) // 12 if range_count is None else int(range_count)
        mesh_capacity = nbytes(mesh_infos) // 128 if mesh_capacity is None else int(mesh_capacity)
        _lib.check(self._lib.orbit_mesh_bounds(self._ctx, _ptr(ranges), range_count, _ptr(vertices), int(vertex_count),
                                               int(vertex_stride), int(position_offset), _ptr(mesh_infos),
                                               mesh_capacity, _stream(stream)), self._ctx)

    # -- the depth prepass of a draw-command buffer in compute (orbit_raster_depth)
    def raster_depth(self, draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data, entity_count,
                     view_proj, depth, width, height, clear=False, cull_none=False, stats=None, vertex_stride=12,
                     position_offset=0, meshlet_data_words=None, stream=None, clip_near=False, wide_guard=False):
        """Rasterises the {u32 count; 28-B commands} of the device tensor `draw_commands` (what meshlet_cull wrote; the
        count is read on the device and clamped by max_commands) into the width x height float tensor `depth`:
        reversed z, max-merged by atomicMax into what it holds, or into zeros with clear=True (LoadOp::Clear(0.0)).
        `view_proj`: 16 floats, column-major; `vertices`: position i = 3 floats at i * vertex_stride + position_offset;
        `entity_data`: 128-B rows.  `stats`: device tensor of 32 bytes (layouts.RASTER_STATS), cleared by the call.
        Back faces are culled unless cull_none.  clip_near (ORBIT_RASTER_CLIP_NEAR): a triangle crossing the near plane
        is cut there and drawn instead of skipped.  wide_guard (ORBIT_RASTER_WIDE_GUARD): a triangle with a vertex
        beyond the guard band (up to 2^60 sub-pixel units) is drawn instead of guard_skipped.  Byte-equal to
        orbit_amd.raster.host_raster_depth on host copies.  Enqueued on `stream`; a command that points out of range is
        skipped and reported by status() (ORBIT_E_RANGE)."""
        j = _raster_job(_lib.RasterDepth(), draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data,
                        entity_count, view_proj, width, height, clear, cull_none, stats, vertex_stride, position_offset,
                        meshlet_data_words, clip_near, wide_guard)
        j.depth = _ptr(depth)
        _lib.check(self._lib.orbit_raster_depth(self._ctx, C.byref(j), _stream(stream)), self._ctx)

    # -- the same pass keeping the winner's identity, and its resolve (orbit_raster_visibility, orbit_visibility_resolve)
    def raster_visibility(self, draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data,
                          entity_count, view_proj, visibility, width, height, command_base=0, clear=False,
                          cull_none=False, stats=None, vertex_stride=12, position_offset=0, meshlet_data_words=None,
                          stream=None, clip_near=False, wide_guard=False):
        """raster_depth into the width x height u64 tensor `visibility` (8-B aligned): an inside sample with depth d > 0
        of triangle t of the i-th command merges float_bits(d) << 32 | (command_base + i) << 8 | t by a 64-bit
        atomicMax into what the buffer holds, or into zeros with clear=True; 0 is an uncovered pixel.  The high halves
        are raster_depth's depth bytes.  A command with more than 256 triangles is skipped like one that points out of
        range (status(): ORBIT_E_RANGE); command_base + max_commands may not exceed 2^24.  clip_near and wide_guard as
        raster_depth's: the pieces of a cut triangle carry its own index.  Byte-equal to
        orbit_amd.raster.host_raster_visibility on host copies.  Enqueued on `stream`."""
        j = _raster_job(_lib.RasterVisibility(), draw_commands, max_commands, meshlet_data, vertices, vertex_count, entity_data,
                        entity_count, view_proj, width, height, clear, cull_none, stats, vertex_stride, position_offset,
                        meshlet_data_words, clip_near, wide_guard)
        j.visibility, j.command_base = _ptr(visibility), int(command_base)
        _lib.check(self._lib.orbit_raster_visibility(self._ctx, C.byref(j), _stream(stream)), self._ctx)

    def visibility_resolve(self, visibility, width, height, command_base=0, max_commands=0, depth=None,
                           command_pixels=None, stats=None, stream=None):
        """One read of the width x height u64 tensor `visibility`.  depth (width * height floats): the high halves, what
        depth_reduce and the late cull read; command_pixels (max_commands u32, cleared by the call): the pixels whose
        winner is command command_base + k; stats (16 bytes, layouts.VIS_STATS, cleared by the call): covered_pixels,
        visible_commands (non-zero entries of command_pixels), foreign_pixels (covered, command outside the range).
        Each output may be None, not all.  Enqueued on `stream`."""
        j = _lib.VisibilityResolve()
        j.visibility, j.depth, j.command_pixels, j.stats = _ptr(visibility), _ptr(depth), _ptr(command_pixels), _ptr(stats)
        j.width, j.height, j.command_base, j.max_commands = int(width), int(height), int(command_base), int(max_commands)
        _lib.check(self._lib.orbit_visibility_resolve(self._ctx, C.byref(j), _stream(stream)), self._ctx)

    # -- the exact visible draw list of a visibility buffer (orbit_visibility_compact)
    def visibility_compact(self, visibility, width, height, draw_commands, max_commands, triangle_masks, visible_commands,
                           visible_capacity, workspace, command_base=0, meshlet_data=None, meshlet_data_words=None,
                           visible_ids=None, visible_data=None, visible_data_words=0, stats=None, triangles=False,
                           workspace_bytes=None, stream=None):
        """From the width x height u64 tensor `visibility` and the {u32 count; 28-B commands} `draw_commands` that were
        rasterised into it with `command_base` to the list of the commands that own a pixel, in the list's order, in
        `visible_commands` ({u32 count; visible_capacity commands}: what raster_depth / raster_visibility read).
        triangle_masks (8 * max_commands u32, cleared by the call): bit t of command k's 256 bits = triangle t owns a
        pixel.  visible_ids (visible_capacity u32 or None): command_base + k of each written command.  triangles=True
        (ORBIT_COMPACT_TRIANGLES): each command is cut down to the triangles that own a pixel, its index words and
        their corner bytes packed into `visible_data` (visible_data_words u32), which the output list then indexes in
        place of `meshlet_data`.  stats (32 bytes, layouts.VIS_COMPACT_STATS, cleared by the call): visible_commands
        and data_words_needed tell what to allocate.  workspace: visibility_compact_workspace(max_commands) bytes,
        8-B aligned.  Byte-equal to orbit_amd.raster.host_visibility_compact.  Enqueued on `stream`; a dropped command
        is reported by status() (ORBIT_E_CAPACITY), a buffer that was not made from this list by ORBIT_E_RANGE."""
        nbytes = lambda t: 0 if t is None or isinstance(t, int) else t.numel() * t.element_size()  # noqa: E731
        j = _lib.VisibilityCompact()
        j.visibility, j.draw_commands, j.meshlet_data = _ptr(visibility), _ptr(draw_commands), _ptr(meshlet_data)
        j.triangle_masks, j.visible_commands, j.visible_ids = _ptr(triangle_masks), _ptr(visible_commands), _ptr(visible_ids)
        j.visible_data, j.stats, j.workspace = _ptr(visible_data), _ptr(stats), _ptr(workspace)
        j.meshlet_data_words = nbytes(meshlet_data) // 4 if meshlet_data_words is None else int(meshlet_data_words)
        j.workspace_bytes = ((nbytes(workspace) if not isinstance(workspace, int) else visibility_compact_workspace(max_commands))
                             if workspace_bytes is None else int(workspace_bytes))
        j.width, j.height, j.command_base, j.max_commands = int(width), int(height), int(command_base), int(max_commands)
        j.visible_capacity, j.visible_data_words = int(visible_capacity), int(visible_data_words)
        j.flags = _lib.COMPACT_TRIANGLES if triangles else 0
        _lib.check(self._lib.orbit_visibility_compact(self._ctx, C.byref(j), _stream(stream)), self._ctx)

    # -- barycentrics, their differences and ids per pixel of a visibility buffer (orbit_visibility_surface)
    def visibility_surface(self, visibility, width, height, draw_commands, max_commands, meshlet_data, vertices, vertex_count,
                           entity_data, entity_count, view_proj, bary=None, grad=None, triangle=None, stats=None,
                           command_base=0, clear=False, vertex_stride=12, position_offset=0, meshlet_data_words=None,
                           stream=None, raster_flags=None):
        """From the width x height u64 tensor `visibility` and the list that was rasterised into it with `command_base`
        (the arguments of raster_visibility) to what a renderer shades from, for every pixel the list owns: bary (2
        floats per pixel: the perspective-correct l1, l2 of the sample in the owning triangle, in meshlet_data's corner
        order; l0 = 1 - l1 - l2), grad (4 floats: their differences to the samples one pixel right and one pixel down, as
        dl1/dx, dl2/dx, dl1/dy, dl2/dy) and triangle (4 u32: entity, three global vertices).  Each may be None, not all.
        Uncovered pixels, pixels of another list, and pixels of a near-cut or wide triangle (unsupported_pixels) are not
        written; clear=True (ORBIT_SURFACE_CLEAR) fills the outputs first (0.0, 0xFFFFFFFF).  stats (32 bytes,
        layouts.SURFACE_STATS, cleared by the call).  A pixel that the list cannot have drawn is counted in stale_pixels
        and reported by status() (ORBIT_E_RANGE).  Byte-equal to orbit_amd.raster.host_visibility_surface.  Enqueued
        on `stream`."""
        nbytes = lambda t: 0 if t is None or isinstance(t, int) else t.numel() * t.element_size()  # noqa: E731
        j = _lib.VisibilitySurface()
        j.visibility, j.draw_commands, j.meshlet_data = _ptr(visibility), _ptr(draw_commands), _ptr(meshlet_data)
        j.vertices, j.entity_data = _ptr(vertices), _ptr(entity_data)
        j.bary, j.grad, j.triangle, j.stats = _ptr(bary), _ptr(grad), _ptr(triangle), _ptr(stats)
        j.meshlet_data_words = nbytes(meshlet_data) // 4 if meshlet_data_words is None else int(meshlet_data_words)
        j.vertex_count, j.max_commands, j.entity_count = int(vertex_count), int(max_commands), int(entity_count)
        j.vertex_stride, j.position_offset, j.width, j.height = int(vertex_stride), int(position_offset), int(width), int(height)
        j.flags, j.command_base = _lib.SURFACE_CLEAR if clear else 0, int(command_base)
        j.view_proj = (C.c_float * 16)(*np.asarray(view_proj, dtype=np.float32).reshape(16))
        if raster_flags is None:
            _lib.check(self._lib.orbit_visibility_surface(self._ctx, C.byref(j), _stream(stream)), self._ctx)
        else:
            _lib.check(self._lib.orbit_visibility_surface_drawn(self._ctx, C.byref(j), C.c_uint32(raster_flags), _stream(stream)),
                       self._ctx)

    def visibility_surface_drawn(self, *args, clip_near=False, wide_guard=False, **kwargs):
        """visibility_surface for a buffer drawn with clip_near (ORBIT_RASTER_CLIP_NEAR) and / or wide_guard
        (ORBIT_RASTER_WIDE_GUARD), the flags raster_visibility was given: the pixels of a near-cut triangle's pieces are
        written with the barycentrics of the UNCUT triangle, those of a wide triangle from 128-bit edge values, and
        nothing is unsupported once both flags are named.  stats: layouts.SURFACE_DRAWN_STATS (cut_pixels, wide_pixels).
        Neither flag: visibility_surface's kernels and bytes.  Byte-equal to
        orbit_amd.raster.host_visibility_surface_drawn.  Enqueued on `stream`."""
        flags = (_lib.RASTER_CLIP_NEAR if clip_near else 0) | (_lib.RASTER_WIDE_GUARD if wide_guard else 0)
        self.visibility_surface(*args, raster_flags=flags, **kwargs)

    # -- forward.frag's inputs per pixel of a visibility buffer and its surface (orbit_surface_fragments)
    def surface_fragments(self, visibility, width, height, draw_commands, max_commands, meshlets, meshlet_count, bary, triangle,
                          vertices, vertex_count, entity_data, entity_count, grad=None, world_pos=None, normal=None,
                          tangent=None, uv=None, uv_grad=None, material=None, stats=None, command_base=0, clear=False,
                          vertex_stride=32, position_offset=0, normal_offset=12, uv_offset=16, tangent_offset=24,
                          stream=None):
        """From the width x height u64 tensor `visibility`, the list that was rasterised into it with `command_base`, what
        visibility_surface[_drawn] left for that list (bary, triangle, and grad when uv_grad is wanted), the 32-B meshlet
        records and the vertex rows (the reference's MeshVertex by default: stride 32, position / snorm8 normal / uv /
        snorm8 tangent at 0 / 12 / 16 / 24) to the inputs of the reference's fragment shader for every pixel the list
        owns: world_pos (4 floats per pixel), normal (3, not renormalised), tangent (4), uv (2), uv_grad (4: du/dx, dv/dx,
        du/dy, dv/dy) and material (1 u32).  Each may be None, not all.  Uncovered pixels, pixels of another list and
        pixels the surface call left out (unshaded_pixels) are not written; clear=True (ORBIT_FRAGMENTS_CLEAR) fills the
        outputs first (0.0, 0xFFFFFFFF).  stats (32 bytes, layouts.SURFACE_FRAGMENT_STATS, cleared by the call).  A pixel
        whose triangle record does not fit the list is counted in stale_pixels and reported by status()
        (ORBIT_E_RANGE).  Byte-equal to orbit_amd.raster.host_surface_fragments.  Enqueued on `stream`."""
        j = _lib.SurfaceFragments()
        j.visibility, j.draw_commands, j.meshlets = _ptr(visibility), _ptr(draw_commands), _ptr(meshlets)
        j.bary, j.grad, j.triangle, j.vertices, j.entity_data = _ptr(bary), _ptr(grad), _ptr(triangle), _ptr(vertices), _ptr(entity_data)
        j.world_pos, j.normal, j.tangent, j.uv = _ptr(world_pos), _ptr(normal), _ptr(tangent), _ptr(uv)
        j.uv_grad, j.material, j.stats = _ptr(uv_grad), _ptr(material), _ptr(stats)
        j.vertex_count, j.meshlet_count, j.max_commands, j.entity_count = int(vertex_count), int(meshlet_count), int(max_commands), int(entity_count)
        j.vertex_stride, j.position_offset, j.normal_offset = int(vertex_stride), int(position_offset), int(normal_offset)
        j.uv_offset, j.tangent_offset, j.width, j.height = int(uv_offset), int(tangent_offset), int(width), int(height)
        j.flags, j.command_base = _lib.FRAGMENTS_CLEAR if clear else 0, int(command_base)
        _lib.check(self._lib.orbit_surface_fragments(self._ctx, C.byref(j), _stream(stream)), self._ctx)

    # -- forward.frag's clustered lighting per pixel of a visibility buffer (orbit_fragments_shade)
    def fragments_shade(self, visibility, width, height, world_pos, normal, material, materials, material_count, lights,
                        light_count, cluster_offset_image, light_index_buffer, index_capacity, cluster_count, tile_size_px,
                        z_scale, z_bias, luminance_cutoff, z_near, view_pos, color, lights_walked=None, stats=None,
                        render_mode=0, clear=False, form=None, stream=None):
        """From the width x height u64 tensor `visibility`, the planes surface_fragments left under clear=True (world_pos,
        normal, material), the 80-B material rows, the 64-B light rows and the cluster chain's light lists (the (offset,
        count) image and ClusterLightIndices with `index_capacity` indices behind its 4-byte header; cluster_count,
        tile_size_px, z_scale, z_bias and luminance_cutoff as in the cluster info buffer) to `color` (4 floats per pixel):
        the texture-free part of the reference's forward.frag, render_mode 0 (material factors, point and directional
        lights) or 8 (the light-count heat map).  lights_walked (1 u32 per pixel) and stats (32 bytes,
        layouts.SHADE_STATS, cleared by the call) may be None.  Uncovered pixels and pixels whose material is 0xFFFFFFFF
        are not written; clear=True (ORBIT_SHADE_CLEAR) fills color and lights_walked first.  A pixel whose material or
        light list does not fit the tables is counted in stale_pixels and reported by status() (ORBIT_E_RANGE).  form:
        None (the library chooses), "per_lane" or "staged" (tile_size_px % 8 == 0): equal bytes.  Byte-equal to
        orbit_amd.raster.host_fragments_shade.  Enqueued on `stream`."""
        j = _lib.FragmentsShade()
        j.visibility, j.world_pos, j.normal, j.material = _ptr(visibility), _ptr(world_pos), _ptr(normal), _ptr(material)
        j.materials, j.lights, j.cluster_offset_image = _ptr(materials), _ptr(lights), _ptr(cluster_offset_image)
        j.light_index_buffer, j.color, j.lights_walked, j.stats = _ptr(light_index_buffer), _ptr(color), _ptr(lights_walked), _ptr(stats)
        j.material_count, j.light_count, j.index_capacity = int(material_count), int(light_count), int(index_capacity)
        _lib.fill_fragments_shade(j, cluster_count, tile_size_px, z_scale, z_bias, luminance_cutoff, z_near, view_pos, render_mode,
                                  width, height, clear, form)
        _lib.check(self._lib.orbit_fragments_shade(self._ctx, C.byref(j), _stream(stream)), self._ctx)

    # -- the same with cascaded PCSS shadows served (orbit_fragments_shade_shadowed)
    def fragments_shade_shadowed(self, visibility, width, height, world_pos, normal, material, materials, material_count, lights,
                                 light_count, cluster_offset_image, light_index_buffer, index_capacity, cluster_count, tile_size_px,
                                 z_scale, z_bias, luminance_cutoff, z_near, view_pos, color, shadows, shadow_count, shadow_maps,
                                 shadow_map_count, shadow_resolution, blocker_search_radius, normal_bias_scale, oriented_bias,
                                 shadow_index_base=0, shadow_factor=None, cascade=None, shadow_stats=None, lights_walked=None,
                                 stats=None, render_mode=0, clear=False, form=None, stream=None):
        """fragments_shade with the reference's shadow term: a directional light whose shadow_data_index is not 0xFFFFFFFF
        takes row shadow_data_index - shadow_index_base of `shadows` (288-B rows, layouts.SHADOW_DATA) and is multiplied
        by forward.frag's cascaded PCSS factor, read from `shadow_maps`: shadow_map_count float32 maps of
        shadow_resolution^2 (reversed z, as raster_depth leaves them with clear=True; orbit_amd.raster.shadow_atlas draws
        them), which a row's shadow_map_indices index.  blocker_search_radius, normal_bias_scale, oriented_bias: the
        reference's ShadowSettings, oriented_bias as it sends it (negated).  shadow_factor (1 float per pixel), cascade (1
        u32 per pixel: 0..3, 4 = no cascade, 0xFFFFFFFF = no shadowed light) and shadow_stats (16 bytes,
        layouts.SHADOW_STATS) may be None; clear=True fills the two planes with 1.0 and 0xFFFFFFFF.  A shadow row or map
        index out of range makes the pixel stale (ORBIT_E_RANGE).  Byte-equal to
        orbit_amd.raster.host_fragments_shade_shadowed.  Enqueued on `stream`."""
        js = _lib.FragmentsShadeShadowed()
        j = js.shade
        j.visibility, j.world_pos, j.normal, j.material = _ptr(visibility), _ptr(world_pos), _ptr(normal), _ptr(material)
        j.materials, j.lights, j.cluster_offset_image = _ptr(materials), _ptr(lights), _ptr(cluster_offset_image)
        j.light_index_buffer, j.color, j.lights_walked, j.stats = _ptr(light_index_buffer), _ptr(color), _ptr(lights_walked), _ptr(stats)
        j.material_count, j.light_count, j.index_capacity = int(material_count), int(light_count), int(index_capacity)
        _lib.fill_fragments_shade(j, cluster_count, tile_size_px, z_scale, z_bias, luminance_cutoff, z_near, view_pos, render_mode,
                                  width, height, clear, form)
        js.shadows, js.shadow_maps, js.shadow_factor = _ptr(shadows), _ptr(shadow_maps), _ptr(shadow_factor)
        js.cascade, js.shadow_stats = _ptr(cascade), _ptr(shadow_stats)
        _lib.fill_shadow_fields(js, shadow_count, shadow_index_base, shadow_map_count, shadow_resolution, blocker_search_radius,
                                normal_bias_scale, oriented_bias)
        _lib.check(self._lib.orbit_fragments_shade_shadowed(self._ctx, C.byref(js), _stream(stream)), self._ctx)

    # -- the same with the sky light's term and the skybox served (orbit_fragments_shade_sky)
    def fragments_shade_sky(self, visibility, width, height, world_pos, normal, material, materials, material_count, lights,
                            light_count, cluster_offset_image, light_index_buffer, index_capacity, cluster_count, tile_size_px,
                            z_scale, z_bias, luminance_cutoff, z_near, view_pos, color, shadows, shadow_count, shadow_maps,
                            shadow_map_count, shadow_resolution, blocker_search_radius, normal_bias_scale, oriented_bias,
                            irradiance=None, irradiance_size=0, prefiltered=None, prefiltered_size=0, prefiltered_levels=0, brdf=None,
                            brdf_size=0, sky=None, sky_size=0, sky_levels=0, skybox_lod=0.0, basis=None, ao=None, sky_stats=None,
                            shadow_index_base=0, shadow_factor=None, cascade=None, shadow_stats=None, lights_walked=None,
                            stats=None, render_mode=0, clear=False, form=None, stream=None):
        """fragments_shade_shadowed with the reference's sky light and skybox.  The environment — irradiance (level 0 of a
        cube), prefiltered (prefiltered_levels levels) and brdf (the R16G16 table), as orbit_amd.env_map.device_env_map
        writes them, given together or not at all — serves every LIGHT_TYPE_SKY light of a pixel's walk
        (forward.frag:378-405); without it such a light is skipped and counted in unserved_pixels as before.  ao (1 float
        per pixel, orbit_ssao's ao_pixel, or None: 1.0) scales the sky term.  sky (sky_levels levels of a cube, or None)
        fills the pixels whose visibility word is 0 with the cube's colour along the ray of `basis` =
        orbit_amd.camera.skybox_basis(...) at the constant lod skybox_lod (render_mode 0 only).  sky_stats (32 bytes,
        layouts.SKY_STATS, cleared by the call) may be None.  With neither given the bytes are
        fragments_shade_shadowed's.  Byte-equal to orbit_amd.raster.host_fragments_shade_sky.  Enqueued on `stream`."""
        jk = _lib.FragmentsShadeSky()
        js = jk.shadowed
        j = js.shade
        j.visibility, j.world_pos, j.normal, j.material = _ptr(visibility), _ptr(world_pos), _ptr(normal), _ptr(material)
        j.materials, j.lights, j.cluster_offset_image = _ptr(materials), _ptr(lights), _ptr(cluster_offset_image)
        j.light_index_buffer, j.color, j.lights_walked, j.stats = _ptr(light_index_buffer), _ptr(color), _ptr(lights_walked), _ptr(stats)
        j.material_count, j.light_count, j.index_capacity = int(material_count), int(light_count), int(index_capacity)
        _lib.fill_fragments_shade(j, cluster_count, tile_size_px, z_scale, z_bias, luminance_cutoff, z_near, view_pos, render_mode,
                                  width, height, clear, form)
        js.shadows, js.shadow_maps, js.shadow_factor = _ptr(shadows), _ptr(shadow_maps), _ptr(shadow_factor)
        js.cascade, js.shadow_stats = _ptr(cascade), _ptr(shadow_stats)
        _lib.fill_shadow_fields(js, shadow_count, shadow_index_base, shadow_map_count, shadow_resolution, blocker_search_radius,
                                normal_bias_scale, oriented_bias)
        jk.irradiance, jk.prefiltered, jk.brdf, jk.sky = _ptr(irradiance), _ptr(prefiltered), _ptr(brdf), _ptr(sky)
        jk.ao, jk.sky_stats = _ptr(ao), _ptr(sky_stats)
        _lib.fill_sky_fields(jk, irradiance_size, prefiltered_size, prefiltered_levels, brdf_size, sky_size, sky_levels, skybox_lod, basis)
        _lib.check(self._lib.orbit_fragments_shade_sky(self._ctx, C.byref(jk), _stream(stream)), self._ctx)

    # -- the reference's bloom chain of a colour plane (orbit_bloom)
    def bloom(self, color, width, height, mips, threshold=0.0, soft_threshold=0.0, filter_radius=0.003, max_levels=6,
              stats=None, form=None, stream=None):
        """From `color` (4 floats per pixel, as the shade calls leave it) to `mips`: one packed B10G11R11 u32 per texel of
        the reference's bloom chain in orbit_amd.post.bloom_layout's layout (level 0 first, full size) — the 13-tap
        downsample with the Karis average and the soft threshold on level 0, then the 3 x 3 tent upsample, each level added
        into the one above.  Afterwards level 0 is the image post_process reads.  threshold, soft_threshold,
        filter_radius: the reference's BloomSettings (these are its defaults).  stats (16 bytes, layouts.BLOOM_STATS,
        cleared by the call) may be None.  form: None, "per_level" (the only launch form built, and the default) or
        "direct" (no LDS staging): equal bytes.  Byte-equal to orbit_amd.post.host_bloom.  Enqueued on `stream`."""
        j = _lib.Bloom()
        j.color, j.mips, j.stats = _ptr(color), _ptr(mips), _ptr(stats)
        _lib.fill_bloom(j, width, height, threshold, soft_threshold, filter_radius, max_levels, form)
        _lib.check(self._lib.orbit_bloom(self._ctx, C.byref(j), _stream(stream)), self._ctx)

    # -- the reference's tone mapping and sRGB encoding of a colour plane (orbit_post_process)
    def post_process(self, color, width, height, bloom=None, ldr=None, rgba8=None, exposure=1.0, bloom_intensity=0.025,
                     render_mode=0, bgra=False, stats=None, stream=None):
        """From `color` (4 floats per pixel) and, with render_mode 0, `bloom` (None, or level 0 of bloom's mips) to `ldr`
        (4 floats per pixel: the ACES fit of (color + bloom * bloom_intensity) * exposure, clamped, alpha 1) and / or
        `rgba8` (4 bytes per pixel: its sRGB encoding, R, G, B, A, or B, G, R, A with bgra=True); at least one of the
        two.  render_mode 8 ignores bloom.  stats (16 bytes, layouts.POST_STATS, cleared by the call) may be None.
        Byte-equal to orbit_amd.post.host_post_process.  Enqueued on `stream`."""
        j = _lib.PostProcess()
        j.color, j.bloom, j.ldr, j.rgba8, j.stats = _ptr(color), _ptr(bloom), _ptr(ldr), _ptr(rgba8), _ptr(stats)
        _lib.fill_post_process(j, width, height, exposure, bloom_intensity, render_mode, bgra)
        _lib.check(self._lib.orbit_post_process(self._ctx, C.byref(j), _stream(stream)), self._ctx)

    # -- the reference's SSAO of a depth plane, its blur and forward.frag's read of it (orbit_ssao)
    def ssao(self, depth, screen_w, screen_h, ssao_w, ssao_h, projection, inverse_projection, noise, noise_size, samples, samples_size,
             raw=None, blurred=None, ao_pixel=None, sample_count=32, min_radius=0.1, max_radius=0.5, stats=None, flags=0, stream=None):
        """From `depth` (screen_w * screen_h floats, reverse-z, 0 = uncovered: raster_depth's or visibility_resolve's) to
        `raw` (ssao_w * ssao_h bytes: ssao.comp's R8 image), `blurred` (the same size: ssao_blur.comp's, which the frame
        uses; needs raw) and `ao_pixel` (screen_w * screen_h floats: what forward.frag:336-337 samples per pixel; needs
        blurred).  ssao_w, ssao_h: the screen's or orbit_amd.post.ssao_resolution's halves.  projection, inverse_projection:
        the camera's, column-major.  noise (noise_size^2 int8 pairs) and samples (samples_size x 4 bytes): the reference's
        two tables (orbit_amd.post.ssao_tables).  sample_count, min_radius, max_radius: SsaoSettings (these are its
        defaults).  stats (24 bytes, layouts.SSAO_STATS, cleared by the call) may be None.  Byte-equal to
        orbit_amd.post.host_ssao.  Enqueued on `stream`."""
        j = _lib.Ssao()
        j.depth, j.noise, j.samples, j.raw, j.blurred, j.ao_pixel, j.stats = (_ptr(depth), _ptr(noise), _ptr(samples), _ptr(raw), _ptr(blurred),
                                                                               _ptr(ao_pixel), _ptr(stats))
        _lib.fill_ssao(j, projection, inverse_projection, screen_w, screen_h, ssao_w, ssao_h, noise_size, samples_size, sample_count, min_radius,
                       max_radius, flags)
        _lib.check(self._lib.orbit_ssao(self._ctx, C.byref(j), _stream(stream)), self._ctx)

    # -- cull statistics: what entity_cull + meshlet_cull with these arguments would do, counted (orbit_cull_stats)
    def cull_stats(self, stats, cull_info, entity_draw_buffer, mesh_info_buffer, meshlet_dispatch_buffer, entity_buffer,
                   entity_draw_count, dispatch_capacity, meshlet_buffer, draw_commands_buffer, material_buffer,
                   draw_capacity, visibility_buffer=None, meshlet_visibility_buffer=None, depth_pyramid=None,
                   depth_pyramid_size=(0, 0), material_count=0, depth_pyramid_levels=None, stream=None):
        """Enqueues orbit_cull_stats into `stats`, a device tensor of at least 256 bytes (8-B aligned) that is
        overwritten with an OrbitCullStats (read it with cull_stats_dict).  The arguments are entity_cull's and
        meshlet_cull's; call it BEFORE the cull they describe — passes 1 and 2 rewrite the visibility words it reads.
        Nothing but `stats` is written; the dispatch and draw buffers are only checked for presence."""
        if stats.numel() * stats.element_size() < layouts.CULL_STATS.itemsize:
            raise ValueError("stats needs 256 bytes")
        ci = _host_bytes(cull_info, 400)
        e, m = _lib.EntityCullBufs(), _lib.MeshletCullBufs()
        e.entity_draw_buffer = _ptr(entity_draw_buffer)
        e.mesh_info_buffer = _ptr(mesh_info_buffer)
        e.meshlet_dispatch_buffer = m.meshlet_dispatch_buffer = _ptr(meshlet_dispatch_buffer)
        e.entity_buffer = m.entity_buffer = _ptr(entity_buffer)
        e.visibility_buffer = _ptr(visibility_buffer)
        e.depth_pyramid = m.depth_pyramid = _ptr(depth_pyramid)
        e.depth_pyramid_size[0], e.depth_pyramid_size[1] = depth_pyramid_size
        m.depth_pyramid_size[0], m.depth_pyramid_size[1] = depth_pyramid_size
        e.depth_pyramid_levels = m.depth_pyramid_levels = _ptr(depth_pyramid_levels)
        e.dispatch_capacity = m.dispatch_capacity = dispatch_capacity
        m.meshlet_buffer = _ptr(meshlet_buffer)
        m.draw_commands_buffer = _ptr(draw_commands_buffer)
        m.material_buffer = _ptr(material_buffer)
        m.meshlet_visibility_buffer = _ptr(meshlet_visibility_buffer)
        m.draw_capacity = draw_capacity
        m.material_count = material_count
        _lib.check(self._lib.orbit_cull_stats(self._ctx, ci.ctypes.data_as(C.c_void_p), C.byref(e), int(entity_draw_count),
                                              C.byref(m), _ptr(stats), _stream(stream)), self._ctx)

    # -- several views side by side (orbit_cull_views)
    def cull_views(self, views, stream=None):
        """views: list of dicts with the arguments of entity_cull + meshlet_cull for one view each:
        cull_info, entity_draw_buffer, mesh_info_buffer, meshlet_dispatch_buffer, entity_buffer, entity_draw_count,
        dispatch_capacity, meshlet_buffer, draw_commands_buffer, material_buffer, draw_capacity and optionally
        visibility_buffer, meshlet_visibility_buffer, depth_pyramid, depth_pyramid_size, depth_pyramid_levels,
        material_count, skip_meshlet_stage."""
        arr, keep = self.prepare_views(views)
        self.cull_views_prepared(arr, stream)
        del keep

    def cull_views_prepared(self, arr, stream=None):
        """orbit_cull_views on a view array built once by prepare_views (per-frame callers keep it)."""
        _lib.check(self._lib.orbit_cull_views(self._ctx, arr, len(arr), _stream(stream)), self._ctx)

    @staticmethod
    def prepare_views(views):
        """-> (ctypes OrbitCullView array, objects that must outlive it)."""
        arr = (_lib.CullView * len(views))()
        keep = []
        for v, a in zip(views, arr):
            ci = _host_bytes(v["cull_info"], 400)
            keep.append(ci)
            a.cull_info = ci.ctypes.data
            e, m = a.entity, a.meshlet
            e.entity_draw_buffer = _ptr(v["entity_draw_buffer"])
            e.mesh_info_buffer = _ptr(v["mesh_info_buffer"])
            e.meshlet_dispatch_buffer = m.meshlet_dispatch_buffer = _ptr(v["meshlet_dispatch_buffer"])
            e.entity_buffer = m.entity_buffer = _ptr(v["entity_buffer"])
            e.visibility_buffer = _ptr(v.get("visibility_buffer"))
            e.depth_pyramid = m.depth_pyramid = _ptr(v.get("depth_pyramid"))
            ps = v.get("depth_pyramid_size", (0, 0))
            e.depth_pyramid_size[0], e.depth_pyramid_size[1] = ps
            m.depth_pyramid_size[0], m.depth_pyramid_size[1] = ps
            # DEVICE array of OrbitDepthPyramidLevel (separate per-mip images), or None for the packed chain
            e.depth_pyramid_levels = m.depth_pyramid_levels = _ptr(v.get("depth_pyramid_levels"))
            e.dispatch_capacity = m.dispatch_capacity = v["dispatch_capacity"]
            m.meshlet_buffer = _ptr(v.get("meshlet_buffer"))
            m.draw_commands_buffer = _ptr(v.get("draw_commands_buffer"))
            m.material_buffer = _ptr(v.get("material_buffer"))
            m.meshlet_visibility_buffer = _ptr(v.get("meshlet_visibility_buffer"))
            m.draw_capacity = v.get("draw_capacity", 0)
            m.material_count = v.get("material_count", 0)
            a.entity_draw_count = v["entity_draw_count"]
            a.skip_meshlet_stage = 1 if v.get("skip_meshlet_stage") else 0
        return arr, keep

    # -- meshlet_cull: create_meshlet_draw_commands body (draw_gen.rs:382-435)
    def meshlet_cull(self, cull_info, meshlet_dispatch_buffer, meshlet_buffer, draw_commands_buffer, entity_buffer,
                     material_buffer, dispatch_capacity, draw_capacity, meshlet_visibility_buffer=None,
                     depth_pyramid=None, depth_pyramid_size=(0, 0), material_count=0, stream=None, task_records=None,
                     depth_pyramid_levels=None, record_buffer=None, record_capacity=None):
        ci = _host_bytes(cull_info, 400)
        b = _lib.MeshletCullBufs()
        b.meshlet_dispatch_buffer = _ptr(meshlet_dispatch_buffer)
        b.meshlet_buffer = _ptr(meshlet_buffer)
        b.draw_commands_buffer = _ptr(draw_commands_buffer)
        b.entity_buffer = _ptr(entity_buffer)
        b.material_buffer = _ptr(material_buffer)
        b.meshlet_visibility_buffer = _ptr(meshlet_visibility_buffer)
        b.depth_pyramid = _ptr(depth_pyramid)
        b.depth_pyramid_size[0], b.depth_pyramid_size[1] = depth_pyramid_size
        b.dispatch_capacity = dispatch_capacity
        b.draw_capacity = draw_capacity
        b.material_count = material_count
        b.depth_pyramid_levels = _ptr(depth_pyramid_levels)
        if record_buffer is not None and record_capacity is not None:
            # sharded engine: the record list AND this rank's own commands (draw_commands_buffer / draw_capacity)
            _lib.check(self._lib.orbit_meshlet_cull_records_and_commands(
                self._ctx, ci.ctypes.data_as(C.c_void_p), C.byref(b), _ptr(record_buffer), record_capacity,
                _stream(stream)), self._ctx)
            return
        if record_buffer is not None:  # sharded engine: the visible list at record granularity (12 B per record)
            _lib.check(self._lib.orbit_meshlet_cull_visible_records(self._ctx, ci.ctypes.data_as(C.c_void_p), C.byref(b),
                                                                    _ptr(record_buffer), draw_capacity, _stream(stream)),
                       self._ctx)
            return
        if task_records is not None:
            _lib.check(self._lib.orbit_meshlet_task_cull(self._ctx, ci.ctypes.data_as(C.c_void_p), C.byref(b),
                                                         _ptr(task_records), _stream(stream)), self._ctx)
            return
        _lib.check(self._lib.orbit_meshlet_cull(self._ctx, ci.ctypes.data_as(C.c_void_p), C.byref(b),
                                                _stream(stream)), self._ctx)

    def meshlet_task_cull(self, cull_info, meshlet_dispatch_buffer, meshlet_buffer, task_records, entity_buffer,
                          material_buffer, dispatch_capacity, **kw):
        """Mesh-shading path (forward_depth_prepass.task): one 44-B OrbitMeshTaskRecord per dispatch record."""
        self.meshlet_cull(cull_info, meshlet_dispatch_buffer, meshlet_buffer, None, entity_buffer, material_buffer,
                          dispatch_capacity, 0, task_records=task_records, **kw)

    # -- DepthPyramid::update (draw_gen.rs:510-566)
    def depth_reduce(self, depth, screen_width, screen_height, pyramid, stream=None):
        _lib.check(self._lib.orbit_depth_reduce(self._ctx, _ptr(depth), screen_width, screen_height, _ptr(pyramid),
                                                _stream(stream)), self._ctx)

    def depth_reduce_multi(self, items, stream=None):
        """orbit_depth_reduce_multi (update_multiple_depth_pyramids::<C>, draw_gen.rs:569-628): one launch pair for up
        to 8 pyramids.  items: dicts with depth, width, height and either pyramid (packed chain) or levels (list of
        (tensor-or-pointer, row_pitch) per mip: separate per-mip images); optional depth_row_pitch."""
        arr, keep = self.prepare_depth_reduce_items(items)
        _lib.check(self._lib.orbit_depth_reduce_multi(self._ctx, arr, len(items), _stream(stream)), self._ctx)

    def prepare_depth_reduce_items(self, items):
        """-> (ctypes OrbitDepthReduceItem array, objects that must outlive it); items as for depth_reduce_multi."""
        arr = (_lib.DepthReduceItem * len(items))()
        keep = []
        for it, a in zip(items, arr):
            a.depth = _ptr(it["depth"])
            a.screen_width, a.screen_height = it["width"], it["height"]
            a.depth_row_pitch = it.get("depth_row_pitch", 0)
            a.pyramid = _ptr(it.get("pyramid"))
            if it.get("levels") is not None:
                lv = (_lib.DepthPyramidLevel * len(it["levels"]))()
                for l, (t, pitch) in zip(lv, it["levels"]):
                    l.texels, l.row_pitch = _ptr(t), pitch
                keep.append(lv)
                a.levels = lv
        return arr, keep

    def prepare_frame_late(self, pyramids=(), late_views=(), cascade_views=(), clusters=None):
        """orbit_frame_late's descriptor, built once (a per-frame caller keeps it): `pyramids` as for depth_reduce_multi,
        `late_views` / `cascade_views` as for cull_views, `clusters` a dict with compute_clusters' arguments (push, info,
        depth, lights, tile_depth_slice_mask, depth_bounds, unique_cluster_buffer, index_capacity, light_index_buffer,
        light_index_capacity, cluster_offset_image).  -> (descriptor, objects that must outlive it)."""
        f, keep = _lib.FrameLate(), []
        if pyramids:
            arr, k = self.prepare_depth_reduce_items(list(pyramids))
            f.pyramids, f.pyramid_count = arr, len(arr)
            keep += [arr, k]
        for name, views in (("late_views", late_views), ("cascade_views", cascade_views)):
            if views:
                arr, k = self.prepare_views(list(views))
                setattr(f, name, arr)
                setattr(f, name[:-1] + "_count", len(arr))
                keep += [arr, k]
        if clusters is not None:
            c = _lib.ClusterFrame()
            pc = _host_bytes(clusters["push"], layouts.MARK_ACTIVE_PUSH.itemsize).copy()
            ib = _host_bytes(clusters["info"], layouts.CLUSTER_CULL_INFO.itemsize).copy()
            c.push, c.info = pc.ctypes.data, ib.ctypes.data
            for k in ("depth", "lights", "tile_depth_slice_mask", "depth_bounds", "unique_cluster_buffer",
                      "light_index_buffer", "cluster_offset_image"):
                setattr(c, k, _ptr(clusters.get(k)))
            c.index_capacity, c.light_index_capacity = clusters["index_capacity"], clusters["light_index_capacity"]
            f.clusters = C.pointer(c)
            keep += [c, pc, ib]
        return f, keep

    def frame_late(self, frame, stream=None):
        """orbit_frame_late on a descriptor of prepare_frame_late: {pyramids -> late culls} || {cascade culls} ||
        {compute_clusters}, forked behind `stream` and joined into it."""
        _lib.check(self._lib.orbit_frame_late(self._ctx, C.byref(frame), _stream(stream)), self._ctx)

    def meshlet_cull_visible_records(self, cull_info, meshlet_dispatch_buffer, meshlet_buffer, record_buffer,
                                     entity_buffer, material_buffer, dispatch_capacity, record_capacity, **kw):
        """orbit_meshlet_cull_visible_records: {records, survivors} + 12-B {entity_index, meshlet_offset, mask} per
        dispatch record, in record order (mask 0: no survivor), written by the evaluation launch itself."""
        self.meshlet_cull(cull_info, meshlet_dispatch_buffer, meshlet_buffer, None, entity_buffer, material_buffer,
                          dispatch_capacity, record_capacity, record_buffer=record_buffer, **kw)

    def meshlet_cull_records_and_commands(self, cull_info, meshlet_dispatch_buffer, meshlet_buffer, record_buffer,
                                          draw_commands_buffer, entity_buffer, material_buffer, dispatch_capacity,
                                          record_capacity, draw_capacity, **kw):
        """orbit_meshlet_cull_records_and_commands: one evaluation, the 12-B record list and the 28-B commands."""
        self.meshlet_cull(cull_info, meshlet_dispatch_buffer, meshlet_buffer, draw_commands_buffer, entity_buffer,
                          material_buffer, dispatch_capacity, draw_capacity, record_buffer=record_buffer,
                          record_capacity=record_capacity, **kw)

    def cull_shard(self, cull_info, entity_draw_buffer, mesh_info_buffer, meshlet_dispatch_buffer, entity_buffer,
                   draw_first, draw_count, dispatch_capacity, meshlet_buffer, material_buffer, record_buffer,
                   record_capacity, draw_commands_buffer=None, draw_capacity=0, material_count=0,
                   visibility_buffer=None, meshlet_visibility_buffer=None, depth_pyramid=None,
                   depth_pyramid_size=(0, 0), stream=None):
        """orbit_cull_shard: a rank's whole cull — entity range, meshlet stage, record list (and, with
        draw_commands_buffer, the rank's own 28-B commands) — as one call; one launch (+ the emit) for pass 0 and up to
        65 536 entity-draws."""
        ci = _host_bytes(cull_info, 400)
        e, m = _lib.EntityCullBufs(), _lib.MeshletCullBufs()
        e.entity_draw_buffer = _ptr(entity_draw_buffer)
        e.mesh_info_buffer = _ptr(mesh_info_buffer)
        e.meshlet_dispatch_buffer = m.meshlet_dispatch_buffer = _ptr(meshlet_dispatch_buffer)
        e.entity_buffer = m.entity_buffer = _ptr(entity_buffer)
        e.visibility_buffer = _ptr(visibility_buffer)
        e.depth_pyramid = m.depth_pyramid = _ptr(depth_pyramid)
        e.depth_pyramid_size[0], e.depth_pyramid_size[1] = depth_pyramid_size
        m.depth_pyramid_size[0], m.depth_pyramid_size[1] = depth_pyramid_size
        e.dispatch_capacity = m.dispatch_capacity = dispatch_capacity
        m.meshlet_buffer = _ptr(meshlet_buffer)
        m.draw_commands_buffer = _ptr(draw_commands_buffer)
        m.material_buffer = _ptr(material_buffer)
        m.meshlet_visibility_buffer = _ptr(meshlet_visibility_buffer)
        m.draw_capacity = draw_capacity
        m.material_count = material_count
        _lib.check(self._lib.orbit_cull_shard(self._ctx, ci.ctypes.data_as(C.c_void_p), C.byref(e), draw_first, draw_count,
                                              C.byref(m), _ptr(record_buffer), record_capacity,
                                              1 if draw_commands_buffer is not None else 0, _stream(stream)), self._ctx)

    def prepare_cull_shard(self, cull_info, entity_draw_buffer, mesh_info_buffer, meshlet_dispatch_buffer, entity_buffer,
                           draw_first, draw_count, dispatch_capacity, meshlet_buffer, material_buffer, record_buffer,
                           record_capacity, draw_commands_buffer=None, draw_capacity=0, material_count=0,
                           visibility_buffer=None, meshlet_visibility_buffer=None, depth_pyramid=None,
                           depth_pyramid_size=(0, 0), stream=None):
        """cull_shard with its argument blocks built ONCE: returns a PreparedShardCull — calling it enqueues the shard
        cull on `stream` (a per-frame caller whose buffers do not change — bench.py's step loop — spends its host time in
        the library, not in filling ctypes structs: ~10 us per call).  The 400-B CullInfo is the object's own copy:
        write the next frame's into `prepared.cull_info` (a uint8[400] numpy view, `prepared.set_cull_info(ci)`) before
        the call.  `stream` is part of what is prepared and must be given (the stream current at prepare time is not
        the stream current at call time)."""
        if stream is None:
            raise ValueError("prepare_cull_shard: pass the stream the prepared call enqueues on")
        return PreparedShardCull(self, cull_info, entity_draw_buffer, mesh_info_buffer, meshlet_dispatch_buffer, entity_buffer,
                                 draw_first, draw_count, dispatch_capacity, meshlet_buffer, material_buffer, record_buffer,
                                 record_capacity, draw_commands_buffer, draw_capacity, material_count, visibility_buffer,
                                 meshlet_visibility_buffer, depth_pyramid, depth_pyramid_size, stream)

    def mesh_side_culls(self):
        """orbit_ctx_mesh_side_culls: entity culls of the bound stream that were handed its mesh side table."""
        return int(self._lib.orbit_ctx_mesh_side_culls(self._ctx))

    def shard_culls(self):
        """orbit_ctx_shard_culls: orbit_cull_shard calls of this context that took the one launch."""
        return int(self._lib.orbit_ctx_shard_culls(self._ctx))

    def expand_visible_records(self, record_buffer, meshlet_buffer, draw_commands_buffer, draw_capacity, stream=None):
        """orbit_expand_visible_records: record list -> MeshletDrawCommandBuffer, in list order."""
        _lib.check(self._lib.orbit_expand_visible_records(self._ctx, _ptr(record_buffer), _ptr(meshlet_buffer),
                                                          _ptr(draw_commands_buffer), draw_capacity, _stream(stream)),
                   self._ctx)

    # -- exchange without a host in the step (orbit_p2p_* / orbit_exchange_list)
    def p2p_alloc(self, nbytes):
        """(device pointer, 64-byte IPC handle) of an exchange buffer peers can map."""
        ptr, handle = C.c_void_p(), (C.c_uint8 * 64)()
        _lib.check(self._lib.orbit_p2p_alloc(self._ctx, int(nbytes), C.byref(ptr), handle), self._ctx)
        return int(ptr.value), bytes(handle)

    def p2p_free(self, ptr):
        _lib.check(self._lib.orbit_p2p_free(self._ctx, C.c_void_p(ptr)), self._ctx)

    def p2p_open(self, handle):
        ptr, h = C.c_void_p(), (C.c_uint8 * 64).from_buffer_copy(handle)
        _lib.check(self._lib.orbit_p2p_open(self._ctx, h, C.byref(ptr)), self._ctx)
        return int(ptr.value)

    def p2p_close(self, ptr):
        _lib.check(self._lib.orbit_p2p_close(self._ctx, C.c_void_p(ptr)), self._ctx)

    def meshlet_stream(self, meshlet_buffer, first, count, stream=None):
        """orbit_meshlet_stream_create + _update: the derived streams of meshlets [first, first + count) of
        `meshlet_buffer` (a device pointer / tensor indexed by GLOBAL meshlet index, like bufs.meshlet_buffer).
        Bind the result with bind_meshlet_stream; call .update() after writing meshlets."""
        return MeshletStream(self, meshlet_buffer, first, count, stream)

    def bind_meshlet_stream(self, ms):
        """orbit_ctx_bind_meshlet_stream (None unbinds).  The engine keeps the stream object alive."""
        _lib.check(self._lib.orbit_ctx_bind_meshlet_stream(self._ctx, ms._h if ms is not None else None), self._ctx)
        self._meshlet_stream = ms

    def fused_culls(self):
        """Views this context has culled through the one-launch path of orbit_cull_views (include/orbit_abi.h)."""
        return int(self._lib.orbit_ctx_fused_culls(self._ctx))

    def meshlet_stream_culls(self):
        """orbit_ctx_meshlet_stream_culls: meshlet culls launched from a bound stream so far."""
        return int(self._lib.orbit_ctx_meshlet_stream_culls(self._ctx))

    def meshlet_class_culls(self):
        """orbit_ctx_meshlet_class_culls: ... of which evaluated from the stream's alpha classes."""
        return int(self._lib.orbit_ctx_meshlet_class_culls(self._ctx))

    def block_culls(self):
        """orbit_ctx_block_culls: ... of which decided per block of 32 meshlets (pass 0; include/orbit_abi_ext.h)."""
        return int(self._lib.orbit_ctx_block_culls(self._ctx))

    def set_block_cull(self, enable):
        """orbit_ctx_set_block_cull: False keeps the per-meshlet evaluation for pass 0 (same outputs either way)."""
        _lib.check(self._lib.orbit_ctx_set_block_cull(self._ctx, 1 if enable else 0), self._ctx)

    def set_block_cull_grid(self, max_workgroups):
        """orbit_ctx_set_block_cull_grid: at most that many workgroups for the per-block evaluation (0 = as sized; tests)."""
        _lib.check(self._lib.orbit_ctx_set_block_cull_grid(self._ctx, int(max_workgroups)), self._ctx)

    def set_raster_grid(self, max_workgroups):
        """orbit_ctx_set_raster_grid: at most that many workgroups for every raster launch and its clear (0 = the resident
        grid; tests)."""
        _lib.check(self._lib.orbit_ctx_set_raster_grid(self._ctx, int(max_workgroups)), self._ctx)

    def set_fused_grid(self, max_workgroups):
        """orbit_ctx_set_fused_grid: at most that many workgroups per view for every launch of the one-launch cull behind
        cull_views, read when the launch is enqueued (0 = as sized; tests)."""
        _lib.check(self._lib.orbit_ctx_set_fused_grid(self._ctx, int(max_workgroups)), self._ctx)

    def set_visibility_grid(self, max_workgroups):
        """orbit_ctx_set_visibility_grid: at most that many workgroups for the strided launches of visibility_resolve,
        visibility_compact (clear and mark), visibility_surface, surface_fragments, fragments_shade and
        fragments_shade_shadowed, and for post_process' pass over the pixels, read when the call is
        enqueued (0 = num_cus * 8; tests)."""
        _lib.check(self._lib.orbit_ctx_set_visibility_grid(self._ctx, int(max_workgroups)), self._ctx)

    def exchange_list(self, local_list, rank, world, out_buffers, ctrl_buffers, out_capacity, header_bytes, stride,
                      stream=None):
        """orbit_exchange_list: the rank-ordered all-gather of the ranks' lists with counts and completion signalled on
        the device (no collective, no host round trip; capturable).  `out_buffers` / `ctrl_buffers`: lists of device
        pointers (ints or tensors), rank r's output buffer / control block as mapped in this process."""
        outs = (C.c_void_p * world)(*[_ptr(b) for b in out_buffers])
        ctrls = (C.c_void_p * world)(*[_ptr(b) for b in ctrl_buffers])
        _lib.check(self._lib.orbit_exchange_list(self._ctx, _ptr(local_list), rank, world, outs, ctrls, out_capacity,
                                                 header_bytes, stride, _stream(stream)), self._ctx)

    def prepare_exchange_list(self, local_list, rank, world, out_buffers, ctrl_buffers, out_capacity, header_bytes, stride,
                              stream=None):
        """exchange_list with its pointer arrays built once: returns a function of no arguments (see prepare_cull_shard)."""
        outs = (C.c_void_p * world)(*[_ptr(b) for b in out_buffers])
        ctrls = (C.c_void_p * world)(*[_ptr(b) for b in ctrl_buffers])
        fn, ctx, lst, st = self._lib.orbit_exchange_list, self._ctx, _ptr(local_list), _stream(stream)
        keep = (outs, ctrls, local_list, stream)

        def call():
            rc = fn(ctx, lst, rank, world, outs, ctrls, out_capacity, header_bytes, stride, st)
            if rc != _lib.OK:
                _lib.check(rc, ctx)
            return keep

        return call

    def allgather_list(self, nccl_comm, rank, world, local_list, segment_capacity, segments, out_list, out_capacity,
                       header_bytes, stride, stream=None):
        """orbit_allgather_list: ONE ncclAllGather of the ranks' fixed-capacity list segments + the compaction launch; no
        count is read back, no stream is synchronised (`nccl_comm`: the ncclComm_t as an integer / c_void_p)."""
        comm = nccl_comm if isinstance(nccl_comm, C.c_void_p) else C.c_void_p(int(nccl_comm))
        _lib.check(self._lib.orbit_allgather_list(self._ctx, comm, rank, world, _ptr(local_list), segment_capacity,
                                                  _ptr(segments), _ptr(out_list), out_capacity, header_bytes, stride,
                                                  _stream(stream)), self._ctx)

    def compact_segments(self, segments, world, segment_capacity, out_list, out_capacity, header_bytes, stride,
                         stream=None):
        """orbit_compact_segments: `world` gathered segments {count | header | segment_capacity items} -> the contiguous
        rank-ordered list {total | header | items}."""
        _lib.check(self._lib.orbit_compact_segments(self._ctx, _ptr(segments), world, segment_capacity, _ptr(out_list),
                                                    out_capacity, header_bytes, stride, _stream(stream)), self._ctx)

    def gather_visible(self, nccl_comm, rank, world, local_draw_buffer, out_draw_buffer, out_capacity, stream=None):
        """Rank-ordered all-gather of the visible lists over the caller's RCCL communicator
        (`nccl_comm`: the ncclComm_t as an integer / c_void_p).  One stream sync (message sizes)."""
        comm = nccl_comm if isinstance(nccl_comm, C.c_void_p) else C.c_void_p(int(nccl_comm))
        _lib.check(self._lib.orbit_gather_visible(self._ctx, comm, rank, world, _ptr(local_draw_buffer),
                                                  _ptr(out_draw_buffer), out_capacity, _stream(stream)), self._ctx)

    def compute_clusters(self, push, info, depth, lights, tile_depth_slice_mask, depth_bounds, unique_cluster_buffer,
                         index_capacity, light_index_buffer, light_index_capacity, cluster_offset_image, stream=None):
        """compute_clusters (cluster.rs:368-397): mark -> compact -> assign in one call."""
        pc = _host_bytes(push, layouts.MARK_ACTIVE_PUSH.itemsize)
        ib = _host_bytes(info, layouts.CLUSTER_CULL_INFO.itemsize)
        _lib.check(self._lib.orbit_compute_clusters(
            self._ctx, pc.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p), _ptr(depth), _ptr(lights),
            _ptr(tile_depth_slice_mask), _ptr(depth_bounds), _ptr(unique_cluster_buffer), index_capacity,
            _ptr(light_index_buffer), light_index_capacity, _ptr(cluster_offset_image), _stream(stream)), self._ctx)

    # -- cluster statistics: the uncapped counts of compute_clusters for these inputs (orbit_cluster_stats)
    def cluster_stats(self, stats, push, info, depth, lights, stream=None):
        """Enqueues orbit_cluster_stats into `stats`, a device tensor of at least 256 bytes (8-B aligned) that is
        overwritten with an OrbitClusterStats (read it with cluster_stats_dict).  The arguments are compute_clusters'
        inputs; nothing but `stats` is written, so it may come before, after or beside the chain."""
        if stats.numel() * stats.element_size() < layouts.CLUSTER_STATS.itemsize:
            raise ValueError("stats needs 256 bytes")
        pc = _host_bytes(push, layouts.MARK_ACTIVE_PUSH.itemsize)
        ib = _host_bytes(info, layouts.CLUSTER_CULL_INFO.itemsize)
        _lib.check(self._lib.orbit_cluster_stats(self._ctx, pc.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p),
                                                 _ptr(depth), _ptr(lights), _ptr(stats), _stream(stream)), self._ctx)

    # -- compute_clusters stages (cluster.rs:399-591)
    def cluster_mark(self, push, depth, tile_depth_slice_mask, depth_bounds, stream=None):
        pc = _host_bytes(push, layouts.MARK_ACTIVE_PUSH.itemsize)
        _lib.check(self._lib.orbit_cluster_mark(self._ctx, pc.ctypes.data_as(C.c_void_p), _ptr(depth),
                                                _ptr(tile_depth_slice_mask), _ptr(depth_bounds), _stream(stream)),
                   self._ctx)

    def cluster_compact(self, cluster_count, tile_depth_slice_mask, unique_cluster_buffer, index_capacity,
                        stream=None):
        cc = (C.c_uint32 * 3)(*[int(v) for v in cluster_count])
        _lib.check(self._lib.orbit_cluster_compact(self._ctx, C.byref(cc), _ptr(tile_depth_slice_mask),
                                                   _ptr(unique_cluster_buffer), index_capacity, _stream(stream)),
                   self._ctx)

    def cluster_assign(self, info, unique_cluster_buffer, depth_bounds, lights, light_index_buffer,
                       light_index_capacity, cluster_offset_image, stream=None):
        ib = _host_bytes(info, layouts.CLUSTER_CULL_INFO.itemsize)
        _lib.check(self._lib.orbit_cluster_assign(self._ctx, ib.ctypes.data_as(C.c_void_p),
                                                  _ptr(unique_cluster_buffer), _ptr(depth_bounds), _ptr(lights),
                                                  _ptr(light_index_buffer), light_index_capacity,
                                                  _ptr(cluster_offset_image), _stream(stream)), self._ctx)
