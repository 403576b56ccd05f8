"""ctypes binding of the asset side of ``liborbit_host.so`` (``orbit_amd/host/orbit_assets.hpp``): a triangle mesh ->
the 32-byte Meshlet records and the packed meshlet data of ``assets::mesh::compute_meshlets``
(src/assets/mesh.rs:292-338), with meshoptimizer's cluster-bounds algorithm restated, and the mesh-level bounds of
``gltf_loader.rs:480-506``.  Python adds nothing; host only."""
import ctypes as C

import numpy as np

from . import layouts as L
from .passes import _check, lib

MAX_MESHLET_VERTICES = 64   # mesh.rs:8
MAX_MESHLET_TRIANGLES = 64  # mesh.rs:9


def compute_meshlets(positions, indices, material=0, vertex_offset=0, data_offset_base=0):
    """-> (meshlets: np[layouts.MESHLET], meshlet_data: np.uint32).  `data_offset_base` = words of meshlet data already
    in the scene-wide buffer (the meshlets' data_offset continue from there)."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    h = lib()
    n_m, n_w = C.c_uint64(), C.c_uint64()
    args = (pos.ctypes.data_as(C.c_void_p), C.c_uint64(len(pos)), idx.ctypes.data_as(C.c_void_p), C.c_uint64(len(idx)),
            C.c_uint32(material), C.c_uint32(vertex_offset), C.c_uint32(data_offset_base))
    _check(h.orbit_host_compute_meshlets(*args, None, None, C.byref(n_m), C.byref(n_w)))
    meshlets = np.zeros(n_m.value, dtype=L.MESHLET)
    data = np.zeros(max(n_w.value, 1), dtype=np.uint32)
    _check(h.orbit_host_compute_meshlets(*args, meshlets.ctypes.data_as(C.c_void_p), data.ctypes.data_as(C.c_void_p),
                                         C.byref(n_m), C.byref(n_w)))
    return meshlets, data[:n_w.value]


def compute_mesh_bounds(positions):
    """-> (aabb_min[3], aabb_max[3], bounding_sphere[4]) as in gltf_loader.rs:480-506."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    mn, mx, sp = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 4)()
    lib().orbit_host_compute_mesh_bounds(pos.ctypes.data_as(C.c_void_p), C.c_uint64(len(pos)), mn, mx, sp)
    return np.array(mn, np.float32), np.array(mx, np.float32), np.array(sp, np.float32)


def meshlet_bounds(meshlets, meshlet_data, vertices, vertex_count, vertex_stride=12, position_offset=0, first=0,
                   count=None, indices=None):
    """The host reference of Engine.meshlet_bounds on host copies of the same buffers (orbit_host_meshlet_bounds: the
    records decoded as the device decodes them, then the mirror's compute_meshlet_bounds) ->
    (full: np[layouts.MESHLET_BOUNDS_FULL] per selected meshlet, range_error: np.int32 flags, updates: np.uint32 growth
    updates of the meshlet's two Ritter spheres).  `vertices`: any contiguous array, read as bytes; the records are not
    written.  A failed range check leaves a zero row."""
    rec = np.ascontiguousarray(meshlets).view(np.uint8).reshape(-1)
    data = np.ascontiguousarray(meshlet_data, dtype=np.uint32).reshape(-1)
    vb = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1)
    if int(vertex_count) and (int(vertex_count) - 1) * int(vertex_stride) + int(position_offset) + 12 > vb.nbytes:
        raise ValueError("vertex_count reaches beyond the vertex array")
    idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    capacity = rec.nbytes // 32
    if count is None:
        count = len(idx) if idx is not None else capacity - first
    full = np.zeros(count, dtype=L.MESHLET_BOUNDS_FULL)
    err, upd = np.zeros(count, np.int32), np.zeros(count, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _check(lib().orbit_host_meshlet_bounds(p(rec), C.c_uint64(capacity), p(idx), C.c_uint64(first), C.c_uint64(count),
                                           p(data), C.c_uint64(len(data)), p(vb), C.c_uint64(vertex_count),
                                           C.c_uint32(vertex_stride), C.c_uint32(position_offset), p(full), p(err), p(upd)))
    return full, err, upd


def meshlet_triangles(meshlet, meshlet_data):
    """The global vertex indices (n_tri, 3) of one meshlet, decoded the way the mesh / vertex shaders read them:
    vertices at data_offset, u8 corners from byte (data_offset + vertex_count) * 4 — the cmd_first_index of the draw
    command the cull path emits (meshlet_cull.comp:216-230)."""
    d0, nv, nt = int(meshlet["data_offset"]), int(meshlet["vertex_count"]), int(meshlet["triangle_count"])
    verts = meshlet_data[d0:d0 + nv]
    corners = meshlet_data.view(np.uint8)[(d0 + nv) * 4:(d0 + nv) * 4 + 3 * nt].reshape(nt, 3)
    return verts[corners]


def pack_snorm8(values):
    """pack_f32_to_snorm_u8 (math.rs:201-203) of an array: clamp to [-1, 1], times 127 in float32, truncated toward zero;
    NaN -> 0 (Rust's `as i8`)."""
    f = np.asarray(values, dtype=np.float32)
    scaled = np.clip(f, np.float32(-1.0), np.float32(1.0)) * np.float32(127.0)
    return np.where(np.isnan(f), np.float32(0.0), np.trunc(scaled)).astype(np.int8)


def pack_mesh_vertices(positions, normals, uvs, tangents):
    """GpuMeshVertex::new (assets/mesh.rs:23-31) of n vertices -> np[layouts.MESH_VERTEX] rows of 32 B: positions (n, 3)
    and uvs (n, 2) as float32, normals (n, 3) and tangents (n, 4) through pack_snorm8; the normal's fourth byte and the
    padding are 0.  What orbit_surface_fragments reads with vertex_stride 32 and offsets 0 / 12 / 16 / 24."""
    pos = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    n = len(pos)
    out = np.zeros(n, L.MESH_VERTEX)
    out["position"] = pos
    out["normal"][:, :3] = pack_snorm8(np.asarray(normals, dtype=np.float32).reshape(n, 3))
    out["uv"] = np.asarray(uvs, dtype=np.float32).reshape(n, 2)
    out["tangent"] = pack_snorm8(np.asarray(tangents, dtype=np.float32).reshape(n, 4))
    return out
