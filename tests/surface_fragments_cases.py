"""Inputs for orbit_surface_fragments (include/orbit_abi_ext.h F1-F8).  As in its neighbours, the expected bytes are never
computed here: the GPU tests' reference is the host mirror (orbit_amd.raster.host_surface_fragments), which
tests/test_surface_fragments_cpu.py holds to the numpy restatement tests/surface_fragments_ref.py.  A case takes a buffer,
a list and the surface outputs of a case of visibility_surface_cases / surface_drawn_cases (the mirror's surface call with
the case's flags and ORBIT_SURFACE_CLEAR, so what it left out holds 0xFFFFFFFF) and adds what only this call reads:
  vertices   the case's positions as the reference's 32-B MeshVertex rows (assets.pack_mesh_vertices) with seeded normals,
             uvs and tangents; the buffer ENDS with the last row's tangent (28 of its 32 bytes)
  meshlets   one 32-B record per command (the packing gives command k meshlet_index k) with material 7 + 3 k and seeded
             junk elsewhere; the buffer ENDS with the last record's material_index (30 of its 32 bytes)
  entities   the case's model matrices with a seeded, asymmetric normal matrix whose fourth row and column are 1e30
Census: visibility_surface_cases' rasterised, hand and clip cases (read without flags: the cut triangles' pixels are
unshaded), surface_drawn_cases' clip, wide and hand
cases (read with the flags they were drawn with).
Shapes (whole_WxH: one triangle over the target; tile_of_64: an 8 x 8 tile whose 64 pixels hold 64 triangles of 64 commands,
4 entities with models of their own and 64 materials):
  whole_1x1, whole_7x3 (less than a tile), whole_8x8, whole_9x9 (four tiles, three partial), whole_65x8 (nine tiles in a row)
  tile_of_64_65x9
Tampered (`tamper(case, ...)`: everything else as in the clean case), see test_surface_fragments_cpu.py."""
from dataclasses import dataclass, field

import numpy as np

import surface_drawn_cases as dc
import visibility_surface_cases as sc
from orbit_amd import assets, raster
from orbit_amd import layouts as L
from raster_cases import Case, poly, tri

F = np.float32
SHAPES = ((1, 1), (7, 3), (8, 8), (9, 9), (65, 8))
VERTEX_END, MESHLET_END = 28, 30  # the last row's bytes that are read
MAX_PIXELS = 256 * 144  # the census' full_target_1920x1080 is left out: a lane's work does not depend on the target's size


def attributes(n, seed):
    """seeded normals (n, 3), uvs (n, 2), tangents (n, 4): directions of any length up to a bit over 1 (the packing
    clamps), uvs up to a few hundred"""
    rng = np.random.default_rng(seed)
    normals = rng.uniform(-1.1, 1.1, (n, 3)).astype(F)
    uvs = (rng.uniform(-4.0, 4.0, (n, 2)) * rng.choice([1.0, 100.0], (n, 1))).astype(F)
    tangents = rng.uniform(-1.1, 1.1, (n, 4)).astype(F)
    tangents[:, 3] = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return normals, uvs, tangents


def vertex_rows(positions, seed=11):
    """-> the uint8 bytes of pack_mesh_vertices, cut behind the last tangent"""
    pos = np.asarray(positions, F).reshape(-1, 3)
    rows = assets.pack_mesh_vertices(pos, *attributes(len(pos), seed))
    return rows.view(np.uint8).reshape(-1)[:len(pos) * 32 - (32 - VERTEX_END)].copy()


def meshlet_records(n, seed=13):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (max(n, 1), 32), dtype=np.uint8)
    rec = raw.view(L.MESHLET).reshape(-1).copy()
    rec["material_index"] = 7 + 3 * np.arange(len(rec))
    return rec.view(np.uint8).reshape(-1)[:len(rec) * 32 - (32 - MESHLET_END)].copy(), len(rec)


def with_normal_matrices(entities, seed=17):
    rng = np.random.default_rng(seed)
    out = np.array(entities, dtype=L.ENTITY_DATA).reshape(-1)
    for e in out:
        m = np.full((4, 4), 1e30, F)
        m[:3, :3] = rng.uniform(-2.0, 2.0, (3, 3))
        e["normal_matrix"] = m.reshape(16)
    return out


@dataclass
class FragCase:
    name: str
    visibility: np.ndarray
    words: np.ndarray
    max_commands: int
    meshlets: np.ndarray      # bytes
    surface: dict             # bary, grad, triangle
    vertices: np.ndarray      # bytes, stride 32
    vertex_count: int
    entities: np.ndarray
    kw: dict = field(default_factory=dict)  # command_base, entity_count, meshlet_count
    source: object = None     # the surface case
    stale: int = 0            # tampered: the pixels that must be stale, nothing else changed
    clean: object = None

    def args(self, **over):
        """-> (args, kwargs) of raster.host_surface_fragments and surface_fragments_ref.fragments"""
        return (self.visibility, self.words, self.max_commands, self.meshlets, self.surface, self.vertices, self.vertex_count,
                self.entities), dict(self.kw, **over)


def of(case, surface_over=None):
    """A SurfaceCase / DrawnCase -> FragCase"""
    (vis, words, mc, data, vb, vcount, ent, vp), kw = case.args()
    flags = kw.pop("raster_flags", 0)
    surf = raster.host_visibility_surface_drawn(vis, words, mc, data, vb, vcount, ent, vp, raster_flags=flags if surface_over is None else surface_over,
                                                clear=True, **kw)
    stride, offset = kw["vertex_stride"], kw["position_offset"]
    rows = np.ascontiguousarray(vb).view(np.uint8).reshape(-1)
    pos = np.stack([rows[g * stride + offset:g * stride + offset + 12].view(F) for g in range(vcount)]) if vcount else np.zeros((0, 3), F)
    meshlets, n_meshlets = meshlet_records(len(case.packed.commands))
    return FragCase(case.name, vis, np.ascontiguousarray(words), mc, meshlets, {k: surf[k] for k in ("bary", "grad", "triangle", "stats")},
                    vertex_rows(pos), vcount, with_normal_matrices(ent),
                    dict(command_base=kw["command_base"], entity_count=kw["entity_count"], meshlet_count=n_meshlets), source=case)


def entity_model(e):
    """scale 2^e and a translation: asymmetric, every product exact"""
    m = np.zeros(16, F)
    m[0] = m[5] = F(2.0) ** e
    m[10], m[15], m[12], m[13] = 1, 1, F(3 * e + 1), F(-2 * e)
    return m


def tile_of_64():
    meshlets = []
    for q in range(64):
        e = q % 4
        s, tx, ty = 2.0 ** e, 3 * e + 1, -2 * e
        corners = [((x - tx) / s, (y - ty) / s, z) for x, y, z in sc.pixel_triangle(8 + q % 8, q // 8)]
        m = poly([tuple(corners)])
        m.entity = e
        meshlets.append(m)
    return Case("tile_of_64_65x9", meshlets, width=65, height=9, entities=[entity_model(e) for e in range(4)])


def shape_cases():
    out = [of(sc.drawn(Case(f"whole_{w}x{h}", [tri((-1, -1), (-1, 3 * h + 2), (3 * w + 2, -1), z=0.75)], width=w, height=h))) for w, h in SHAPES]
    out.append(of(sc.drawn(tile_of_64())))
    return out


def census():
    flat = [of(c) for c in sc.rasterised_cases() + sc.hand_cases() + sc.clip_cases() if c.visibility.size <= MAX_PIXELS]
    drawn = [of(c) for c in dc.clip_cases() + dc.wide_cases() + dc.hand_cases()]
    return flat + drawn


def both_flag_cases():
    """the clip and wide cases drawn with both flags where the case allows it and read with both"""
    return [c for c in census() if getattr(c.source, "raster_flags", 0) == dc.BOTH]


def tamper(case, name, stale, **fields):
    """`case` with the named fields replaced (surface: a dict of replaced outputs)"""
    new = FragCase(name, case.visibility, case.words, case.max_commands, case.meshlets, dict(case.surface), case.vertices, case.vertex_count,
                   case.entities, dict(case.kw), source=case.source, stale=stale, clean=case)
    for k, v in fields.items():
        if k == "surface":
            new.surface.update(v)
        elif k in new.kw:
            new.kw[k] = v
        else:
            setattr(new, k, v)
    return new


def all_cases():
    return shape_cases() + census()
