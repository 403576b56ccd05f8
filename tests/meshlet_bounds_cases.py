"""Inputs for orbit_meshlet_bounds (include/orbit_abi_ext.h): hand-built meshlets at the edges of
meshopt_computeClusterBounds as the host mirror restates it, packed into the buffers the call reads, and a census of what
they reach.  The expected bytes are never computed here: the reference is orbit_amd.assets.meshlet_bounds (the host
export on the same buffers).  Shared by tests/test_meshlet_bounds_cpu.py and tests/test_meshlet_bounds_gpu.py.

A case is (name, positions float32 [nv, 3], corners uint8 [nt, 3], tags)."""
import numpy as np

from orbit_amd import assets
from orbit_amd import layouts as L

F = np.float32
SENTINEL = 0xA5  # fill of every byte a call must not write
GUARD = 256      # bytes in front of and behind every buffer


def strip(nt, curve=0.05, seed=0, nv_max=255):
    """A gently curved triangle strip (narrow normal cone) of nt triangles; triangles beyond what nv_max vertices give
    reuse earlier corners."""
    nv = min(nt + 2, nv_max)
    i = np.arange(nv)
    rng = np.random.default_rng(seed)
    x, y = (i // 2).astype(F) * F(0.25), (i % 2).astype(F)
    pos = np.stack([x, y, F(curve) * (x * x + y * y) + rng.uniform(0, 0.01, nv).astype(F)], axis=1).astype(F)
    tri = []
    for t in range(nt):
        k = t % (nv - 2)
        tri.append((k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2))
    return pos, np.array(tri, np.uint8)


def soup(nt, nv, seed, scale=1.0):
    """Random triangles over random vertices: a wide cone and many sphere updates."""
    rng = np.random.default_rng(seed)
    pos = (rng.normal(size=(nv, 3)) * scale).astype(F)
    return pos, rng.integers(0, nv, (nt, 3)).astype(np.uint8)


def helix(nt, per_turn=2.3, pitch=0.01):
    """Triangles whose corners wind up a unit helix, 3 nt points in all.  The Ritter seed is the longest of the three
    axis-extreme pairs — here a chord, no diameter — and the sphere then creeps after the points: most of them lie
    outside what the points before them left and update it, so the result depends on their order.  (EVERY point
    cannot update: the seed pair's two ends lie on the seed sphere, and points on a ray, whose extremes are its two
    ends, all lie inside it.)"""
    i = np.arange(3 * nt)
    a = i * (2 * np.pi / per_turn) + 0.3
    pos = np.stack([np.cos(a), np.sin(a), pitch * i], axis=1).astype(F)
    return pos, np.arange(3 * nt, dtype=np.uint8).reshape(nt, 3)


def with_degenerate(case, where):
    pos, tri = case
    tri = tri.copy()
    for t in where:
        tri[t] = (tri[t][0], tri[t][0], tri[t][2])
    return pos, tri


def build_cases():
    cases = []

    def add(name, case, *tags):
        pos, tri = case
        cases.append((name, np.ascontiguousarray(pos, F), np.ascontiguousarray(tri, np.uint8), set(tags)))

    add("one_triangle", (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.uint8)), "count_1_3")
    # a closed band: 64 vertices, 64 triangles (the reference's limits, mesh.rs:8-9)
    a = np.arange(32) * (2 * np.pi / 32)
    ring = np.concatenate([np.stack([np.cos(a), np.sin(a), np.zeros(32)], 1), np.stack([np.cos(a), np.sin(a), np.ones(32)], 1)]).astype(F)
    band = [(k, (k + 1) % 32, 32 + k) for k in range(32)] + [((k + 1) % 32, 32 + (k + 1) % 32, 32 + k) for k in range(32)]
    add("band_64_64", (ring, np.array(band, np.uint8)), "count_64_64")
    add("strip_40", strip(40, seed=1))
    add("strip_64", strip(64, seed=2))
    add("strip_65", strip(65, seed=3), "count_65")
    add("strip_128", strip(128, seed=4), "count_128")
    add("strip_255", strip(255, seed=5), "count_255", "verts_255")
    add("soup_255", soup(255, 255, 6), "count_255", "verts_255")
    add("soup_64", soup(64, 64, 7))
    add("soup_130", soup(130, 100, 8))
    add("helix_21", helix(21), "helix")
    add("helix_64", helix(64), "helix")
    add("helix_64_slow", helix(64, 7.1), "helix")
    add("helix_85", helix(85, pitch=0.004), "helix")  # 255 vertices, two chunks of triangles
    add("helix_85_slow", helix(85, 7.1, 0.004), "helix")
    add("helix_soup_200", (helix(85)[0], soup(200, 255, 16)[1]), "helix")  # updates in every chunk
    add("degenerate_interior", with_degenerate(strip(30, seed=9), [7, 8, 20]), "degenerate_interior")
    add("degenerate_first", with_degenerate(strip(30, seed=10), [0]), "degenerate_first")
    add("degenerate_last", with_degenerate(strip(30, seed=11), [29]), "degenerate_last")
    add("degenerate_first_of_second_chunk", with_degenerate(strip(100, seed=12), [0, 63, 64, 65, 99]), "degenerate_interior",
        "degenerate_first", "degenerate_last")
    add("degenerate_all", with_degenerate(strip(12, seed=13), range(12)), "degenerate_all")
    collinear = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], F)
    add("degenerate_all_collinear", (collinear, np.array([[0, 1, 2], [1, 2, 3]], np.uint8)), "degenerate_all")
    fold = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    # a tent whose two faces look along (+-1, 0, 0.05): mindp is about 0.05, below the 0.1 of the exit, the axis is not 0
    tent = np.array([[0, 0, 1], [0, 1, 1], [0.05, 0, 0], [0.05, 1, 0], [-0.05, 0, 0], [-0.05, 1, 0]], F)
    add("wide_cone", (tent, np.array([[0, 1, 2], [1, 3, 2], [1, 0, 4], [1, 4, 5]], np.uint8)), "wide_cone")
    # the same triangle with both windings: the normals' sphere is centred on 0, the axis has length 0
    add("opposite_triangles", (fold[:3], np.array([[0, 1, 2], [0, 2, 1]], np.uint8)), "zero_axis")
    # an axis-aligned box corner region with every extreme attained several times, and zeros of both signs
    q = np.array([[-1, -1, 0.0], [1, -1, -0.0], [1, 1, 0.0], [-1, 1, -0.0], [-1, -1, -0.0], [1, 1, -0.0], [0.0, -0.0, 0.0]], F)
    add("ties_and_signed_zeros", (q, np.array([[0, 1, 2], [4, 5, 3], [6, 1, 2], [0, 2, 3], [6, 3, 4]], np.uint8)), "ties", "signed_zero")
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F)
    faces = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    add("cube_ties", (cube, np.array(faces, np.uint8)), "ties")
    p, t = strip(20, seed=14)
    add("denormal_all", (p * F(1e-41), t), "denormal")
    pz = p.copy()
    pz[:, 2] *= F(1e-39)
    add("denormal_one_axis", (pz, t), "denormal")
    add("huge_1e30", (p * F(1e30), t), "huge")
    add("huge_3e38", (p * F(3e37), t), "huge")
    for name, v, val in (("nan_first_vertex", 0, np.nan), ("nan_later_vertex", 9, np.nan), ("inf_vertex", 5, np.inf),
                         ("neg_inf_vertex", 6, -np.inf)):
        pn = p.copy()
        pn[v, 1] = val
        add(name, (pn, t), name)
    pn = p.copy()
    pn[0] = np.nan
    pn[13, 0] = np.nan
    pn[17, 2] = np.inf
    add("nan_and_inf_mixed", (pn, t), "nan_first_vertex", "nan_later_vertex", "inf_vertex")
    pn, tn = soup(100, 80, 15)
    pn[3, 0], pn[50, 2], pn[77, 1] = np.nan, -np.inf, np.nan
    add("soup_with_nan", (pn, tn), "nan_later_vertex", "neg_inf_vertex")
    add("no_triangles", (fold, np.zeros((0, 3), np.uint8)), "degenerate_all")
    return cases


class Packed:
    """The cases as one set of buffers: records (32 B, every byte the call leaves alone filled with SENTINEL apart from
    the fields it reads), meshlet_data and a vertex buffer of `stride` bytes per vertex with the position at `offset`."""

    def __init__(self, cases, stride=12, offset=0, vertex_offset=0, spare_records=3):
        self.names = [c[0] for c in cases]
        self.stride, self.offset = stride, offset
        n = len(cases)
        self.count = n
        rec = np.full((n + spare_records) * 32, SENTINEL, np.uint8).view(L.MESHLET)
        data, verts = [np.full(5, 0xFFFFFFFF, np.uint32)], []  # five words nothing points at
        nv_total = vertex_offset
        for k, (_, pos, tri, _tags) in enumerate(cases):
            d0 = sum(len(x) for x in data)
            # the meshes of a scene share one vertex buffer: even meshlets address it through vertex_offset, odd ones
            # through their indices
            base = nv_total if k % 2 == 0 else 0
            data.append(np.arange(len(pos), dtype=np.uint32) + np.uint32(nv_total - base))
            corner_bytes = np.zeros((3 * len(tri) + 3) // 4 * 4, np.uint8)
            corner_bytes[:3 * len(tri)] = tri.reshape(-1)
            data.append(corner_bytes.view(np.uint32))
            rec[k]["vertex_offset"], rec[k]["data_offset"] = base, d0
            rec[k]["vertex_count"], rec[k]["triangle_count"] = len(pos), len(tri)
            verts.append(pos)
            nv_total += len(pos)
        self.records = rec
        self.meshlet_data = np.concatenate(data)
        self.vertex_count = nv_total
        vb = np.full(nv_total * stride, SENTINEL, np.uint8)
        allpos = np.concatenate(verts).astype(F)
        view = np.lib.stride_tricks.as_strided(vb[vertex_offset * stride + offset:].view(np.uint8), (len(allpos), 12), (stride, 1))
        view[:] = allpos.view(np.uint8).reshape(-1, 12)
        self.vertices = vb

    def host(self, **kw):
        return assets.meshlet_bounds(self.records, self.meshlet_data, self.vertices, self.vertex_count, self.stride,
                                     self.offset, **kw)


def expected_records(records, full, err, selection):
    """`records` with bytes 0..19 of the selected, error-free meshlets replaced by the reference's."""
    out = records.copy()
    for row, m in enumerate(selection):
        if not err[row]:
            out[m]["bounding_sphere"][:3], out[m]["bounding_sphere"][3] = full[row]["center"], full[row]["radius"]
            out[m]["cone_axis"], out[m]["cone_cutoff"] = full[row]["cone_axis_s8"], full[row]["cone_cutoff_s8"]
    return out


def census(cases, full, updates):
    """{category: number of cases in it}: the tags the builders set, and what the reference reports."""
    c = {}

    def hit(k):
        c[k] = c.get(k, 0) + 1

    for (name, pos, tri, tags), f, u in zip(cases, full, updates):
        for t in tags:
            hit(t)
        u = int(u)
        hit("updates_0" if u == 0 else "updates_1_plus")
        if u >= 8:
            hit("updates_8_plus")
        if u >= 2 * len(tri) and len(tri) >= 21:  # half of the 3 nt corners + nt normals, or more
            hit("most_points_update")
        if f["cone_cutoff_s8"] == 127 and f["cone_cutoff"] == 1 and not f["cone_axis"].any():
            hit("wide_cone_exit")
        if not f.tobytes().strip(b"\0"):
            hit("zero_bounds")
        if len(tri) > 64:
            hit("more_than_one_chunk")
    return c
