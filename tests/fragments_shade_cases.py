"""Hand-built cases of orbit_fragments_shade (include/orbit_abi_ext.h L1-L9).  The call reads planes and tables only, so
no raster is needed: seeded world_pos / normal / material planes, visibility words whose high halves are chosen depths,
a hand-built (offset, count) image and index list.  The smallest shapes that can go wrong: targets of 1 x 1, 7 x 3, 8 x 8,
9 x 9 and 65 x 8; tile_size_px 8 and 16 (eligible for the staged walk) and 4 and 12 (per lane only); lists of 0, 1, 63, 64,
65 and 256 lights and a count of 300; 1, 2 and 32 distinct slices in one 8 x 8 tile; knife-edge depths; every light type."""
import numpy as np

import fragments_shade_ref as ref
from orbit_amd import layouts as L
from orbit_amd import raster

F = np.float32
NONE = 0xFFFFFFFF
Z_NEAR, Z_FAR, CZ, CUTOFF = 0.1, 200.0, 32, 0.01
TARGETS = ((1, 1), (7, 3), (8, 8), (9, 9), (65, 8))
TILES = (8, 16, 4, 12)
LENGTHS = (0, 1, 63, 64, 65, 256, 300)


def grid(oracle):
    return oracle.cluster_grid_info(Z_NEAR, Z_FAR, CZ)


def depth_of_slice(zs, zb, s, frac=0.5):
    """a depth whose slice is s: linear z = 2 ^ ((s + frac - z_bias) / z_scale)"""
    return F(Z_NEAR / 2.0 ** ((s + frac - zb) / zs))


def make_materials(rng, n=12):
    m = np.zeros(n, L.MATERIAL)
    m["base_color"] = rng.uniform(0.05, 1.0, (n, 4))
    m["emissive_factor"] = rng.uniform(0.0, 0.3, (n, 3))
    m["metallic_factor"], m["roughness_factor"] = rng.uniform(0, 1, n), rng.uniform(0.05, 1, n)
    m["occlusion_factor"], m["texture_indices"] = 1.0, NONE
    m["roughness_factor"][:4], m["metallic_factor"][:4] = (0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0)
    m["texture_indices"][5, 0], m["texture_indices"][6, 3] = 3, 0  # textured: shaded from the factors, counted
    return m


def make_lights(rng, n=40):
    l = np.zeros(n, L.LIGHT)
    l["light_type"], l["shadow_data_index"] = L.LIGHT_TYPE_POINT, NONE
    l["irradiance_map_index"] = l["prefiltered_map_index"] = NONE
    l["color"], l["intensity"] = rng.uniform(0.1, 1.0, (n, 3)), rng.uniform(1.0, 20.0, n)
    l["position"], l["inner_radius"] = rng.uniform(-6, 6, (n, 3)), 0.05
    d = rng.normal(size=(n, 3))
    l["direction"] = d / np.linalg.norm(d, axis=1)[:, None]
    l["outer_radius"] = np.sqrt(l["intensity"] / CUTOFF) * rng.uniform(0.2, 1.0, n)
    l["light_type"][0] = L.LIGHT_TYPE_DIRECTIONAL
    l["light_type"][1], l["shadow_data_index"][1] = L.LIGHT_TYPE_DIRECTIONAL, 2  # shadowed: lit unshadowed, unserved
    l["light_type"][2] = L.LIGHT_TYPE_SKY  # skipped, unserved
    l["light_type"][3] = 7  # ignored
    return l


class Case:
    """One call's inputs.  lists: {cluster linear index: list of light indices}; counts: {cluster: count word} where
    the image's count is not the list's length."""

    def __init__(self, name, depth, tile, zs, zb, seed=1, lists=None, default_lengths=LENGTHS, cluster_count=None, lights=None,
                 materials=None, counts=None, view_pos=(0.5, 4.0, 7.0), extra_indices=0):
        rng = np.random.default_rng(seed)
        self.name, self.tile, self.zs, self.zb = name, tile, zs, zb
        depth = np.asarray(depth, F)
        h, w = depth.shape
        ids = rng.integers(1, 1 << 24, (h, w)).astype(np.uint64) << np.uint64(8) | np.uint64(1)
        bits = depth.view(np.uint32).astype(np.uint64)
        self.visibility = np.where(np.isnan(depth) | (depth != 0) | (bits != 0), bits << np.uint64(32) | ids, np.uint64(0))
        self.materials = make_materials(rng) if materials is None else materials
        self.lights = make_lights(rng) if lights is None else lights
        self.world_pos = np.concatenate([rng.uniform(-5, 5, (h, w, 3)), np.ones((h, w, 1))], axis=2).astype(F)
        n = rng.normal(size=(h, w, 3))
        self.normal = (n / np.linalg.norm(n, axis=2)[..., None]).astype(F)
        self.material = rng.integers(0, len(self.materials), (h, w)).astype(np.uint32)
        cx, cy = -(-w // tile), -(-h // tile)
        self.cluster_count = (cx, cy, CZ) if cluster_count is None else cluster_count
        cx, cy, cz = self.cluster_count
        image = np.zeros((cx * cy * cz, 2), np.uint32)
        indices = []
        lists = {} if lists is None else lists
        for c in range(cx * cy * cz):
            if c in lists:
                walk = list(lists[c])
            else:
                length = default_lengths[int(rng.integers(0, len(default_lengths)))]
                walk = rng.integers(0, len(self.lights), length).tolist()
            image[c] = (len(indices), len(walk))
            indices += walk
        for c, count in (counts or {}).items():
            image[c, 1] = count
        indices += [0] * extra_indices
        self.image = image
        self.index_buffer = np.concatenate([np.array([len(indices)], np.uint32), np.array(indices, np.uint32)]).view(np.uint8)
        self.view_pos = view_pos
        self.over = {}

    def args(self, **kw):
        """(positional, keyword) arguments of raster.host_fragments_shade and fragments_shade_ref.shade"""
        a = (self.visibility, self.world_pos, self.normal, self.material, self.materials, self.lights, self.image, self.index_buffer,
             self.cluster_count, self.tile, self.zs, self.zb, CUTOFF, Z_NEAR, self.view_pos)
        return a, dict(self.over, **kw)

    @property
    def staged(self):
        return self.tile % 8 == 0

    def cluster(self, x, y, s):
        cx, cy, _ = self.cluster_count
        return x // self.tile + (y // self.tile) * cx + s * cx * cy

    def copy(self, name):
        import copy

        c = copy.copy(self)
        c.name, c.over = name, dict(self.over)
        for k in ("visibility", "world_pos", "normal", "material", "materials", "lights", "image", "index_buffer"):
            setattr(c, k, getattr(self, k).copy())
        return c


def shape_cases(oracle):
    """every target with every tile size: two slices per cluster column, lists of every length"""
    zs, zb = grid(oracle)
    out = []
    for k, (w, h) in enumerate(TARGETS):
        for tile in TILES:
            rng = np.random.default_rng(100 * k + tile)
            pick = np.array([depth_of_slice(zs, zb, 3), depth_of_slice(zs, zb, 9), F(0)])
            depth = pick[rng.choice(3, (h, w), p=(0.45, 0.45, 0.1))] if w * h > 1 else pick[:1].reshape(1, 1)
            lengths = LENGTHS if w * h > 8 else (1, 65)
            out.append(Case(f"shape_{w}x{h}_tile{tile}", depth, tile, zs, zb, seed=100 * k + tile, default_lengths=lengths,
                            cluster_count=(-(-w // tile), -(-h // tile), 12)))
    return out


def slice_cases(oracle):
    """an 8 x 8 tile whose pixels fall in 1, 2 and 32 distinct slices, each cluster with a list of its own"""
    zs, zb = grid(oracle)
    out = []
    for distinct in (1, 2, 32):
        s = (np.arange(64).reshape(8, 8) * 7 + 3) % distinct if distinct > 1 else np.full((8, 8), 5)
        depth = np.array([[depth_of_slice(zs, zb, int(v)) for v in row] for row in s], F)
        for tile in (8, 4):
            out.append(Case(f"{distinct}_slices_tile{tile}", depth, tile, zs, zb, seed=distinct, default_lengths=(1, 63, 64, 65, 256)))
    return out


def knife_edge_depths(oracle, zs, zb, targets=range(4, 33)):
    """depths d found with oracle.log2f whose fma(log2f(z_near / d), z_scale, z_bias) lies within one ulp of an integer k, on
    both sides: [(d, k, t)].  One ulp of d moves t by about one ulp of k, so not every k has such a d on both sides: every
    k of `targets` is searched and what is found is kept (at least four on each side)."""
    found = []
    for k in targets:
        d = F(Z_NEAR / 2.0 ** ((k - zb) / zs))
        for _ in range(100):
            d = np.nextafter(d, F(0), dtype=F)
        ulp = float(np.spacing(F(k)))
        for _ in range(200):
            d = np.nextafter(d, F(np.inf), dtype=F)
            t = float(ref.fma32(F(oracle.log2f(float(F(Z_NEAR) / d))), F(zs), F(zb)))
            if k - ulp <= t <= k + ulp:
                found.append((d, k, t))
    below, above = [f for f in found if f[2] < f[1]], [f for f in found if f[2] >= f[1]]
    assert len(below) >= 4 and len(above) >= 4, (len(below), len(above))
    return found


def special_depths():
    """denormal, +inf, NaN bits and negative in the word's high half; a depth beyond the last slice and one before the first"""
    bits = np.array([0x00000001, 0x007FFFFF, 0x7F800000, 0x7FC00001, 0xFFC00000, 0xBF000000, 0x80000000, 0x00800000], np.uint32)
    return np.concatenate([bits.view(F), np.array([1e-9, 0.99999, 1.0, 2.0], F)])


def edge_case(oracle, tile):
    """65 x 8: knife-edge and special depths, every cluster of a column with a list of its own; the image is one tile
    narrower than the target, so the last columns are OUTSIDE"""
    zs, zb = grid(oracle)
    edges = [d for d, _, _ in knife_edge_depths(oracle, zs, zb)]
    pool = np.concatenate([np.array(edges, F), special_depths(), np.array([depth_of_slice(zs, zb, s) for s in (0, 31, 32, 40)], F)])
    depth = np.resize(pool, 65 * 8).reshape(8, 65)
    cx = -(-65 // tile) - 1
    return Case(f"edges_tile{tile}", depth, tile, zs, zb, seed=7 + tile, default_lengths=(1, 2, 3, 64, 65), cluster_count=(cx, 1, CZ))


def light_case(oracle, tile):
    """9 x 9, one slice: every cluster walks every light type, a point light at a pixel's own position, roughness and
    metallic 0 and 1, textured materials; pixel (1, 1) looks from its own position (V is not finite)"""
    zs, zb = grid(oracle)
    depth = np.full((9, 9), depth_of_slice(zs, zb, 4), F)
    depth[0, 0] = 0
    cx = -(-9 // tile)
    walk = list(range(12))
    c = Case(f"lights_tile{tile}", depth, tile, zs, zb, seed=11, lists={4 * cx * cx + t: walk for t in range(cx * cx)}, default_lengths=(0,))
    c.lights["position"][5] = c.world_pos[2, 3, :3]  # dist = 0: Ld = 0 / 0
    c.material[4, :4] = (0, 1, 2, 3)
    c.material[5, :2] = (5, 6)
    c.material[8, 8] = NONE  # unshaded
    c.view_pos = tuple(float(v) for v in c.world_pos[1, 1, :3])
    return c


def tampers(oracle):
    """each counts exactly its pixels stale: [(case, the pixels (y, x) that must be stale)]"""
    zs, zb = grid(oracle)
    out = []
    for tile in (8, 4):
        depth = np.full((8, 16), depth_of_slice(zs, zb, 2), F)
        depth[:, 8:] = depth_of_slice(zs, zb, 6)
        cx = -(-16 // tile)
        mk = lambda name, **kw: Case(f"{name}_tile{tile}", depth, tile, zs, zb, seed=5, **kw)  # noqa: E731
        base = mk("tamper_base", default_lengths=(2,))
        t = base.copy(f"material_is_material_count_tile{tile}")
        t.material[3, 4], t.material[7, 15] = len(t.materials), 0x7FFFFFFF
        out.append((t, [(3, 4), (7, 15)]))
        # the last cluster's walk ends one past index_capacity
        t = base.copy(f"offset_plus_n_one_past_capacity_tile{tile}")
        walked = sorted({base.cluster(x, y, 2 if x < 8 else 6) for y in range(8) for x in range(16)})
        ends = [int(t.image[c, 0] + t.image[c, 1]) for c in walked]
        last = walked[int(np.argmax(ends))]
        t.over["index_capacity"] = max(ends) - 1
        out.append((t, ("cluster", last)))
        for pos in (0, 63, 64, 255):
            walk = list(np.random.default_rng(pos).integers(0, 40, 256))
            walk[pos] = 40  # = light_count
            target = base.cluster(0, 0, 2)
            t = mk(f"bad_index_at_{pos}", lists={target: walk}, default_lengths=(2,))
            out.append((t, ("cluster", target)))
    return out


def stale_pixels(case, spec, oracle):
    """the (h, w) mask of pixels a tamper must count stale"""
    h, w = case.visibility.shape
    mask = np.zeros((h, w), bool)
    if spec[0] == "cluster":
        sl = ref.slices(oracle, case.visibility, Z_NEAR, case.zs, case.zb)
        ys, xs = np.divmod(np.arange(h * w), w)
        cx, cy, cz = case.cluster_count
        inside = sl.reshape(-1) < cz
        idx = xs // case.tile + (ys // case.tile) * cx + np.minimum(sl.reshape(-1), cz - 1).astype(np.int64) * cx * cy
        mask = ((idx == spec[1]) & inside & (case.visibility.reshape(-1) != 0)).reshape(h, w)
    else:
        for y, x in spec:
            mask[y, x] = True
    return mask


def all_cases(oracle):
    return shape_cases(oracle) + slice_cases(oracle) + [edge_case(oracle, t) for t in TILES] + [light_case(oracle, t) for t in (8, 4)]


def mirror(case, **kw):
    a, k = case.args(**kw)
    return raster.host_fragments_shade(*a, **k)


def restated(case, oracle, **kw):
    a, k = case.args(**kw)
    return ref.shade(oracle, *a, **{key: v for key, v in k.items() if key not in ("form", "want_walked", "want_stats")})
