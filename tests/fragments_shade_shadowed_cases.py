"""Hand-built cases of orbit_fragments_shade_shadowed (include/orbit_abi_ext.h H1-H10), on the builders of
tests/fragments_shade_cases.py: its planes, lists and tables, with shadow rows, maps and settings beside them.  A cascade
matrix here is an axis-aligned orthographic map, c = (a * x + bx, a * y + by, az * z + bz, 1): with the seeded world
positions in [-5, 5]^3, a = 0.2 and az = 0.1, bz = 0.5 hold every pixel.  The smallest shapes that can go wrong: the
targets and tile sizes of the base cases, maps of resolution 1, 2, 3, 8 and 64."""
import numpy as np

import fragments_shade_cases as fc
import fragments_shade_shadowed_ref as ref
from orbit_amd import layouts as L
from orbit_amd import raster

F = np.float32
NONE = 0xFFFFFFFF
RESOLUTIONS = (1, 2, 3, 8, 64)
BASE = 4096  # shadow_index_base: MAX_SHADOW_COMMANDS * frame_index of some frame
SETTINGS = dict(blocker_search_radius=0.3, normal_bias_scale=2.0, oriented_bias=-0.02)


def ortho(a=0.2, bx=0.0, by=0.0, az=0.1, bz=0.5, w=1.0):
    m = np.zeros(16, F)
    m[0], m[5], m[10], m[12], m[13], m[14], m[15] = a, a, az, bx, by, bz, w
    return m


def row(matrices=None, world_sizes=(1.0, 1.0, 1.0, 1.0), map_indices=(0, 1, 2, 3)):
    """one shadow row; the default cascades hold |x|, |y| up to 2, 3.33, 4 and 8.33"""
    matrices = [ortho(0.5), ortho(0.3), ortho(0.25), ortho(0.12)] if matrices is None else matrices
    return raster.shadow_rows(matrices, world_sizes, map_indices)


def rows_of(*rows):
    return np.concatenate(rows)


def make_lights(rng, n=40):
    """the base lights (0: directional, 2: sky, 3: ignored, points) with 1 and 4 shadowed directional lights on rows 1 and 0"""
    l = fc.make_lights(rng, n)
    l["shadow_data_index"][1] = BASE + 1
    l["light_type"][4], l["shadow_data_index"][4], l["inner_radius"][4] = L.LIGHT_TYPE_DIRECTIONAL, BASE, 0.4
    l["inner_radius"][1] = 0.2
    return l


def random_maps(rng, count, res, kind="uniform"):
    if kind == "uniform":
        return rng.uniform(0.0, 1.0, (count, res, res)).astype(F)
    if kind == "binary":  # a blocker with probability 1 / 12 in map 0 ... 11 / 12 in the last
        p = np.linspace(1 / 12, 11 / 12, count)[:, None, None]
        return (rng.uniform(0, 1, (count, res, res)) < p).astype(F)
    raise ValueError(kind)


class ShadowCase:
    """a base Case with the shadow rows, maps and settings of one call"""

    def __init__(self, case, rows, maps, settings=None, shadow_index_base=BASE):
        self.case, self.rows, self.maps = case, rows, np.ascontiguousarray(maps, F)
        self.res = self.maps.shape[-1]
        self.settings = dict(SETTINGS, **(settings or {}))
        self.shadow_index_base = shadow_index_base
        self.over = {}

    name = property(lambda self: self.case.name)
    staged = property(lambda self: self.case.staged)

    def args(self, **kw):
        a, k = self.case.args(**kw)
        s = self.settings
        a = a + (self.rows, self.maps, self.res, s["blocker_search_radius"], s["normal_bias_scale"], s["oriented_bias"])
        return a, dict(k, shadow_index_base=self.shadow_index_base, **self.over)

    def copy(self, name):
        c = ShadowCase(self.case.copy(name), self.rows.copy(), self.maps.copy(), self.settings, self.shadow_index_base)
        c.over = dict(self.over)
        return c


def base_case(name, oracle, w, h, tile, seed, lists=None, default_lengths=fc.LENGTHS, cz=12, slices=(3, 9)):
    zs, zb = fc.grid(oracle)
    rng = np.random.default_rng(seed)
    pick = np.array([fc.depth_of_slice(zs, zb, s) for s in slices] + [F(0)])
    depth = pick[rng.choice(len(pick), (h, w), p=[0.9 / len(slices)] * len(slices) + [0.1])] if w * h > 1 else pick[:1].reshape(1, 1)
    return fc.Case(name, depth, tile, zs, zb, seed=seed, lists=lists, default_lengths=default_lengths,
                   cluster_count=(-(-w // tile), -(-h // tile), cz), lights=make_lights(rng))


def shape_cases(oracle):
    """every target with every tile size, a resolution each, uniform maps: every blocker count, every light kind"""
    out = []
    for k, (w, h) in enumerate(fc.TARGETS):
        for t, tile in enumerate(fc.TILES):
            res = RESOLUTIONS[(k + t) % len(RESOLUTIONS)]
            rng = np.random.default_rng(1000 + 10 * k + t)
            lengths = (0, 1, 3, 64, 65) if w * h > 8 else (3, 65)
            c = base_case(f"shadow_shape_{w}x{h}_tile{tile}_res{res}", oracle, w, h, tile, 50 * k + tile, default_lengths=lengths)
            rows = rows_of(row(world_sizes=(0.5, 1.0, 2.0, 4.0)), row(map_indices=(3, 2, 1, 0)))
            out.append(ShadowCase(c, rows, random_maps(rng, 4, res)))
    return out


def one_list_case(name, oracle, w, h, tile, seed, walk, cz=12):
    """every pixel in one slice, every cluster of it walking `walk`"""
    zs, zb = fc.grid(oracle)
    cx, cy = -(-w // tile), -(-h // tile)
    depth = np.full((h, w), fc.depth_of_slice(zs, zb, 4), F)
    rng = np.random.default_rng(seed)
    return fc.Case(name, depth, tile, zs, zb, seed=seed, lists={4 * cx * cy + t: list(walk) for t in range(cx * cy)}, default_lengths=(0,),
                   cluster_count=(cx, cy, cz), lights=make_lights(rng))


def map_cases(oracle):
    """what the maps can do to a pixel: constant maps (blocker count 0 and 12 only), binary maps (every count, 1 and 11
    among them), z equal to a texel bit for bit, NaN and +inf texels, uv far outside the map"""
    out = []
    rows = rows_of(row(matrices=[ortho(0.2)] * 4), row(matrices=[ortho(0.2)] * 4))
    for tile in (8, 4):
        for value, tag in ((-1.0, "no_blockers"), (2.0, "all_blockers")):  # t > z never and always
            c = one_list_case(f"constant_{tag}_tile{tile}", oracle, 9, 9, tile, 3, (1, 5, 6))
            out.append(ShadowCase(c, rows, np.full((4, 8, 8), value, F)))
        rng = np.random.default_rng(17)
        c = one_list_case(f"binary_maps_tile{tile}", oracle, 9, 9, tile, 4, (1, 4, 7))
        split = rows_of(row(matrices=[ortho(0.2)] * 4, map_indices=(0, 0, 0, 0)), row(matrices=[ortho(0.2)] * 4, map_indices=(3, 3, 3, 3)))
        out.append(ShadowCase(c, split, random_maps(rng, 4, 64, "binary")))
        # z = 0.5 exactly under this matrix: texels equal to it, one ulp either side of it, and blockers
        c = one_list_case(f"z_equals_texel_tile{tile}", oracle, 9, 9, tile, 5, (1,))
        half = np.array([0.5, np.nextafter(F(0.5), F(1)), np.nextafter(F(0.5), F(0)), 1.0], F)
        maps = half[rng.integers(0, 4, (4, 8, 8))]
        out.append(ShadowCase(c, rows_of(row(), row(matrices=[ortho(0.2, az=0.0)] * 4)), maps))
        c = one_list_case(f"nan_inf_texels_tile{tile}", oracle, 9, 9, tile, 6, (1, 4))
        odd = np.array([np.nan, np.inf, 0.2, 0.9, -np.inf, 0.5], F)
        out.append(ShadowCase(c, rows, odd[rng.integers(0, 6, (4, 3, 3))]))
        c = one_list_case(f"uv_far_outside_tile{tile}", oracle, 9, 9, tile, 7, (1,))
        out.append(ShadowCase(c, rows, random_maps(rng, 4, 8), settings=dict(oriented_bias=-100.0)))
        c = one_list_case(f"res1_tile{tile}", oracle, 7, 3, tile, 8, (4, 1))
        out.append(ShadowCase(c, rows, np.full((4, 1, 1), 0.55, F)))
    return out


def cascade_case(oracle, tile):
    """8 x 8: cascade 0 is the identity, so q = world_pos: pixels exactly at -1, 0 and 1 and one ulp beyond each; cascade 1 has
    c.w = 0; cascade 2 holds what is left inside [-5, 5]; row 1 has world sizes 0 and different ones; pixels nothing holds
    and a pixel with NaN in world_pos"""
    c = one_list_case(f"cascade_edges_tile{tile}", oracle, 8, 8, tile, 9, (2, 1, 4, 0))
    up, down = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    edge = [(-1, -1, 0), (1, 1, 1), (down(-1), 0, 0.5), (0, down(-1), 0.5), (up(1), 0, 0.5), (0, up(1), 0.5), (0, 0, down(0)), (0, 0, -0.0),
            (0, 0, up(1)), (0.5, -0.5, 1), (up(-1), down(1), up(0)), (1, -1, 0.0)]
    for i, p in enumerate(edge):
        c.world_pos[i // 8, i % 8, :3] = p
    c.world_pos[2, 0, :3], c.world_pos[2, 1, :3], c.world_pos[2, 2, 0] = (50, 0, 0), (0, 0, -30), np.nan
    c.world_pos[2, 3, 3], c.world_pos[2, 4, 3], c.world_pos[2, 5, 3] = 0.0, 2.0, -1.0  # world_pos.w as it arrives
    identity = ortho(1.0, az=1.0, bz=0.0)
    matrices = [identity, ortho(0.2, w=0.0), ortho(0.2), ortho(0.2)]
    rows = rows_of(row(matrices, world_sizes=(1.0, 1.0, 3.0, 1.0)), row(matrices, world_sizes=(0.0, 2.0, 0.5, 1.0)))
    return ShadowCase(c, rows, random_maps(np.random.default_rng(23), 4, 8))


def position_case(oracle, tile):
    """the shadowed light at list positions 0, 63, 64 and 255 of a 256-light walk, one per cluster column; a walk with two
    shadowed lights"""
    zs, zb = fc.grid(oracle)
    w, h = 4 * max(tile, 8), 8
    cx, cy = -(-w // tile), -(-h // tile)
    depth = np.full((h, w), fc.depth_of_slice(zs, zb, 4), F)
    depth[:, ::5] = fc.depth_of_slice(zs, zb, 5)
    lists = {}
    rng = np.random.default_rng(31)
    for column, pos in enumerate((0, 63, 64, 255)):
        walk = rng.integers(5, 40, 256).tolist()  # point lights
        walk[pos] = 1
        for t in range(cx * cy):
            if (t % cx) * tile // max(tile, 8) == column:
                lists[4 * cx * cy + t] = walk
                lists[5 * cx * cy + t] = [4, 6, 1]  # two shadowed lights: the factor is the first's
    c = fc.Case(f"positions_tile{tile}", depth, tile, zs, zb, seed=31, lists=lists, default_lengths=(0,), cluster_count=(cx, cy, 12),
                lights=make_lights(rng))
    rows = rows_of(row(matrices=[ortho(0.2)] * 4), row(matrices=[ortho(0.2)] * 4, map_indices=(1, 1, 1, 1)))
    return ShadowCase(c, rows, random_maps(rng, 2, 8))


def ndl_case(oracle, tile):
    """H4's branch: N . direction exactly 0, 1 and -1 and a rounding away from 0 on both sides"""
    c = one_list_case(f"ndl_tile{tile}", oracle, 8, 8, tile, 41, (1,))
    c.lights["direction"][1] = (0, 1, 0)
    tiny = np.nextafter(F(0), F(1))
    for i, n in enumerate([(1, 0, 0), (0, 1, 0), (0, -1, 0), (1, tiny, 0), (1, -tiny, 0), (0.6, 0.8, 0), (0.6, -0.8, 0), (0, 0, 0)]):
        c.normal[0, i] = n
    return ShadowCase(c, rows_of(row(), row(matrices=[ortho(0.2)] * 4)), random_maps(np.random.default_rng(43), 4, 8),
                      settings=dict(oriented_bias=-0.5))


def tampers(oracle):
    """each counts exactly its own pixels stale: [(case, spec)], spec = ("light", i): the pixels whose walk contains light i,
    or ("cascade", i, c): those among them that light's clean evaluation puts in cascade c"""
    out = []
    for tile in (8, 4):
        zs, zb = fc.grid(oracle)
        depth = np.full((8, 16), fc.depth_of_slice(zs, zb, 2), F)
        depth[:, 8:] = fc.depth_of_slice(zs, zb, 6)
        cx = -(-16 // tile)
        rng = np.random.default_rng(5)
        lists = {c: ([1, 7] if (c // cx) % 2 == 0 and c % cx == 0 else [7, 8]) for c in range(cx * (8 // tile) * 12)}
        base = fc.Case(f"shadow_tamper_base_tile{tile}", depth, tile, zs, zb, seed=5, lists=lists, default_lengths=(0,),
                       cluster_count=(cx, 8 // tile, 12), lights=make_lights(rng))
        clean = ShadowCase(base, rows_of(row(), row()), random_maps(rng, 4, 8))
        t = clean.copy(f"row_is_shadow_count_tile{tile}")
        t.case.lights["shadow_data_index"][1] = BASE + 2
        out.append((t, ("light", 1)))
        t = clean.copy(f"index_below_base_tile{tile}")
        t.case.lights["shadow_data_index"][1] = BASE - 1
        out.append((t, ("light", 1)))
        t = clean.copy(f"map_is_map_count_tile{tile}")
        t.rows["shadow_map_indices"][1, 2] = 4
        out.append((t, ("cascade", 1, 2)))
        out.append((clean, ("none",)))
    return out


def stale_pixels(case, spec, oracle):
    """the (h, w) mask of pixels a tamper must count stale, from the restatement of the clean inputs"""
    b = case.case
    h, w = b.visibility.shape
    if spec[0] == "none":
        return np.zeros((h, w), bool)
    a, k = b.args()
    cl = ref.base.classify(oracle, a[0], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[13])
    walks = np.zeros(h * w, bool)
    for p in np.flatnonzero(cl["live"]):
        walks[p] = spec[1] in cl["indices"][cl["offset"][p]:cl["offset"][p] + cl["n"][p]]
    if spec[0] == "light":
        return walks.reshape(h, w)
    clean = case.copy("clean")
    clean.rows["shadow_map_indices"][:] = (0, 1, 2, 3)
    cascade = restated(clean, oracle)["cascade"]
    return walks.reshape(h, w) & (cascade == spec[2])


def all_cases(oracle):
    return (shape_cases(oracle) + map_cases(oracle) + [cascade_case(oracle, t) for t in (8, 4)] + [position_case(oracle, t) for t in (8, 16, 4, 12)]
            + [ndl_case(oracle, t) for t in (8, 4)])


def mirror(case, **kw):
    a, k = case.args(**kw)
    return raster.host_fragments_shade_shadowed(*a, **k)


def restated(case, oracle, **kw):
    a, k = case.args(**kw)
    drop = ("form", "want_walked", "want_stats", "want_factor", "want_cascade", "want_shadow_stats")
    return ref.shade(oracle, *a, **{key: v for key, v in k.items() if key not in drop})
