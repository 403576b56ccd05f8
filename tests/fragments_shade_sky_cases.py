"""Hand-built cases of orbit_fragments_shade_sky (include/orbit_abi_ext.h K1-K10), on the builders of
tests/fragments_shade_shadowed_cases.py: its planes, lists, tables, shadow rows and maps, with an environment (seeded fp16
cubes and a table, one set holding NaN and inf halves), a sky cube with its full chain, an ao plane and K9's basis beside
them.  The smallest shapes that can go wrong: targets of 1 x 1, 8 x 8, 9 x 7 and a 73 x 33 layout of
tests/shade_tile_cases.py; irradiance cubes of 1, 2, 5 and 8, prefiltered cubes of 1, 2, 5 and 16 with 1, 2 and 5 levels,
tables of 1, 2, 16 and 17, sky cubes of 1, 2 and 16."""
import numpy as np

import fragments_shade_cases as fc
import fragments_shade_shadowed_cases as sc
import fragments_shade_sky_ref as ref
import shade_tile_cases as tc
from orbit_amd import layouts as L
from orbit_amd import raster

F = np.float32
NONE = 0xFFFFFFFF
SKY, SKY_DARK = 2, 9          # the light table's SKY rows: fc.make_lights' and one with intensity 0
SUN, SUN2 = 1, 4              # sc.make_lights' shadowed directional lights
IRRADIANCE_SIZES, PREFILTERED_SIZES, PREFILTERED_LEVELS, TABLE_SIZES, SKY_SIZES = (1, 2, 5, 8), (1, 2, 5, 16), (1, 2, 5), (1, 2, 16, 17), (1, 2, 16)
ROUGHNESS = (0.0, 0.25, 0.3, 1.0, 1.5, np.nan)  # with 5 levels 0.25 gives lod 1: E4's one-level path
METALLIC = (0.0, 0.5, 1.0)
AO_VALUES = (0.0, 0.5, 1.0, 2.0, -1.0, np.nan)
IDENTITY_BASIS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0))


def cube_words(rng, size, levels, special=False):
    """a cube in E0's layout: seeded colours in [0, 4), alpha 1; special: NaN, +inf, -inf and 65504 halves among them"""
    texels = sum(6 * max(1, size >> m) ** 2 for m in range(levels))
    v = rng.uniform(0.0, 4.0, (texels, 4)).astype(np.float16)
    v[:, 3] = 1.0
    if special:
        odd = np.array([np.nan, np.inf, -np.inf, 65504.0], np.float16)
        at = rng.integers(0, texels, max(4, texels // 5))
        v[at, rng.integers(0, 3, len(at))] = odd[rng.integers(0, 4, len(at))]
    return v.view(np.uint16).reshape(-1)


def table_words(rng, n, special=False):
    v = rng.uniform(0.0, 1.0, (n, n, 2)).astype(np.float16)
    if special:
        v[0, 0, 0], v[n - 1, n - 1, 1] = np.nan, np.inf
    return v.view(np.uint16).reshape(-1)


def make_env(seed, irradiance_size, prefiltered_size, prefiltered_levels, brdf_size, special=False):
    rng = np.random.default_rng(seed)
    return dict(irradiance=cube_words(rng, irradiance_size, 1, special), irradiance_size=irradiance_size,
                prefiltered=cube_words(rng, prefiltered_size, prefiltered_levels, special), prefiltered_size=prefiltered_size,
                prefiltered_levels=prefiltered_levels, brdf=table_words(rng, brdf_size, special), brdf_size=brdf_size)


def make_sky(seed, size, special=False):
    levels = int(size).bit_length()  # the full chain
    return dict(cube=cube_words(np.random.default_rng(seed), size, levels, special), size=size, levels=levels)


def make_materials(rng, n=24):
    """every roughness with every metallic, base colours 0 and above 1 among them; rows 18 and 19 textured"""
    m = fc.make_materials(rng, n)
    for i in range(18):
        m["roughness_factor"][i], m["metallic_factor"][i] = ROUGHNESS[i % 6], METALLIC[i // 6]
    m["base_color"][1, :3], m["base_color"][8, :3], m["base_color"][15, :3] = 0.0, (1.5, 2.0, 3.0), (0.0, 1.25, 0.5)
    m["texture_indices"][:] = NONE
    m["texture_indices"][18, 0], m["texture_indices"][19, 3] = 3, 0  # textured (19: occlusion): shaded from the factors, counted
    return m


def make_lights(rng, n=40):
    """sc.make_lights (0 directional, 1 and 4 shadowed, 2 sky, 3 ignored, points) with a second sky light of intensity 0"""
    l = sc.make_lights(rng, n)
    l["light_type"][SKY_DARK], l["intensity"][SKY_DARK] = L.LIGHT_TYPE_SKY, 0.0
    l["irradiance_map_index"][SKY], l["prefiltered_map_index"][SKY] = 7, 0x7FFFFFFF  # not read (K1)
    return l


class SkyCase:
    """a ShadowCase with the environment, the sky cube, K9's lod and basis and the ao plane of one call"""

    def __init__(self, shadow, env=None, sky=None, skybox_lod=0.0, basis=IDENTITY_BASIS, ao=None):
        self.shadow, self.env, self.sky, self.skybox_lod, self.basis, self.ao = shadow, env, sky, skybox_lod, basis, ao

    name = property(lambda self: self.shadow.name)
    staged = property(lambda self: self.shadow.staged)
    case = property(lambda self: self.shadow.case)

    def args(self, **kw):
        a, k = self.shadow.args(**kw)
        return a, dict(dict(env=self.env, sky=self.sky, skybox_lod=self.skybox_lod, basis=self.basis, ao=self.ao), **k)

    def without(self, *what):
        """the same call with the environment and / or the sky cube NULL"""
        return SkyCase(self.shadow, None if "env" in what else self.env, None if "sky" in what else self.sky, self.skybox_lod, self.basis, self.ao)


def base_case(name, oracle, w, h, tile, seed, walks, slices=(3, 9), uncovered=0.15, materials=24):
    """a w x h target over `slices`; walks: one list per slice (every cluster of the slice walks it)"""
    zs, zb = fc.grid(oracle)
    rng = np.random.default_rng(seed)
    pick = np.array([fc.depth_of_slice(zs, zb, s) for s in slices] + [F(0)])
    p = [(1.0 - uncovered) / len(slices)] * len(slices) + [uncovered]
    depth = pick[rng.choice(len(pick), (h, w), p=p)] if w * h > 1 else pick[:1].reshape(1, 1)
    cx, cy = -(-w // tile), -(-h // tile)
    lists = {s * cx * cy + t: list(walk) for s, walk in zip(slices, walks) for t in range(cx * cy)}
    c = fc.Case(name, depth, tile, zs, zb, seed=seed, lists=lists, default_lengths=(0,), cluster_count=(cx, cy, 12), lights=make_lights(rng),
                materials=make_materials(rng, materials))
    rows = sc.rows_of(sc.row(world_sizes=(0.5, 1.0, 2.0, 4.0)), sc.row(map_indices=(3, 2, 1, 0)))
    return sc.ShadowCase(c, rows, sc.random_maps(rng, 4, 8))


def ao_plane(rng, h, w):
    return np.array(AO_VALUES, F)[rng.integers(0, len(AO_VALUES), (h, w))]


def shape_cases(oracle):
    """every target with tile_size_px 8 and 4, the sizes of every image cycling: the sky light first, in the middle, last and
    twice in a list, beside shadowed suns and point lights, with intensity 0; a mixed wave (only slice 3's list holds it)"""
    out = []
    walks = [([SKY, 12, SUN, 13], [14, SUN2, SKY]), ([15, SKY, 16, SKY_DARK, SUN], [17, 18]), ([SKY, SKY], [SUN, 19, 20, SKY]),
             ([21, 22, SKY_DARK], [SKY, SUN2, 23, SKY])]
    for k, (w, h) in enumerate(((1, 1), (8, 8), (9, 7))):
        for t, tile in enumerate((8, 4)):
            i = 2 * k + t
            rng = np.random.default_rng(900 + i)
            s = base_case(f"sky_shape_{w}x{h}_tile{tile}", oracle, w, h, tile, 300 + i, walks[i % 4])
            env = make_env(400 + i, IRRADIANCE_SIZES[i % 4], PREFILTERED_SIZES[(i + 1) % 4], PREFILTERED_LEVELS[i % 3], TABLE_SIZES[(i + 2) % 4],
                           special=i == 3)
            out.append(SkyCase(s, env, make_sky(500 + i, SKY_SIZES[i % 3], special=i == 3), skybox_lod=(0.0, 0.5, 20.0)[i % 3],
                               ao=ao_plane(rng, h, w) if i % 2 == 0 else None))
    return out


def size_cases(oracle):
    """8 x 8, one list [SKY]: the sizes and level counts shape_cases does not reach, so that every one of them occurs"""
    out = []
    combos = [(1, 1, 1, 1, 1), (2, 2, 2, 2, 2), (5, 5, 5, 16, 16), (8, 16, 5, 17, 16), (8, 16, 1, 16, 1), (5, 1, 5, 2, 2), (2, 5, 2, 17, 16)]
    for i, (n, m, levels, t, s) in enumerate(combos):
        c = base_case(f"sky_sizes_{n}_{m}x{levels}_{t}_{s}", oracle, 8, 8, 8 if i % 2 == 0 else 4, 600 + i, ([SKY], [SKY, 30]))
        out.append(SkyCase(c, make_env(610 + i, n, m, levels, t), make_sky(620 + i, s), skybox_lod=0.5 * i))
    return out


def direction_case(oracle, tile):
    """8 x 8, one slice, one list [SKY], the eye at the origin: row 0 puts N on a face centre, an edge, a corner and one ulp
    either side of each; row 1 does the same to R (N perpendicular to V: R is V with y negated); row 2 has dot(N, V) negative,
    0 and 1, a zero normal and a pixel at the eye (V is not finite); rows 3 and 4 meet the table's corners: (ndv0, roughness)
    exactly (0, 0) and (1, 1)"""
    zs, zb = fc.grid(oracle)
    depth = np.full((8, 8), fc.depth_of_slice(zs, zb, 4), F)
    rng = np.random.default_rng(71)
    c = fc.Case(f"sky_directions_tile{tile}", depth, tile, zs, zb, seed=71, lists={4 * (8 // tile) ** 2 + t: [SKY] for t in range((8 // tile) ** 2)},
                default_lengths=(0,), cluster_count=(8 // tile, 8 // tile, 12), lights=make_lights(rng), materials=make_materials(rng),
                view_pos=(0.0, 0.0, 0.0))
    up, down = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    c.material[:] = 2  # roughness 0.3, metallic 0
    normals = [(1, 0, 0), (0, -1, 0), (1, 1, 0), (up(1), 1, 0), (down(1), 1, 0), (1, 1, 1), (1, up(1), 1), (1, 1, down(1))]
    for i, n in enumerate(normals):
        c.normal[0, i] = n
    # V = normalize(-world_pos): equal components stay equal under the division
    views = [(-1, 0, 0), (0, 0, -2), (-1, -1, 0), (-up(1), -1, 0), (-down(1), -1, 0), (-1, -1, -1), (-1, -up(1), -1), (-1, -1, -down(1))]
    perpendicular = [(0, 1, 0), (0, 1, 0), (0, 0, 1), (0, 0, 1), (0, 0, 1), (1, -1, 0), (1, 0, -1), (1, -1, 0)]
    for i, (v, n) in enumerate(zip(views, perpendicular)):
        c.world_pos[1, i, :3], c.normal[1, i] = v, n
    c.world_pos[2, :, :3] = (-2, 0, 0)  # V = (1, 0, 0)
    for i, n in enumerate([(-1, 0, 0), (-0.5, 0.5, 0), (0, 1, 0), (0, 0, -1), (1, 0, 0), (0, 0, 0), (0.6, 0.8, 0), (1, 0, 0)]):
        c.normal[2, i] = n
    c.world_pos[2, 7, :3] = 0.0  # at the eye: V = 0 / 0
    c.world_pos[3:5, :, :3] = (-2, 0, 0)
    c.normal[3, :], c.normal[4, :] = (0, 1, 0), (1, 0, 0)  # ndv0 exactly 0, exactly 1
    c.material[3, :], c.material[4, :] = np.arange(8) % 6, 3 + 6 * (np.arange(8) % 3)  # every roughness; roughness 1
    c.material[3, 0] = 0  # roughness 0 at ndv0 0
    rows = sc.rows_of(sc.row(), sc.row())
    s = sc.ShadowCase(c, rows, sc.random_maps(rng, 4, 8))
    return SkyCase(s, make_env(72, 8, 16, 5, 16), None)


def list_cases(oracle):
    """a list capped at 256 with the sky light at positions 0, 255 and 256 (not walked) of a count of 300; lists of 64 and 65
    with it at the chunk's edge"""
    out = []
    for tile in (8, 4):
        rng = np.random.default_rng(81)
        long = rng.integers(12, 40, 300).tolist()
        long[0], long[255], long[256] = SKY, SKY, SKY_DARK
        edge = rng.integers(12, 40, 65).tolist()
        edge[63], edge[64] = SKY, SKY
        c = base_case(f"sky_lists_tile{tile}", oracle, 9, 7, tile, 82, (long, edge), uncovered=0.0)
        out.append(SkyCase(c, make_env(83, 5, 5, 2, 2), None, ao=ao_plane(rng, 7, 9)))
    return out


def stale_map_case(oracle):
    """8 x 8, two slices whose walks hold the sun between or behind evaluated sky lights, the sun's row naming a map that is
    not there (H3): every pixel lies inside a cascade, so every walk goes stale at the sun and nothing is written"""
    s = base_case("sky_stale_map", oracle, 8, 8, 8, 85, ([SKY, SUN, SKY, 12], [13, SKY, SUN]), uncovered=0.0)
    s.rows["shadow_map_indices"][1, :] = len(s.maps)
    return SkyCase(s, make_env(86, 2, 2, 2, 2), None)


def skybox_cases(oracle):
    """8 x 8: every pixel uncovered; none; a checkerboard; a basis whose rays run along an edge; one whose rays hit two corners; a
    zero basis (every direction bad)"""
    out = []
    zs, zb = fc.grid(oracle)
    d = fc.depth_of_slice(zs, zb, 3)
    depths = dict(all_uncovered=np.zeros((8, 8), F), none_uncovered=np.full((8, 8), d, F),
                  checkerboard=np.where((np.arange(8)[:, None] + np.arange(8)[None, :]) % 2 == 0, d, F(0)).astype(F))
    bases = dict(all_uncovered=IDENTITY_BASIS, none_uncovered=IDENTITY_BASIS, checkerboard=((0.5, 0.0, 0.5), (0.0, 0.7, 0.0), (0.3, 0.2, -1.0)),
                 edge_rays=((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), (1.0, 1.0, 0.0)), corner_rays=((0.0, 0.0, 8.0), (0.0, 0.0, 0.0), (1.0, 1.0, 0.0)),
                 zero_basis=((0.0,) * 3,) * 3)
    for i, (name, basis) in enumerate(bases.items()):
        rng = np.random.default_rng(90 + i)
        depth = depths.get(name, depths["checkerboard"] if name == "edge_rays" else depths["all_uncovered"])
        cx = 1
        c = fc.Case(f"skybox_{name}", depth, 8, zs, zb, seed=90 + i, lists={3 * cx * cx: [SKY, SUN, 12]}, default_lengths=(0,),
                    cluster_count=(1, 1, 12), lights=make_lights(rng), materials=make_materials(rng))
        s = sc.ShadowCase(c, sc.rows_of(sc.row(), sc.row()), sc.random_maps(rng, 4, 8))
        out.append(SkyCase(s, make_env(95 + i, 2, 2, 2, 2) if i % 2 == 0 else None, make_sky(96 + i, SKY_SIZES[i % 3], special=name == "checkerboard"),
                           skybox_lod=(0.0, 0.5, 20.0)[i % 3], basis=basis))
    return out


def tile_case(oracle):
    """one of tests/shade_tile_cases.py's 73 x 33 layouts (second trips under a capped grid, empty tiles, stale pixels), eight of
    its point lights turned into sky lights"""
    p = tc.programme(oracle, "sky_tiles_73x33", tc.MAIN_W, tc.MAIN_H, 8, tc.SHADOW_KINDS, seed=2)
    p.case.lights["light_type"][8:12] = L.LIGHT_TYPE_SKY
    rng = np.random.default_rng(99)
    return SkyCase(p.shadow, make_env(97, 8, 16, 5, 17), make_sky(98, 16), skybox_lod=0.5, basis=((1.7, 0.0, 0.2), (0.0, 1.0, 0.0), (0.1, 0.0, -1.0)),
                   ao=ao_plane(rng, tc.MAIN_H, tc.MAIN_W))


def all_cases(oracle):
    return (shape_cases(oracle) + size_cases(oracle) + [direction_case(oracle, t) for t in (8, 4)] + list_cases(oracle) + skybox_cases(oracle)
            + [tile_case(oracle), stale_map_case(oracle)])


DROP = ("form", "want_walked", "want_stats", "want_factor", "want_cascade", "want_shadow_stats", "want_sky_stats", "want_census", "over", "into")


def mirror(case, **kw):
    a, k = case.args(**kw)
    return raster.host_fragments_shade_sky(*a, **k)


def restated(case, oracle, **kw):
    a, k = case.args(**kw)
    return ref.shade(oracle, *a, **{key: v for key, v in k.items() if key not in DROP})
