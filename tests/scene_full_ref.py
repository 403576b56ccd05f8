"""Inputs and an independent restatement for orbit_scene_update (include/orbit_abi_ext.h).

`update` restates SceneData::update_scene (src/scene.rs:404-492; the host mirror's orbit_scene.cpp) over the arrays the
device reads — one layouts.SCENE_ENTITY and one layouts.ENTITY_TRANSFORM per entity, in entity order — in numpy: the
three compactions are boolean masks with cumsum ranks, the EntityData rows are scene_update_ref.entity_rows, the light
rows restate EntityData::light_gpu_data in float32, product by product in the host's association (quat_mul_vec3 with
its zero products kept; sqrt of a float32 quotient, both correctly rounded in numpy).
"""
import numpy as np

import scene_update_ref as RU
from orbit_amd import layouts as L
from orbit_amd import scene as S

F = np.float32
NONE = 0xFFFFFFFF
MAX_SHADOW_COMMANDS = 256  # shadow_renderer.rs:204

MESH_PATTERNS = ("all", "none", "alternating", "wave_last", "group_first", "random90")
LIGHT_PATTERNS = ("none", "all", "random3")


def mesh_mask(pattern, n, seed=0):
    i = np.arange(n)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "alternating":
        return i % 2 == 0
    if pattern == "wave_last":  # only the last lane of each wave of 64
        return i % 64 == 63
    if pattern == "group_first":  # only the first lane of each workgroup of 256
        return i % 256 == 0
    assert pattern == "random90"
    return np.random.default_rng(seed).random(n) < 0.9


def light_mask(pattern, n, seed=0):
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "all":
        return np.ones(n, bool)
    assert pattern == "random3"
    return np.random.default_rng(seed + 1).random(n) < 0.03


def edge_light_values():
    """(intensity, orientation) pairs at the edges: zero, denormal, inf and NaN intensities; non-normalised, zero,
    inf-bearing and signed-zero quaternions."""
    intensities = [0.0, -0.0, 1e-40, 1e-45, np.inf, np.nan, 1.0, 3.0e38, -1.0, 2.5e-39]
    quats = [(0, 0, 0, 1), (0, 0, 0, 0), (-0.0, 0.0, -0.0, -1.0), (3.0, -2.0, 0.5, 4.0), (np.inf, 0, 0, 1),
             (0, -np.inf, 0, 0), (1, 2, 3, np.inf), (np.nan, 0, 0, 1), (1e-30, 1e-30, 1e-30, 1e-30), (1e20, 1e20, 0, 1e20)]
    return [(F(i), np.asarray(q, F)) for i in intensities for q in quats]


def make_inputs(seed, n, mesh_pattern, light_pattern, n_meshes=1, edges=True):
    """(table, transforms) of n entities: layouts.SCENE_ENTITY with visibility_offset left 0 (the host allocator's to
    fill: SceneData.update_scene_device) and layouts.ENTITY_TRANSFORM.  Lights mix the three kinds; directional lights
    at the wave and workgroup boundaries (entities 63, 64, 255, 256, ... where they carry a light) cast shadows, a few
    others at random do."""
    rng = np.random.default_rng(seed)
    t = RU.edge_transforms(seed, n)
    tab = np.zeros(n, dtype=L.SCENE_ENTITY)
    m = mesh_mask(mesh_pattern, n, seed)
    tab["mesh_index"] = np.where(m, rng.integers(0, n_meshes, n), NONE)
    lm = light_mask(light_pattern, n, seed)
    kind = rng.integers(0, 3, n).astype(np.uint32)
    cast = rng.random(n) < 0.1
    i = np.arange(n)
    boundary = np.isin(i % 256, (0, 63, 64, 127, 128, 191, 192, 255))
    kind[boundary] = S.DIRECTIONAL
    cast |= boundary
    tab["light_kind"] = np.where(lm, kind, NONE)
    tab["light_flags"] = np.where(lm & cast, 1, 0)
    tab["light_color"] = np.where(lm[:, None], rng.uniform(0, 1, (n, 3)), 0).astype(F)
    tab["light_intensity"] = np.where(lm, rng.uniform(0.1, 50, n), 0).astype(F)
    tab["light_param"] = np.where(lm, rng.uniform(0.0, 1.0, n), 0).astype(F)
    tab["irradiance_map_index"] = np.where(lm, rng.integers(0, 1 << 20, n), 0)
    tab["prefiltered_map_index"] = np.where(lm, rng.integers(0, 1 << 20, n), 0)
    if edges:  # edge intensities and orientations on the first lights that are not at a boundary
        lit = np.flatnonzero(lm & ~boundary)
        for e, (inten, q) in zip(lit, edge_light_values()):
            tab["light_intensity"][e] = inten
            t["orientation"][e] = q
    return tab, t


def host_scene(tab, t, mesh_infos):
    """The host mirror holding these entities, and the table with the allocator's visibility offsets."""
    sd = S.SceneData()
    sd.add_entities(tab, t)
    sd.update_scene_device(mesh_infos)
    return sd, sd.entity_table()


def quat_mul_vec3(q, v):
    """glam Quat::mul_vec3 as the host mirror writes it; q (n, 4) xyzw, v (3,)."""
    with np.errstate(all="ignore"):
        bx, by, bz, w = (q[:, k].astype(F) for k in range(4))
        vx, vy, vz = (np.full(len(q), c, F) for c in v)
        b2 = bx * bx + by * by + bz * bz
        vb = (vx * bx + vy * by + vz * bz) * F(2)
        cx, cy, cz = by * vz - vy * bz, bz * vx - vz * bx, bx * vy - by * vx
        s, w2 = w * w - b2, w * F(2)
        return np.stack([vx * s + bx * vb + cx * w2, vy * s + by * vb + cy * w2, vz * s + bz * vb + cz * w2], axis=1)


def light_rows(tab, t, cutoff):
    """layouts.LIGHT rows (shadow_data_index NONE) of light-bearing descriptors and their transforms."""
    out = np.zeros(len(tab), dtype=L.LIGHT)
    kind = tab["light_kind"]
    out["light_type"] = kind
    out["shadow_data_index"] = NONE
    out["color"] = tab["light_color"]
    out["intensity"] = tab["light_intensity"]
    sky, dr, pt = kind == S.SKY, kind == S.DIRECTIONAL, kind == S.POINT
    out["irradiance_map_index"][sky] = tab["irradiance_map_index"][sky]
    out["prefiltered_map_index"][sky] = tab["prefiltered_map_index"][sky]
    out["direction"][dr] = -quat_mul_vec3(t["orientation"][dr], (0.0, 0.0, -1.0))
    out["inner_radius"][dr | pt] = tab["light_param"][dr | pt]
    out["position"][pt] = t["position"][pt]
    with np.errstate(all="ignore"):
        out["outer_radius"][pt] = np.sqrt(tab["light_intensity"][pt] / F(cutoff))
    return out


def update(tab, t, cutoff=0.25, frame_index=0):
    """dict(rows, draws, lights, shadow_orientations, instance_of_entity, light_of_entity, counts) of update_scene."""
    tab = np.ascontiguousarray(tab, dtype=L.SCENE_ENTITY)
    t = np.ascontiguousarray(t, dtype=L.ENTITY_TRANSFORM)
    n = len(tab)
    mesh = tab["mesh_index"] != NONE
    light = tab["light_kind"] <= 2
    shadow = (tab["light_kind"] == S.DIRECTIONAL) & ((tab["light_flags"] & 1) != 0)
    rank = lambda m: (np.cumsum(m) - m).astype(np.uint32)  # noqa: E731  exclusive
    draws = np.zeros(int(mesh.sum()), dtype=L.ENTITY_DRAW)
    draws["entity_index"] = np.arange(len(draws))
    draws["mesh_index"] = tab["mesh_index"][mesh]
    draws["visibility_offset"] = tab["visibility_offset"][mesh]
    lights = light_rows(tab[light], t[light], cutoff)
    sidx = (np.uint64(MAX_SHADOW_COMMANDS * frame_index) + rank(shadow)[light].astype(np.uint64)).astype(np.uint32)
    lights["shadow_data_index"] = np.where(shadow[light], sidx, NONE)
    return dict(rows=RU.entity_rows(t[mesh]), draws=draws, lights=lights,
                shadow_orientations=t["orientation"][shadow].copy(),
                instance_of_entity=np.where(mesh, rank(mesh), NONE).astype(np.uint32),
                light_of_entity=np.where(light, rank(light), NONE).astype(np.uint32),
                counts=np.array([mesh.sum(), light.sum(), shadow.sum(), n], dtype=np.uint32))


def host_update(sd, mesh_infos, n, cutoff=0.25, frame_index=0):
    """The same dict out of the host mirror's update_scene on `sd` (the pin)."""
    sd.update_scene(mesh_infos, luminance_cutoff=cutoff, frame_index=frame_index)
    inst = np.array([sd.instance_index(e) for e in range(n)], dtype=np.int64)
    lidx = np.array([sd.light_index(e) for e in range(n)], dtype=np.int64)
    draws, lights = sd.entity_draw_cache(), sd.light_data_cache()
    so = sd.shadow_orientations()
    return dict(rows=sd.entity_data_cache(), draws=draws, lights=lights, shadow_orientations=so,
                instance_of_entity=np.where(inst < 0, NONE, inst).astype(np.uint32),
                light_of_entity=np.where(lidx < 0, NONE, lidx).astype(np.uint32),
                counts=np.array([len(draws), len(lights), len(so), n], dtype=np.uint32))


def assert_words_equal(got, want, what):
    """Float words: bit-exact where the expected lane is not NaN, NaN only where it is (x86's default NaN has its sign
    bit set, gfx950's does not).  `got` / `want`: arrays of the same bytes length, compared as 32-bit words."""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1).view(np.uint32)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1).view(np.uint32)
    assert g.shape == w.shape, f"{what}: {g.shape} words vs {w.shape}"
    wn, gn = np.isnan(w.view(F)), np.isnan(g.view(F))
    bad = np.flatnonzero(np.where(wn, ~gn, g != w))
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at word {bad[0]}: {g[bad[0]]:#x} vs {w[bad[0]]:#x}"


# the float fields of a LightData row (words 4..15); words 0..3 are integers and compare as bits
def assert_lights_equal(got, want, what="light rows"):
    g = np.ascontiguousarray(got, dtype=L.LIGHT).view(np.uint32).reshape(-1, 16)
    w = np.ascontiguousarray(want, dtype=L.LIGHT).view(np.uint32).reshape(-1, 16)
    assert g.shape == w.shape, f"{what}: {len(g)} rows vs {len(w)}"
    assert np.array_equal(g[:, :4], w[:, :4]), f"{what}: integer words differ at rows {np.flatnonzero((g[:, :4] != w[:, :4]).any(axis=1))[:8]}"
    assert_words_equal(g[:, 4:].copy(), w[:, 4:].copy(), what)


def assert_update_equal(got, want):
    """Two dicts of `update` / `host_update` / a device run."""
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    RU.assert_rows_equal(got["rows"], want["rows"])
    assert got["draws"].tobytes() == want["draws"].tobytes(), "draws differ"
    assert_lights_equal(got["lights"], want["lights"])
    assert_words_equal(got["shadow_orientations"], want["shadow_orientations"], "shadow orientations")
    assert np.array_equal(got["instance_of_entity"], want["instance_of_entity"]), "instance map differs"
    assert np.array_equal(got["light_of_entity"], want["light_of_entity"]), "light map differs"
