"""CPU checks of the whole scene update (orbit_scene_update, include/orbit_abi_ext.h): the descriptor table the host
mirror's update_scene_device makes, put through an independent numpy restatement of the three compactions and the
light arithmetic (tests/scene_full_ref.py), reproduces the host mirror's update_scene; the light rows at their edges;
the new layouts against the header; the entry point without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scene_full_ref as R
import scene_update_ref as RU
from orbit_amd import _lib, layouts as L
from orbit_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _mesh_infos(n, seed=3):
    mi = np.zeros(n, dtype=L.MESH_INFO)
    mi["lod_count"] = 1
    mi["mesh_lods"][:, 0, 0] = np.arange(n) * 100
    mi["mesh_lods"][:, 0, 1] = np.random.default_rng(seed).integers(1, 100, n)  # 1 .. 4 visibility words
    return mi


def test_layouts_match_the_header(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "orbit_abi_ext.h"\n'
                   "int main(void){return sizeof(OrbitSceneEntity)==48 && offsetof(OrbitSceneEntity,light_kind)==8"
                   " && offsetof(OrbitSceneEntity,light_color)==16 && offsetof(OrbitSceneEntity,light_intensity)==28"
                   " && offsetof(OrbitSceneEntity,light_param)==32 && offsetof(OrbitSceneEntity,prefiltered_map_index)==40"
                   " && sizeof(OrbitSceneCounts)==16 && sizeof(OrbitSceneUpdate)==96"
                   " && offsetof(OrbitSceneUpdate,light_data)==32 && offsetof(OrbitSceneUpdate,counts)==64"
                   " && offsetof(OrbitSceneUpdate,entity_count)==72 && offsetof(OrbitSceneUpdate,shadow_capacity)==84"
                   " && offsetof(OrbitSceneUpdate,luminance_cutoff)==88 && offsetof(OrbitSceneUpdate,shadow_index_base)==92"
                   " && ORBIT_SCENE_NONE==0xFFFFFFFFu ? 0 : 1;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    assert L.SCENE_ENTITY.itemsize == 48 and L.SCENE_COUNTS.itemsize == 16 and C.sizeof(_lib.SceneUpdate) == 96
    f = L.SCENE_ENTITY.fields
    assert (f["light_kind"][1], f["light_color"][1], f["light_intensity"][1], f["light_param"][1],
            f["prefiltered_map_index"][1]) == (8, 16, 28, 32, 40)
    u = _lib.SceneUpdate
    assert (u.light_data.offset, u.counts.offset, u.entity_count.offset, u.shadow_capacity.offset,
            u.luminance_cutoff.offset, u.shadow_index_base.offset) == (32, 64, 72, 84, 88, 92)


@pytest.mark.parametrize("mesh_pattern", R.MESH_PATTERNS)
@pytest.mark.parametrize("light_pattern", R.LIGHT_PATTERNS)
def test_table_and_restatement_reproduce_update_scene(mesh_pattern, light_pattern):
    n, frame = 777, 3
    mi = _mesh_infos(16)
    tab0, t = R.make_inputs(11, n, mesh_pattern, light_pattern, n_meshes=16)
    sd, tab = R.host_scene(tab0, t, mi)
    # the table is the input with the allocator's offsets; the transform cache is every entity's, in entity order
    for name in L.SCENE_ENTITY.names:
        if name != "visibility_offset":
            assert tab[name].tobytes() == tab0[name].tobytes(), name
    assert sd.transform_cache().tobytes() == t.tobytes()
    want = R.host_update(sd, mi, n, cutoff=0.3, frame_index=frame)
    R.assert_update_equal(R.update(tab, t, cutoff=0.3, frame_index=frame), want)
    assert want["counts"][0] == R.mesh_mask(mesh_pattern, n, 11).sum()
    if light_pattern != "none":
        kinds = set(want["lights"]["light_type"].tolist())
        assert kinds == {S.SKY, S.DIRECTIONAL, S.POINT} and want["counts"][2] > 0
        assert (want["lights"]["shadow_data_index"] != R.NONE).sum() == want["counts"][2]


def test_repeated_updates_keep_visibility_offsets_and_add_new_ones():
    mi = _mesh_infos(8)
    tab0, t = R.make_inputs(5, 300, "random90", "random3", n_meshes=8)
    sd, tab = R.host_scene(tab0, t, mi)
    first = R.host_update(sd, mi, 300)
    R.assert_update_equal(R.update(tab, t), first)
    # entities added after an update: existing offsets are kept, the new ones come behind them
    sd.add_entity(position=(1, 2, 3), mesh=5, light=dict(kind=S.DIRECTIONAL, cast_shadows=True, intensity=3.0))
    sd.add_entity(position=(4, 5, 6), light=dict(kind=S.SKY, irradiance_map_index=7, prefiltered_map_index=9))
    tab1, t1 = R.make_inputs(6, 50, "alternating", "all", n_meshes=8)
    sd.add_entities(tab1, t1)
    # an entity that loses and regains its mesh keeps its words
    drawn = int(np.flatnonzero(tab["mesh_index"] != R.NONE)[3])
    sd.set_mesh(drawn, None)
    sd.update_scene_device(mi)
    assert sd.entity_table()["mesh_index"][drawn] == R.NONE
    sd.set_mesh(drawn, 2)
    sd.update_scene_device(mi)
    tab2, t2 = sd.entity_table(), sd.transform_cache()
    assert len(tab2) == 352 and tab2["visibility_offset"][:300].tobytes() == tab["visibility_offset"].tobytes()
    used = tab["visibility_offset"][tab["mesh_index"] != R.NONE].max()
    assert (tab2["visibility_offset"][300:][tab2["mesh_index"][300:] != R.NONE] > used).all()
    for frame in (0, 1, 200):  # shadow_data_index = 256 * frame + rank
        R.assert_update_equal(R.update(tab2, t2, frame_index=frame), R.host_update(sd, mi, 352, frame_index=frame))
    # update_scene_device after update_scene changes nothing update_scene made
    before = sd.entity_draw_cache().tobytes(), sd.light_data_cache().tobytes(), sd.shadow_command_count()
    sd.update_scene_device(mi)
    assert before == (sd.entity_draw_cache().tobytes(), sd.light_data_cache().tobytes(), sd.shadow_command_count())
    assert sd.entity_table().tobytes() == tab2.tobytes()


@pytest.mark.parametrize("cutoff", [0.25, 0.0, -0.0, -1.0, 1e-40, np.inf, np.nan])
def test_light_rows_at_their_edges_equal_the_host_mirror(cutoff):
    """Intensity 0, denormal, inf, NaN; cutoff 0 and negative; non-normalised, zero and inf quaternions — every
    combination, as each of the three kinds, against the host mirror's light_gpu_data."""
    edges = R.edge_light_values()
    n = 3 * len(edges)
    tab = np.zeros(n, dtype=L.SCENE_ENTITY)
    t = RU.edge_transforms(2, n)
    tab["mesh_index"] = R.NONE
    tab["light_kind"] = np.repeat([S.SKY, S.DIRECTIONAL, S.POINT], len(edges))
    tab["light_flags"] = np.arange(n) % 2
    tab["light_color"] = np.random.default_rng(1).uniform(0, 1, (n, 3))
    tab["light_param"] = 0.5
    tab["irradiance_map_index"], tab["prefiltered_map_index"] = 11, 12
    for k in range(3):
        for j, (inten, q) in enumerate(edges):
            tab["light_intensity"][k * len(edges) + j] = inten
            t["orientation"][k * len(edges) + j] = q
    sd, tab_h = R.host_scene(tab, t, RU.ONE_MESH)
    assert tab_h.tobytes() == tab.tobytes()
    want = R.host_update(sd, RU.ONE_MESH, n, cutoff=cutoff)
    got = R.update(tab, t, cutoff=cutoff)
    R.assert_update_equal(got, want)
    assert len(want["lights"]) == n
    assert want["counts"][2] == ((tab["light_kind"] == S.DIRECTIONAL) & (tab["light_flags"] == 1)).sum() > 0
    with np.errstate(all="ignore"):  # the edges are reached: the outputs hold NaN, inf and signed zeros
        pt = want["lights"][want["lights"]["light_type"] == S.POINT]
        assert np.isnan(pt["outer_radius"]).any()
        dr = want["lights"][want["lights"]["light_type"] == S.DIRECTIONAL]
        assert np.isnan(dr["direction"]).any() and (dr["direction"] == 0).any()


def test_bulk_add_refuses_a_light_kind_that_is_none():
    tab, t = R.make_inputs(1, 4, "all", "all")
    tab["light_kind"][2] = 3
    from orbit_amd.passes import Panic

    with pytest.raises(Panic, match="light_kind is not a LightKind"):
        S.SceneData().add_entities(tab, t)


def test_entry_point_fails_loudly_without_a_device():
    lib = _lib.load()
    u = _lib.SceneUpdate()
    assert lib.orbit_scene_update(None, C.byref(u), None) == _lib.E_INVALID
    assert lib.orbit_scene_update(None, None, None) == _lib.E_INVALID
    assert b"ctx is NULL" in lib.orbit_last_error(None)
