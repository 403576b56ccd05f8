"""CPU checks of the scene update (orbit_scene_update_entities, include/orbit_abi_ext.h): the 40-B transform layout, an
independent numpy restatement of the pin against the host mirror's update_scene, the host mirror's deferred update
(transform cache, instance indices), and a loud failure without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scene_update_ref as R
from orbit_amd import _lib, layouts as L
from orbit_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entity_transform_layout(tmp_path):
    assert L.ENTITY_TRANSFORM.itemsize == 40
    assert [L.ENTITY_TRANSFORM.fields[f][1] for f in ("position", "orientation", "scale")] == [0, 12, 28]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "orbit_abi_ext.h"\n'
                   "int main(void){return sizeof(OrbitEntityTransform)==40 && offsetof(OrbitEntityTransform,orientation)==12"
                   " && offsetof(OrbitEntityTransform,scale)==28 ? 0 : 1;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


@pytest.mark.parametrize("seed,n", [(1, 2000), (2, 257), (3, 64)])
def test_numpy_restatement_equals_host_update_scene(seed, n):
    t = R.edge_transforms(seed, n)
    R.assert_rows_equal(R.entity_rows(t), R.host_rows(t))


def test_numpy_restatement_of_ordinary_transforms_is_byte_exact():
    rng = np.random.default_rng(7)
    t = np.zeros(500, dtype=L.ENTITY_TRANSFORM)
    t["position"] = rng.uniform(-50, 50, (500, 3))
    q = rng.normal(size=(500, 4))
    t["orientation"] = q / np.linalg.norm(q, axis=1, keepdims=True)
    t["scale"] = rng.uniform(0.5, 2.0, (500, 3))
    assert R.entity_rows(t).tobytes() == R.host_rows(t).tobytes()


def _scene_with_lights(seed, n=400):
    rng = np.random.default_rng(seed)
    mesh_infos = np.zeros(5, dtype=L.MESH_INFO)
    mesh_infos["lod_count"] = 1
    mesh_infos["mesh_lods"][:, 0, 1] = rng.integers(1, 120, 5)
    sd = S.SceneData()
    kinds = [None, None, None, dict(kind=S.POINT, intensity=3.0),
             dict(kind=S.DIRECTIONAL, cast_shadows=True), dict(kind=S.SKY)]
    for i in range(n):
        q = rng.normal(size=4)
        sd.add_entity(position=rng.uniform(-20, 20, 3), orientation=q / np.linalg.norm(q), scale=rng.uniform(0.5, 2, 3),
                      mesh=int(rng.integers(5)) if rng.random() < 0.8 else None, light=kinds[i % len(kinds)],
                      name=f"e{i}" if i % 7 == 0 else None)
    return sd, mesh_infos


def test_update_deferred_matches_update_scene_except_entity_data():
    a, mi = _scene_with_lights(3)
    b, _ = _scene_with_lights(3)
    for frame in (0, 1):  # the second frame reuses the visibility ranges of the first
        a.update_scene(mi, luminance_cutoff=0.3, frame_index=frame)
        b.update_scene_deferred(mi, luminance_cutoff=0.3, frame_index=frame)
        assert a.entity_draw_cache().tobytes() == b.entity_draw_cache().tobytes()
        assert a.light_data_cache().tobytes() == b.light_data_cache().tobytes()
        assert a.shadow_command_count() == b.shadow_command_count() > 0
        assert len(b.entity_data_cache()) == 0 and len(a.transform_cache()) == 0
        # the transforms the device turns into a's entity data
        t = b.transform_cache()
        assert len(t) == len(a.entity_data_cache()) > 0
        assert R.entity_rows(t).tobytes() == a.entity_data_cache().tobytes()


def test_transform_cache_is_in_instance_order_and_instance_index_maps():
    sd = S.SceneData()
    meshes = [0, None, 0, 0, None, 0]
    for i, m in enumerate(meshes):
        sd.add_entity(position=(i, 2 * i, -i), orientation=(0, 0, 0, 1), scale=(1 + i, 1, 1), mesh=m)
    assert sd.instance_index(0) == -1  # no update yet
    sd.update_scene_deferred(R.ONE_MESH)
    assert [sd.instance_index(e) for e in range(len(meshes))] == [0, -1, 1, 2, -1, 3]
    assert sd.instance_index(len(meshes)) == -1 and sd.instance_index(10 ** 9) == -1
    t = sd.transform_cache()
    assert t["position"][:, 0].tolist() == [0, 2, 3, 5] and t["scale"][:, 0].tolist() == [1, 3, 4, 6]
    assert (t["orientation"] == (0, 0, 0, 1)).all()
    # a moved entity: its new transform lands in its row at the next update; its index is how a dirty list is built
    sd.set_transform(3, (7, 8, 9), (0, 0, 1, 0), (2, 2, 2))
    sd.update_scene_deferred(R.ONE_MESH)
    row = sd.transform_cache()[sd.instance_index(3)]
    assert row["position"].tolist() == [7, 8, 9] and row["orientation"].tolist() == [0, 0, 1, 0]
    sd.add_entity(position=(1, 1, 1), mesh=0)
    assert sd.instance_index(len(meshes)) == -1  # added since the latest update
    sd.update_scene(R.ONE_MESH)  # update_scene records the indices too
    assert sd.instance_index(len(meshes)) == 4


def test_scene_update_entry_point_fails_loudly_without_a_device():
    import torch

    lib = _lib.load()
    t = np.zeros(4, dtype=L.ENTITY_TRANSFORM)
    out = np.zeros(4, dtype=L.ENTITY_DATA)
    rc = lib.orbit_scene_update_entities(None, t.ctypes.data_as(C.c_void_p), None, 4, out.ctypes.data_as(C.c_void_p), 4,
                                         None)
    assert rc == _lib.E_INVALID and b"ctx is NULL" in lib.orbit_last_error(None)
    assert lib.orbit_scene_update_entities(None, None, None, 0, None, 0, None) == _lib.E_INVALID
    assert not out.view(np.uint8).any()  # nothing was computed on the host instead
    if not torch.cuda.is_available():  # and no context to call it with
        from orbit_amd.engine import Engine

        with pytest.raises(_lib.OrbitError):
            Engine(0)
