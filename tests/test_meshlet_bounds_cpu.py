"""CPU checks of the geometry-bounds surface (orbit_meshlet_bounds / orbit_mesh_bounds, include/orbit_abi_ext.h): the
host export that is the GPU tests' reference reproduces what compute_meshlets already produces, the case set of
tests/meshlet_bounds_cases.py reaches every edge it claims to (a census with asserted counts), the host's result depends
on the order of the points, and the entry points validate before they touch a device."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import meshlet_bounds_cases as mc
import scenes as sc
from orbit_amd import _lib, assets, gltf
from orbit_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cube_mesh():
    pos = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    idx = np.array([0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3],
                   np.uint32)
    return pos, idx


def _assert_reproduces(meshlets, data, positions):
    """bytes 0..19 of every record == the export's bounds of the record decoded from the packed buffers"""
    full, err, _ = assets.meshlet_bounds(meshlets, data, positions, len(positions))
    assert len(full) == len(meshlets) > 0 and not err.any()
    want = meshlets.copy()
    want.view(np.uint8).reshape(-1, 32)[:, :20] = 0
    got = mc.expected_records(want, full, err, range(len(meshlets)))
    assert got.tobytes() == meshlets.tobytes()


@pytest.mark.parametrize("name", ["torus", "cube"])
def test_host_export_reproduces_compute_meshlets(name):
    pos, idx = sc.torus() if name == "torus" else _cube_mesh()
    meshlets, data = assets.compute_meshlets(pos, idx, material=3)
    _assert_reproduces(meshlets, data, pos)


def test_host_export_reproduces_the_gltf_assets_records(tmp_path):
    spec = importlib.util.spec_from_file_location("make_test_glb", os.path.join(ROOT, "tools", "make_test_glb.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    glb = str(tmp_path / "scene.glb")
    tool.write(glb, instances=4)
    d = gltf.load(glb)
    assert len(d["meshlets"]) > 100 and d["meshlets"]["vertex_offset"].max() > 0
    _assert_reproduces(d["meshlets"], d["meshlet_data"], d["vertex_positions"])


def test_the_case_set_reaches_every_edge():
    cases = mc.build_cases()
    pk = mc.Packed(cases)
    full, err, upd = pk.host(count=len(cases))
    assert not err.any()
    c = mc.census(cases, full, upd)
    for category in ("updates_0", "updates_1_plus", "updates_8_plus", "most_points_update", "degenerate_interior",
                     "degenerate_first", "degenerate_last", "degenerate_all", "zero_bounds", "wide_cone", "wide_cone_exit",
                     "zero_axis", "ties", "signed_zero", "count_1_3", "count_64_64", "count_65", "count_128", "count_255",
                     "verts_255", "denormal", "huge", "nan_first_vertex", "nan_later_vertex", "inf_vertex",
                     "neg_inf_vertex", "more_than_one_chunk"):
        assert c.get(category, 0) > 0, (category, c)
    by_name = dict(zip(pk.names, zip(full, upd)))
    # what the tags promise, on the reference's own output
    assert by_name["wide_cone"][0]["cone_cutoff_s8"] == 127 and by_name["wide_cone"][0]["radius"] > 0
    assert by_name["opposite_triangles"][0]["cone_cutoff_s8"] == 127
    for n in ("degenerate_all", "degenerate_all_collinear", "no_triangles"):
        assert not by_name[n][0].tobytes().strip(b"\0")
    assert np.isinf(by_name["huge_1e30"][0]["radius"])  # d2 overflows
    assert by_name["helix_85_slow"][1] >= 64  # many rounds in a meshlet of two chunks
    assert by_name["strip_64"][0]["cone_cutoff_s8"] < 127 and by_name["strip_255"][0]["cone_cutoff_s8"] < 127
    assert (pk.records["vertex_offset"][:pk.count] > 0).sum() > 5


def test_the_hosts_bits_depend_on_the_order_of_the_points():
    """An order-free implementation cannot pass the GPU tests: the same triangles in reverse order give another sphere."""
    name, pos, tri, tags = next(c for c in mc.build_cases() if c[0] == "helix_64")
    twins = [(name, pos, tri, tags), ("reversed", pos, tri[::-1].copy(), tags)]
    full, err, upd = mc.Packed(twins).host(count=2)
    assert not err.any() and upd.min() >= 64
    assert full[0]["center"].tobytes() + full[0]["radius"].tobytes() != full[1]["center"].tobytes() + full[1]["radius"].tobytes()


def test_host_export_applies_the_four_range_checks():
    cases = mc.build_cases()[:6]
    pk = mc.Packed(cases)
    good, _, _ = pk.host(count=6)
    # index beyond the capacity (index list); data beyond the words; vertex beyond the count; corner beyond the vertices
    full, err, _ = pk.host(indices=[0, len(pk.records), 2])
    assert err.tolist() == [0, 1, 0] and not full[1].tobytes().strip(b"\0") and full[2] == good[2]
    r = pk.records.copy()
    r[1]["data_offset"] = len(pk.meshlet_data) - 3
    full, err, _ = assets.meshlet_bounds(r, pk.meshlet_data, pk.vertices, pk.vertex_count, count=6)
    assert err.tolist() == [0, 1, 0, 0, 0, 0] and full[0] == good[0]
    full, err, _ = assets.meshlet_bounds(pk.records, pk.meshlet_data, pk.vertices, pk.vertex_count - 1, count=6)
    assert err.tolist() == [0, 0, 0, 0, 0, 1]
    d = pk.meshlet_data.copy()
    rec = pk.records[3]
    d.view(np.uint8)[(int(rec["data_offset"]) + int(rec["vertex_count"])) * 4 + 5] = rec["vertex_count"]
    full, err, _ = assets.meshlet_bounds(pk.records, d, pk.vertices, pk.vertex_count, count=6)
    assert err.tolist() == [0, 0, 0, 1, 0, 0] and full[4] == good[4]


def test_layouts_match_the_header(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "orbit_abi_ext.h"\nint main(void){return sizeof(OrbitMeshletBoundsFull)==48'
                   " && sizeof(OrbitMeshletBoundsJob)==96 && offsetof(OrbitMeshletBoundsJob,full)==32"
                   " && offsetof(OrbitMeshletBoundsJob,vertex_count)==72 && offsetof(OrbitMeshletBoundsJob,flags)==88"
                   " && offsetof(OrbitMeshletBoundsFull,cone_axis_s8)==44 && sizeof(OrbitMeshBoundsRange)==12"
                   " && ORBIT_BOUNDS_KEEP_RECORDS==1?0:1;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    assert C.sizeof(_lib.MeshletBoundsJob) == 96 and _lib.MeshletBoundsJob.flags.offset == 88
    assert L.MESHLET_BOUNDS_FULL.itemsize == 48 and L.MESH_BOUNDS_RANGE.itemsize == 12
    assert L.MESHLET_BOUNDS_FULL.fields["cone_axis_s8"][1] == 44 and _lib.BOUNDS_KEEP_RECORDS == 1


def test_entry_points_reject_a_null_context_without_a_device():
    lib = _lib.load()
    j = _lib.MeshletBoundsJob()
    assert lib.orbit_meshlet_bounds(None, C.byref(j), None) == _lib.E_INVALID
    assert lib.orbit_meshlet_bounds(None, None, None) == _lib.E_INVALID
    assert lib.orbit_mesh_bounds(None, None, 0, None, 0, 12, 0, None, 0, None) == _lib.E_INVALID
    assert lib.orbit_abi_version() == 6  # additive
