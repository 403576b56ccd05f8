"""GPU tests of the per-block evaluation's record setup on four lanes per record (orbit_amd/csrc/meshlet_eval_blocks.hip
blk_setup: lane k of a quad computes a share, the quad exchanges, plane i goes to lane i & 3 and `inside` is ANDed over the
quad; plane norms once per workgroup).  Every case is a few tiles on one workgroup (orbit_ctx_set_block_cull_grid), culled
with the path on and off and compared byte for byte with the oracle (both_ways); what a case is meant to reach is asserted
on the host first, from the BlockRecords the host's quad form derives (orbit_host_block_record)."""
import numpy as np
import pytest

import scenes as sc
from orbit_amd import layouts as L
from test_block_cull_gpu import both_ways, engine, far_camera, info  # noqa: F401
from test_block_pipeline_gpu import capped, dispatched  # noqa: F401
from test_block_pretest_cpu import F, bounds_of, slab_scale
from test_block_setup_quad_cpu import icosahedron_planes, records
from test_gpu_parity import torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

SPARSE, INSIDE = 1, 2


def host_flags(scene, view, planes, recs, alone=False, part=32):
    """The flags blk_setup derives on the device for each part of `part` (the dispatch size) / 32 parts per dispatched
    record, in tile order, from the host's quad form: -> flags[n_parts] (a part without meshlets: SPARSE alone, as the
    device sets it); alone=True: -> [n_planes, n_parts] `inside` under plane i alone.  The slab's affine flag is ROW-wide
    (setup_write ANDs it over the eight lanes of a row), so a record is affine here only if its row's other record is
    too — and a part without meshlets, whose matrix is all zeros, is not: a record beside one is dense."""
    model = scene.entities["model_matrix"].reshape(-1, 4, 4).transpose(0, 2, 1).astype(F)
    view = np.asarray(view, dtype=F)
    vm = np.zeros_like(model)
    for k in range(4):  # mat4_mul_col: term by term in binary32
        vm = (vm + view[None, :, k, None] * model[:, None, k, :]).astype(F)
    per = part // 32
    ent = np.repeat(recs["entity_index"], per)
    off = np.repeat(recs["meshlet_offset"], per) + np.tile(np.arange(per) * 32, len(recs))
    cnt = np.clip(np.repeat(recs["meshlet_count"].astype(np.int64), per) - np.tile(np.arange(per) * 32, len(recs)), 0, 32)
    assert (off % 32 == 0).all() and ((cnt == 32) | (cnt == 0)).all()
    none = cnt == 0
    cols = np.ascontiguousarray(vm.transpose(0, 2, 1)).reshape(-1, 16)[ent]
    with np.errstate(invalid="ignore"):
        own = (cols[:, 3] == 0) & (cols[:, 7] == 0) & (cols[:, 11] == 0) & (cols[:, 15] == 1) & \
            (cols[:, 12:15] * F(0) == 0).all(1) & ~none
    padded = np.zeros(len(own) + (len(own) & 1), dtype=bool)  # (a last record without a partner: beside no record)
    padded[:len(own)] = own
    affine = np.repeat(padded.reshape(-1, 2).all(1), 2)[:len(own)]
    bnd = bounds_of(scene.meshlets["bounding_sphere"])[np.where(none, 0, off // 32)]
    planes = np.ascontiguousarray(planes, dtype=F).reshape(-1, 4)
    if alone:
        return np.stack([(records(cols, affine, slab_scale(cols), bnd, planes[i:i + 1], -1.0, 1)["flags"] & INSIDE) != 0
                         for i in range(len(planes))]) & ~none
    return np.where(none, SPARSE, records(cols, affine, slab_scale(cols), bnd, planes, -1.0, 1)["flags"])


def row_sparse(flags):
    """-> per row of two parts (tiles padded with parts without meshlets): both SPARSE — what the row word holds."""
    n = (len(flags) + 15) // 16 * 16
    f = np.full(n, SPARSE, dtype=np.uint32)
    f[:len(flags)] = flags
    return ((f & SPARSE) != 0).reshape(-1, 2).all(1)


def small_scene(seed, n):
    """n entities of one 32-meshlet mesh each, in draw order: record r is entity r's."""
    return sc.make_scene(seed, n, meshlets_per_mesh=(32, 32), n_materials=3, shuffle=False, unit_scale=True,
                         mesh_radius=(0.5, 1.0))


@pytest.mark.parametrize("n_planes", [1, 4, 5, 6, 12])
def test_plane_counts(torch_mod, engine, capped, oracle, n_planes):  # noqa: F811
    """1, 4, 5, 6 and 12 cull planes — the edges of the rounds of plane i -> lane i & 3, and the ABI's maximum —, tangent
    to a sphere of radius 12 around the scene's middle, so they cut through it; entity i < n sits on plane i, 63 degrees
    or more from every other plane's normal: its record is sparse and not inside because of plane i alone."""
    scene = small_scene(400 + n_planes, 96)
    cam = far_camera()
    view = np.asarray(cam.view, dtype=np.float64)
    mid_view = view[:3, :3] @ np.zeros(3) + view[:3, 3]
    pl = icosahedron_planes(n_planes, 12.0).astype(np.float64)
    pl[:, 3] -= pl[:, :3] @ mid_view  # n . (p - mid) + 12
    planes = pl.astype(F)
    at = (-pl[:, :3] * 12.0) @ view[:3, :3]  # world = R^T (view position - t), and mid is world's origin
    scene.entities["model_matrix"][:n_planes, 12:15] = at.astype(F)  # column-major: the translation
    ci = sc.make_cull_info(cam.view, planes, alpha_mode_flag=L.ALPHA_ALL)
    recs = dispatched(oracle, scene, ci)
    flags = host_flags(scene, cam.view, planes, recs)
    alone = host_flags(scene, cam.view, planes, recs, alone=True)
    sparse = (flags & SPARSE) != 0
    # (a last record without a row partner is dense: host_flags)
    assert sparse[:len(recs) & ~1].all() and 16 < len(recs) <= 96
    assert ((flags & INSIDE) != 0).sum() >= 4, "and some records inside every plane"
    for i in range(n_planes):
        only = sparse & ~alone[i] & np.delete(alone, i, axis=0).all(0)
        assert only.any(), f"no sparse record is outside plane {i} alone"
        assert i in recs["entity_index"][only]
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


@pytest.mark.parametrize("n_records", [1, 3, 4, 5, 16, 17])
def test_record_counts(torch_mod, engine, capped, oracle, n_records):  # noqa: F811
    """Quads without a record beside quads with one (1, 3, 5), one full group of four (4), a whole tile (16) and a tile
    plus one record (17); every record with a row partner is sparse, a last one without is dense (the row-wide affine
    flag), so 1, 3, 5 and 17 end in a dense row followed by rows without records."""
    scene = small_scene(500 + n_records, n_records)
    cam = far_camera()
    ci = info(cam)
    recs = dispatched(oracle, scene, ci)
    assert len(recs) == n_records
    sparse = (host_flags(scene, cam.view, cam.planes, recs) & SPARSE) != 0
    assert sparse[:n_records & ~1].all() and not sparse[n_records & ~1:].any()
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


def test_empty_records_between_sparse_ones(torch_mod, oracle):  # noqa: F811
    """At a dispatch size of 128 a record of 64 meshlets is split into two full parts and two EMPTY ones (meshlet_count
    0): the rows of a tile are in turn (sparse, sparse) and (no record, no record), which must stay an all-sparse tile."""
    from orbit_amd.engine import Engine

    scene = sc.make_scene(520, 11, meshlets_per_mesh=(64, 64), n_materials=3, shuffle=False, unit_scale=True,
                          mesh_radius=(0.5, 1.0))  # 44 parts: two tiles and three quarters
    cam = far_camera()
    ci = info(cam)
    eng = Engine(0, max_entities=50_000, max_dispatches=400_000, max_draws=1_000_000, dispatch_size=128)
    try:
        with oracle.dispatch_size(128):
            recs = dispatched(oracle, scene, ci)
            assert len(recs) == 11 and (recs["meshlet_count"] == 64).all(), "each record's second half is empty"
            flags = host_flags(scene, cam.view, cam.planes, recs, part=128)
            assert len(flags) == 44 and (flags[np.arange(44) % 4 < 2] & SPARSE).all() and (flags[np.arange(44) % 4 >= 2] == SPARSE).all()
            assert row_sparse(flags).all()
            eng.set_block_cull_grid(1)
            both_ways(torch_mod, eng, oracle, scene, ci)
    finally:
        eng.close()


@pytest.mark.parametrize("reason", ["near", "bound"])
def test_mixed_rows(torch_mod, engine, capped, oracle, reason):  # noqa: F811
    """A row whose two records differ, for a reason of the one record alone: record 5 (second of its row) and record 10
    (first of its row) are dense — too near the camera for their size (D <= 8 Rc'), or with a block bound that is not
    valid (a negative radius) — while their row partners 4 and 11 are sparse (affine, the row-wide flag included), and so
    are the quads on both sides.  Rows 2 and 5 are dense, every other row of the tile is sparse: the row word is held to
    account for BOTH records of a row, either one first."""
    scene = small_scene(560, 33)
    cam = far_camera()
    ci = info(cam)
    dense = (5, 10)
    if reason == "near":
        for e in dense:  # two units in front of the camera
            scene.entities["model_matrix"][e, 12:15] = (0.0, 2.0, 598.0)
    else:
        for e in dense:
            scene.meshlets["bounding_sphere"][32 * e + 7, 3] = -1.0
    recs = dispatched(oracle, scene, ci)
    assert np.array_equal(recs["entity_index"], np.arange(33)) and np.array_equal(recs["meshlet_offset"], 32 * np.arange(33))
    flags = host_flags(scene, cam.view, cam.planes, recs)
    sparse = (flags & SPARSE) != 0
    assert np.array_equal(np.flatnonzero(~sparse), [5, 10, 32]), "(32: the last record, beside no record)"
    rows = row_sparse(flags)
    assert np.array_equal(np.flatnonzero(~rows), [2, 5, 16])
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


@pytest.mark.parametrize("dense", [(5, 10), (0, 15), (3, 4, 16)], ids=["5-10", "0-15", "3-4-16"])
def test_projective_records_among_sparse_ones(torch_mod, engine, capped, oracle, dense):  # noqa: F811
    """Records under a slightly projective matrix (w = 1 + x / 1000, as handover_scene makes them) stay dense inside
    otherwise all-sparse tiles.  The slab's affine flag is row-wide, so the record beside a projective one is dense too
    (test_mixed_rows has the rows whose records differ); the rows on both sides are sparse; 3 and 4 are the neighbouring
    halves of two rows, 16 the first record of the second tile."""
    scene = small_scene(540, 33)
    cam = far_camera()
    ci = info(cam)
    recs = dispatched(oracle, scene, ci)
    for e in dense:
        scene.entities["model_matrix"][e][3] = 1e-3
    assert np.array_equal(dispatched(oracle, scene, ci), recs) and np.array_equal(recs["entity_index"], np.arange(33))
    sparse = (host_flags(scene, cam.view, cam.planes, recs) & SPARSE) != 0
    assert np.array_equal(np.flatnonzero(~sparse), sorted({e for d in dense for e in (d, d ^ 1)} | {32}))
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)
