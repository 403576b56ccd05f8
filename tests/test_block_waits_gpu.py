"""GPU tests of the per-block evaluation's steady-state arm (orbit_amd/csrc/meshlet_eval_blocks.hip): an all-sparse tile
followed by an all-sparse tile runs its eight rows in a copy of its own, with the setup loads of the tile after the next
issued ahead of the next tile's eight cone loads, and the class planes are selected between two pointer VALUES
(meshlet_common.h setup_load_cls).  Reached here are the ways into and out of that arm, a wave's last tiles, launches of a
few records, mid-tile flushes inside the arm, and both words of both class planes — with a few hundred records, by capping
the launch's grid (tests/test_block_pipeline_gpu.py: under a cap of c workgroups wave w of 4 c takes tiles w, w + 4 c, ...).
Every case is culled with the path on and off and compared byte for byte with the oracle (both_ways), the path must have
been taken, and the tile sequences and candidate counts are asserted on the host before the GPU runs."""
import numpy as np
import pytest

import scenes as sc
from orbit_amd import layouts as L
from test_block_cull_gpu import both_ways, engine, far_camera, info, sparse_share  # noqa: F401
from test_block_pipeline_gpu import (RECS, capped, dispatched, handover_scene, record_sparse_flags, tile_kinds,  # noqa: F401
                                     wave_sequences)
from test_gpu_parity import GpuScene, _expected_visible_records, host, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu


def steady_scene(oracle):
    """handover_scene with two more wholly dense tiles, 16 and 25 (their entities under the same slightly projective
    matrix): behind two all-sparse tiles of wave 0 under a cap of 1 (tiles 8, 12, 16) and of wave 1 under a cap of 2 (tiles
    9, 17, 25), so that the steady arm is also left into a dense tile."""
    scene, cam = handover_scene(oracle)
    recs = dispatched(oracle, scene, info(cam))
    for t in (16, 25):
        for e in set(recs["entity_index"][RECS * t:RECS * t + RECS].tolist()):
            scene.entities["model_matrix"][e][3] = 1e-3
    assert np.array_equal(dispatched(oracle, scene, info(cam)), recs), "the entity stage must dispatch the same records"
    return scene, cam


@pytest.mark.parametrize("cap", [1, 2])
def test_in_and_out_of_the_steady_arm(torch_mod, engine, capped, oracle, cap):  # noqa: F811
    """4 and 8 waves over 75 tiles.  Some wave runs the arm twice in a row (SSS), enters it from a mixed and from a dense
    tile (MSS, DSS), leaves it through the other arm of the same branch into a mixed and into a dense tile (SSM, SSD), and
    ends on an all-sparse tile behind an all-sparse one: the tile past a wave's last counts as all-sparse, so the arm runs
    there with eight loads that read nothing."""
    scene, cam = steady_scene(oracle)
    ci = info(cam)
    kinds = tile_kinds(record_sparse_flags(scene, cam, dispatched(oracle, scene, ci)))
    assert len(kinds) == 75
    seqs = wave_sequences(kinds, cap)
    for h in ("SSS", "MSS", "DSS", "SSM", "SSD"):
        assert any(h in s for s in seqs), f"no wave passes through {h} under a cap of {cap}: {seqs}"
    assert any(s.endswith("SS") for s in seqs), seqs
    capped(cap)
    both_ways(torch_mod, engine, oracle, scene, ci)


@pytest.mark.parametrize("records", [1, 16, 17, 33, 65, 81])
def test_short_launches(torch_mod, engine, capped, oracle, records):  # noqa: F811
    """One workgroup of four waves over 1 / 1 / 2 / 3 / 5 / 6 all-sparse tiles: a wave with one tile (the ramp straight
    into the steady arm, whose loads read nothing), waves with none, a wave with two (65, 81: tiles 0 and 4), and a last
    tile that holds a single record (17, 33, 65, 81)."""
    scene = sc.make_scene(500 + records, records, meshlets_per_mesh=(32, 32), n_materials=3, shuffle=False)
    cam = far_camera()
    ci = info(cam)
    recs = dispatched(oracle, scene, ci)
    assert len(recs) == records
    kinds = tile_kinds(record_sparse_flags(scene, cam, recs))
    assert kinds == "S" * ((records + RECS - 1) // RECS), "these scenes are meant to take the whole-tile path"
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


def _tile(rows01, rows23, rest=0):
    """Open lanes of a tile's 16 records: `rows01` over records 0-3 (rows 0 and 1), `rows23` over records 4-7, `rest` over
    the other eight, each filled from its first record on."""
    fill = lambda total, n: [min(32, max(0, total - 32 * r)) for r in range(n)]  # noqa: E731
    return fill(rows01, 4) + fill(rows23, 4) + fill(rest, 8)


# under a cap of 1 wave w takes tiles w, w + 4, w + 8: the columns
_FLUSH_TILES = [_tile(64, 64, 39), _tile(128, 64), _tile(65, 63, 7), _tile(20, 19),   # tiles 0-3
                _tile(0, 0), _tile(0, 0), _tile(0, 0), _tile(20, 19),                 # tiles 4-7: none behind a flushing tile
                _tile(96, 100, 256), _tile(0, 0), _tile(128, 128, 256), _tile(20, 19)]  # tiles 8-11


def test_mid_tile_flushes_inside_the_steady_arm(torch_mod, engine, capped, oracle):  # noqa: F811
    """Twelve all-sparse tiles on four waves, each wave in the steady arm from its first tile on.  Wave 0: a tile with
    exactly 64 candidates behind rows 0-1 and 64 more behind rows 2-3 (a flush at both mid-tile checks, 39 left for the
    end), then a tile with none (the end-of-tile flush loop does not run), then one that flushes at both checks again with
    candidates left over at each.  Wave 1: two flushes at the first check and one at the second, then two tiles with none.
    Wave 2: 65 and 63 (one candidate waits for the second check), none, then every lane.  Wave 3: the benchmark's 39 per
    tile throughout.

    The counts are set cone by cone (test_block_cull_gpu._cone_scene) and asserted through the host pre-test.  A camera
    distance alone does not give them: bench.py's generator at a 32nd of its extent leaves at most a quarter of the lanes
    open at every distance at which its records are still sparse (about 20 candidates behind rows 0-1)."""
    from test_block_cull_gpu import _cone_scene

    open_lanes = [k for t in _FLUSH_TILES for k in t]
    scene = _cone_scene(open_lanes)
    cam = sc.default_camera(position=(0.0, 0.0, 900.0))
    share, counts = sparse_share(scene, cam)
    assert share == 1.0 and list(counts) == open_lanes, "the scene must queue exactly these candidates"
    per = counts.reshape(12, RECS)
    for t in (0, 1, 2, 8, 10):
        first = int(per[t, :4].sum())
        assert first >= 64 and first % 64 + int(per[t, 4:8].sum()) >= 64, (t, per[t])
    assert [int(per[t].sum()) for t in (4, 5, 6, 9)] == [0, 0, 0, 0]
    ci = info(cam)
    recs = dispatched(oracle, scene, ci)
    assert len(recs) == 12 * RECS and tile_kinds(record_sparse_flags(scene, cam, recs)) == "S" * 12
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


def _class_scene():
    """300 entities over 300 meshes of 33-70 meshlets: every mesh but the first starts off a multiple of 32 (both words of
    both planes are read and the record's shift matters), three materials of the three alpha modes."""
    scene = sc.make_scene(61, 300, meshlets_per_mesh=(33, 70), n_materials=3)
    scene.materials["alpha_mode"] = (0, 1, 2)
    offs = scene.mesh_infos["mesh_lods"][:, 0, 0]
    assert (offs % 32 != 0).sum() > 250 and len(set((offs % 32).tolist())) > 20
    assert set(scene.meshlets["material_index"].tolist()) == {0, 1, 2}
    return scene


@pytest.mark.parametrize("flag", [L.ALPHA_OPAQUE | L.ALPHA_MASKED, L.ALPHA_ALL, L.ALPHA_ALL & ~L.ALPHA_OPAQUE],
                         ids=["opaque-masked", "all", "not-opaque"])
def test_class_planes_through_meshlet_cull(torch_mod, engine, capped, oracle, flag):  # noqa: F811
    """orbit_meshlet_cull with alpha classes from records at every offset inside a block, with the per-block kernel and
    with the per-meshlet one (both_ways), under alpha flags that keep two, three and the other two of the three modes; and
    over a stream that ends inside the buffer, where a record outside the stream stands beside one inside (it reads the
    zero page for its class words): lists and status the same with the path on and off."""
    torch = torch_mod
    scene = _class_scene()
    cam = far_camera(z=300.0)
    ci = sc.make_cull_info(cam.view, cam.planes, alpha_mode_flag=flag)
    capped(1)
    both_ways(torch, engine, oracle, scene, ci)
    from orbit_amd import _lib
    from test_gpu_parity import run_gpu

    gs = GpuScene(torch, scene)
    short = len(scene.meshlets) - 700
    ms = engine.meshlet_stream(gs.meshlets, 0, short)
    ms.set_materials(gs.materials, len(scene.materials))
    engine.bind_meshlet_stream(ms)
    torch.cuda.synchronize()
    out = []
    for on in (True, False):
        engine.set_block_cull(on)
        before = engine.block_culls()
        got = run_gpu(torch, engine, gs, ci)
        assert engine.block_culls() == before + (1 if on else 0)
        with pytest.raises(_lib.OrbitError) as err:
            engine.status()
        out.append((got[1], str(err.value)))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    engine.set_block_cull(True)
    engine.bind_meshlet_stream(None)
    ms.close()


def test_class_planes_through_cull_shard(torch_mod, engine, oracle):  # noqa: F811
    """The same scene through orbit_cull_shard with a record list (shard_cull_kernel with class planes): dispatch records,
    record list and commands are the oracle's."""
    torch = torch_mod
    scene = _class_scene()
    cam = far_camera(z=300.0)
    ci = sc.make_cull_info(cam.view, cam.planes)
    gs = GpuScene(torch, scene)
    ms = engine.meshlet_stream(gs.meshlets, 0, len(scene.meshlets))
    ms.set_materials(gs.materials, len(scene.materials))
    engine.bind_meshlet_stream(ms)
    torch.cuda.synchronize()
    n, cap_d, cap_c = scene.entity_draw_count, scene.max_dispatches() + 8, scene.lod0_meshlets + 8
    disp = torch.full((L.DISPATCH_HEADER + 16 * cap_d + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    rec = torch.full((L.VISIBLE_HEADER + 12 * cap_d + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    cmd = torch.full((L.DRAW_HEADER + 28 * cap_c + 64,), 0xEF, dtype=torch.uint8, device="cuda")
    shards, classes = engine.shard_culls(), engine.meshlet_class_culls()
    engine.cull_shard(ci, gs.draws, gs.mesh_infos, disp, gs.entities, 0, n, cap_d, gs.meshlets, gs.materials, rec, cap_d,
                      draw_commands_buffer=cmd, draw_capacity=cap_c)
    torch.cuda.synchronize()
    engine.status()
    assert engine.shard_culls() == shards + 1 and engine.meshlet_class_culls() == classes + 1
    odisp, _, _ = oracle.entity_cull(ci, scene.entity_draw_buffer(), n, scene.mesh_infos, scene.entities, cap_d)
    odraw, _, _ = oracle.meshlet_cull(ci, odisp, scene.meshlets, cap_c, scene.entities, scene.materials)
    n_rec, orecs = L.dispatch_buffer_records(odisp)
    on, ocmds = L.draw_buffer_commands(odraw)
    n_rec = int(n_rec[0])
    assert n_rec > 300 and 0 < on < scene.lod0_meshlets
    hd, hr, hc = host(disp), host(rec), host(cmd)
    assert np.array_equal(hd[:12 + 16 * n_rec], odisp[:12 + 16 * n_rec]), "dispatch records differ from the oracle"
    assert list(hr[:8].view(np.uint32)) == [n_rec, on]
    assert np.array_equal(hr[8:8 + 12 * n_rec].view(np.uint32), _expected_visible_records(orecs, ocmds).view(np.uint32))
    assert bool((hr[8 + 12 * n_rec:] == 0xCD).all()), "write behind the record list"
    assert np.array_equal(hc[:4 + 28 * on], odraw[:4 + 28 * on]), "commands differ from the oracle"
    assert bool((hc[4 + 28 * cap_c:] == 0xEF).all()), "write behind the commands"
    engine.bind_meshlet_stream(None)
    ms.close()
