"""GPU tests of the per-block pass-0 evaluation (orbit_amd/csrc/meshlet_eval_blocks.hip; include/orbit_abi_ext.h
orbit_ctx_block_culls): every case is culled with the path on and with it off and compared byte for byte with the oracle,
and the path must have been taken.  The whole parity suite also runs through it (tests/stream_engine.py with classes)."""
import os
import sys

import numpy as np
import pytest

import scenes as sc
from orbit_amd import _lib, layouts as L
from test_block_pretest_cpu import BOUND, bounds_of
from test_gpu_parity import GpuScene, assert_same, dev, host, run_gpu, run_oracle, torch_mod  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))  # make_spirv_vectors

pytestmark = pytest.mark.gpu


@pytest.fixture()
def engine(torch_mod):
    from orbit_amd.engine import Engine

    e = Engine(0, max_entities=50_000, max_dispatches=400_000, max_draws=1_000_000)
    yield e
    e.close()


def both_ways(torch, engine, oracle, scene, ci):
    """-> the draw buffer; asserts on == off == oracle and that the counter advanced only with the path on."""
    gs = GpuScene(torch, scene)
    ms = engine.meshlet_stream(gs.meshlets, 0, len(scene.meshlets))
    ms.set_materials(gs.materials, len(scene.materials))
    engine.bind_meshlet_stream(ms)
    torch.cuda.synchronize()
    ref = run_oracle(oracle, scene, ci)
    out = []
    for on in (True, False):
        engine.set_block_cull(on)
        before, classes = engine.block_culls(), engine.meshlet_class_culls()
        got = run_gpu(torch, engine, gs, ci)
        assert engine.meshlet_class_culls() == classes + 1
        assert engine.block_culls() == before + (1 if on else 0)
        engine.status()
        assert_same(got, ref)
        out.append(got[1])
    assert np.array_equal(out[0], out[1])
    engine.set_block_cull(True)
    engine.bind_meshlet_stream(None)
    ms.close()
    return out[0]


def far_camera(z=600.0, rot=(1.0, 0.0)):
    return sc.default_camera(position=(0.0, 2.0, z), rot=rot)


def info(cam):
    return sc.make_cull_info(cam.view, cam.planes, alpha_mode_flag=L.ALPHA_ALL)


def sparse_share(scene, cam):
    """Host pre-test (orbit_host_block_pretest) of a scene whose meshes start on multiples of 32 and whose entity i draws
    mesh i: -> (share of its records that are sparse, open lanes per record)."""
    from test_block_pretest_cpu import F, pretest

    model = scene.entities["model_matrix"].reshape(-1, 4, 4).transpose(0, 2, 1).astype(F)
    view = np.asarray(cam.view, dtype=F)
    vm = np.zeros_like(model)
    for k in range(4):  # mat4_mul_col: term by term in binary32
        vm = (vm + view[None, :, k, None] * model[:, None, k, :]).astype(F)
    lod0 = scene.mesh_infos["mesh_lods"][scene.entity_draws["mesh_index"], 0]
    assert (lod0[:, 0] % 32 == 0).all() and (lod0[:, 1] % 32 == 0).all()
    per = lod0[:, 1] // 32
    models = np.repeat(np.ascontiguousarray(vm.transpose(0, 2, 1)).reshape(-1, 16)[scene.entity_draws["entity_index"]], per, axis=0)
    first = np.concatenate([np.arange(o, o + c, 32) for o, c in lod0])
    idx = (first[:, None] + np.arange(32)[None, :]).reshape(-1)
    m = scene.meshlets[idx]
    cones = (m["cone_axis"].view(np.uint8).astype(np.uint32) << np.array([0, 8, 16], dtype=np.uint32)).sum(1).astype(np.uint32) \
        | m["cone_cutoff"].view(np.uint8).astype(np.uint32) << 24
    v, flags, _ = pretest(models, m["bounding_sphere"], cones, cam.planes, -1.0)
    open_lanes = (((v & 3) == 0) | (((v & 3) == 2) & ((v & 4) == 0))) & ((flags & 1) != 0)[:, None]
    return float(((flags & 1) != 0).mean()), open_lanes.sum(1)


# Every launch of this file gives each tile a wave of its own except test_many_tiles_per_wave below: the evaluation's grid
# follows the dispatch capacity, and a wave gets a second tile only beyond CUs x 16 tiles (a quarter of a million records).
@pytest.mark.parametrize("entities,per_mesh", [(14, 32), (30, 32), (96, 64), (40, 1), (40, 31), (40, 33), (300, 96)])
def test_tile_and_record_shapes(torch_mod, engine, oracle, entities, per_mesh):
    """Meshlet counts 1 / 31 / 32 / 33 per record, aligned and unaligned meshlet offsets (1, 31 and 33 per mesh put every
    mesh but the first off a multiple of 32: dense rows; 32, 64 and 96 keep them on one: sparse rows), one tile, two
    tiles and more, each on a wave of its own — from far away."""
    scene = sc.make_scene(100 + per_mesh, entities, meshlets_per_mesh=(per_mesh, per_mesh), n_materials=3, shuffle=False)
    cam = far_camera()
    if per_mesh % 32 == 0:
        assert sparse_share(scene, cam)[0] > 0.9, "these scenes are meant to take the pre-test"
    both_ways(torch_mod, engine, oracle, scene, info(cam))


def test_many_tiles_per_wave(torch_mod, oracle):
    """The tile-to-tile hand-over of one wave — the slabs' rotation, the two BlockRecord slabs, the next tile's first rows
    loaded by its own sparse flags, the ring's state starting over — needs more tiles than the device holds waves: three
    static tiles per wave and the ticketed ones behind them.  bench.py's generator (every record sparse from its far camera,
    about 40 candidates per tile), path on against path off and against the oracle."""
    torch = torch_mod
    from orbit_amd import camera, synth
    from orbit_amd.engine import Engine

    dev_ = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = 3 * cus * 4 * 4 + 1000           # beyond three rounds of CUs x 4 waves per SIMD x 4 SIMDs
    spec = synth.C5Spec(entities=(tiles * 16 + 7) // 8)  # 8 records of 32 per entity
    E, M = spec.entities, spec.meshlets_per_entity
    draws, mesh, ent, half = synth.gen_entity_tables(spec, dev_)
    mlt = synth.gen_meshlets(spec, 0, E, dev_, half)
    mat = synth.gen_materials(spec, dev_)
    ci = camera.frame_cull_info((0.0, 0.0, 1300.0))
    cap_d, cap_c = E * spec.records_per_entity + 8, E * M // 2
    eng = Engine(0, max_entities=E + 256, max_dispatches=cap_d, max_draws=cap_c)
    ms = eng.meshlet_stream(mlt, 0, E * M)
    ms.set_materials(mat, spec.materials)
    eng.bind_meshlet_stream(ms)
    torch.cuda.synchronize()
    disp = torch.zeros(L.DISPATCH_HEADER + 16 * cap_d, dtype=torch.uint8, device=dev_)
    got = []
    for on in (True, False):
        eng.set_block_cull(on)
        before = eng.block_culls()
        draw = torch.zeros(L.DRAW_HEADER + 28 * cap_c, dtype=torch.uint8, device=dev_)
        eng.entity_cull(ci, draws, mesh, disp, ent, E, cap_d)
        eng.meshlet_cull(ci, disp, mlt, draw, ent, mat, cap_d, cap_c, material_count=spec.materials)
        torch.cuda.synchronize()
        eng.status()
        assert eng.block_culls() == before + (1 if on else 0)
        got.append(host(draw))
    assert int(host(disp)[:4].view("<u4")[0]) // 16 >= tiles - 1
    assert np.array_equal(got[0], got[1])
    _, ref, _, _, dropped = oracle.cull_frame_mt(bytes(ci), host(draws), E, host(mesh), host(ent), host(mlt), host(mat), cap_d,
                                                 cap_c, oracle.max_threads())
    assert dropped == (0, 0)
    n = int(ref[:4].view("<u4")[0])
    assert n > 1000 and np.array_equal(got[0][:4 + 28 * n], ref[:4 + 28 * n])
    eng.bind_meshlet_stream(None)
    ms.close()
    eng.close()


@pytest.mark.parametrize("position,rot", [((0.0, 2.0, 0.0), (1.0, 0.0)), ((3.0, 2.0, 5.0), (0.6, 0.8)),
                                          ((0.0, 2.0, 60.0), (1.0, 0.0)), ((40.0, 2.0, 0.0), (0.0, 1.0)),
                                          ((0.0, 2.0, -70.0), (-1.0, 0.0))])
def test_camera_inside_and_blocks_across_the_planes(torch_mod, engine, oracle, position, rot):
    """The camera inside the scene (inside blocks' bounds: dense rows beside sparse ones, rows where every lane is a
    candidate) and just outside it on three sides, so that blocks straddle the near, the side and the top / bottom
    planes.  Every mesh starts on a multiple of 32, so a record is dense only because of where the camera is."""
    scene = sc.make_scene(7, 600, meshlets_per_mesh=(64, 64), n_materials=3)
    both_ways(torch_mod, engine, oracle, scene, info(sc.default_camera(position=position, rot=rot)))


def _cone_scene(open_lanes):
    """One entity per record, all at the origin under the identity, every meshlet the same sphere at the origin: from a
    camera on +z looking down -z the view-space centre is (0, 0, -z) for every lane and the block's radius is nothing.
    Lanes < open_lanes[r] of record r have the cone (127, 0, 0 | 0): the cone quantity is exactly 0 - radius, inside the
    band, so the lane is a candidate; the others have (0, 0, -127 | 64): z / 2 above zero, certainly culled.  The count
    of candidates per record is therefore open_lanes[r] by construction (asserted on the host before the GPU runs)."""
    scene = sc.make_scene(5, len(open_lanes), meshlets_per_mesh=(32, 32), n_materials=3, shuffle=False, unit_scale=True)
    scene.entities["model_matrix"] = np.eye(4, dtype=np.float32).reshape(-1)
    scene.entities["normal_matrix"] = np.eye(4, dtype=np.float32).reshape(-1)
    scene.mesh_infos["bounding_sphere"] = (0.0, 0.0, 0.0, 1.0)
    m = scene.meshlets
    m["bounding_sphere"] = (0.0, 0.0, 0.0, 0.25)
    m["cone_axis"] = (0, 0, -127)
    m["cone_cutoff"] = 64
    for r, k in enumerate(open_lanes):
        m["cone_axis"][32 * r: 32 * r + k] = (127, 0, 0)
        m["cone_cutoff"][32 * r: 32 * r + k] = 0
    return scene


@pytest.mark.parametrize("open_lanes", [[0] * 16, [32] * 16, [32, 32] + [0] * 14, [32, 32, 1] + [0] * 13,
                                        [0] * 8 + [32] * 8, [31, 32] + [0] * 14, [5, 0, 32, 7] * 8],
                         ids=["none", "all-512", "64", "65", "256-at-the-end", "63", "two-tiles-mixed"])
def test_candidate_counts(torch_mod, engine, oracle, open_lanes):
    """A tile without candidates; one where every lane is one (a flush at both mid-tile checks and four at the end); exactly
    64 (one mid-tile flush, nothing left) and 65 (one left for the end); 256 queued behind the last check (four flushes
    in a row: the ring's head goes round); 63 (no mid-tile flush); two tiles of mixed rows."""
    scene = _cone_scene(open_lanes)
    cam = sc.default_camera(position=(0.0, 0.0, 900.0))
    share, counts = sparse_share(scene, cam)
    assert share == 1.0 and list(counts) == list(open_lanes), "the scene must queue exactly these candidates"
    both_ways(torch_mod, engine, oracle, scene, info(cam))


def test_literal_path_mix(torch_mod, engine, oracle):
    """Projective matrices, infinite and NaN translations, centres and radii, a negative radius and a zero scale among
    ordinary records: such records and blocks stay dense, the rest of their tiles does not."""
    scene = sc.make_scene(19, 200, meshlets_per_mesh=(64, 64), n_materials=3, shuffle=False)
    cam = far_camera(z=300.0)
    assert sparse_share(scene, cam)[0] > 0.9  # before the damage: the ordinary records beside the damaged ones are sparse
    e, m = scene.entities, scene.meshlets
    e["model_matrix"][3][3] = 0.5          # projective
    e["model_matrix"][7][7] = 0.25
    e["model_matrix"][11][12] = np.inf     # translations
    e["model_matrix"][12][13] = np.nan
    e["model_matrix"][20][:12] = 0.0       # zero scale
    m["bounding_sphere"][40, 0] = np.inf
    m["bounding_sphere"][75, 2] = np.nan
    m["bounding_sphere"][110, 3] = np.nan
    m["bounding_sphere"][150, 3] = np.inf
    m["bounding_sphere"][200, 3] = -1.0
    both_ways(torch_mod, engine, oracle, scene, info(cam))


@pytest.mark.parametrize("seed", [31, 32])
@pytest.mark.parametrize("aligned", [False, True])
def test_knife_edge_generators(torch_mod, engine, oracle, seed, aligned):
    """The cone knife-edge generator of tests/test_knife_edge_gpu.py (cone quantities within rounding of zero), on its own
    ragged scene and on one whose records all start blocks, from its near camera and from far away."""
    import make_spirv_vectors as gen

    rng = np.random.default_rng(seed)
    scene = sc.make_scene(seed, 300, meshlets_per_mesh=(64, 64) if aligned else (1, 70), lods=1 if aligned else 3,
                          shuffle=not aligned)
    gen.quantise(scene, rng)
    for z in (float(rng.integers(4, 30)), 400.0):
        cam = sc.default_camera(position=(0.0, 0.0, z), rot=(1.0, 0.0))
        gen.cone_knife_edge(scene, cam, False)
        both_ways(torch_mod, engine, oracle, scene, sc.make_cull_info(cam.view, cam.planes))


def test_partial_updates_keep_the_bounds_right_and_an_edit_is_stale(torch_mod, engine, oracle):
    torch = torch_mod
    scene = sc.make_scene(29, 300, meshlets_per_mesh=(64, 64), n_materials=3, shuffle=False)
    ci = info(far_camera())
    gs = GpuScene(torch, scene)
    n = len(scene.meshlets)
    ms = engine.meshlet_stream(gs.meshlets, 0, n)
    ms.set_materials(gs.materials, len(scene.materials))
    engine.bind_meshlet_stream(ms)
    # rewrite [45, 1003): begins and ends inside blocks
    lo, hi = 45, 1003
    scene.meshlets["bounding_sphere"][lo:hi, :3] += np.float32(25.0)
    scene.meshlets["bounding_sphere"][lo:hi, 3] *= np.float32(3.0)
    gs.meshlets.copy_(dev(torch, scene.meshlets))
    ms.update(gs.meshlets, lo, hi - lo)
    ms.validate(gs.meshlets, gs.materials)
    engine.status()
    got = np.zeros((n + 31) // 32, dtype=BOUND)
    _lib.check(engine._lib.orbit_meshlet_stream_block_bounds(engine._ctx, ms._h, 0, len(got), got.ctypes.data, None), engine._ctx)
    want = bounds_of(scene.meshlets["bounding_sphere"])
    assert got.tobytes() == want.tobytes(), "the device derives what the host export derives"
    assert_same(run_gpu(torch, engine, gs, ci), run_oracle(oracle, scene, ci))
    assert engine.block_culls() == 1
    # an edit without an update: the stream's copy and its bounds no longer mirror the buffer.  (The copy's byte compare
    # fails here too: through the ABI a bound cannot be wrong while the copy is right, so validate's containment check
    # is never seen to fire alone; what holds the bounds to account is the read-back against the host export above.)
    scene.meshlets["bounding_sphere"][500, 0] += np.float32(1000.0)
    gs.meshlets.copy_(dev(torch, scene.meshlets))
    ms.validate(gs.meshlets, gs.materials)
    torch.cuda.synchronize()
    with pytest.raises(_lib.OrbitError):
        engine.status()
    engine.bind_meshlet_stream(None)
    ms.close()


def test_meshlets_outside_the_stream_answer_as_with_the_path_off(torch_mod, engine):
    """A stream over the first part of the buffer only: the dispatched meshlets behind it are not read, the status says
    ORBIT_E_RANGE, and list and status are the same with the path on and off."""
    torch = torch_mod
    scene = sc.make_scene(33, 200, meshlets_per_mesh=(32, 32), n_materials=3, shuffle=False)
    ci = info(far_camera())
    gs = GpuScene(torch, scene)
    ms = engine.meshlet_stream(gs.meshlets, 0, len(scene.meshlets) - 200)
    ms.set_materials(gs.materials, len(scene.materials))
    engine.bind_meshlet_stream(ms)
    torch.cuda.synchronize()
    out = []
    for on in (True, False):
        engine.set_block_cull(on)
        got = run_gpu(torch, engine, gs, ci)
        with pytest.raises(_lib.OrbitError) as err:
            engine.status()
        out.append((got[1], str(err.value)))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    engine.bind_meshlet_stream(None)
    ms.close()
