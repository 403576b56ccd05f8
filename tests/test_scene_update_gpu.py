"""orbit_scene_update_entities on the MI355X (include/orbit_abi_ext.h): EntityData rows computed on the
device from 40-B transforms equal the host mirror's update_scene bytes — dense, as a sparse scatter, with out-of-range
indices latched, feeding entity_cull + meshlet_cull on one stream, captured into a graph on its first call, and the
same in both arithmetic profiles."""
import numpy as np
import pytest

import scenes as sc
import scene_update_ref as R
from orbit_amd import _lib, layouts as L
from orbit_amd import scene as S
from test_gpu_parity import GpuScene, assert_same, dev, host, run_gpu, run_oracle

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def engine(torch_mod):
    from orbit_amd.engine import Engine

    e = Engine(0, max_entities=20000, max_dispatches=200000, max_draws=400000)
    yield e
    e.close()


def _rows_buffer(torch, rows, guard_rows=8):
    """Device buffer of `rows` EntityData rows and a guard region behind them, every byte SENTINEL."""
    return torch.full(((rows + guard_rows) * 128,), SENTINEL, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 195_313])
def test_dense_equals_host_update_scene(torch_mod, engine, n):
    torch = torch_mod
    t = R.edge_transforms(100 + n, n)
    out = _rows_buffer(torch, n)
    engine.scene_update_entities(dev(torch, t), out, count=n, entity_capacity=n)
    torch.cuda.synchronize()
    engine.status()
    got = host(out)
    R.assert_rows_equal(got[:128 * n].view(L.ENTITY_DATA), R.host_rows(t))
    assert (got[128 * n:] == SENTINEL).all(), "write past entity_capacity"


@pytest.mark.parametrize("n", [257, 1000])
def test_dense_from_transforms_without_16_byte_alignment(torch_mod, engine, n):
    torch = torch_mod
    t = R.edge_transforms(7 + n, n)
    raw = torch.zeros(40 * n + 16, dtype=torch.uint8, device="cuda")
    raw[4:4 + 40 * n] = dev(torch, t)
    out = _rows_buffer(torch, n)
    engine.scene_update_entities(raw.data_ptr() + 4, out, count=n, entity_capacity=n)
    torch.cuda.synchronize()
    engine.status()
    got = host(out)
    R.assert_rows_equal(got[:128 * n].view(L.ENTITY_DATA), R.host_rows(t))
    assert (got[128 * n:] == SENTINEL).all()


def test_sparse_scatter_touches_only_the_named_rows(torch_mod, engine):
    torch = torch_mod
    cap, m = 5000, 777
    rng = np.random.default_rng(5)
    idx = rng.choice(cap, m, replace=False).astype(np.uint32)
    t = R.edge_transforms(5, m)
    out = _rows_buffer(torch, cap)
    engine.scene_update_entities(dev(torch, t), out, instance_indices=dev(torch, idx), entity_capacity=cap)
    torch.cuda.synchronize()
    engine.status()
    got = host(out)
    rows = got[:128 * cap].reshape(cap, 128)
    R.assert_rows_equal(rows[idx].copy().view(L.ENTITY_DATA), R.host_rows(t))
    untouched = np.ones(cap, bool)
    untouched[idx] = False
    assert (rows[untouched] == SENTINEL).all() and (got[128 * cap:] == SENTINEL).all()


def test_out_of_range_index_writes_nothing_and_latches_range(torch_mod, engine):
    torch = torch_mod
    cap = 1000
    rng = np.random.default_rng(9)
    good = rng.choice(cap, 300, replace=False).astype(np.uint32)
    idx = good.copy()
    bad_at = np.array([0, 17, 150, 299])
    idx[bad_at] = (cap, cap + 3, cap + 7, 0xFFFFFFFF)  # the first three would land in the guard region
    t = R.edge_transforms(9, len(idx))
    out = _rows_buffer(torch, cap, guard_rows=16)
    engine.scene_update_entities(dev(torch, t), out, instance_indices=dev(torch, idx), entity_capacity=cap)
    torch.cuda.synchronize()
    with pytest.raises(_lib.OrbitError) as e:
        engine.status()
    assert e.value.code == _lib.E_RANGE
    engine.status()  # reading the latch clears it
    got = host(out)
    assert (got[128 * cap:] == SENTINEL).all(), "an out-of-range index was written"
    rows = got[:128 * cap].reshape(cap, 128)
    ok = np.setdiff1d(np.arange(len(idx)), bad_at)
    R.assert_rows_equal(rows[idx[ok]].copy().view(L.ENTITY_DATA), R.host_rows(t[ok]))
    untouched = np.ones(cap, bool)
    untouched[idx[ok]] = False
    assert (rows[untouched] == SENTINEL).all()


def test_argument_checks(torch_mod, engine):
    torch = torch_mod
    t = dev(torch, R.edge_transforms(1, 8))
    out = _rows_buffer(torch, 8)
    for kw in (dict(count=9, entity_capacity=8),                      # dense past the capacity
               dict(count=8, entity_capacity=8, misalign=True)):      # entity_data not 16-B aligned
        with pytest.raises(_lib.OrbitError) as e:
            dst = out.data_ptr() + 4 if kw.pop("misalign", False) else out
            engine.scene_update_entities(t, dst, **kw)
        assert e.value.code == _lib.E_INVALID
    with pytest.raises(_lib.OrbitError) as e:
        engine.scene_update_entities(None, out, count=1, entity_capacity=8)
    assert e.value.code == _lib.E_INVALID
    engine.scene_update_entities(None, None, count=0, entity_capacity=0)  # nothing to do: OK, no launch
    torch.cuda.synchronize()
    engine.status()
    assert (host(out) == SENTINEL).all()


def _scene(seed, n_entities, n_meshes):
    base = sc.make_scene(seed, n_meshes, meshlets_per_mesh=(1, 90))  # meshes / meshlets / materials only
    rng = np.random.default_rng(seed)
    sd = S.SceneData()
    for _ in range(n_entities):
        q = rng.normal(size=4)
        k = float(rng.choice([0.5, 1.0, 2.0]))
        sd.add_entity(position=rng.uniform((-40, -6, -40), (40, 10, 40)), orientation=q / np.linalg.norm(q),
                      scale=(k, k * 1.5, k), mesh=int(rng.integers(n_meshes)) if rng.random() < 0.9 else None)
    return sd, base


def _cull_scene(sd, base):
    """sc.Scene of the host mirror's update_scene output (what the device must reproduce)."""
    sd.update_scene(base.mesh_infos)
    draws, ents = sd.entity_draw_cache(), sd.entity_data_cache()
    counts = base.mesh_infos["mesh_lods"][draws["mesh_index"], 0, 1].astype(np.int64)
    return sc.Scene(draws, ents, base.mesh_infos, base.meshlets, base.materials, int(((counts + 31) // 32).sum()),
                    int(counts.sum()), {})


def test_end_to_end_sparse_update_then_cull(torch_mod, engine, oracle):
    torch = torch_mod
    sd, base = _scene(21, 3000, 300)
    cam = sc.default_camera(rot=(0.8, 0.6))
    ci = sc.make_cull_info(cam.view, cam.planes)
    # frame 1: the whole scene from its transforms
    sd.update_scene_deferred(base.mesh_infos)
    t = sd.transform_cache()
    ent = torch.zeros(128 * len(t), dtype=torch.uint8, device="cuda")
    engine.scene_update_entities(dev(torch, t), ent)
    scene = _cull_scene(sd, base)
    gs = GpuScene(torch, scene)
    gs.entities = ent
    assert_same(run_gpu(torch, engine, gs, ci), run_oracle(oracle, scene, ci))
    assert host(ent).tobytes() == scene.entities.tobytes()
    # frame 2: 1 % of the entities move; only their rows are uploaded and scattered
    rng = np.random.default_rng(22)
    drawn = [e for e in range(3000) if sd.instance_index(e) >= 0]
    moved = rng.choice(drawn, len(drawn) // 100, replace=False)
    for e in moved:
        q = rng.normal(size=4)
        sd.set_transform(int(e), rng.uniform(-40, 40, 3), q / np.linalg.norm(q), rng.uniform(0.3, 3.0, 3))
    sd.update_scene_deferred(base.mesh_infos)
    dirty = np.array([sd.instance_index(int(e)) for e in moved], dtype=np.uint32)
    engine.scene_update_entities(dev(torch, sd.transform_cache()[dirty]), ent, instance_indices=dev(torch, dirty))
    scene2 = _cull_scene(sd, base)
    assert scene2.entities.tobytes() != scene.entities.tobytes()
    gs2 = GpuScene(torch, scene2)
    gs2.entities = ent
    assert_same(run_gpu(torch, engine, gs2, ci), run_oracle(oracle, scene2, ci))  # same stream: update, then the culls
    assert host(ent).tobytes() == scene2.entities.tobytes()


def test_update_and_cull_capture_into_a_graph_on_the_first_call(torch_mod, oracle):
    torch = torch_mod
    from orbit_amd.engine import Engine

    sd, base = _scene(31, 1500, 150)
    sd.update_scene_deferred(base.mesh_infos)
    transforms = sd.transform_cache()
    scene = _cull_scene(sd, base)  # update_scene: the host's rows (and no transform cache any more)
    cam = sc.default_camera()
    ci = sc.make_cull_info(cam.view, cam.planes)
    eng = Engine(0, max_entities=4096, max_dispatches=100000, max_draws=200000)  # a context that never ran the update
    try:
        gs = GpuScene(torch, scene)
        src = dev(torch, transforms)
        assert len(transforms) == scene.entity_draw_count > 0
        gs.entities = torch.zeros(128 * scene.entity_draw_count, dtype=torch.uint8, device="cuda")
        cap_d, cap_c = scene.max_dispatches() + 8, scene.lod0_meshlets + 8
        disp = torch.zeros(L.DISPATCH_HEADER + 16 * cap_d, dtype=torch.uint8, device="cuda")
        draw = torch.zeros(L.DRAW_HEADER + 28 * cap_c, dtype=torch.uint8, device="cuda")
        n = scene.entity_draw_count
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.scene_update_entities(src, gs.entities)
            eng.entity_cull(ci, gs.draws, gs.mesh_infos, disp, gs.entities, n, cap_d)
            eng.meshlet_cull(ci, disp, gs.meshlets, draw, gs.entities, gs.materials, cap_d, cap_c)
        for frame in range(2):
            if frame == 1:  # rewrite the source transforms in place; the graph reads them on replay
                rng = np.random.default_rng(32)
                for e in range(0, 1500, 3):
                    q = rng.normal(size=4)
                    sd.set_transform(e, rng.uniform(-30, 30, 3), q / np.linalg.norm(q), rng.uniform(0.5, 2.0, 3))
                sd.update_scene_deferred(base.mesh_infos)
                src.copy_(dev(torch, sd.transform_cache()))
                scene = _cull_scene(sd, base)
            g.replay()
            torch.cuda.synchronize()
            eng.status()
            assert host(gs.entities).tobytes() == scene.entities.tobytes()
            odisp, odraw = run_oracle(oracle, scene, ci, disp_cap=cap_d, draw_cap=cap_c)[:2]
            on, ocmds = L.draw_buffer_commands(odraw)
            gn, gcmds = L.draw_buffer_commands(host(draw))
            assert on > 0 and gn == on and np.array_equal(gcmds.view(np.uint32), ocmds.view(np.uint32))
            assert np.array_equal(L.dispatch_buffer_records(host(disp))[1], L.dispatch_buffer_records(odisp)[1])
    finally:
        eng.close()


def test_both_arithmetic_profiles_give_the_same_bytes(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine

    n = 5000
    t = R.edge_transforms(77, n)
    src = dev(torch, t)
    outs = []
    for profile in (0, 1):
        eng = Engine(0, max_entities=1024, arith_profile=profile)
        try:
            out = _rows_buffer(torch, n)
            eng.scene_update_entities(src, out)
            torch.cuda.synchronize()
            eng.status()
            outs.append(host(out))
        finally:
            eng.close()
    assert outs[0].tobytes() == outs[1].tobytes()
    R.assert_rows_equal(outs[0][:128 * n].view(L.ENTITY_DATA), R.host_rows(t))
