"""orbit_scene_update on the MI355X (include/orbit_abi_ext.h): EntityData rows, the EntityDrawBuffer, the
LightData rows with their shadow indices, the shadow orientations and both entity maps, built on the device from one
descriptor and one transform per entity, equal the host mirror's update_scene byte for byte — at every size where the
kernel takes another path, under every capacity, and as the head of the cull and cluster chains with no read-back."""
import numpy as np
import pytest

import scenes as sc
import scene_full_ref as R
import scene_update_ref as RU
from orbit_amd import _lib, layouts as L
from orbit_amd import scene as S
from test_gpu_parity import GpuScene, assert_same, cluster_inputs, dev, host, run_gpu, run_oracle
from test_scene_update_gpu import _cull_scene, _scene

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
GUARD = 256  # bytes behind every output buffer


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def engine(torch_mod):
    from orbit_amd.engine import Engine

    e = Engine(0, max_entities=80000, max_dispatches=200000, max_draws=400000)
    yield e
    e.close()


class Outputs:
    """Sentinel-filled output buffers of one orbit_scene_update call, each with a guard region behind its capacity."""

    def __init__(self, torch, n, instance_capacity, light_capacity, shadow_capacity):
        full = lambda nbytes: torch.full((nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")  # noqa: E731
        self.caps = (instance_capacity, light_capacity, shadow_capacity)
        self.n = n
        self.rows = full(128 * instance_capacity)
        self.draws = full(4 + 12 * instance_capacity)
        self.lights = full(64 * light_capacity)
        self.shadows = full(16 * shadow_capacity)
        self.inst = full(4 * n)
        self.lmap = full(4 * n)
        self.counts = full(16)

    def kwargs(self):
        ci, cl, cs = self.caps
        return dict(entity_data=self.rows, entity_draw_buffer=self.draws, light_data=self.lights,
                    shadow_orientations=self.shadows, instance_of_entity=self.inst, light_of_entity=self.lmap,
                    counts=self.counts, instance_capacity=ci, light_capacity=cl, shadow_capacity=cs)

    def read(self):
        """The dict of scene_full_ref.update out of the buffers (capped at the capacities), after checking that every
        byte behind a count and behind a capacity still holds the sentinel."""
        ci, cl, cs = self.caps
        counts = host(self.counts)[:16].view(np.uint32).copy()
        nd, nl, ns = min(int(counts[0]), ci), min(int(counts[1]), cl), min(int(counts[2]), cs)
        rows, draws, lights, shadows = host(self.rows), host(self.draws), host(self.lights), host(self.shadows)
        assert int(draws[:4].view(np.uint32)[0]) == nd, "count word"
        for name, buf, used in (("rows", rows, 128 * nd), ("draws", draws, 4 + 12 * nd), ("lights", lights, 64 * nl),
                                ("shadows", shadows, 16 * ns), ("instance map", host(self.inst), 4 * self.n),
                                ("light map", host(self.lmap), 4 * self.n), ("counts", host(self.counts), 16)):
            assert (buf[used:] == SENTINEL).all(), f"{name}: a byte behind the count / capacity was written"
        return dict(rows=rows[:128 * nd].view(L.ENTITY_DATA), draws=draws[4:4 + 12 * nd].view(L.ENTITY_DRAW),
                    lights=lights[:64 * nl].view(L.LIGHT), shadow_orientations=shadows[:16 * ns].view(np.float32).reshape(-1, 4),
                    instance_of_entity=host(self.inst)[:4 * self.n].view(np.uint32),
                    light_of_entity=host(self.lmap)[:4 * self.n].view(np.uint32), counts=counts)


def capped(want, ci, cl, cs):
    """What the device leaves of the host mirror's update under these capacities: prefixes; counts and maps uncapped."""
    return dict(want, rows=want["rows"][:ci], draws=want["draws"][:ci], lights=want["lights"][:cl],
                shadow_orientations=want["shadow_orientations"][:cs])


def device_update(torch, engine, tab, t, caps=None, cutoff=0.25, frame_index=0, transforms_ptr=None):
    n = len(tab)
    out = Outputs(torch, n, *(caps or (n, n, n)))
    d_tab, d_t = dev(torch, tab), dev(torch, t)
    engine.scene_update(d_tab if n else None, (transforms_ptr or d_t) if n else None, entity_count=n,
                        luminance_cutoff=cutoff, shadow_index_base=R.MAX_SHADOW_COMMANDS * frame_index, **out.kwargs())
    torch.cuda.synchronize()
    return out


# -- 1. parity with the host mirror
@pytest.mark.parametrize("mesh_pattern", R.MESH_PATTERNS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 70_001])
def test_equals_host_update_scene(torch_mod, engine, n, mesh_pattern):
    for k, light_pattern in enumerate(R.LIGHT_PATTERNS):
        tab0, t = R.make_inputs(1000 + n, n, mesh_pattern, light_pattern)
        sd, tab = R.host_scene(tab0, t, RU.ONE_MESH)
        want = R.host_update(sd, RU.ONE_MESH, n, cutoff=0.3, frame_index=k)
        out = device_update(torch_mod, engine, tab, t, cutoff=0.3, frame_index=k)
        engine.status()
        R.assert_update_equal(out.read(), want)
        if n >= 256 and light_pattern == "all":
            assert want["counts"][2] >= 8  # the shadow casters at the wave and workgroup boundaries


# -- 2. the same bits as the dense kernel
def test_rows_equal_the_dense_kernel(torch_mod, engine):
    torch = torch_mod
    n = 5000
    tab0, t = R.make_inputs(77, n, "random90", "random3")
    sd, tab = R.host_scene(tab0, t, RU.ONE_MESH)
    out = device_update(torch, engine, tab, t)
    sd.update_scene_deferred(RU.ONE_MESH)
    ordered = sd.transform_cache()  # the drawn entities' transforms in instance order
    dense = torch.full((128 * len(ordered),), SENTINEL, dtype=torch.uint8, device="cuda")
    engine.scene_update_entities(dev(torch, ordered), dense)
    torch.cuda.synchronize()
    engine.status()
    got = out.read()
    assert len(got["rows"]) == len(ordered) > 4000
    assert got["rows"].tobytes() == host(dense).tobytes()


# -- 3. capacities
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("short", ["one", "all"])
def test_capacities_cut_the_rows_and_nothing_else(torch_mod, engine, which, short):
    n = 1500
    tab0, t = R.make_inputs(31, n, "random90", "all")
    sd, tab = R.host_scene(tab0, t, RU.ONE_MESH)
    want = R.host_update(sd, RU.ONE_MESH, n)
    caps = [int(c) for c in want["counts"][:3]]
    assert min(caps) > 40
    caps[which] = caps[which] - 1 if short == "one" else 0
    out = device_update(torch_mod, engine, tab, t, caps=tuple(caps))
    with pytest.raises(_lib.OrbitError) as e:
        engine.status()
    assert e.value.code == _lib.E_CAPACITY
    engine.status()  # reading the latch clears it
    got = out.read()  # the prefix and the clamped count word; guards intact
    R.assert_update_equal(got, capped(want, *caps))
    assert np.array_equal(got["counts"], want["counts"])  # uncapped


# -- 4. light kinds the host cannot produce
def test_bad_light_kinds_are_skipped_and_latch_range(torch_mod, engine):
    n = 1000
    tab0, t = R.make_inputs(41, n, "random90", "all")
    bad_at = np.array([0, 63, 64, 255, 256, 700, 999])
    _, tab = R.host_scene(tab0, t, RU.ONE_MESH)
    tab["light_kind"][bad_at] = (3, 0xFFFFFFFE, 4, 3, 0x80000000, 0xFFFFFFFE, 3)  # the flags and parameters stay
    stripped = tab0.copy()
    stripped["light_kind"][bad_at] = R.NONE  # the pin: the scene whose bad entities carry no light
    sd, _ = R.host_scene(stripped, t, RU.ONE_MESH)
    want = R.host_update(sd, RU.ONE_MESH, n)
    out = device_update(torch_mod, engine, tab, t)
    with pytest.raises(_lib.OrbitError) as e:
        engine.status()
    assert e.value.code == _lib.E_RANGE
    engine.status()
    R.assert_update_equal(out.read(), want)
    assert want["counts"][1] == n - len(bad_at)


# -- 5. argument checks
def test_argument_checks(torch_mod, engine):
    torch = torch_mod
    tab0, t = R.make_inputs(5, 8, "all", "all")
    _, tab = R.host_scene(tab0, t, RU.ONE_MESH)
    d_tab, d_t = dev(torch, tab), dev(torch, t)
    out = Outputs(torch, 8, 8, 8, 8)
    for missing in ("entities", "transforms", "entity_data", "entity_draw_buffer", "light_data"):
        kw = dict(out.kwargs(), entities=d_tab, transforms=d_t, entity_count=8)
        kw[missing] = None
        with pytest.raises(_lib.OrbitError) as e:
            engine.scene_update(**kw)
        assert e.value.code == _lib.E_INVALID, missing
    with pytest.raises(_lib.OrbitError) as e:
        engine.scene_update(d_tab, d_t, entity_count=8, **dict(out.kwargs(), entity_data=out.rows.data_ptr() + 4))
    assert e.value.code == _lib.E_INVALID  # entity_data not 16-B aligned
    with pytest.raises(_lib.OrbitError) as e:
        engine.scene_update(d_tab, d_t, entity_count=engine.caps.max_entities + 1, **out.kwargs())
    assert e.value.code == _lib.E_CAPACITY
    assert engine._lib.orbit_scene_update(engine._ctx, None, None) == _lib.E_INVALID  # NULL update
    torch.cuda.synchronize()
    engine.status()
    for buf in (out.rows, out.draws, out.lights, out.shadows, out.inst, out.lmap, out.counts):
        assert (host(buf) == SENTINEL).all(), "a refused call wrote"


def test_no_entities_writes_the_zero_count_and_counts_only(torch_mod, engine):
    out = Outputs(torch_mod, 0, 4, 4, 4)
    engine.scene_update(None, None, entity_count=0, **out.kwargs())
    torch_mod.cuda.synchronize()
    engine.status()
    assert (host(out.draws)[:4] == 0).all() and (host(out.draws)[4:] == SENTINEL).all()
    assert (host(out.counts)[:16] == 0).all() and (host(out.counts)[16:] == SENTINEL).all()
    for buf in (out.rows, out.lights, out.shadows, out.inst, out.lmap):
        assert (host(buf) == SENTINEL).all()


@pytest.mark.parametrize("n", [257, 1000])
def test_transforms_without_16_byte_alignment_give_the_same_bytes(torch_mod, engine, n):
    torch = torch_mod
    tab0, t = R.make_inputs(9 + n, n, "random90", "random3")
    sd, tab = R.host_scene(tab0, t, RU.ONE_MESH)
    want = R.host_update(sd, RU.ONE_MESH, n)
    raw = torch.zeros(40 * n + 16, dtype=torch.uint8, device="cuda")
    raw[4:4 + 40 * n] = dev(torch, t)
    out = device_update(torch, engine, tab, t, transforms_ptr=raw.data_ptr() + 4)
    engine.status()
    R.assert_update_equal(out.read(), want)


# -- 6. end to end without a read-back
def _vis_words(scene):
    d = scene.entity_draws
    words = (scene.mesh_infos["mesh_lods"][d["mesh_index"], 0, 1].astype(np.int64) + 31) // 32
    return int((d["visibility_offset"].astype(np.int64) + words).max())  # entities that lost their mesh keep theirs


def _device_scene_buffers(torch, n):
    return (torch.zeros(128 * n, dtype=torch.uint8, device="cuda"),
            torch.zeros(4 + 12 * n, dtype=torch.uint8, device="cuda"),
            torch.zeros(64 * 16, dtype=torch.uint8, device="cuda"))


def test_end_to_end_update_then_cull_without_a_read_back(torch_mod, engine, oracle):
    torch = torch_mod
    n = 3000
    sd, base = _scene(21, n, 300)
    cam = sc.default_camera(rot=(0.8, 0.6))
    ci0 = sc.make_cull_info(cam.view, cam.planes)
    ci2 = sc.make_cull_info(cam.view, cam.planes, occlusion_pass=2, p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
    W, H = 256, 144
    opyr, d = oracle.depth_reduce(sc.make_depth(7, W, H, cam), W, H)
    ps = (d.width, d.height)
    sd.update_scene_device(base.mesh_infos)
    d_tab, d_t = dev(torch, sd.entity_table()), dev(torch, sd.transform_cache())
    ent, draws, lights = _device_scene_buffers(torch, n)
    rng = np.random.default_rng(23)
    for frame in range(2):
        if frame == 1:  # 1 % of the entities gain or lose their mesh: only their descriptors change, on the device
            flipped = rng.choice(n, n // 100, replace=False)
            for e in flipped:
                sd.set_mesh(int(e), None if sd.instance_index(int(e)) >= 0 else int(rng.integers(300)))
            sd.update_scene_device(base.mesh_infos)
            idx = torch.from_numpy(flipped.astype(np.int64)).cuda()
            d_tab.view(n, 48)[idx] = dev(torch, sd.entity_table()[flipped]).view(-1, 48)
        scene = _cull_scene(sd, base)  # the host mirror's update_scene: what the device must reproduce
        assert 0 < scene.entity_draw_count < n
        evis = np.zeros((n + 31) // 32, dtype=np.uint32)
        mvis = np.zeros(_vis_words(scene), dtype=np.uint32)
        gs = GpuScene(torch, scene)
        gs.draws, gs.entities = draws, ent  # the culls read the device-built buffers
        for ci, vis in ((ci0, (None, None, None, (0, 0))), (ci2, (evis, mvis, opyr, ps))):
            # one stream: the update, then the culls with the entity count as the draw count's upper bound
            engine.scene_update(d_tab, d_t, ent, draws, lights, entity_count=n)
            gpu = run_gpu(torch, engine, gs, ci, *vis, entity_draw_count=n, disp_cap=scene.max_dispatches() + 8,
                          draw_cap=scene.lod0_meshlets + 8)
            ref = run_oracle(oracle, scene, ci, *vis, entity_draw_count=n)
            recs, cmds = assert_same(gpu, ref)
            assert len(cmds) > 0
        engine.status()
        nd = scene.entity_draw_count
        assert host(ent)[:128 * nd].tobytes() == scene.entities.tobytes()
        assert host(draws)[:4 + 12 * nd].tobytes() == scene.entity_draw_buffer().tobytes()


# -- 7. captured into a graph on the first call of a fresh context
def test_update_and_cull_capture_into_a_graph_on_the_first_call(torch_mod, oracle):
    torch = torch_mod
    from orbit_amd.engine import Engine

    n = 1500
    sd, base = _scene(31, n, 150)
    sd.update_scene_device(base.mesh_infos)
    d_tab, d_t = dev(torch, sd.entity_table()), dev(torch, sd.transform_cache())
    scene = _cull_scene(sd, base)
    cam = sc.default_camera()
    ci = sc.make_cull_info(cam.view, cam.planes)
    eng = Engine(0, max_entities=4096, max_dispatches=100000, max_draws=200000)  # a context that never ran the update
    try:
        gs = GpuScene(torch, scene)
        ent, draws, lights = _device_scene_buffers(torch, n)
        cap_d, cap_c = scene.max_dispatches() + 64, scene.lod0_meshlets + 2048
        disp = torch.zeros(L.DISPATCH_HEADER + 16 * cap_d, dtype=torch.uint8, device="cuda")
        draw = torch.zeros(L.DRAW_HEADER + 28 * cap_c, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.scene_update(d_tab, d_t, ent, draws, lights, entity_count=n)
            eng.entity_cull(ci, draws, gs.mesh_infos, disp, ent, n, cap_d)
            eng.meshlet_cull(ci, disp, gs.meshlets, draw, ent, gs.materials, cap_d, cap_c)
        rng = np.random.default_rng(32)
        for frame in range(2):
            if frame == 1:  # transforms and descriptors rewritten in place; the graph reads them on replay
                for e in range(0, n, 3):
                    q = rng.normal(size=4)
                    sd.set_transform(e, rng.uniform(-30, 30, 3), q / np.linalg.norm(q), rng.uniform(0.5, 2.0, 3))
                for e in rng.choice(n, 15, replace=False):
                    sd.set_mesh(int(e), None if sd.instance_index(int(e)) >= 0 else int(rng.integers(150)))
                sd.update_scene_device(base.mesh_infos)
                d_tab.copy_(dev(torch, sd.entity_table()))
                d_t.copy_(dev(torch, sd.transform_cache()))
                scene = _cull_scene(sd, base)
                assert scene.max_dispatches() <= cap_d and scene.lod0_meshlets <= cap_c
            g.replay()
            torch.cuda.synchronize()
            eng.status()
            nd = scene.entity_draw_count
            assert host(ent)[:128 * nd].tobytes() == scene.entities.tobytes()
            assert host(draws)[:4 + 12 * nd].tobytes() == scene.entity_draw_buffer().tobytes()
            odisp, odraw = run_oracle(oracle, scene, ci, disp_cap=cap_d, draw_cap=cap_c, entity_draw_count=n)[:2]
            on, ocmds = L.draw_buffer_commands(odraw)
            gn, gcmds = L.draw_buffer_commands(host(draw))
            assert on > 0 and gn == on and np.array_equal(gcmds.view(np.uint32), ocmds.view(np.uint32))
            assert np.array_equal(L.dispatch_buffer_records(host(disp))[1], L.dispatch_buffer_records(odisp)[1])
    finally:
        eng.close()


# -- 8. the device-built lights feed the cluster chain
def test_device_built_lights_feed_the_cluster_chain(torch_mod, engine, oracle):
    torch = torch_mod
    n_lights, W, H = 300, 160, 90  # the shape of tests/golden/cluster_small.npz
    push, depth, info, src = cluster_inputs(oracle, 103, W, H, n_lights)
    assert (src["light_type"] == L.LIGHT_TYPE_POINT).all()
    n = 900  # every third entity carries one of the point lights
    tab0, t = R.make_inputs(51, n, "random90", "none")
    lit = np.arange(0, n, 3)
    tab0["light_kind"][lit] = S.POINT
    tab0["light_color"][lit], tab0["light_intensity"][lit] = src["color"], src["intensity"]
    tab0["light_param"][lit] = src["inner_radius"]
    t["position"][lit] = src["position"]
    sd, tab = R.host_scene(tab0, t, RU.ONE_MESH)
    want = R.host_update(sd, RU.ONE_MESH, n, cutoff=0.25)["lights"]
    out = device_update(torch, engine, tab, t, cutoff=0.25)
    engine.status()
    assert len(want) == n_lights and host(out.lights)[:64 * n_lights].tobytes() == want.tobytes()
    cc = [int(v) for v in push["cluster_count"]]
    total, cap = cc[0] * cc[1] * cc[2], cc[0] * cc[1] * max(4, cc[2])
    lcap = total * 256

    def chain(lights_dev):
        gm = torch.full((cc[0] * cc[1],), 0x55, dtype=torch.int32, device="cuda")
        gb = torch.full((total, 2), 0x55, dtype=torch.int32, device="cuda")
        gu = torch.full((L.COMPACT_HEADER + 4 * cap,), 0xEE, dtype=torch.uint8, device="cuda")
        gl = torch.full((L.LIGHT_INDEX_HEADER + 4 * lcap,), 0xEE, dtype=torch.uint8, device="cuda")
        gimg = torch.zeros((total, 2), dtype=torch.int32, device="cuda")
        engine.compute_clusters(push, info, dev(torch, depth), lights_dev, gm, gb, gu, cap, gl, lcap, gimg)
        torch.cuda.synchronize()
        engine.status()
        return host(gu), host(gl), host(gimg, np.uint32)

    got, ref = chain(out.lights), chain(dev(torch, want))  # the device-built array in place, no copy
    n_idx = int(ref[1][:4].view(np.uint32)[0])
    assert n_idx > 0 and int(got[1][:4].view(np.uint32)[0]) == n_idx
    assert np.array_equal(got[1][:4 + 4 * n_idx], ref[1][:4 + 4 * n_idx]), "cluster light index lists differ"
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0])
