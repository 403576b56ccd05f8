"""orbit_raster_depth on the MI355X (include/orbit_abi_ext.h): the depth bytes, the counters and the
latched status equal the host mirror's (orbit_amd.raster.host_raster_depth on the same buffers — never a restatement)
on every case of tests/raster_cases.py, on a scene whose draw list never leaves the device, in any command order, over a
loaded buffer, through the two-pass frame, and captured into a graph on a context's first call.  Every buffer sits
between sentinel guards; inputs come back unchanged."""
import numpy as np
import pytest

import raster_cases as rc
import raster_scene as rs
import raster_vis_cases as vc
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = rc.SENTINEL, rc.GUARD
CASES = rc.all_cases()


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def engine(torch_mod):
    from orbit_amd.engine import Engine

    e = Engine(0, max_entities=4096, max_dispatches=100000, max_draws=200000)
    yield e
    e.close()


class Guarded:
    """A device copy of `a` between two guard regions of SENTINEL bytes (16-B aligned: GUARD is a multiple of 16)."""

    def __init__(self, torch, a, nbytes=None):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.n = len(a) if nbytes is None else nbytes
        buf = np.full(self.n + 2 * GUARD, SENTINEL, np.uint8)
        buf[GUARD:GUARD + len(a)] = a
        self.before = buf[GUARD:GUARD + self.n].copy()
        self.t = torch.from_numpy(buf).cuda()
        self.ptr = self.t.data_ptr() + GUARD

    def read(self):
        b = host(self.t)
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + self.n:] == SENTINEL).all(), "a guard byte was written"
        return b[GUARD:GUARD + self.n].copy()

    def unchanged(self):
        assert self.read().tobytes() == self.before.tobytes(), "an input was written"


def run(torch, engine, words, max_commands, data, vertices, vertex_count, entities, view_proj, width, height, depth=None,
        clear=True, cull_none=False, stride=12, offset=0, entity_count=None, data_words=None, with_stats=True):
    """One orbit_raster_depth call on guarded copies -> (depth (h, w) float32, stats row or None)."""
    cmd, dat, vb, ent = Guarded(torch, words), Guarded(torch, data), Guarded(torch, vertices), Guarded(torch, entities)
    out = Guarded(torch, np.full(width * height, np.float32(0.123), np.float32) if depth is None else depth)
    st = Guarded(torch, np.zeros(0, np.uint8), nbytes=32) if with_stats else None  # sentinel-filled: the call clears it
    engine.raster_depth(cmd.ptr, max_commands, dat.ptr, vb.ptr, vertex_count, ent.ptr,
                        ent.n // 128 if entity_count is None else entity_count, view_proj, out.ptr, width, height,
                        clear=clear, cull_none=cull_none, stats=None if st is None else st.ptr, vertex_stride=stride,
                        position_offset=offset, meshlet_data_words=dat.n // 4 if data_words is None else data_words)
    torch.cuda.synchronize()
    for g in (cmd, dat, vb, ent):
        g.unchanged()
    return out.read().view(np.float32).reshape(height, width), None if st is None else st.read().view(L.RASTER_STATS)[0]


def run_case(torch, engine, pk, **kw):
    opts, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    return run(torch, engine, words, mc, data, vb, vc, ent, vp, w, h, cull_none=pk.case.cull_none, stride=pk.stride,
               offset=pk.offset, entity_count=opts["entity_count"], data_words=opts["meshlet_data_words"], **kw)


def latched(engine):
    try:
        engine.status()
        return 0
    except _lib.OrbitError as e:
        return e.code


def assert_equal(name, got_depth, got_stats, want_depth, want_stats):
    assert got_stats.tobytes() == want_stats.tobytes(), f"{name}: device stats {got_stats} != host {want_stats}"
    diff = np.argwhere(got_depth.view(np.uint32) != want_depth.view(np.uint32))
    assert len(diff) == 0, (f"{name}: {len(diff)} pixels differ, first at (y, x) = {diff[0]}: device "
                            f"{got_depth[tuple(diff[0])]!r}, host {want_depth[tuple(diff[0])]!r}")


# -- 1. every census case: bytes, counters, latched status
@pytest.mark.parametrize("stride,offset", [(12, 0), (32, 0), (32, 20)])
def test_every_case_equals_the_host_mirror(torch_mod, engine, stride, offset):
    assert latched(engine) == 0
    for case in CASES:
        pk = rc.Packed(case, stride, offset)
        want_depth, want_stats, err = pk.host()
        got_depth, got_stats = run_case(torch_mod, engine, pk)
        assert latched(engine) == (_lib.E_RANGE if err.any() else 0), case.name
        assert_equal(case.name, got_depth, got_stats, want_depth, want_stats)
        assert not rc.check_claims(case, got_depth, got_stats, err, pk.restated()[3] if case.extra else None), case.name


def test_a_command_of_more_than_256_triangles_is_drawn(torch_mod, engine):
    """The depth call has no triangle limit (V3 is the visibility call's): the 257-triangle strip between two neighbours
    is drawn, where orbit_raster_visibility skips it.  The reference is held to tests/raster_ref.py by
    tests/test_raster_depth_cpu.py on the same case."""
    assert latched(engine) == 0
    pk = rc.Packed(next(c for c in vc.new_cases() if c.name == "nt_257_between_neighbours"))
    assert (pk.case.width, pk.case.height) == (64, 48) and [len(m.corners) for m in pk.case.meshlets] == [1, 257, 1]
    want_depth, want_stats, err = pk.host()
    got_depth, got_stats = run_case(torch_mod, engine, pk)
    assert latched(engine) == 0 and not err.any()
    assert_equal(pk.case.name, got_depth, got_stats, want_depth, want_stats)
    assert (int(got_stats["range_errors"]), int(got_stats["commands"]), int(got_stats["triangles"])) == (0, 3, 259)


def test_no_stats_and_a_loaded_buffer(torch_mod, engine):
    a, b = rc.Packed(CASES[0]), rc.Packed(CASES[2])
    da, _, _ = a.host()
    want, _, _ = b.host(depth=da, clear=False)
    got, none = run_case(torch_mod, engine, b, depth=da, clear=False, with_stats=False)
    assert none is None and latched(engine) == 0
    assert got.tobytes() == want.tobytes() and got.tobytes() != da.tobytes()


# -- 2. a scene whose draw list is produced on the device and never read back before the raster
@pytest.fixture(scope="module")
def scene100(oracle):
    scene = rs.glb_scene(100)
    w, h = 256, 144
    cam = rs.camera(w, h)
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    return scene, cam, w, h, draw, scene.host_raster(draw, cam, w, h)


class DeviceScene:
    def __init__(self, torch, scene):
        self.g = {k: Guarded(torch, getattr(scene, k)) for k in ("entity_draws", "mesh_infos", "entities", "meshlets",
                                                                 "materials", "meshlet_data", "vertices")}
        self.scene = scene

    def cull(self, torch, engine, ci, disp, draw, evis=None, mvis=None, pyramid=None, pyramid_size=(0, 0)):
        s, g = self.scene, self.g
        engine.entity_cull(ci, g["entity_draws"].ptr, g["mesh_infos"].ptr, disp, g["entities"].ptr, s.n, s.cap_d,
                           visibility_buffer=evis, depth_pyramid=pyramid, depth_pyramid_size=pyramid_size)
        engine.meshlet_cull(ci, disp, g["meshlets"].ptr, draw, g["entities"].ptr, g["materials"].ptr, s.cap_d, s.cap_c,
                            meshlet_visibility_buffer=mvis, material_count=len(s.materials), depth_pyramid=pyramid,
                            depth_pyramid_size=pyramid_size)

    def raster(self, engine, draw, cam, depth, w, h, clear, stats=None):
        s, g = self.scene, self.g
        engine.raster_depth(draw, s.cap_c, g["meshlet_data"].ptr, g["vertices"].ptr, len(s.vertices), g["entities"].ptr,
                            s.entity_count, rs.view_proj(cam), depth, w, h, clear=clear, stats=stats,
                            meshlet_data_words=len(s.meshlet_data))

    def unchanged(self):
        for g in self.g.values():
            g.unchanged()


def test_device_draw_list_rasterises_to_the_host_mirrors_depth(torch_mod, engine, scene100):
    torch = torch_mod
    scene, cam, w, h, odraw, (want_depth, want_stats, err) = scene100
    assert not err.any()
    ds = DeviceScene(torch, scene)
    ci = rs.sc.make_cull_info(cam.view, cam.planes, p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
    disp = torch.zeros(12 + 16 * scene.cap_d, dtype=torch.uint8, device="cuda")
    draw = torch.zeros(4 + 28 * scene.cap_c, dtype=torch.uint8, device="cuda")
    depth, stats = Guarded(torch, np.full(w * h, np.float32(7), np.float32)), Guarded(torch, np.zeros(0, np.uint8), nbytes=32)
    ds.cull(torch, engine, ci, disp, draw)
    ds.raster(engine, draw, cam, depth.ptr, w, h, True, stats.ptr)  # the count is still on the device
    torch.cuda.synchronize()
    assert latched(engine) == 0
    ds.unchanged()
    n = int(odraw[:4].view(np.uint32)[0])
    assert host(draw)[:4 + 28 * n].tobytes() == odraw[:4 + 28 * n].tobytes()
    assert_equal("scene", depth.read().view(np.float32).reshape(h, w), stats.read().view(L.RASTER_STATS)[0], want_depth, want_stats)
    assert int(want_stats["commands"]) == n > 8000


# -- 3. order and load
def test_command_order_load_and_repetition_do_not_matter(torch_mod, engine, scene100):
    torch = torch_mod
    scene, cam, w, h, odraw, (want_depth, want_stats, _) = scene100
    n, cmds = L.draw_buffer_commands(odraw)
    rng = np.random.default_rng(11)
    args = (scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, rs.view_proj(cam), w, h)
    shuffled, stats = run(torch, engine, raster.command_buffer(cmds[rng.permutation(n)]), n, *args)
    assert shuffled.tobytes() == want_depth.tobytes() and stats.tobytes() == want_stats.tobytes()
    pick = rng.random(n) < 0.5
    a, b = raster.command_buffer(cmds[pick]), raster.command_buffer(cmds[~pick])
    da, sa = run(torch, engine, a, int(pick.sum()), *args)
    dab, sb = run(torch, engine, b, int((~pick).sum()), *args, depth=da, clear=False)
    assert dab.tobytes() == want_depth.tobytes() and da.tobytes() != want_depth.tobytes()
    assert int(sa["fragments"]) + int(sb["fragments"]) == int(want_stats["fragments"])
    again, s2 = run(torch, engine, b, int((~pick).sum()), *args, depth=dab, clear=False)
    assert again.tobytes() == dab.tobytes() and s2.tobytes() == sb.tobytes()
    assert latched(engine) == 0


# -- 4. the two-pass frame on one scene's own geometry, every stage against the CPU chain
def test_two_pass_frame_equals_the_cpu_chain(torch_mod, engine, oracle):
    torch = torch_mod
    from orbit_amd.engine import depth_pyramid_desc

    scene = rs.glb_scene(100)
    w, h = 320, 180
    cams = (rs.camera(w, h, (0.0, 1.0, 6.0)), rs.camera(w, h, (0.0, 1.0, 3.0)))
    cpu = rs.two_pass_frame(scene, oracle, cams[0], cams[1], w, h)
    rejected = rs.hiz_rejected(scene, oracle, cams[1], cpu[1])
    print(f"frame 1: early {int(cpu[1]['draw1'][:4].view(np.uint32)[0])} commands, late "
          f"{int(cpu[1]['draw2'][:4].view(np.uint32)[0])}, HiZ rejected {rejected} meshlets")
    assert rejected > 0, "powerless: the late pass's HiZ test rejected nothing"
    assert int(cpu[1]["draw1"][:4].view(np.uint32)[0]) > 0 and int(cpu[1]["draw2"][:4].view(np.uint32)[0]) > 0
    ds = DeviceScene(torch, scene)
    pd = depth_pyramid_desc(w, h)
    evis = torch.zeros((scene.n + 31) // 32, dtype=torch.int32, device="cuda")
    mvis = torch.zeros(scene.vis_words, dtype=torch.int32, device="cuda")
    depth = torch.full((h * w,), 9.0, dtype=torch.float32, device="cuda")
    pyr = torch.zeros(pd.total_texels, dtype=torch.float32, device="cuda")
    for f, cam in enumerate(cams):
        want = cpu[f]
        draws, depths = [], []
        for p in (1, 2):
            ci = rs.sc.make_cull_info(cam.view, cam.planes, occlusion_pass=p, p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
            disp = torch.zeros(12 + 16 * scene.cap_d, dtype=torch.uint8, device="cuda")
            draw = torch.zeros(4 + 28 * scene.cap_c, dtype=torch.uint8, device="cuda")
            if p == 2:
                engine.depth_reduce(depth, w, h, pyr)
            ds.cull(torch, engine, ci, disp, draw, evis, mvis, pyr if p == 2 else None, (pd.width, pd.height) if p == 2 else (0, 0))
            ds.raster(engine, draw, cam, depth, w, h, clear=p == 1)
            draws.append(draw)
            depths.append(depth.clone())
        torch.cuda.synchronize()
        assert latched(engine) == 0
        for k, name in enumerate(("draw1", "draw2")):
            n = int(want[name][:4].view(np.uint32)[0])
            assert host(draws[k])[:4 + 28 * n].tobytes() == want[name][:4 + 28 * n].tobytes(), f"frame {f}: {name}"
        assert host(depths[0], np.float32).tobytes() == want["depth1"].tobytes(), f"frame {f}: early depth"
        assert host(depths[1], np.float32).tobytes() == want["depth2"].tobytes(), f"frame {f}: late depth"
        assert host(pyr, np.float32).tobytes() == want["pyramid"].tobytes(), f"frame {f}: pyramid"
        assert np.array_equal(host(evis, np.uint32), want["evis"]) and np.array_equal(host(mvis, np.uint32), want["mvis"])
    ds.unchanged()


# -- 5. captured into a graph on the first call of a fresh context
def test_the_first_call_captures_into_a_graph(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine

    cases = [c for c in CASES if c.name in ("fan_at_centre", "strip_255_255", "mirrored_scale")]
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        pks = [rc.Packed(c) for c in cases]
        size = lambda f: max(len(f(p)) for p in pks)  # noqa: E731
        pad = lambda a, n: np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1),  # noqa: E731
                                           np.zeros(n - np.ascontiguousarray(a).nbytes, np.uint8)])
        nb = dict(words=4 * size(lambda p: p.words), data=4 * size(lambda p: p.meshlet_data),
                  vb=size(lambda p: p.vertices), ent=128 * size(lambda p: p.entities))
        g_words, g_data, g_vb, g_ent = (torch.zeros(nb[k], dtype=torch.uint8, device="cuda") for k in ("words", "data", "vb", "ent"))
        vc = nb["vb"] // 12  # every vertex the buffers can hold
        depth = torch.full((48 * 64,), 5.0, dtype=torch.float32, device="cuda")
        stats = torch.full((32,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.raster_depth(g_words, 3, g_data, g_vb, vc, g_ent, 2, rc.pixel_proj(64, 48), depth, 64, 48, clear=True,
                             stats=stats, meshlet_data_words=nb["data"] // 4)
        for pk in pks[:2] + pks[:1]:  # replayed: new commands, new geometry, the first ones again
            assert pk.vertex_count <= vc and len(pk.commands) <= 3
            g_words.copy_(dev(torch, pad(pk.words, nb["words"])))
            g_data.copy_(dev(torch, pad(pk.meshlet_data, nb["data"])))
            g_vb.copy_(dev(torch, pad(pk.vertices, nb["vb"])))
            g_ent.copy_(dev(torch, pad(pk.entities, nb["ent"])))
            g.replay()
            torch.cuda.synchronize()
            eng.status()
            want_depth, want_stats, _ = raster.host_raster_depth(pk.words, len(pk.commands), pad(pk.meshlet_data, nb["data"]).view(np.uint32),
                                                                 pad(pk.vertices, nb["vb"]), vc, pad(pk.entities, nb["ent"]),
                                                                 rc.pixel_proj(64, 48), 64, 48, entity_count=2)
            assert_equal(pk.case.name, host(depth, np.float32).reshape(48, 64), host(stats).view(L.RASTER_STATS)[0],
                         want_depth, want_stats)
            assert int(want_stats["fragments"]) > 0
    finally:
        eng.close()


# -- argument errors and the empty call
def test_argument_errors_and_the_empty_call(torch_mod, engine):
    torch = torch_mod
    pk = rc.Packed(CASES[0])
    _, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    g = dict(cmd=Guarded(torch, words), dat=Guarded(torch, data), vb=Guarded(torch, vb), ent=Guarded(torch, ent),
             depth=Guarded(torch, np.zeros(0, np.uint8), nbytes=4 * w * h), stats=Guarded(torch, np.zeros(0, np.uint8), nbytes=32))

    def call(**over):
        kw = dict(draw_commands=g["cmd"].ptr, max_commands=mc, meshlet_data=g["dat"].ptr, vertices=g["vb"].ptr, vertex_count=vc,
                  entity_data=g["ent"].ptr, entity_count=1, view_proj=vp, depth=g["depth"].ptr, width=w, height=h,
                  stats=g["stats"].ptr, meshlet_data_words=g["dat"].n // 4)
        kw.update(over)
        engine.raster_depth(**kw)

    assert engine._lib.orbit_raster_depth(engine._ctx, None, None) == _lib.E_INVALID
    for over in (dict(draw_commands=None), dict(meshlet_data=None), dict(vertices=None), dict(entity_data=None),
                 dict(depth=None), dict(vertex_stride=8), dict(vertex_stride=14), dict(vertex_stride=32, position_offset=24),
                 dict(vertex_stride=32, position_offset=6), dict(width=0), dict(height=0), dict(width=_lib.RASTER_MAX_DIM + 1),
                 dict(draw_commands=g["cmd"].ptr + 2), dict(meshlet_data=g["dat"].ptr + 1), dict(vertices=g["vb"].ptr + 2),
                 dict(entity_data=g["ent"].ptr + 8), dict(depth=g["depth"].ptr + 2), dict(stats=g["stats"].ptr + 1)):
        with pytest.raises(_lib.OrbitError) as e:
            call(**over)
        assert e.value.code == _lib.E_INVALID, over
    j = _lib.RasterDepth()
    j.flags = 4
    assert engine._lib.orbit_raster_depth(engine._ctx, j, None) == _lib.E_INVALID
    torch.cuda.synchronize()
    assert (g["depth"].read() == SENTINEL).all() and (g["stats"].read() == SENTINEL).all()  # nothing was launched
    call(max_commands=0)  # LoadOp::Load of nothing: the stats are cleared, the depth stays
    torch.cuda.synchronize()
    assert (g["depth"].read() == SENTINEL).all() and not g["stats"].read().any()
    call(max_commands=0, clear=True)
    torch.cuda.synchronize()
    assert not g["depth"].read().any() and latched(engine) == 0
