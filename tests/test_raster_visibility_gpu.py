"""orbit_raster_visibility and orbit_visibility_resolve on the MI355X (include/orbit_abi_ext.h V1-V4):
the visibility words, the counters and the latched status equal the host mirror's (orbit_amd.raster.host_raster_visibility
/ host_visibility_resolve on the same buffers — never a restatement) on every case of tests/raster_cases.py and
tests/raster_vis_cases.py; the high halves and the counters are what orbit_raster_depth leaves on the device; a draw
list that never leaves the device, a shuffled one, two lists in one buffer, the two-pass frame driven by the visibility
call alone, and both calls captured into a graph on a context's first call.  Every buffer sits between sentinel guards;
inputs come back unchanged."""
import importlib.util
import json
import os

import numpy as np
import pytest

import raster_cases as rc
import raster_scene as rs
import raster_vis_cases as vc
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import DeviceScene, Guarded, latched
from test_raster_depth_gpu import run as run_depth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = rc.SENTINEL
CENSUS, NEW = vc.census_as_vis_cases(), vc.new_cases()
FILL = np.uint64(0x0123456789ABCDEF)  # what an output holds before a call that must overwrite it


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


def high_halves(vis):
    return (np.asarray(vis, np.uint64) >> np.uint64(32)).astype(np.uint32)


def run(torch, engine, words, max_commands, data, vertices, vertex_count, entities, view_proj, width, height,
        visibility=None, command_base=0, clear=True, cull_none=False, stride=12, offset=0, entity_count=None,
        data_words=None, with_stats=True):
    """One orbit_raster_visibility call on guarded copies -> (visibility (h, w) uint64, stats row or None)."""
    cmd, dat, vb, ent = Guarded(torch, words), Guarded(torch, data), Guarded(torch, vertices), Guarded(torch, entities)
    out = Guarded(torch, np.full(width * height, FILL, np.uint64) if visibility is None else visibility)
    st = Guarded(torch, np.zeros(0, np.uint8), nbytes=32) if with_stats else None  # sentinel-filled: the call clears it
    engine.raster_visibility(cmd.ptr, max_commands, dat.ptr, vb.ptr, vertex_count, ent.ptr,
                             ent.n // 128 if entity_count is None else entity_count, view_proj, out.ptr, width, height,
                             command_base=command_base, clear=clear, cull_none=cull_none,
                             stats=None if st is None else st.ptr, vertex_stride=stride, position_offset=offset,
                             meshlet_data_words=dat.n // 4 if data_words is None else data_words)
    torch.cuda.synchronize()
    for g in (cmd, dat, vb, ent):
        g.unchanged()
    return out.read().view(np.uint64).reshape(height, width), None if st is None else st.read().view(L.RASTER_STATS)[0]


def run_case(torch, engine, pk, **kw):
    opts, (words, mc, data, vb, vcount, ent, vp, w, h) = pk.args()
    kw.setdefault("command_base", pk.case.command_base)
    return run(torch, engine, words, mc, data, vb, vcount, ent, vp, w, h, cull_none=pk.case.cull_none, stride=pk.stride,
               offset=pk.offset, entity_count=opts["entity_count"], data_words=opts["meshlet_data_words"], **kw)


def resolve(torch, engine, vis, command_base, max_commands, want=("depth", "pixels", "stats")):
    """One orbit_visibility_resolve call on guarded buffers -> (depth (h, w) float32, command_pixels, stats row); None
    for an output that was not asked for."""
    h, w = vis.shape
    src = Guarded(torch, vis)
    depth = Guarded(torch, np.zeros(0, np.uint8), nbytes=4 * w * h) if "depth" in want else None
    pixels = Guarded(torch, np.zeros(0, np.uint8), nbytes=4 * max_commands) if "pixels" in want else None
    stats = Guarded(torch, np.zeros(0, np.uint8), nbytes=16) if "stats" in want else None
    engine.visibility_resolve(src.ptr, w, h, command_base, max_commands, depth=depth and depth.ptr,
                              command_pixels=pixels and pixels.ptr, stats=stats and stats.ptr)
    torch.cuda.synchronize()
    src.unchanged()
    return (depth and depth.read().view(np.float32).reshape(h, w), pixels and pixels.read().view(np.uint32),
            stats and stats.read().view(L.VIS_STATS)[0])


def assert_equal(name, got_vis, got_stats, want_vis, want_stats):
    assert got_stats.tobytes() == want_stats.tobytes(), f"{name}: device stats {got_stats} != host {want_stats}"
    diff = np.argwhere(got_vis != want_vis)
    assert len(diff) == 0, (f"{name}: {len(diff)} words differ, first at (y, x) = {diff[0]}: device "
                            f"{int(got_vis[tuple(diff[0])]):#018x}, host {int(want_vis[tuple(diff[0])]):#018x}")


def assert_resolve_equal(name, got, want):
    for g, w, what in zip(got, want, ("depth", "command_pixels", "stats")):
        assert g.tobytes() == w.tobytes(), f"{name}: {what}: device {g} != host {w}"


# -- 1. the census and the new cases: words, counters, latched status
@pytest.mark.parametrize("stride,offset", [(12, 0), (32, 0), (32, 20)])
def test_every_case_equals_the_host_mirror(torch_mod, engine, stride, offset):
    assert latched(engine) == 0
    for case in CENSUS + NEW:
        pk = rc.Packed(case, stride, offset)
        want_vis, want_stats, err = vc.host(pk)
        got_vis, got_stats = run_case(torch_mod, engine, pk)
        assert latched(engine) == (_lib.E_RANGE if err.any() else 0), case.name
        assert_equal(case.name, got_vis, got_stats, want_vis, want_stats)
        extras = dict(vc.restated(pk)[3], won=vc.vref.winners(got_vis, case.command_base, pk.max_commands)) if case.winners else {}
        assert not vc.check_claims(case, got_vis, got_stats, err, extras), case.name


def test_no_stats_and_two_lists_in_one_buffer(torch_mod, engine):
    a, b, cap = vc.two_lists()
    pa, pb = rc.Packed(a), rc.Packed(b)
    va = vc.host(pa)[0]
    want = vc.host(pb, visibility=va, clear=False)[0]
    got_a, _ = run_case(torch_mod, engine, pa)
    got, none = run_case(torch_mod, engine, pb, visibility=got_a, clear=False, with_stats=False)
    assert none is None and latched(engine) == 0
    assert got_a.tobytes() == va.tobytes() and got.tobytes() == want.tobytes() != va.tobytes()
    for base, count in ((0, cap), (cap, len(pb.commands))):  # resolved once per base
        assert_resolve_equal(f"base {base}", resolve(torch_mod, engine, got, base, count),
                             raster.host_visibility_resolve(want, base, count))
    pix_a, st_a = resolve(torch_mod, engine, got, 0, cap)[1:]
    pix_b, st_b = resolve(torch_mod, engine, got, cap, len(pb.commands))[1:]
    assert int(st_a["foreign_pixels"]) == int(pix_b.sum()) > 0 and int(st_b["foreign_pixels"]) == int(pix_a.sum()) > 0


# -- 2. against the depth call on the device
def test_high_halves_and_stats_are_the_depth_calls_on_the_census(torch_mod, engine):
    for case in CENSUS + NEW:
        pk = rc.Packed(case)
        if (pk.commands["cmd_index_count"] // 3 > 256).any():
            continue  # V3: the two calls differ there by definition (tests/test_raster_visibility_cpu.py holds how)
        opts, (words, mc, data, vb, vcount, ent, vp, w, h) = pk.args()
        depth, dstats = run_depth(torch_mod, engine, words, mc, data, vb, vcount, ent, vp, w, h, cull_none=case.cull_none,
                                  entity_count=opts["entity_count"], data_words=opts["meshlet_data_words"])
        vis, stats = run_case(torch_mod, engine, pk)
        assert high_halves(vis).tobytes() == depth.view(np.uint32).tobytes(), case.name
        assert stats.tobytes() == dstats.tobytes(), case.name
        latched(engine)  # (the R9 cases latch; test 1 holds the status)


@pytest.fixture(scope="module")
def scene100(oracle):
    scene = rs.glb_scene(100)
    w, h = 256, 144
    cam = rs.camera(w, h)
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    n = int(draw[:4].view(np.uint32)[0])
    want = raster.host_raster_visibility(draw, scene.cap_c, scene.meshlet_data, scene.vertices, len(scene.vertices),
                                         scene.entities, rs.view_proj(cam), w, h)
    return scene, cam, w, h, draw, n, want


# -- 3. a scene whose draw list is produced on the device and never read back before the raster
def test_device_draw_list_gives_the_mirrors_buffer_resolve_and_pyramid(torch_mod, engine, scene100):
    torch = torch_mod
    from orbit_amd.engine import depth_pyramid_desc

    scene, cam, w, h, odraw, n, (want_vis, want_stats, err) = scene100
    assert not err.any() and n > 8000
    ds = DeviceScene(torch, scene)
    ci = rs.sc.make_cull_info(cam.view, cam.planes, p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
    disp = torch.zeros(12 + 16 * scene.cap_d, dtype=torch.uint8, device="cuda")
    draw = torch.zeros(4 + 28 * scene.cap_c, dtype=torch.uint8, device="cuda")
    vis, stats = Guarded(torch, np.full(w * h, FILL, np.uint64)), Guarded(torch, np.zeros(0, np.uint8), nbytes=32)
    g = ds.g
    args = (draw, scene.cap_c, g["meshlet_data"].ptr, g["vertices"].ptr, len(scene.vertices), g["entities"].ptr,
            scene.entity_count, rs.view_proj(cam))
    rdepth, pixels, rstats = (Guarded(torch, np.zeros(0, np.uint8), nbytes=k) for k in (4 * w * h, 4 * scene.cap_c, 16))
    pd = depth_pyramid_desc(w, h)
    pyr_vis = torch.zeros(pd.total_texels, dtype=torch.float32, device="cuda")
    pyr_depth = torch.zeros(pd.total_texels, dtype=torch.float32, device="cuda")
    depth = torch.full((h * w,), 7.0, dtype=torch.float32, device="cuda")
    dstats = torch.zeros(32, dtype=torch.uint8, device="cuda")
    ds.cull(torch, engine, ci, disp, draw)
    engine.raster_visibility(*args, vis.ptr, w, h, clear=True, stats=stats.ptr, meshlet_data_words=len(scene.meshlet_data))
    engine.visibility_resolve(vis.ptr, w, h, 0, scene.cap_c, depth=rdepth.ptr, command_pixels=pixels.ptr, stats=rstats.ptr)
    engine.depth_reduce(rdepth.ptr, w, h, pyr_vis)  # the count is still on the device
    engine.raster_depth(*args, depth, w, h, clear=True, stats=dstats, meshlet_data_words=len(scene.meshlet_data))
    engine.depth_reduce(depth, w, h, pyr_depth)
    torch.cuda.synchronize()
    assert latched(engine) == 0
    ds.unchanged()
    assert host(draw)[:4 + 28 * n].tobytes() == odraw[:4 + 28 * n].tobytes()
    got_vis, got_stats = vis.read().view(np.uint64).reshape(h, w), stats.read().view(L.RASTER_STATS)[0]
    assert_equal("scene", got_vis, got_stats, want_vis, want_stats)
    assert int(want_stats["commands"]) == n
    assert_resolve_equal("scene", (rdepth.read().view(np.float32), pixels.read().view(np.uint32), rstats.read().view(L.VIS_STATS)[0]),
                         raster.host_visibility_resolve(want_vis, 0, scene.cap_c))
    assert int(rstats.read().view(L.VIS_STATS)[0]["visible_commands"]) > 1000
    # V4 on the device, and the pyramid of the depth path from the resolve's depth
    assert high_halves(got_vis).tobytes() == host(depth, np.uint32).tobytes() and host(dstats).tobytes() == got_stats.tobytes()
    assert host(pyr_vis).tobytes() == host(pyr_depth).tobytes() and host(pyr_vis, np.float32).max() > 0


# -- 4. order, repetition
def test_shuffled_list_keeps_the_depth_and_a_repeated_call_changes_nothing(torch_mod, engine, scene100):
    torch = torch_mod
    scene, cam, w, h, odraw, n, (want_vis, want_stats, _) = scene100
    _, cmds = L.draw_buffer_commands(odraw)
    rng = np.random.default_rng(11)
    args = (scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, rs.view_proj(cam), w, h)
    words = raster.command_buffer(cmds[rng.permutation(n)])
    shuffled, stats = run(torch, engine, words, n, *args, command_base=77)
    assert high_halves(shuffled).tobytes() == high_halves(want_vis).tobytes() and stats.tobytes() == want_stats.tobytes()
    mirror = raster.host_raster_visibility(words, n, *args, command_base=77)[0]
    assert shuffled.tobytes() == mirror.tobytes() != want_vis.tobytes()
    again, s2 = run(torch, engine, words, n, *args, command_base=77, visibility=shuffled, clear=False)
    assert again.tobytes() == shuffled.tobytes() and s2.tobytes() == stats.tobytes()
    assert latched(engine) == 0


# -- 5. the resolve on buffers built without the rasteriser
def test_resolve_shapes_equal_the_host_mirror(torch_mod, engine):
    for name, vis, base, count in vc.resolve_buffers():
        want = raster.host_visibility_resolve(vis, base, count)
        assert_resolve_equal(name, resolve(torch_mod, engine, vis, base, count), want)
        only_stats = resolve(torch_mod, engine, vis, base, count, want=("stats",))
        assert only_stats[0] is None and only_stats[1] is None
        assert (int(only_stats[2]["covered_pixels"]), int(only_stats[2]["visible_commands"]), int(only_stats[2]["foreign_pixels"])) == \
               (int(want[2]["covered_pixels"]), 0, int(want[2]["foreign_pixels"])), name
        only_depth = resolve(torch_mod, engine, vis, base, count, want=("depth",))
        assert only_depth[0].tobytes() == want[0].tobytes(), name
    assert latched(engine) == 0


# -- 6. the two-pass frame on the visibility call and its resolve alone, every stage against the CPU chain
def test_two_pass_frame_on_the_visibility_call_equals_the_cpu_chain(torch_mod, engine, oracle):
    torch = torch_mod
    from orbit_amd.engine import depth_pyramid_desc

    spec = importlib.util.spec_from_file_location("count_false_occlusion", os.path.join(ROOT, "tools", "count_false_occlusion.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "profiles", "false_occlusion_cpu.json")) as fh:
        committed = json.load(fh)
    scene = rs.glb_scene(tool.INSTANCES)
    w, h = tool.WIDTH, tool.HEIGHT
    cams = [rs.camera(w, h, p) for p in tool.CAMERAS]
    cpu = rs.two_pass_frame(scene, oracle, cams[0], cams[1], w, h)
    ds = DeviceScene(torch, scene)
    g, cap = ds.g, scene.cap_c
    pd = depth_pyramid_desc(w, h)
    evis = torch.zeros((scene.n + 31) // 32, dtype=torch.int32, device="cuda")
    mvis = torch.zeros(scene.vis_words, dtype=torch.int32, device="cuda")
    vis = torch.full((h * w,), 9, dtype=torch.int64, device="cuda")
    depth = torch.full((h * w,), 9.0, dtype=torch.float32, device="cuda")
    pyr = torch.zeros(pd.total_texels, dtype=torch.float32, device="cuda")
    pixels = [torch.full((cap,), 9, dtype=torch.int32, device="cuda") for _ in range(2)]

    def raster_vis(draw, max_commands, cam, target, base, clear):
        engine.raster_visibility(draw, max_commands, g["meshlet_data"].ptr, g["vertices"].ptr, len(scene.vertices),
                                 g["entities"].ptr, scene.entity_count, rs.view_proj(cam), target, w, h, command_base=base,
                                 clear=clear, meshlet_data_words=len(scene.meshlet_data))

    for f, cam in enumerate(cams):
        want = cpu[f]
        draws, depths = [], []
        for p in (1, 2):
            ci = rs.sc.make_cull_info(cam.view, cam.planes, occlusion_pass=p, p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
            disp = torch.zeros(12 + 16 * scene.cap_d, dtype=torch.uint8, device="cuda")
            draw = torch.zeros(4 + 28 * cap, dtype=torch.uint8, device="cuda")
            if p == 2:
                engine.depth_reduce(depth, w, h, pyr)
            ds.cull(torch, engine, ci, disp, draw, evis, mvis, pyr if p == 2 else None, (pd.width, pd.height) if p == 2 else (0, 0))
            raster_vis(draw, cap, cam, vis, (p - 1) * cap, p == 1)  # the late list's ids start at the capacity
            engine.visibility_resolve(vis, w, h, 0, cap, depth=depth, command_pixels=pixels[0] if p == 2 else None)
            draws.append(draw)
            depths.append(depth.clone())
        engine.visibility_resolve(vis, w, h, cap, cap, command_pixels=pixels[1])
        # the unculled list of this camera, for the three counts
        all_words = scene.all_commands(oracle, cam)
        n_all = int(all_words[0])
        vis_all = torch.zeros(h * w, dtype=torch.int64, device="cuda")
        depth_all = torch.zeros(h * w, dtype=torch.float32, device="cuda")
        pixels_all = torch.zeros(n_all, dtype=torch.int32, device="cuda")
        raster_vis(dev(torch, all_words), n_all, cam, vis_all, 0, True)
        engine.visibility_resolve(vis_all, w, h, 0, n_all, depth=depth_all, command_pixels=pixels_all)
        torch.cuda.synchronize()
        assert latched(engine) == 0
        for k, name in enumerate(("draw1", "draw2")):
            n = int(want[name][:4].view(np.uint32)[0])
            assert host(draws[k])[:4 + 28 * n].tobytes() == want[name][:4 + 28 * n].tobytes(), f"frame {f}: {name}"
        assert host(depths[0], np.float32).tobytes() == want["depth1"].tobytes(), f"frame {f}: early depth"
        assert host(depths[1], np.float32).tobytes() == want["depth2"].tobytes(), f"frame {f}: late depth"
        assert host(pyr, np.float32).tobytes() == want["pyramid"].tobytes(), f"frame {f}: pyramid"
        assert np.array_equal(host(evis, np.uint32), want["evis"]) and np.array_equal(host(mvis, np.uint32), want["mvis"])
        counts = tool.frame_counts(host(depths[1], np.float32), host(depth_all, np.float32), tool.command_rows(all_words),
                                   host(pixels_all, np.uint32), tool.command_rows(host(draws[0])), tool.command_rows(host(draws[1])),
                                   host(pixels[0], np.uint32), host(pixels[1], np.uint32))
        print(f"frame {f}: {counts}")
        assert dict(camera=list(tool.CAMERAS[f]), **counts) == committed["frames"][f], f"frame {f}"
    ds.unchanged()


# -- 7. captured into a graph on the first call of a fresh context
def test_the_first_calls_capture_into_a_graph(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine

    by_name = {c.name: c for c in CENSUS + NEW}
    pks = [rc.Packed(by_name[k]) for k in ("fan_at_centre", "nt_256", "tie_between_commands")]
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran either call
    try:
        size = lambda f: max(len(f(p)) for p in pks)  # noqa: E731
        pad = lambda a, n: np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1),  # noqa: E731
                                           np.zeros(n - np.ascontiguousarray(a).nbytes, np.uint8)])
        nb = dict(words=4 * size(lambda p: p.words), data=4 * size(lambda p: p.meshlet_data),
                  vb=size(lambda p: p.vertices), ent=128 * size(lambda p: p.entities))
        g_words, g_data, g_vb, g_ent = (torch.zeros(nb[k], dtype=torch.uint8, device="cuda") for k in ("words", "data", "vb", "ent"))
        vcount, base = nb["vb"] // 12, 500
        vis = torch.full((48 * 64,), 5, dtype=torch.int64, device="cuda")
        stats = torch.full((32,), SENTINEL, dtype=torch.uint8, device="cuda")
        depth = torch.full((48 * 64,), 5.0, dtype=torch.float32, device="cuda")
        pixels = torch.full((3,), 5, dtype=torch.int32, device="cuda")
        rstats = torch.full((16,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.raster_visibility(g_words, 3, g_data, g_vb, vcount, g_ent, 1, rc.pixel_proj(64, 48), vis, 64, 48, command_base=base,
                                  clear=True, stats=stats, meshlet_data_words=nb["data"] // 4)
            eng.visibility_resolve(vis, 64, 48, base, 3, depth=depth, command_pixels=pixels, stats=rstats)
        for pk in pks[:2] + pks[2:] + pks[:1]:  # replayed: new commands, new geometry, the first ones again
            assert pk.vertex_count <= vcount and len(pk.commands) <= 3
            g_words.copy_(dev(torch, pad(pk.words, nb["words"])))
            g_data.copy_(dev(torch, pad(pk.meshlet_data, nb["data"])))
            g_vb.copy_(dev(torch, pad(pk.vertices, nb["vb"])))
            g_ent.copy_(dev(torch, pad(pk.entities, nb["ent"])))
            g.replay()
            torch.cuda.synchronize()
            eng.status()
            want_vis, want_stats, _ = raster.host_raster_visibility(
                pk.words, len(pk.commands), pad(pk.meshlet_data, nb["data"]).view(np.uint32), pad(pk.vertices, nb["vb"]),
                vcount, pad(pk.entities, nb["ent"]), rc.pixel_proj(64, 48), 64, 48, command_base=base, entity_count=1)
            assert_equal(pk.case.name, host(vis, np.uint64).reshape(48, 64), host(stats).view(L.RASTER_STATS)[0], want_vis, want_stats)
            assert_resolve_equal(pk.case.name, (host(depth, np.float32), host(pixels, np.uint32), host(rstats).view(L.VIS_STATS)[0]),
                                 raster.host_visibility_resolve(want_vis, base, 3))
            assert int(want_stats["fragments"]) > 0
    finally:
        eng.close()


# -- argument errors and the empty call
def test_argument_errors_and_the_empty_call(torch_mod, engine):
    torch = torch_mod
    pk = rc.Packed(CENSUS[0])
    _, (words, mc, data, vb, vcount, ent, vp, w, h) = pk.args()
    g = dict(cmd=Guarded(torch, words), dat=Guarded(torch, data), vb=Guarded(torch, vb), ent=Guarded(torch, ent),
             vis=Guarded(torch, np.zeros(0, np.uint8), nbytes=8 * w * h), stats=Guarded(torch, np.zeros(0, np.uint8), nbytes=32))

    def call(**over):
        kw = dict(draw_commands=g["cmd"].ptr, max_commands=mc, meshlet_data=g["dat"].ptr, vertices=g["vb"].ptr, vertex_count=vcount,
                  entity_data=g["ent"].ptr, entity_count=1, view_proj=vp, visibility=g["vis"].ptr, width=w, height=h,
                  stats=g["stats"].ptr, meshlet_data_words=g["dat"].n // 4)
        kw.update(over)
        engine.raster_visibility(**kw)

    top = _lib.VIS_MAX_COMMANDS
    assert engine._lib.orbit_raster_visibility(engine._ctx, None, None) == _lib.E_INVALID
    for over in (dict(draw_commands=None), dict(meshlet_data=None), dict(vertices=None), dict(entity_data=None),
                 dict(visibility=None), dict(visibility=g["vis"].ptr + 4), dict(visibility=g["vis"].ptr + 2),
                 dict(command_base=top - mc + 1), dict(command_base=top), dict(max_commands=top + 1),
                 dict(vertex_stride=8), dict(vertex_stride=14), dict(vertex_stride=32, position_offset=24),
                 dict(vertex_stride=32, position_offset=6), dict(width=0), dict(height=0), dict(width=_lib.RASTER_MAX_DIM + 1),
                 dict(draw_commands=g["cmd"].ptr + 2), dict(meshlet_data=g["dat"].ptr + 1), dict(vertices=g["vb"].ptr + 2),
                 dict(entity_data=g["ent"].ptr + 8), dict(stats=g["stats"].ptr + 1)):
        with pytest.raises(_lib.OrbitError) as e:
            call(**over)
        assert e.value.code == _lib.E_INVALID, over
    j = _lib.RasterVisibility()
    j.flags = 4
    assert engine._lib.orbit_raster_visibility(engine._ctx, j, None) == _lib.E_INVALID
    # the resolve
    out = dict(depth=Guarded(torch, np.zeros(0, np.uint8), nbytes=4 * w * h), pix=Guarded(torch, np.zeros(0, np.uint8), nbytes=16),
               stats=Guarded(torch, np.zeros(0, np.uint8), nbytes=16))

    def res(**over):
        kw = dict(visibility=g["vis"].ptr, width=w, height=h, command_base=0, max_commands=4, depth=out["depth"].ptr,
                  command_pixels=out["pix"].ptr, stats=out["stats"].ptr)
        kw.update(over)
        engine.visibility_resolve(**kw)

    assert engine._lib.orbit_visibility_resolve(engine._ctx, None, None) == _lib.E_INVALID
    for over in (dict(visibility=None), dict(visibility=g["vis"].ptr + 4), dict(depth=None, command_pixels=None, stats=None),
                 dict(depth=out["depth"].ptr + 2), dict(command_pixels=out["pix"].ptr + 1), dict(stats=out["stats"].ptr + 2),
                 dict(width=0), dict(height=0), dict(height=_lib.RASTER_MAX_DIM + 1), dict(command_base=top - 3),
                 dict(command_base=top, max_commands=1)):
        with pytest.raises(_lib.OrbitError) as e:
            res(**over)
        assert e.value.code == _lib.E_INVALID, over
    torch.cuda.synchronize()
    for k in ("vis", "stats"):
        assert (g[k].read() == SENTINEL).all()  # nothing was launched
    for k in out:
        assert (out[k].read() == SENTINEL).all()
    call(command_base=top - mc, clear=True)  # the last base that fits
    call(max_commands=0)  # a merge of nothing: the stats are cleared, the buffer stays
    torch.cuda.synchronize()
    kept = g["vis"].read()
    assert kept.any() and not g["stats"].read().any()
    words0 = words.copy()
    words0[0] = 0
    empty = Guarded(torch, words0)
    call(draw_commands=empty.ptr, clear=True)  # a count of 0 with CLEAR still clears
    torch.cuda.synchronize()
    assert not g["vis"].read().any() and not g["stats"].read().any() and latched(engine) == 0
    call(max_commands=0, clear=True, stats=None)
    res()
    torch.cuda.synchronize()
    assert not g["vis"].read().any() and not out["depth"].read().any() and not out["pix"].read().any() and not out["stats"].read().any()
