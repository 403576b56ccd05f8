"""ORBIT_RASTER_WIDE_GUARD on the MI355X (include/orbit_abi_ext.h R4w): the depth bytes, the visibility
words, the counters and the latched status of the two flagged raster calls equal the host mirror's (orbit_amd.raster on
the same buffers — never a restatement; tests/test_raster_wide_cpu.py holds the mirror to tests/raster_wide_ref.py) on
every case of tests/raster_wide_cases.py, with and without ORBIT_RASTER_CLIP_NEAR as the case asks; V4 holds with the
flag on both calls; flagged and unflagged calls back to back on one context; the camera inside the glTF scene and its
two-pass frame; a flagged call captured into a graph as a fresh context's first call; an unknown flag word launches
nothing.  Every buffer sits between sentinel guards; inputs come back unchanged."""
import importlib.util
import os

import numpy as np
import pytest

import raster_cases as rc
import raster_scene as rs
import raster_wide_cases as wc
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import DeviceScene, Guarded, latched

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = rc.SENTINEL
CASES = wc.all_cases()
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


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("count_near_clip", os.path.join(ROOT, "tools", "count_near_clip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def high_halves(vis):
    return (np.asarray(vis, np.uint64) >> np.uint64(32)).astype(np.uint32)


def run(torch, engine, kind, words, max_commands, data, vertices, vertex_count, entities, view_proj, width, height,
        target=None, command_base=0, clear=True, cull_none=False, clip_near=False, wide_guard=True, stride=12, offset=0,
        entity_count=None, data_words=None):
    """One raster call (`kind`: "depth" or "visibility") on guarded copies -> (target (h, w), stats row)."""
    cmd, dat, vb, ent = Guarded(torch, words), Guarded(torch, data), Guarded(torch, vertices), Guarded(torch, entities)
    dtype = np.float32 if kind == "depth" else np.uint64
    fill = np.full(width * height, np.float32(0.123) if kind == "depth" else FILL, dtype)
    out = Guarded(torch, fill if target is None else np.ascontiguousarray(target, dtype))
    st = Guarded(torch, np.zeros(0, np.uint8), nbytes=32)  # sentinel-filled: the call clears it
    common = dict(clear=clear, cull_none=cull_none, clip_near=clip_near, wide_guard=wide_guard, stats=st.ptr, vertex_stride=stride,
                  position_offset=offset, meshlet_data_words=dat.n // 4 if data_words is None else data_words)
    args = (cmd.ptr, max_commands, dat.ptr, vb.ptr, vertex_count, ent.ptr, ent.n // 128 if entity_count is None else entity_count,
            view_proj, out.ptr, width, height)
    if kind == "depth":
        engine.raster_depth(*args, **common)
    else:
        engine.raster_visibility(*args, command_base=command_base, **common)
    torch.cuda.synchronize()
    for g in (cmd, dat, vb, ent):
        g.unchanged()
    return out.read().view(dtype).reshape(height, width), st.read().view(L.RASTER_STATS)[0]


def run_case(torch, engine, kind, pk, **kw):
    opts, (words, mc, data, vb, vcount, ent, vp, w, h) = pk.args()
    kw.setdefault("clip_near", getattr(pk.case, "clip_near", False))
    return run(torch, engine, kind, words, mc, data, vb, vcount, ent, vp, w, h, command_base=getattr(pk.case, "command_base", 0),
               cull_none=pk.case.cull_none, stride=pk.stride, offset=pk.offset, entity_count=opts["entity_count"],
               data_words=opts["meshlet_data_words"], **kw)


def assert_equal(name, got, got_stats, want, want_stats):
    assert got_stats.tobytes() == want_stats.tobytes(), f"{name}: device stats {got_stats} != host {want_stats}"
    view = np.uint32 if got.dtype == np.float32 else np.uint64
    diff = np.argwhere(got.view(view) != want.view(view))
    assert len(diff) == 0, (f"{name}: {len(diff)} pixels differ, first at (y, x) = {diff[0]}: device "
                            f"{int(got.view(view)[tuple(diff[0])]):#x}, host {int(want.view(view)[tuple(diff[0])]):#x}")


# -- 1. every case: depth bytes, visibility words, counters, latched status; V4 on the device
@pytest.mark.parametrize("stride,offset", [(12, 0), (32, 20)])
def test_every_case_equals_the_host_mirror(torch_mod, engine, stride, offset):
    assert latched(engine) == 0
    for case in CASES:
        pk = rc.Packed(case, stride, offset)
        want_vis, want_vstats, err = wc.host_vis(pk)
        want_depth, want_dstats, _ = wc.host_depth(pk)
        got_vis, got_vstats = run_case(torch_mod, engine, "visibility", pk)
        got_depth, got_dstats = run_case(torch_mod, engine, "depth", pk)
        assert latched(engine) == (_lib.E_RANGE if err.any() else 0), case.name
        assert_equal(case.name, got_vis, got_vstats, want_vis, want_vstats)
        assert_equal(case.name, got_depth, got_dstats, want_depth, want_dstats)
        assert high_halves(got_vis).tobytes() == got_depth.view(np.uint32).tobytes(), case.name
        assert got_vstats.tobytes() == got_dstats.tobytes(), case.name
        # (None: the route is claimed on the restatement's extras, on the CPU)
        assert not wc.check_claims(case, got_vis, got_vstats, err, None), case.name


def test_flagged_and_unflagged_calls_back_to_back_and_a_loaded_buffer_merges(torch_mod, engine):
    """One context, the kernels in alternation: without the flag a case's wide triangles stay guard_skipped (the
    earlier kernels, with or without CLIP_NEAR), with it they are drawn; then a flagged call without CLEAR into the
    buffer an unflagged call left."""
    for case in CASES[::4]:
        pk = rc.Packed(case)
        for kind, host_call in (("depth", wc.host_depth), ("visibility", wc.host_vis)):
            for wide in (False, True, False):
                want, want_stats, _ = host_call(pk, wide=wide)
                got, got_stats = run_case(torch_mod, engine, kind, pk, wide_guard=wide)
                assert_equal(f"{case.name}, wide_guard={wide}", got, got_stats, want, want_stats)
    by_name = {c.name: c for c in CASES}
    pk, left = rc.Packed(by_name["fan_of_wide_triangles"]), rc.Packed(by_name["strip_of_narrow_and_wide"])
    for kind, host_call in (("depth", wc.host_depth), ("visibility", wc.host_vis)):
        before, _ = run_case(torch_mod, engine, kind, left, wide_guard=False)
        assert before.view(np.uint8).any()
        want, want_stats, _ = host_call(pk, before, clear=False)
        got, got_stats = run_case(torch_mod, engine, kind, pk, target=before, clear=False)
        assert_equal(f"load {kind}", got, got_stats, want, want_stats)
        assert got.tobytes() != before.tobytes()
    assert latched(engine) == 0


# -- 2. the camera inside the scene: both calls with flags 8 | 32, and the two-pass frame
def test_inside_camera_scene_both_calls(torch_mod, engine, oracle, tool):
    scene = rs.glb_scene(tool.INSTANCES)
    w, h = 256, 144
    cam = rs.camera(w, h, tool.CAMERAS[1])
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    n = int(draw[:4].view(np.uint32)[0])
    args = (scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, rs.view_proj(cam), w, h)
    want_vis, want_stats, err = raster.host_raster_visibility(draw, n, *args, clip_near=True, wide_guard=True)
    _, clip_stats, _ = raster.host_raster_visibility(draw, n, *args, clip_near=True)
    assert not err.any() and int(want_stats["guard_skipped"]) == 0 and int(clip_stats["guard_skipped"]) >= 100
    words = np.ascontiguousarray(draw).view(np.uint8)[:4 + 28 * n]
    got_vis, got_stats = run(torch_mod, engine, "visibility", words, n, *args, clip_near=True)
    assert_equal("inside, visibility", got_vis, got_stats, want_vis, want_stats)
    got_depth, got_dstats = run(torch_mod, engine, "depth", words, n, *args, clip_near=True)
    want_depth, want_dstats, _ = raster.host_raster_depth(draw, n, *args, clip_near=True, wide_guard=True)
    assert_equal("inside, depth", got_depth, got_dstats, want_depth, want_dstats)
    assert high_halves(got_vis).tobytes() == got_depth.view(np.uint32).tobytes() and got_stats.tobytes() == got_dstats.tobytes()
    # the unculled list with CULL_NONE: every triangle that leaves the guard band reaches the wide walk
    all_words = scene.all_commands(oracle, cam)
    want_all, want_all_stats, _ = raster.host_raster_visibility(all_words, int(all_words[0]), *args, clip_near=True, wide_guard=True,
                                                                cull_none=True)
    got_all, got_all_stats = run(torch_mod, engine, "visibility", all_words, int(all_words[0]), *args, clip_near=True, cull_none=True)
    assert_equal("inside, unculled", got_all, got_all_stats, want_all, want_all_stats)
    assert latched(engine) == 0


def test_inside_camera_two_pass_frame_on_the_device(torch_mod, engine, oracle, tool):
    """The two-pass frame of tools/count_near_clip.py with flags 8 | 32 on both raster calls on the device: every stage
    equals the CPU chain, so its counts — nothing lost to occlusion, no triangle guard_skipped — are the device's."""
    torch = torch_mod
    from orbit_amd.engine import depth_pyramid_desc

    scene = rs.glb_scene(tool.INSTANCES)
    w, h = 256, 144
    cams = [rs.camera(w, h, p) for p in tool.CAMERAS]
    counts, cpu, depth_all = tool.frame_counts(scene, oracle, cams, w, h, True, wide_guard=True)
    assert counts["missing_by_occlusion"] == 0 and counts["false_occlusion_pixels_vs_pass0"] == 0 and counts["guard_skipped"] == 0
    ds = DeviceScene(torch, scene)
    g, cap = ds.g, scene.cap_c
    pd = depth_pyramid_desc(w, h)
    evis = torch.zeros((scene.n + 31) // 32, dtype=torch.int32, device="cuda")
    mvis = torch.zeros(scene.vis_words, dtype=torch.int32, device="cuda")
    depth = torch.full((h * w,), 9.0, dtype=torch.float32, device="cuda")
    pyr = torch.zeros(pd.total_texels, dtype=torch.float32, device="cuda")
    for cam in cams:
        draws = []
        for p in (1, 2):
            ci = rs.sc.make_cull_info(cam.view, cam.planes, occlusion_pass=p, p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
            disp = torch.zeros(12 + 16 * scene.cap_d, dtype=torch.uint8, device="cuda")
            draw = torch.zeros(4 + 28 * cap, dtype=torch.uint8, device="cuda")
            if p == 2:
                engine.depth_reduce(depth, w, h, pyr)
            ds.cull(torch, engine, ci, disp, draw, evis, mvis, pyr if p == 2 else None, (pd.width, pd.height) if p == 2 else (0, 0))
            engine.raster_depth(draw, cap, g["meshlet_data"].ptr, g["vertices"].ptr, len(scene.vertices), g["entities"].ptr,
                                scene.entity_count, rs.view_proj(cam), depth, w, h, clear=p == 1, clip_near=True, wide_guard=True,
                                meshlet_data_words=len(scene.meshlet_data))
            draws.append(draw)
    torch.cuda.synchronize()
    assert latched(engine) == 0
    for k, name in enumerate(("draw1", "draw2")):  # the last camera's frame
        n = int(cpu[name][:4].view(np.uint32)[0])
        assert host(draws[k])[:4 + 28 * n].tobytes() == cpu[name][:4 + 28 * n].tobytes(), name
    assert host(depth, np.float32).tobytes() == cpu["depth2"].tobytes()
    assert int((host(depth, np.float32) < depth_all.reshape(-1)).sum()) == counts["false_occlusion_pixels"]
    ds.unchanged()


# -- 3. captured into a graph as a fresh context's first call, replayed with new geometry
def test_a_flagged_first_call_captures_into_a_graph(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine

    by_name = {c.name: c for c in CASES}
    pks = [rc.Packed(by_name[k]) for k in ("fan_of_wide_triangles", "wide_in_the_second_chunk", "strip_of_narrow_and_wide")]
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran a raster call
    try:
        size = lambda f: max(len(f(p)) for p in pks)  # noqa: E731
        pad = lambda a, n: np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1),  # noqa: E731
                                           np.zeros(n - np.ascontiguousarray(a).nbytes, np.uint8)])
        nb = dict(words=4 * size(lambda p: p.words), data=4 * size(lambda p: p.meshlet_data),
                  vb=size(lambda p: p.vertices), ent=128 * size(lambda p: p.entities))
        g_words, g_data, g_vb, g_ent = (torch.zeros(nb[k], dtype=torch.uint8, device="cuda") for k in ("words", "data", "vb", "ent"))
        vcount, vp = nb["vb"] // 12, wc.sub_proj()
        vis = torch.full((48 * 64,), 5, dtype=torch.int64, device="cuda")
        stats = torch.full((32,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.raster_visibility(g_words, 1, g_data, g_vb, vcount, g_ent, 1, vp, vis, 64, 48, command_base=3, clear=True,
                                  cull_none=True, wide_guard=True, stats=stats, meshlet_data_words=nb["data"] // 4)
        for pk in pks:  # replayed: new commands and geometry each time
            assert pk.vertex_count <= vcount and len(pk.commands) == 1
            g_words.copy_(dev(torch, pad(pk.words, nb["words"])))
            g_data.copy_(dev(torch, pad(pk.meshlet_data, nb["data"])))
            g_vb.copy_(dev(torch, pad(pk.vertices, nb["vb"])))
            g_ent.copy_(dev(torch, pad(pk.entities, nb["ent"])))
            g.replay()
            torch.cuda.synchronize()
            eng.status()
            want_vis, want_stats, _ = raster.host_raster_visibility(
                pk.words, 1, pad(pk.meshlet_data, nb["data"]).view(np.uint32), pad(pk.vertices, nb["vb"]), vcount,
                pad(pk.entities, nb["ent"]), vp, 64, 48, command_base=3, cull_none=True, wide_guard=True, entity_count=1)
            assert_equal(pk.case.name, host(vis, np.uint64).reshape(48, 64), host(stats).view(L.RASTER_STATS)[0], want_vis, want_stats)
            assert int(want_stats["fragments"]) > 0 and int(want_stats["guard_skipped"]) == 0
    finally:
        eng.close()


# -- 4. bits 2 and 4 are still no flags
def test_an_invalid_flag_word_launches_nothing(torch_mod, engine):
    torch = torch_mod
    pk = rc.Packed(CASES[1])
    _, (words, mc, data, vb, vcount, ent, vp, w, h) = pk.args()
    g = dict(cmd=Guarded(torch, words), dat=Guarded(torch, data), vb=Guarded(torch, vb), ent=Guarded(torch, ent),
             depth=Guarded(torch, np.zeros(0, np.uint8), nbytes=4 * w * h), vis=Guarded(torch, np.zeros(0, np.uint8), nbytes=8 * w * h),
             stats=Guarded(torch, np.zeros(0, np.uint8), nbytes=32))
    import ctypes as C

    jobs = ((_lib.RasterDepth(), engine._lib.orbit_raster_depth, "depth"),
            (_lib.RasterVisibility(), engine._lib.orbit_raster_visibility, "visibility"))
    for job, call, target in jobs:
        job.draw_commands, job.meshlet_data, job.vertices, job.entity_data = g["cmd"].ptr, g["dat"].ptr, g["vb"].ptr, g["ent"].ptr
        setattr(job, target, g["depth" if target == "depth" else "vis"].ptr)
        job.stats, job.meshlet_data_words, job.vertex_count = g["stats"].ptr, g["dat"].n // 4, vcount
        job.max_commands, job.entity_count, job.vertex_stride, job.position_offset, job.width, job.height = mc, 1, 12, 0, w, h
        job.view_proj = (C.c_float * 16)(*vp)
        for flags in (4, 16, 36, 48, 64 | _lib.RASTER_WIDE_GUARD):
            job.flags = flags
            assert call(engine._ctx, C.byref(job), None) == _lib.E_INVALID, flags
    torch.cuda.synchronize()
    for k in ("depth", "vis", "stats"):
        assert (g[k].read() == SENTINEL).all()  # nothing was launched
    for job, call, target in jobs:  # the same jobs with known flag words run
        for flags in (33, 34 | _lib.RASTER_CLEAR, 40 | _lib.RASTER_CLEAR):
            job.flags = flags
            assert call(engine._ctx, C.byref(job), None) == 0
    torch.cuda.synchronize()
    assert not (g["depth"].read() == SENTINEL).all() and not (g["vis"].read() == SENTINEL).all()
    assert latched(engine) == 0
