"""orbit_fragments_shade_shadowed on the device (include/orbit_abi_ext.h H1-H10) against the host mirror
(orbit_amd.raster.host_fragments_shade_shadowed, which tests/test_fragments_shade_shadowed_cpu.py holds to the numpy
restatement): every hand-built case and tamper, byte for byte, with both forms of the walk where the grid is eligible and
with the library's choice, with and without ORBIT_SHADE_CLEAR, between guards, inputs unchanged; NULL outputs; a
one-workgroup grid; render_mode 8; the argument errors; with no shadowed light the device bytes of orbit_fragments_shade;
the first call of a fresh context captured into a graph and replayed; the whole frame on the device, cascades drawn by
orbit_raster_depth into the atlas.  No test provokes a fault: stale rows and maps are ordinary data that the checks
reject."""
import importlib.util
import os

import numpy as np
import pytest

import fragments_shade_cases as fc
import fragments_shade_shadowed_cases as sc
import raster_cases as rc
import raster_scene as rs
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import Guarded, latched

pytestmark = pytest.mark.gpu
FILL = 0x01010101 * rc.SENTINEL  # the mirror's outputs start as the guards' bytes do
PLANES = ("color", "lights_walked", "shadow_factor", "cascade")


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
def cases(oracle):
    return sc.all_cases(oracle) + [c for c, _ in sc.tampers(oracle)]


def forms_of(case):
    return (None, "per_lane", "staged") if case.staged else (None, "per_lane")


def run(torch, engine, case, clear=False, form=None, render_mode=0, without=()):
    """One orbit_fragments_shade_shadowed call on guarded copies -> the dict of raster.host_fragments_shade_shadowed
    (status: what the context latched); `without`: the optional outputs passed as NULL."""
    a, kw = case.args()
    vis, wp, nrm, mat, mats, lights, image, index_buffer, cc, tile, zs, zb, cutoff, z_near, view_pos, rows, maps, res, brs, nbs, ob = a
    h, w = vis.shape
    inputs = [Guarded(torch, x) for x in (vis, wp, nrm, mat, mats, lights, image, index_buffer, rows, maps)]
    g_vis, g_wp, g_nrm, g_mat, g_mats, g_lights, g_image, g_index, g_rows, g_maps = inputs
    sizes = dict(color=16 * w * h, lights_walked=4 * w * h, stats=32, shadow_factor=4 * w * h, cascade=4 * w * h, shadow_stats=16)
    out = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=n) for k, n in sizes.items()}
    ptr = lambda k: None if k in without else out[k].ptr  # noqa: E731
    engine.fragments_shade_shadowed(g_vis.ptr, w, h, g_wp.ptr, g_nrm.ptr, g_mat.ptr, g_mats.ptr, len(mats), g_lights.ptr, len(lights), g_image.ptr,
                                    g_index.ptr, (np.ascontiguousarray(index_buffer).view(np.uint8).size - 4) // 4, cc, tile, zs, zb, cutoff,
                                    z_near, view_pos, out["color"].ptr, g_rows.ptr, len(rows), g_maps.ptr, len(maps), res, brs, nbs, ob,
                                    shadow_index_base=kw["shadow_index_base"], shadow_factor=ptr("shadow_factor"), cascade=ptr("cascade"),
                                    shadow_stats=ptr("shadow_stats"), lights_walked=ptr("lights_walked"), stats=ptr("stats"),
                                    render_mode=render_mode, clear=clear, form=form)
    torch.cuda.synchronize()
    for g in inputs:
        g.unchanged()
    for k in without:
        out[k].unchanged()
    views = dict(color=(np.float32, (h, w, 4)), lights_walked=(np.uint32, (h, w)), shadow_factor=(np.float32, (h, w)), cascade=(np.uint32, (h, w)))
    got = {k: None if k in without else out[k].read().view(t).reshape(s) for k, (t, s) in views.items()}
    got["stats"] = None if "stats" in without else out["stats"].read().view(L.SHADE_STATS)[0]
    got["shadow_stats"] = None if "shadow_stats" in without else out["shadow_stats"].read().view(L.SHADOW_STATS)[0]
    return dict(got, status=latched(engine))


def mirror(case, clear=False, render_mode=0):
    return sc.mirror(case, clear=clear, render_mode=render_mode, fill=FILL)


def assert_equal(name, got, want):
    for k in ("stats", "shadow_stats"):
        if got[k] is not None:
            assert got[k].tobytes() == want[k].tobytes(), f"{name}: device {k} {got[k]} != host {want[k]}"
    assert got["status"] == want["status"], f"{name}: latched {got['status']}, the mirror says {want['status']}"
    for k in PLANES:
        if got[k] is None:
            continue
        diff = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(diff) == 0, (f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}: device {got[k][tuple(diff[0])]!r}, "
                                f"host {want[k][tuple(diff[0])]!r}")


# -- 1. every case and tamper, each form, with and without CLEAR: bytes, counters, latched status, guards, inputs
@pytest.mark.parametrize("clear", (False, True))
@pytest.mark.parametrize("form", (None, "per_lane", "staged"))
def test_every_case_equals_the_host_mirror(torch_mod, engine, cases, clear, form):
    assert latched(engine) == 0
    written = stale = shadowed = early = evaluations = 0
    for case in cases:
        if form not in forms_of(case):
            continue
        got = run(torch_mod, engine, case, clear=clear, form=form)
        assert_equal(f"{case.name} (clear={clear}, form={form})", got, mirror(case, clear=clear))
        st, sh = got["stats"], got["shadow_stats"]
        written, stale = written + int(st["written_pixels"]), stale + int(st["stale_pixels"])
        shadowed, early, evaluations = shadowed + int(sh["shadowed_pixels"]), early + int(sh["early_out_pixels"]), evaluations + int(sh["shadow_evaluations"])
    assert written > 1500 and stale > 50 and shadowed > 1000 and 100 < early < shadowed < evaluations  # (staged runs the eligible half)


# -- 2. NULL optional outputs, one at a time and all five
def test_null_outputs(torch_mod, engine, cases):
    by_name = {c.name: c for c in cases}
    optional = ("lights_walked", "stats", "shadow_factor", "cascade", "shadow_stats")
    for name in ("shadow_shape_65x8_tile8_res64", "shadow_shape_9x9_tile4_res1", "map_is_map_count_tile8"):
        for form in forms_of(by_name[name]):
            for clear in (False, True):
                full = mirror(by_name[name], clear=clear)
                for without in [(k,) for k in optional] + [optional]:
                    assert_equal(f"{name} without {without}", run(torch_mod, engine, by_name[name], clear=clear, form=form, without=without), full)


# -- 3. render_mode 8: H1 still checks the rows, nothing else of H runs
def test_the_heat_map(torch_mod, engine, cases):
    stale = 0
    for case in cases:
        for form in forms_of(case):
            got = run(torch_mod, engine, case, clear=True, form=form, render_mode=8)
            assert_equal(f"{case.name} heat map (form={form})", got, mirror(case, clear=True, render_mode=8))
            assert not any(got["shadow_stats"])
            stale += int(got["stats"]["stale_pixels"])
    assert stale > 100


# -- 4. a grid of one workgroup
def test_one_workgroup_walks_every_tile(torch_mod, engine, cases):
    by_name = {c.name: c for c in cases}
    engine.set_visibility_grid(1)
    try:
        for name in ("shadow_shape_65x8_tile8_res64", "shadow_shape_65x8_tile4_res2", "positions_tile16", "row_is_shadow_count_tile8"):
            for form in forms_of(by_name[name]):
                for clear in (False, True):
                    assert_equal(f"{name}, one workgroup (clear={clear}, form={form})", run(torch_mod, engine, by_name[name], clear=clear, form=form),
                                 mirror(by_name[name], clear=clear))
    finally:
        engine.set_visibility_grid(0)


def device_job(torch, case):
    """the case's inputs on the device and zeroed outputs -> (inputs: 10 tensors, outputs: dict, the call's other arguments)"""
    a, kw = case.args()
    h, w = a[0].shape
    bufs = [dev(torch, x) for x in a[:8]] + [dev(torch, a[15]), dev(torch, a[16])]
    sizes = dict(color=16 * w * h, lights_walked=4 * w * h, stats=32, shadow_factor=4 * w * h, cascade=4 * w * h, shadow_stats=16)
    outs = {k: torch.zeros(n, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
    return bufs, outs, a, kw


# -- 5. the argument errors, each checked before the context is looked at
def test_argument_errors(torch_mod, engine, cases):
    torch = torch_mod
    case = next(c for c in cases if c.name == "shadow_shape_9x9_tile4_res1")
    bufs, outs, a, kw = device_job(torch, case)
    h, w = a[0].shape
    ic = (np.ascontiguousarray(a[7]).view(np.uint8).size - 4) // 4

    def call(ptrs=None, w_=w, h_=h, cc=a[8], tile=a[9], render_mode=0, form=None, shadow_count=len(a[15]), map_count=len(a[16]), res=a[17], **o):
        p = [b.data_ptr() for b in bufs] if ptrs is None else ptrs
        o = dict({k: v.data_ptr() for k, v in outs.items()}, **o)
        try:
            engine.fragments_shade_shadowed(p[0], w_, h_, p[1], p[2], p[3], p[4], len(a[4]), p[5], len(a[5]), p[6], p[7], ic, cc, tile, a[10], a[11],
                                            a[12], a[13], a[14], o["color"], p[8], shadow_count, p[9], map_count, res, a[18], a[19], a[20],
                                            shadow_index_base=kw["shadow_index_base"], shadow_factor=o["shadow_factor"], cascade=o["cascade"],
                                            shadow_stats=o["shadow_stats"], lights_walked=o["lights_walked"], stats=o["stats"],
                                            render_mode=render_mode, form=form)
        except _lib.OrbitError as e:
            assert "fragments_shade_shadowed:" in str(e), str(e)
            return e.code
        return 0

    ptrs = [b.data_ptr() for b in bufs]
    assert call() == 0
    for k in range(10):  # NULL, misaligned by 4 where more is asked (visibility, materials, lights, image, shadows) or by 2
        assert call(ptrs[:k] + [None] + ptrs[k + 1:]) == _lib.E_INVALID, k
        assert call(ptrs[:k] + [ptrs[k] + (4 if k in (0, 4, 5, 6, 8) else 2)] + ptrs[k + 1:]) == _lib.E_INVALID, k
        for name in ("color", "shadow_factor", "cascade"):
            assert call(**{name: ptrs[k]}) == _lib.E_INVALID, (k, name)  # an output that is an input
    assert call(color=None) == _lib.E_INVALID
    for name in outs:
        assert call(**{name: outs[name].data_ptr() + 2}) == _lib.E_INVALID, name
    assert call(w_=0) == call(h_=0) == call(w_=32769) == _lib.E_INVALID
    for cc in ((0, 3, 12), (3, 3, 33), (1 << 16, 1 << 16, 1)):
        assert call(cc=cc) == _lib.E_INVALID, cc
    assert call(tile=0) == call(render_mode=1) == call(form=8) == call(form=6) == call(form="staged") == _lib.E_INVALID
    assert call(res=0) == call(res=32769) == call(res=32768, map_count=3) == _lib.E_INVALID
    # shadow_count == 0 needs neither pointer nor a resolution: valid, the shadowed lights' pixels stale
    assert call(ptrs[:8] + [None, None], shadow_count=0, map_count=0, res=0) == 0
    torch.cuda.synchronize()
    assert latched(engine) == _lib.E_RANGE
    assert call() == 0 and latched(engine) == 0


# -- 6. with no shadowed light: the device bytes of orbit_fragments_shade on the same job
def test_without_shadowed_lights_it_is_the_old_call(torch_mod, engine, oracle):
    torch = torch_mod
    rows, maps = dev(torch, sc.row()), dev(torch, np.zeros(1, np.float32))
    picked = [c for c in fc.all_cases(oracle) if c.name in ("shape_65x8_tile8", "shape_9x9_tile4", "edges_tile16", "lights_tile8", "32_slices_tile8")]
    assert len(picked) == 5
    for case in picked:
        case = case.copy(case.name)
        case.lights["shadow_data_index"] = 0xFFFFFFFF
        a, _ = case.args()
        h, w = a[0].shape
        bufs = [dev(torch, x) for x in a[:8]]
        ic = (np.ascontiguousarray(a[7]).view(np.uint8).size - 4) // 4
        for form in ((None, "per_lane", "staged") if case.staged else (None, "per_lane")):
            for mode in (0, 8):
                old, new = ([torch.full((n,), 9, dtype=torch.uint8, device="cuda") for n in (16 * w * h, 4 * w * h, 32)] for _ in range(2))
                common = (bufs[0], w, h, bufs[1], bufs[2], bufs[3], bufs[4], len(a[4]), bufs[5], len(a[5]), bufs[6], bufs[7], ic, a[8], a[9], a[10],
                          a[11], a[12], a[13], a[14])
                engine.fragments_shade(*common, old[0], lights_walked=old[1], stats=old[2], render_mode=mode, form=form)
                engine.fragments_shade_shadowed(*common, new[0], rows, 1, maps, 1, 1, 0.3, 0.0, -0.02, lights_walked=new[1], stats=new[2],
                                                render_mode=mode, form=form)
                torch.cuda.synchronize()
                for o, n in zip(old, new):
                    assert host(o).tobytes() == host(n).tobytes(), (case.name, form, mode)
                latched(engine)


# -- 7. captured into a graph as the first call of a fresh context, replayed twice on changed buffers
def test_the_first_call_captures_into_a_graph(torch_mod, cases):
    torch = torch_mod
    from orbit_amd.engine import Engine

    base = next(c for c in cases if c.name == "shadow_shape_65x8_tile8_res64")
    other = base.copy("other planes, another map, a stale row")
    other.case.world_pos, other.maps = base.case.world_pos[::-1].copy(), base.maps[::-1].copy()
    other.case.lights["shadow_data_index"][4] = sc.BASE + 2
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        bufs, outs, a, kw = device_job(torch, base)
        h, w = a[0].shape
        ic = (np.ascontiguousarray(a[7]).view(np.uint8).size - 4) // 4
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.fragments_shade_shadowed(bufs[0], w, h, bufs[1], bufs[2], bufs[3], bufs[4], len(a[4]), bufs[5], len(a[5]), bufs[6], bufs[7], ic, a[8],
                                         a[9], a[10], a[11], a[12], a[13], a[14], outs["color"], bufs[8], len(a[15]), bufs[9], len(a[16]), a[17],
                                         a[18], a[19], a[20], shadow_index_base=kw["shadow_index_base"], shadow_factor=outs["shadow_factor"],
                                         cascade=outs["cascade"], shadow_stats=outs["shadow_stats"], lights_walked=outs["lights_walked"],
                                         stats=outs["stats"], clear=True)
        for c in (base, other, base):  # replayed: new planes, maps and a stale row, the first ones again
            ca = c.args()[0]
            for t, x in zip(bufs, list(ca[:8]) + [ca[15], ca[16]]):
                t.copy_(dev(torch, x))
            want = sc.mirror(c, clear=True)
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == want["status"], c.name
                for k in ("color", "lights_walked", "stats", "shadow_factor", "cascade", "shadow_stats"):
                    assert host(outs[k]).tobytes() == want[k].tobytes(), (c.name, k, replay)
        assert int(want["shadow_stats"]["shadowed_pixels"]) > 100 and want["status"] == 0
    finally:
        eng.close()


# -- 8. the whole frame on the device: four cascades by raster_depth into the atlas, raster_visibility -> visibility_resolve ->
#       compute_clusters -> visibility_surface_drawn -> surface_fragments (clear) -> fragments_shade_shadowed, nothing copied
#       to the host in between
def count_tool():
    spec = importlib.util.spec_from_file_location("count_fragments_shade_shadowed", os.path.join(rs.ROOT, "tools", "count_fragments_shade_shadowed.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_frame_on_the_device(torch_mod, engine, oracle):
    torch = torch_mod
    assert latched(engine) == 0
    tool = count_tool()
    base = tool._tool("count_fragments_shade")
    f = tool.host_frame(oracle)
    scene, frame, w, h, cap = f["scene"], f["frame"], f["width"], f["height"], f["scene"].cap_c
    vp, cc, res = frame["view_proj"], f["cluster_count"], f["atlas"].shape[-1]
    meshlets = np.ascontiguousarray(scene.meshlets).view(np.uint8).reshape(-1)
    d_data, d_pos, d_rows, d_ent, d_mlt = (dev(torch, x) for x in (scene.meshlet_data, scene.vertices, f["rows"], scene.entities, meshlets))
    d_shadow = dev(torch, f["shadow_rows"])
    d_lists = [dev(torch, frame[n]) for n in ("draw1", "draw2")]
    d_casters = dev(torch, f["casters"])
    d_lights, d_materials = dev(torch, f["lights"]), dev(torch, scene.materials)
    vcount, ecount = len(scene.vertices), scene.entity_count
    kw = dict(clip_near=True, wide_guard=True)
    atlas = torch.full((4, res, res), 7.0, dtype=torch.float32, device="cuda")
    raster.shadow_atlas(engine, atlas, d_casters, f["max_casters"], d_data, d_pos, vcount, d_ent, ecount, [m for m, _ in f["cascades"]], res,
                        cull_none=True, meshlet_data_words=len(scene.meshlet_data), **kw)
    vis = torch.zeros(w * h, dtype=torch.int64, device="cuda")
    depth = torch.zeros(w * h, dtype=torch.float32, device="cuda")
    surf = dict(bary=torch.zeros(2 * w * h, dtype=torch.float32, device="cuda"), grad=torch.zeros(4 * w * h, dtype=torch.float32, device="cuda"),
                triangle=torch.zeros(4 * w * h, dtype=torch.int32, device="cuda"))
    planes = dict(world_pos=torch.zeros(4 * w * h, dtype=torch.float32, device="cuda"), normal=torch.zeros(3 * w * h, dtype=torch.float32, device="cuda"),
                  material=torch.zeros(w * h, dtype=torch.int32, device="cuda"))
    clusters, capacity = cc[0] * cc[1] * cc[2], f["index_capacity"]
    masks = torch.zeros(cc[0] * cc[1], dtype=torch.int32, device="cuda")
    bounds, image = (torch.zeros((clusters, 2), dtype=torch.int32, device="cuda") for _ in range(2))
    unique = torch.zeros(L.COMPACT_HEADER + 4 * clusters, dtype=torch.uint8, device="cuda")
    lists = torch.zeros(L.LIGHT_INDEX_HEADER + 4 * capacity, dtype=torch.uint8, device="cuda")
    color = torch.full((4 * w * h,), 7, dtype=torch.float32, device="cuda")
    walked, cascade = (torch.full((w * h,), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    factor = torch.full((w * h,), 7, dtype=torch.float32, device="cuda")
    stats, shadow_stats = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    for k, d in enumerate(d_lists):
        engine.raster_visibility(d, cap, d_data, d_pos, vcount, d_ent, ecount, vp, vis, w, h, command_base=k * cap, clear=k == 0,
                                 meshlet_data_words=len(scene.meshlet_data), **kw)
    engine.visibility_resolve(vis, w, h, depth=depth)
    engine.compute_clusters(f["push"], f["info"], depth, d_lights, masks, bounds, unique, clusters, lists, capacity, image)
    for k, d in enumerate(d_lists):
        engine.visibility_surface_drawn(vis, w, h, d, cap, d_data, d_pos, vcount, d_ent, ecount, vp, **surf, command_base=k * cap, clear=k == 0,
                                        meshlet_data_words=len(scene.meshlet_data), **kw)
    for k, d in enumerate(d_lists):
        engine.surface_fragments(vis, w, h, d, cap, d_mlt, len(meshlets) // 32, surf["bary"], surf["triangle"], d_rows, vcount, d_ent, ecount,
                                 **planes, command_base=k * cap, clear=k == 0)
    s = f["settings"]
    engine.fragments_shade_shadowed(vis, w, h, planes["world_pos"], planes["normal"], planes["material"], d_materials, len(scene.materials), d_lights,
                                    len(f["lights"]), image, lists, capacity, cc, base.TILE, f["z_scale"], f["z_bias"], base.CUTOFF,
                                    frame["cam"].z_near, f["view_pos"], color, d_shadow, 1, atlas, 4, res, s["blocker_search_radius"],
                                    s["normal_bias_scale"], s["oriented_bias"], shadow_index_base=f["shadow_index_base"], shadow_factor=factor,
                                    cascade=cascade, shadow_stats=shadow_stats, lights_walked=walked, stats=stats, clear=True)
    torch.cuda.synchronize()
    assert latched(engine) == 0
    assert host(atlas, np.float32).tobytes() == f["atlas"].tobytes()  # the maps the device drew are the host raster's
    want = raster.host_fragments_shade_shadowed(*f["args"], **f["kw"])
    assert want["status"] == 0 and f["dropped"] == 0
    got = dict(color=host(color, np.float32).reshape(h, w, 4), lights_walked=host(walked, np.uint32).reshape(h, w),
               shadow_factor=host(factor, np.float32).reshape(h, w), cascade=host(cascade, np.uint32).reshape(h, w),
               stats=host(stats, np.uint32).view(L.SHADE_STATS)[0], shadow_stats=host(shadow_stats, np.uint32).view(L.SHADOW_STATS)[0], status=0)
    assert_equal("the frame", got, want)
    sh = got["shadow_stats"]
    assert int(sh["shadowed_pixels"]) == int(got["stats"]["written_pixels"]) > 40000 and 0 < int(sh["early_out_pixels"]) < int(sh["shadowed_pixels"])
    assert ((got["shadow_factor"] > 0) & (got["shadow_factor"] < 1)).any() and int(got["stats"]["unserved_pixels"]) == 0
