"""orbit_fragments_shade on the device (include/orbit_abi_ext.h L1-L9) against the host mirror
(orbit_amd.raster.host_fragments_shade, which tests/test_fragments_shade_cpu.py holds to the numpy restatement): every
hand-built case and tamper, byte for byte, with both forms of the walk where the grid is eligible and with the library's
choice, with and without ORBIT_SHADE_CLEAR, between guards, inputs unchanged; NULL outputs; a one-workgroup grid;
render_mode 8; the argument errors; the first call of a fresh context captured into a graph and replayed; the whole frame
on the device, where shading from the cluster lists equals shading from all lights.  No test provokes a fault: stale
records are ordinary data that the checks reject."""
import importlib.util
import os

import numpy as np
import pytest

import fragments_shade_cases as fc
import raster_cases as rc
import raster_scene as rs
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import Guarded, latched

pytestmark = pytest.mark.gpu
FILL = 0x01010101 * rc.SENTINEL  # the mirror's outputs start as the guards' bytes do


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
    return fc.all_cases(oracle) + [c for c, _ in fc.tampers(oracle)]


def forms_of(case):
    return (None, "per_lane", "staged") if case.staged else (None, "per_lane")


def counts_of(a, kw):
    return (kw.get("material_count", len(a[4])), kw.get("light_count", len(a[5])),
            kw.get("index_capacity", (np.ascontiguousarray(a[7]).view(np.uint8).size - 4) // 4))


def run(torch, engine, case, clear=False, form=None, render_mode=0, with_walked=True, with_stats=True):
    """One orbit_fragments_shade call on guarded copies -> the dict of raster.host_fragments_shade (status: what the
    context latched)."""
    a, kw = case.args()
    vis, wp, nrm, mat, mats, lights, image, index_buffer, cc, tile, zs, zb, cutoff, z_near, view_pos = a
    h, w = vis.shape
    inputs = [Guarded(torch, x) for x in (vis, wp, nrm, mat, mats, lights, image, index_buffer)]
    g_vis, g_wp, g_nrm, g_mat, g_mats, g_lights, g_image, g_index = inputs
    color, walked, stats = (Guarded(torch, np.zeros(0, np.uint8), nbytes=n) for n in (16 * w * h, 4 * w * h, 32))
    mc, lc, ic = counts_of(a, kw)
    engine.fragments_shade(g_vis.ptr, w, h, g_wp.ptr, g_nrm.ptr, g_mat.ptr, g_mats.ptr, mc, g_lights.ptr, lc, g_image.ptr, g_index.ptr, ic, cc,
                           tile, zs, zb, cutoff, z_near, view_pos, color.ptr, lights_walked=walked.ptr if with_walked else None,
                           stats=stats.ptr if with_stats else None, render_mode=render_mode, clear=clear, form=form)
    torch.cuda.synchronize()
    for g in inputs:
        g.unchanged()
    if not with_walked:
        walked.unchanged()
    if not with_stats:
        stats.unchanged()
    return dict(color=color.read().view(np.float32).reshape(h, w, 4), lights_walked=walked.read().view(np.uint32).reshape(h, w) if with_walked else None,
                stats=stats.read().view(L.SHADE_STATS)[0] if with_stats else None, status=latched(engine))


def mirror(case, clear=False, render_mode=0):
    return fc.mirror(case, clear=clear, render_mode=render_mode, fill=FILL)


def assert_equal(name, got, want):
    if got["stats"] is not None:
        assert got["stats"].tobytes() == want["stats"].tobytes(), f"{name}: device stats {got['stats']} != host {want['stats']}"
    assert got["status"] == want["status"], f"{name}: latched {got['status']}, the mirror says {want['status']}"
    for k in ("color", "lights_walked"):
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
    written = stale = degenerate = unserved = 0
    for case in cases:
        if form not in forms_of(case):
            continue
        got = run(torch_mod, engine, case, clear=clear, form=form)
        assert_equal(f"{case.name} (clear={clear}, form={form})", got, mirror(case, clear=clear))
        st = got["stats"]
        written, stale = written + int(st["written_pixels"]), stale + int(st["stale_pixels"])
        degenerate, unserved = degenerate + int(st["degenerate_pixels"]), unserved + int(st["unserved_pixels"])
    assert written > 2000 and stale > 100 and degenerate >= 2 and unserved > 100  # (the staged form runs the eligible half)


# -- 2. NULL lights_walked and NULL stats
def test_null_outputs(torch_mod, engine, cases):
    by_name = {c.name: c for c in cases}
    for name in ("shape_65x8_tile8", "shape_9x9_tile4", "edges_tile16", "bad_index_at_64_tile8"):
        for form in forms_of(by_name[name]):
            for clear in (False, True):
                full = mirror(by_name[name], clear=clear)
                assert_equal(f"{name} without lights_walked", run(torch_mod, engine, by_name[name], clear=clear, form=form, with_walked=False), full)
                assert_equal(f"{name} without stats", run(torch_mod, engine, by_name[name], clear=clear, form=form, with_stats=False), full)


# -- 3. render_mode 8
def test_the_heat_map(torch_mod, engine, cases):
    colours = set()
    for case in cases:
        for form in forms_of(case):
            got = run(torch_mod, engine, case, clear=True, form=form, render_mode=8)
            assert_equal(f"{case.name} heat map (form={form})", got, mirror(case, clear=True, render_mode=8))
            colours |= {bytes(c) for c in got["color"].reshape(-1, 4)[::7].view(np.uint8)}
    assert len(colours) > 4


# -- 4. a grid of one workgroup
def test_one_workgroup_walks_every_tile(torch_mod, engine, cases):
    by_name = {c.name: c for c in cases}
    engine.set_visibility_grid(1)
    try:
        for name in ("shape_65x8_tile8", "shape_65x8_tile4", "edges_tile16", "32_slices_tile8", "bad_index_at_255_tile8"):
            for form in forms_of(by_name[name]):
                for clear in (False, True):
                    assert_equal(f"{name}, one workgroup (clear={clear}, form={form})", run(torch_mod, engine, by_name[name], clear=clear, form=form),
                                 mirror(by_name[name], clear=clear))
    finally:
        engine.set_visibility_grid(0)


# -- 5. the argument errors, each checked before the context is looked at
def test_argument_errors(torch_mod, engine, cases):
    torch = torch_mod
    case = next(c for c in cases if c.name == "shape_9x9_tile4")
    a, kw = case.args()
    h, w = a[0].shape
    bufs = [dev(torch, x) for x in a[:8]]
    color, walked, stats = (torch.zeros(n, dtype=torch.uint8, device="cuda") for n in (16 * w * h, 4 * w * h, 32))
    mc, lc, ic = counts_of(a, kw)

    def call(ptrs=None, color_=color, walked_=walked, stats_=stats, w_=w, h_=h, cc=a[8], tile=a[9], render_mode=0, form=None):
        p = [b.data_ptr() for b in bufs] if ptrs is None else ptrs
        try:
            engine.fragments_shade(p[0], w_, h_, p[1], p[2], p[3], p[4], mc, p[5], lc, p[6], p[7], ic, cc, tile, a[10], a[11], a[12], a[13], a[14],
                                   color_, lights_walked=walked_, stats=stats_, render_mode=render_mode, form=form)
        except _lib.OrbitError as e:
            return e.code
        return 0

    ptrs = [b.data_ptr() for b in bufs]
    assert call() == 0
    for k in range(8):  # NULL, and misaligned by 4 where more is asked (visibility, materials, lights, image) or by 2
        assert call(ptrs[:k] + [None] + ptrs[k + 1:]) == _lib.E_INVALID, k
        assert call(ptrs[:k] + [ptrs[k] + (4 if k in (0, 4, 5, 6) else 2)] + ptrs[k + 1:]) == _lib.E_INVALID, k
        assert call(color_=ptrs[k]) == _lib.E_INVALID, k  # an output that is an input
    assert call(color_=None) == _lib.E_INVALID
    assert call(color_=color.data_ptr() + 2) == _lib.E_INVALID and call(walked_=walked.data_ptr() + 1) == _lib.E_INVALID
    assert call(w_=0) == call(h_=0) == call(w_=32769) == _lib.E_INVALID
    for cc in ((0, 3, 12), (3, 0, 12), (3, 3, 0), (3, 3, 33), (1 << 16, 1 << 16, 1)):
        assert call(cc=cc) == _lib.E_INVALID, cc
    assert call(tile=0) == _lib.E_INVALID
    assert call(render_mode=1) == call(render_mode=9) == _lib.E_INVALID
    assert call(form=8) == call(form=6) == _lib.E_INVALID  # an unknown flag; both forms
    assert call(form="staged") == _lib.E_INVALID  # tile_size_px 4
    assert call() == 0 and latched(engine) == 0


# -- 6. captured into a graph as the first call of a fresh context, replayed twice on changed buffers
def test_the_first_call_captures_into_a_graph(torch_mod, cases):
    torch = torch_mod
    from orbit_amd.engine import Engine

    base = next(c for c in cases if c.name == "shape_65x8_tile8")
    other = base.copy("other planes, one stale material")
    other.world_pos, other.normal = base.world_pos[::-1].copy(), base.normal[:, ::-1].copy()
    other.material[2, 5] = len(other.materials)
    picked = [base, other, base]  # replayed: new planes and a stale pixel, the first ones again
    w, h, cc = 65, 8, base.cluster_count
    nbytes = lambda x: np.ascontiguousarray(x).view(np.uint8).size  # noqa: E731
    sizes = [max(nbytes(c.args()[0][k]) for c in picked) for k in range(8)]

    def padded(x, n):
        out = np.zeros(n, np.uint8)
        x = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        out[:len(x)] = x
        return out

    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        z = lambda n: torch.full(((n + 15) // 16 * 16,), 5, dtype=torch.uint8, device="cuda")  # noqa: E731
        g_in = [z(n) for n in sizes]
        color, walked, stats = z(16 * w * h), z(4 * w * h), z(32)
        a0 = picked[0].args()[0]
        mc, lc, ic = sizes[4] // 80, sizes[5] // 64, (sizes[7] - 4) // 4
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.fragments_shade(g_in[0], w, h, g_in[1], g_in[2], g_in[3], g_in[4], mc, g_in[5], lc, g_in[6], g_in[7], ic, cc, 8, a0[10], a0[11],
                                a0[12], a0[13], a0[14], color, lights_walked=walked, stats=stats, clear=True)
        for c in picked:
            a = list(c.args()[0])
            full = [padded(a[k], sizes[k]) for k in range(8)]
            for t, x in zip(g_in, full):
                t[:len(x)].copy_(torch.from_numpy(x).cuda())
            want = raster.host_fragments_shade(a[0], a[1], a[2], a[3], full[4], full[5], full[6], full[7], *a[8:], material_count=mc, light_count=lc,
                                               index_capacity=ic)
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == want["status"], c.name
                assert host(color)[:want["color"].nbytes].tobytes() == want["color"].tobytes(), (c.name, replay)
                assert host(walked)[:want["lights_walked"].nbytes].tobytes() == want["lights_walked"].tobytes(), (c.name, replay)
                assert host(stats)[:32].tobytes() == want["stats"].tobytes(), c.name
        assert int(want["stats"]["written_pixels"]) > 400 and want["status"] == 0
    finally:
        eng.close()


# -- 7. the whole frame on the device: raster_visibility -> visibility_resolve -> compute_clusters -> visibility_surface_drawn ->
#       surface_fragments (clear) -> fragments_shade, nothing copied to the host in between
def count_tool():
    spec = importlib.util.spec_from_file_location("count_fragments_shade", os.path.join(rs.ROOT, "tools", "count_fragments_shade.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_frame_on_the_device(torch_mod, engine, oracle):
    torch = torch_mod
    assert latched(engine) == 0
    tool = count_tool()
    f = tool.host_frame(oracle)
    scene, frame, w, h, cap = f["scene"], f["frame"], f["width"], f["height"], f["scene"].cap_c
    vp, cc = frame["view_proj"], f["cluster_count"]
    meshlets = np.ascontiguousarray(scene.meshlets).view(np.uint8).reshape(-1)
    d_data, d_pos, d_rows, d_ent, d_mlt = (dev(torch, x) for x in (scene.meshlet_data, scene.vertices, f["rows"], scene.entities, meshlets))
    d_lists = [dev(torch, frame[n]) for n in ("draw1", "draw2")]
    d_lights, d_materials = dev(torch, f["lights"]), dev(torch, scene.materials)
    vcount, ecount = len(scene.vertices), scene.entity_count
    kw = dict(clip_near=True, wide_guard=True)
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
    color, every = (torch.full((4 * w * h,), 7, dtype=torch.float32, device="cuda") for _ in range(2))
    walked = torch.full((w * h,), 7, dtype=torch.int32, device="cuda")
    stats = torch.zeros(8, dtype=torch.int32, device="cuda")
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
    shade = lambda c, img, idx, ic, n, **more: engine.fragments_shade(  # noqa: E731
        vis, w, h, planes["world_pos"], planes["normal"], planes["material"], d_materials, len(scene.materials), d_lights, n, img, idx, ic, cc,
        tool.TILE, f["z_scale"], f["z_bias"], tool.CUTOFF, frame["cam"].z_near, f["view_pos"], c, clear=True, **more)
    shade(color, image, lists, capacity, len(f["lights"]), lights_walked=walked, stats=stats)
    assert latched(engine) == 0
    want = raster.host_fragments_shade(*f["args"])
    assert want["status"] == 0 and f["dropped"] == 0 and int(want["lights_walked"].max()) <= 256
    assert int(want["stats"]["stale_pixels"]) == int(want["stats"]["unshaded_pixels"]) == 0
    got = dict(color=host(color, np.float32).reshape(h, w, 4), lights_walked=host(walked, np.uint32).reshape(h, w),
               stats=host(stats, np.uint32).view(L.SHADE_STATS)[0], status=0)
    assert_equal("the frame", got, want)
    assert int(got["stats"]["written_pixels"]) == int((frame["visibility"] != 0).sum()) > 40000 and int(got["lights_walked"].max()) > 0
    # clustered = all lights, on the device, with both forms
    a_img, a_idx = tool.all_lights_args(f["args"], len(f["lights"]))[6:8]
    for form in ("per_lane", "staged"):
        shade(every, dev(torch, a_img), dev(torch, a_idx), len(f["lights"]), len(f["lights"]), form=form)
        assert latched(engine) == 0
        assert host(every).tobytes() == host(color).tobytes(), form
