"""orbit_surface_fragments on the MI355X (include/orbit_abi_ext.h F1-F8): every output — world_pos,
normal, tangent, uv, uv_grad, material, the counters — and the latched status equal the host mirror's
(orbit_amd.raster.host_surface_fragments on the same buffers; tests/test_surface_fragments_cpu.py holds it to the
restatement) on every case of tests/surface_fragments_cases.py and on the tampered ones, with and without
ORBIT_FRAGMENTS_CLEAR; each output NULL in turn and alone, NULL stats, NULL grad; two calls with two bases into shared
outputs; the chain raster -> surface -> fragments on the device with nothing copied to the host in between; a grid of one
workgroup; the call captured into a graph as a fresh context's first call and replayed twice; the scene's two-pass frame.
Every buffer sits between sentinel guards, the vertex and meshlet buffers end with their last legal byte, inputs come
back unchanged.  No test provokes a fault: a stale record is ordinary data that the checks reject."""
import importlib.util
import os

import numpy as np
import pytest

import raster_cases as rc
import raster_scene as rs
import surface_drawn_cases as dc
import surface_fragments_cases as fc
from orbit_amd import raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import Guarded, latched

pytestmark = pytest.mark.gpu
SENTINEL = rc.SENTINEL
FILL = 0x01010101 * SENTINEL  # the mirror's outputs start as the guards' bytes do
KEYS = tuple(n for n, _, _ in raster.FRAGMENT_OUTPUTS)
WORDS = {n: per for n, per, _ in raster.FRAGMENT_OUTPUTS}
DTYPE = {n: dtype for n, _, dtype in raster.FRAGMENT_OUTPUTS}
TORCH_KIND = dict(material="int32")


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
def cases():
    return fc.all_cases()


def tampered_cases():
    import test_surface_fragments_cpu as cpu

    base = next(c for c in fc.shape_cases() if c.name == "tile_of_64_65x9")
    t = base.surface["triangle"].copy()
    t[1, 8:12] = 0xFFFFFFFF
    bary = base.surface["bary"].copy()
    bary[0, 8], bary[0, 9], bary[0, 10] = (np.nan, 0.25), (0.25, np.inf), (0.75, 0.75)
    return cpu.stale_cases() + [fc.tamper(base, "four_left_out", 0, surface=dict(triangle=t)),
                                fc.tamper(base, "non_finite_bary", 0, surface=dict(bary=bary))]


def run(torch, engine, case, clear=False, want=KEYS, with_stats=True, with_grad=True):
    """One orbit_surface_fragments call on guarded copies -> the dict of raster.host_surface_fragments (status: what the
    context latched)."""
    (vis, words, mc, meshlets, surface, vb, vcount, ent), kw = case.args()
    h, w = vis.shape
    inputs = [Guarded(torch, a) for a in (vis, words, meshlets, surface["bary"], surface["grad"], surface["triangle"], vb, ent)]
    g_vis, g_cmd, g_mlt, g_bary, g_grad, g_tri, g_vb, g_ent = inputs
    outs = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=4 * WORDS[k] * w * h) for k in KEYS}
    stats = Guarded(torch, np.zeros(0, np.uint8), nbytes=32)
    engine.surface_fragments(g_vis.ptr, w, h, g_cmd.ptr, mc, g_mlt.ptr, kw["meshlet_count"], g_bary.ptr, g_tri.ptr, g_vb.ptr, vcount,
                             g_ent.ptr, kw["entity_count"], grad=g_grad.ptr if with_grad else None, **{k: outs[k].ptr for k in want},
                             stats=stats.ptr if with_stats else None, command_base=kw["command_base"], clear=clear)
    torch.cuda.synchronize()
    for g in inputs:
        g.unchanged()
    for k in KEYS:
        if k not in want:
            outs[k].unchanged()
    if not with_stats:
        stats.unchanged()
    got = {k: outs[k].read().view(DTYPE[k]).reshape(h, w, -1) if k in want else None for k in KEYS}
    return dict(got, stats=stats.read().view(L.SURFACE_FRAGMENT_STATS)[0] if with_stats else None, status=latched(engine))


def mirror(case, clear=False, want=KEYS):
    a, kw = case.args(fill=FILL, clear=clear, want=want)
    return raster.host_surface_fragments(*a, **kw)


def assert_equal(name, got, want):
    if got["stats"] is not None:
        assert got["stats"].tobytes() == want["stats"].tobytes(), f"{name}: device stats {got['stats']} != host {want['stats']}"
    assert got["status"] == want["status"], f"{name}: latched {got['status']}, the mirror says {want['status']}"
    for k in KEYS:
        if got[k] is None or want[k] is None:  # (an output the call was not given)
            continue
        diff = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(diff) == 0, (f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}: device "
                                f"{got[k][tuple(diff[0])]!r}, host {want[k][tuple(diff[0])]!r}")


# -- 1. every case, with and without CLEAR: bytes, counters, latched status, guards, inputs
@pytest.mark.parametrize("clear", (False, True))
def test_every_case_equals_the_host_mirror(torch_mod, engine, cases, clear):
    assert latched(engine) == 0
    written = stale = unshaded = degenerate = 0
    for case in cases + tampered_cases():
        got = run(torch_mod, engine, case, clear=clear)
        assert_equal(f"{case.name} (clear={clear})", got, mirror(case, clear=clear))
        st = got["stats"]
        written, stale = written + int(st["written_pixels"]), stale + int(st["stale_pixels"])
        unshaded, degenerate = unshaded + int(st["unshaded_pixels"]), degenerate + int(st["degenerate_pixels"])
    assert written > 100000 and stale == 4 and unshaded > 1000 and degenerate == 2


# -- 2. each output NULL in turn, alone, NULL stats, NULL grad
def test_null_outputs_null_stats_and_null_grad(torch_mod, engine, cases):
    by_name = {c.name: c for c in cases + tampered_cases()}
    for name in ("tile_of_64_65x9", "whole_9x9", "cut_with_a_wide_piece_65x9@40", "entity_is_entity_count", "non_finite_bary"):
        case = by_name[name]
        for clear in (False, True):
            full = mirror(case, clear=clear)
            for k in KEYS:
                rest = tuple(q for q in KEYS if q != k)
                assert_equal(f"{name} without {k}", run(torch_mod, engine, case, clear=clear, want=rest), full)
                assert_equal(f"{name} {k} alone", run(torch_mod, engine, case, clear=clear, want=(k,)), full)
            assert_equal(f"{name} without stats", run(torch_mod, engine, case, clear=clear, with_stats=False), full)
            no_grad = tuple(q for q in KEYS if q != "uv_grad")
            assert_equal(f"{name} without grad", run(torch_mod, engine, case, clear=clear, want=no_grad, with_grad=False), full)


# -- 3, 4. the chain on the device: raster_visibility -> visibility_surface_drawn -> surface_fragments, nothing copied in between
def on_device(torch, engine, lists, data, positions, rows, vertex_count, entities, entity_count, meshlets, meshlet_count, view_proj, w, h,
              flags, cull_none=False):
    """lists: [(draw words, max_commands, command_base)], drawn into one buffer with `flags`, surfaced with the same and
    turned into fragments, each into shared outputs -> (outputs, stats rows, the latch after each of the three stages)"""
    d_data, d_pos, d_rows, d_ent, d_mlt = dev(torch, data), dev(torch, positions), dev(torch, rows), dev(torch, entities), dev(torch, meshlets)
    d_lists = [dev(torch, words) for words, _, _ in lists]
    kw = dict(clip_near=bool(flags & dc.CLIP), wide_guard=bool(flags & dc.WIDE))
    vis = torch.zeros(w * h, dtype=torch.int64, device="cuda")
    surf = dict(bary=torch.zeros(2 * w * h, dtype=torch.float32, device="cuda"), grad=torch.zeros(4 * w * h, dtype=torch.float32, device="cuda"),
                triangle=torch.zeros(4 * w * h, dtype=torch.int32, device="cuda"))
    outs = {k: torch.full((WORDS[k] * w * h,), 7, dtype=getattr(torch, TORCH_KIND.get(k, "float32")), device="cuda") for k in KEYS}
    stats = [torch.zeros(8, dtype=torch.int32, device="cuda") for _ in lists]
    for k, (d, (_, mc, base)) in enumerate(zip(d_lists, lists)):
        engine.raster_visibility(d, mc, d_data, d_pos, vertex_count, d_ent, entity_count, view_proj, vis, w, h, command_base=base,
                                 clear=k == 0, meshlet_data_words=len(data), cull_none=cull_none, **kw)
    raster_status = latched(engine)
    for k, (d, (_, mc, base)) in enumerate(zip(d_lists, lists)):
        engine.visibility_surface_drawn(vis, w, h, d, mc, d_data, d_pos, vertex_count, d_ent, entity_count, view_proj, **surf,
                                        command_base=base, clear=k == 0, meshlet_data_words=len(data), **kw)
    surface_status = latched(engine)
    for k, (d, (_, mc, base)) in enumerate(zip(d_lists, lists)):
        engine.surface_fragments(vis, w, h, d, mc, d_mlt, meshlet_count, surf["bary"], surf["triangle"], d_rows, vertex_count, d_ent,
                                 entity_count, grad=surf["grad"], **outs, stats=stats[k], command_base=base, clear=k == 0)
    status = latched(engine)
    got = {k: host(outs[k], DTYPE[k]).reshape(h, w, -1) for k in KEYS}
    return got, [host(s, np.uint32).view(L.SURFACE_FRAGMENT_STATS)[0] for s in stats], (raster_status, surface_status, status)


def test_the_chain_on_the_device(torch_mod, engine):
    assert latched(engine) == 0
    written = 0
    sources = [c.source for c in fc.shape_cases()] + dc.device_cases()
    for src in sources:
        case = fc.of(src)
        (_, words, mc, data, vb, vcount, ent, vp), kw = src.args()
        h, w = src.visibility.shape
        flags = kw.get("raster_flags", 0)
        got, rows, statuses = on_device(torch_mod, engine, [(words, mc, src.command_base)], data, vb, case.vertices, vcount, case.entities,
                                        kw["entity_count"], case.meshlets, case.kw["meshlet_count"], vp, w, h, flags,
                                        cull_none=src.packed.case.cull_none)
        assert statuses == (0, 0, 0), src.name
        want = mirror(case, clear=True)
        assert_equal(src.name, dict(got, stats=rows[0], status=0), want)
        assert int(rows[0]["stale_pixels"]) == int(rows[0]["unshaded_pixels"]) == 0, src.name
        written += int(rows[0]["written_pixels"])
    assert written > 100000


def test_two_lists_two_calls_into_shared_outputs(torch_mod, engine, cases):
    """visibility_surface_cases' two lists in one buffer: one call per base, the second without CLEAR"""
    a, b = (next(c for c in cases if c.name == n) for n in ("two_lists_base_0", "two_lists_base_cap"))
    assert a.visibility.tobytes() == b.visibility.tobytes() and a.kw["command_base"] != b.kw["command_base"]
    h, w = a.visibility.shape
    shared = {k: np.where((b.surface["triangle"][..., :1] != 0xFFFFFFFF), b.surface[k], a.surface[k]) for k in ("bary", "grad", "triangle")}
    lists = [fc.tamper(a, "list a", 0, surface=shared), fc.tamper(b, "list b", 0, surface=shared)]
    want = None
    for k, c in enumerate(lists):
        args, kw = c.args()
        want = raster.host_surface_fragments(*args, **kw, clear=k == 0, into=want)
    torch = torch_mod
    outs = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=4 * WORDS[k] * w * h) for k in KEYS}
    stats = Guarded(torch, np.zeros(0, np.uint8), nbytes=32)
    d_vis, d_surf = dev(torch, a.visibility), {k: dev(torch, v) for k, v in shared.items()}
    for k, c in enumerate(lists):
        engine.surface_fragments(d_vis, w, h, dev(torch, c.words), c.max_commands, dev(torch, c.meshlets), c.kw["meshlet_count"], d_surf["bary"],
                                 d_surf["triangle"], dev(torch, c.vertices), c.vertex_count, dev(torch, c.entities), c.kw["entity_count"],
                                 grad=d_surf["grad"], **{q: outs[q].ptr for q in KEYS}, stats=stats.ptr, command_base=c.kw["command_base"],
                                 clear=k == 0)
    torch.cuda.synchronize()
    assert latched(engine) == 0
    got = {k: outs[k].read().view(DTYPE[k]).reshape(h, w, -1) for k in KEYS}
    assert_equal("two lists", dict(got, stats=stats.read().view(L.SURFACE_FRAGMENT_STATS)[0], status=0), want)
    assert int(want["stats"]["foreign_pixels"]) > 0 and int(want["stats"]["written_pixels"]) > 0
    assert ((got["material"][..., 0] != 0xFFFFFFFF) == (a.visibility != 0)).all()  # every covered pixel by one list or the other


# -- 5, 7. the scene's two-pass frame, and a grid of one workgroup
def count_tool():
    spec = importlib.util.spec_from_file_location("count_surface_fragments", os.path.join(rs.ROOT, "tools", "count_surface_fragments.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@pytest.fixture(scope="module")
def scene_frame(oracle):
    """(tool, scene, rows, the second frame of the outside cameras' two-pass frame, the mirror's fragments and stats rows)"""
    tool = count_tool()
    outside = tool._tool("count_visible_surface")
    scene = rs.glb_scene(tool.INSTANCES)
    rows = tool.scene_rows(scene)
    w, h = tool.WIDTH, tool.HEIGHT
    frame = tool._tool("count_surface_drawn").flagged_frames(scene, oracle, [rs.camera(w, h, p) for p in outside.CAMERAS], w, h)[1]
    want, want_rows = None, []
    for k, c in enumerate(tool.frame_cases(scene, rows, frame)):
        a, kw = c.args()
        want = raster.host_surface_fragments(*a, **kw, clear=k == 0, into=want)
        want_rows.append(want["stats"])
    return tool, scene, rows, frame, want, want_rows


def scene_on_device(torch, engine, scene_frame):
    tool, scene, rows, frame, want, want_rows = scene_frame
    cap = scene.cap_c
    meshlets = np.ascontiguousarray(scene.meshlets).view(np.uint8).reshape(-1)
    got, got_rows, statuses = on_device(torch, engine, [(frame["draw1"], cap, 0), (frame["draw2"], cap, cap)], scene.meshlet_data, scene.vertices,
                                        rows, len(scene.vertices), scene.entities, scene.entity_count, meshlets, len(meshlets) // 32,
                                        frame["view_proj"], tool.WIDTH, tool.HEIGHT, tool.BOTH)
    assert statuses == (0, 0, 0)
    for k in range(2):
        assert_equal(f"scene frame, list {k}", dict(got, stats=got_rows[k], status=0), dict(want, stats=want_rows[k], status=0))
    assert sum(int(r["written_pixels"]) for r in got_rows) == int((frame["visibility"] != 0).sum()) > 40000
    assert len(np.unique(got["material"])) > 3


def test_the_scene_frame_on_the_device(torch_mod, engine, scene_frame):
    assert latched(engine) == 0
    scene_on_device(torch_mod, engine, scene_frame)


def test_one_workgroup_walks_every_tile(torch_mod, engine, cases, scene_frame):
    by_name = {c.name: c for c in cases}
    engine.set_visibility_grid(1)
    try:
        for name in ("whole_65x8", "whole_9x9", "tile_of_64_65x9", "two_lists_base_cap"):
            for clear in (False, True):
                assert_equal(f"{name}, one workgroup (clear={clear})", run(torch_mod, engine, by_name[name], clear=clear),
                             mirror(by_name[name], clear=clear))
        scene_on_device(torch_mod, engine, scene_frame)
    finally:
        engine.set_visibility_grid(0)


# -- 6. captured into a graph as the first call of a fresh context, replayed twice on changed buffers
def test_the_first_call_captures_into_a_graph(torch_mod, cases):
    torch = torch_mod
    from orbit_amd.engine import Engine

    picked = [next(c for c in cases + tampered_cases() if c.name == n) for n in ("one_out_full_65x9@8", "tile_of_64_65x9", "entity_is_entity_count",
                                                                                   "64_keys_cut_and_wide_65x9@40")]
    w, h = 65, 9
    assert all(c.visibility.shape == (h, w) for c in picked)
    size = lambda f: max(len(np.ascontiguousarray(f(c)).view(np.uint8).reshape(-1)) for c in picked)  # noqa: E731
    n_words, n_mlt, n_vb, n_ent = size(lambda c: c.words), size(lambda c: c.meshlets), size(lambda c: c.vertices), size(lambda c: c.entities)
    mc = max(c.max_commands for c in picked)

    def padded(a, nbytes):
        out = np.zeros(nbytes, np.uint8)
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        out[:len(a)] = a
        return out

    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        z = lambda nbytes: torch.full(((nbytes + 15) // 16 * 16,), 5, dtype=torch.uint8, device="cuda")  # noqa: E731
        g_vis, g_words, g_mlt, g_vb, g_ent = z(8 * w * h), z(max(n_words, 4 + 28 * mc)), z(n_mlt), z(n_vb), z(n_ent)
        g_surf = dict(bary=z(8 * w * h), grad=z(16 * w * h), triangle=z(16 * w * h))
        outs = {k: z(4 * WORDS[k] * w * h) for k in KEYS}
        stats = z(32)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.surface_fragments(g_vis, w, h, g_words, mc, g_mlt, (n_mlt + 31) // 32, g_surf["bary"], g_surf["triangle"], g_vb, (n_vb + 31) // 32,
                                  g_ent, n_ent // 128, grad=g_surf["grad"], **outs, stats=stats, clear=True)
        for c in picked + picked[:1]:  # replayed: new buffers, new lists, the first ones again
            assert c.kw["command_base"] == 0
            words = padded(c.words, len(g_words))
            for t, a in ((g_vis, c.visibility), (g_words, words), (g_mlt, padded(c.meshlets, len(g_mlt))), (g_vb, padded(c.vertices, len(g_vb))),
                         (g_ent, padded(c.entities, len(g_ent))), (g_surf["bary"], c.surface["bary"]), (g_surf["grad"], c.surface["grad"]),
                         (g_surf["triangle"], c.surface["triangle"])):
                t[:np.ascontiguousarray(a).nbytes].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda())
            want = raster.host_surface_fragments(c.visibility, words, mc, padded(c.meshlets, len(g_mlt)), c.surface, padded(c.vertices, len(g_vb)),
                                                 (n_vb + 31) // 32, padded(c.entities, len(g_ent)), entity_count=n_ent // 128,
                                                 meshlet_count=(n_mlt + 31) // 32)
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == want["status"], c.name
                for k in KEYS:
                    assert host(outs[k])[:want[k].nbytes].tobytes() == want[k].tobytes(), (c.name, k, replay)
                assert host(stats)[:32].tobytes() == want["stats"].tobytes(), c.name
        assert want["status"] == 0 and int(want["stats"]["written_pixels"]) == 65 * 9
    finally:
        eng.close()
