"""orbit_visibility_surface_drawn on the MI355X (include/orbit_abi_ext.h S2d, S3c, S3w): every output —
bary, grad, triangle, the eight counters — and the latched status equal the host mirror's
(orbit_amd.raster.host_visibility_surface_drawn on the same buffers; tests/test_surface_drawn_cpu.py holds it to the
restatement) on every case of tests/surface_drawn_cases.py, with and without ORBIT_SURFACE_CLEAR; raster_flags = 0 equals
Engine.visibility_surface byte for byte; on buffers that orbit_raster_visibility made on the device with the flags, nothing
copied to the host in between, for the clip, wide and hand cases and the inside-terrain frame; each output NULL in turn and
alone, NULL stats; two calls with two bases into shared outputs; a grid of one workgroup, whose waves then walk slow and
fast tiles in one sequence; the call captured into a graph as a fresh context's first call and replayed twice.  Every
buffer sits between sentinel guards; inputs come back unchanged.  No test provokes a fault: a stale buffer is ordinary data
that the checks reject."""
import importlib.util
import os

import numpy as np
import pytest

import raster_cases as rc
import raster_scene as rs
import surface_drawn_cases as dc
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import Guarded, latched

pytestmark = pytest.mark.gpu
SENTINEL = rc.SENTINEL
FILL = 0x01010101 * SENTINEL  # the mirror's outputs start as the guards' bytes do
KEYS = ("bary", "grad", "triangle")
PER_PIXEL = dict(bary=8, grad=16, triangle=16)
DTYPE = dict(bary=np.float32, grad=np.float32, triangle=np.uint32)
CLIP, WIDE, BOTH = dc.CLIP, dc.WIDE, dc.BOTH


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
    return dc.all_cases()


def flag_kw(flags):
    return dict(clip_near=bool(flags & CLIP), wide_guard=bool(flags & WIDE))


def run(torch, engine, case, clear=False, want=KEYS, with_stats=True, old_call=False):
    """One orbit_visibility_surface_drawn call (old_call: orbit_visibility_surface) on guarded copies -> the dict of
    raster.host_visibility_surface_drawn (status: what the context latched)."""
    (vis, words, mc, data, vb, vcount, ent, vp), kw = case.args()
    h, w = vis.shape
    g_vis, g_cmd, g_dat, g_vb, g_ent = (Guarded(torch, a) for a in (vis, words, data, vb, ent))
    outs = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=PER_PIXEL[k] * w * h) for k in KEYS}
    stats = Guarded(torch, np.zeros(0, np.uint8), nbytes=32)
    call = engine.visibility_surface if old_call else engine.visibility_surface_drawn
    call(g_vis.ptr, w, h, g_cmd.ptr, mc, g_dat.ptr, g_vb.ptr, vcount, g_ent.ptr, kw["entity_count"], vp,
         **{k: outs[k].ptr for k in want}, stats=stats.ptr if with_stats else None, command_base=kw["command_base"], clear=clear,
         vertex_stride=kw["vertex_stride"], position_offset=kw["position_offset"], meshlet_data_words=kw["meshlet_data_words"],
         **({} if old_call else flag_kw(kw["raster_flags"])))
    torch.cuda.synchronize()
    for g in (g_vis, g_cmd, g_dat, g_vb, g_ent):
        g.unchanged()
    for k in KEYS:
        if k not in want:
            outs[k].unchanged()
    if not with_stats:
        stats.unchanged()
    got = {k: outs[k].read().view(DTYPE[k]).reshape(h, w, -1) if k in want else None for k in KEYS}
    return dict(got, stats=stats.read().view(L.SURFACE_DRAWN_STATS)[0] if with_stats else None, status=latched(engine))


def mirror(case, clear=False, want=KEYS):
    a, kw = case.args(fill=FILL, clear=clear, want=want)
    return raster.host_visibility_surface_drawn(*a, **kw)


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
    written = stale = unsupported = cut = wide = 0
    for case in cases:
        got = run(torch_mod, engine, case, clear=clear)
        assert_equal(f"{case.name} (clear={clear})", got, mirror(case, clear=clear))
        st = got["stats"]
        written, stale, unsupported = written + int(st["written_pixels"]), stale + int(st["stale_pixels"]), unsupported + int(st["unsupported_pixels"])
        cut, wide = cut + int(st["cut_pixels"]), wide + int(st["wide_pixels"])
    assert written > 10000 and stale >= 20 and unsupported > 1000 and cut > 30000 and wide > 80000


# -- 2. raster_flags = 0 is Engine.visibility_surface, byte for byte, on the device
def test_no_flags_is_the_old_call_on_the_device(torch_mod, engine, cases):
    n = 0
    for case in cases:
        if case.raster_flags != 0 or n % 3:  # (every third: the mirror's own equality is held on all of them on the CPU)
            n += case.raster_flags == 0
            continue
        n += 1
        for clear in (False, True):
            new, old = run(torch_mod, engine, case, clear=clear), run(torch_mod, engine, case, clear=clear, old_call=True)
            assert_equal(f"{case.name} (clear={clear})", new, old)
    assert n > 100


# -- 3. each output NULL in turn, alone, and NULL stats
def test_null_outputs_and_null_stats(torch_mod, engine, cases):
    by_name = {c.name: c for c in cases}
    for name in ("one_out_full_65x9@8", "cut_with_a_wide_piece_65x9@40", "64_keys_cut_and_wide_65x9@40", "stale_depth_bit_in_piece_1@8",
                 "fan_of_wide_triangles@32", "unsupported_cut_key_without_clip@32"):
        case = by_name[name]
        for clear in (False, True):
            full = mirror(case, clear=clear)
            for k in KEYS:
                rest = tuple(q for q in KEYS if q != k)
                assert_equal(f"{name} without {k}", run(torch_mod, engine, case, clear=clear, want=rest), full)
                assert_equal(f"{name} {k} alone", run(torch_mod, engine, case, clear=clear, want=(k,)), full)
            assert_equal(f"{name} without stats", run(torch_mod, engine, case, clear=clear, with_stats=False), full)


# -- 4. buffers made on the device with the flags: raster_visibility -> visibility_surface_drawn, nothing copied in between
def on_device(torch, engine, lists, data, vertices, vertex_count, entities, entity_count, view_proj, w, h, flags, cull_none=False):
    """lists: [(draw words, max_commands, command_base)], drawn into one buffer with `flags` and surfaced into shared outputs
    with the same -> (the buffer read back afterwards, outputs, stats rows, the raster's latch, the surface's latch)"""
    d_data, d_vb, d_ent = dev(torch, data), dev(torch, vertices), dev(torch, entities)
    d_lists = [dev(torch, words) for words, _, _ in lists]
    vis = torch.zeros(w * h, dtype=torch.int64, device="cuda")
    outs = dict(bary=torch.zeros(2 * w * h, dtype=torch.float32, device="cuda"), grad=torch.zeros(4 * w * h, dtype=torch.float32, device="cuda"),
                triangle=torch.zeros(4 * w * h, dtype=torch.int32, device="cuda"))
    stats = [torch.zeros(8, dtype=torch.int32, device="cuda") for _ in lists]
    for k, (d, (_, mc, base)) in enumerate(zip(d_lists, lists)):
        engine.raster_visibility(d, mc, d_data, d_vb, vertex_count, d_ent, entity_count, view_proj, vis, w, h, command_base=base,
                                 clear=k == 0, meshlet_data_words=len(data), cull_none=cull_none, **flag_kw(flags))
    raster_status = latched(engine)
    for k, (d, (_, mc, base)) in enumerate(zip(d_lists, lists)):
        engine.visibility_surface_drawn(vis, w, h, d, mc, d_data, d_vb, vertex_count, d_ent, entity_count, view_proj, **outs,
                                        stats=stats[k], command_base=base, clear=k == 0, meshlet_data_words=len(data), **flag_kw(flags))
    surface_status = latched(engine)
    got = {k: host(outs[k], DTYPE[k]).reshape(h, w, -1) for k in KEYS}
    return (host(vis, np.uint64).reshape(h, w), got, [host(s, np.uint32).view(L.SURFACE_DRAWN_STATS)[0] for s in stats], raster_status,
            surface_status)


def mirror_lists(vis, lists, data, vertices, vertex_count, entities, view_proj, flags, entity_count=None):
    want, rows = None, []
    for k, (words, mc, base) in enumerate(lists):
        want = raster.host_visibility_surface_drawn(vis, words, mc, data, vertices, vertex_count, entities, view_proj, command_base=base,
                                                    clear=k == 0, into=want, entity_count=entity_count, raster_flags=flags)
        rows.append(want["stats"])
    return want, rows


def test_clip_wide_and_hand_buffers_made_on_the_device(torch_mod, engine):
    assert latched(engine) == 0
    written = cut = wide = 0
    for case in dc.device_cases():
        (_, words, mc, data, vb, vcount, ent, vp), kw = case.args()
        h, w = case.visibility.shape
        flags = case.raster_flags
        vis, got, rows, raster_status, surface_status = on_device(
            torch_mod, engine, [(words, mc, case.command_base)], data, vb, vcount, ent, kw["entity_count"], vp, w, h, flags,
            cull_none=case.packed.case.cull_none)
        assert raster_status == 0, case.name
        assert vis.tobytes() == case.visibility.tobytes(), case.name
        want, _ = mirror_lists(vis, [(words, mc, case.command_base)], data, vb, vcount, ent, vp, flags, kw["entity_count"])
        assert_equal(case.name, dict(got, stats=rows[0], status=surface_status), want)
        assert surface_status == 0 and int(rows[0]["stale_pixels"]) == 0, case.name
        assert int(rows[0]["unsupported_pixels"]) == 0, case.name  # (drawn and read with the same flags: nothing is left out)
        written, cut, wide = written + int(rows[0]["written_pixels"]), cut + int(rows[0]["cut_pixels"]), wide + int(rows[0]["wide_pixels"])
    assert written > 100000 and cut > 30000 and wide > 80000


def count_tool():
    spec = importlib.util.spec_from_file_location("count_surface_drawn", os.path.join(rs.ROOT, "tools", "count_surface_drawn.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_inside_terrain_frame_on_the_device(torch_mod, engine, oracle):
    """tools/count_near_clip.py's inside-terrain cameras, both frames of the two-pass frame: the lists come from the CPU
    culls, the buffer from the device's raster with both flags, two surface calls with two bases into shared outputs."""
    tool = count_tool()
    near = tool._tool("count_near_clip")
    scene = rs.glb_scene(tool.INSTANCES)
    w, h, cap = tool.WIDTH, tool.HEIGHT, scene.cap_c
    common = (scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities)
    assert latched(engine) == 0
    for f, frame in enumerate(tool.flagged_frames(scene, oracle, [rs.camera(w, h, p) for p in near.CAMERAS], w, h)):
        lists = [(frame["draw1"], cap, 0), (frame["draw2"], cap, cap)]
        vis, got, rows, raster_status, surface_status = on_device(torch_mod, engine, lists, *common, scene.entity_count, frame["view_proj"],
                                                                  w, h, BOTH)
        assert raster_status == 0 and surface_status == 0
        assert vis.tobytes() == frame["visibility"].tobytes()
        want, want_rows = mirror_lists(vis, lists, *common, frame["view_proj"], BOTH)
        for k in range(2):
            assert_equal(f"inside frame {f}, list {k}", dict(got, stats=rows[k], status=0), dict(want, stats=want_rows[k], status=0))
            assert int(rows[k]["stale_pixels"]) == int(rows[k]["unsupported_pixels"]) == 0
        assert sum(int(r["written_pixels"]) for r in rows) == int((vis != 0).sum())
        if f == 1:
            assert int((vis != 0).sum()) == w * h and sum(int(r["cut_pixels"]) for r in rows) == 18184


# -- 5. a grid of one workgroup: each wave walks many tiles, slow and fast ones in one sequence
def test_one_workgroup_walks_slow_and_fast_tiles(torch_mod, engine, cases):
    by_name = {c.name: c for c in cases}
    engine.set_visibility_grid(1)
    try:
        for name in ("one_out_one_narrow_one_wide_piece@40", "strip_of_narrow_and_wide@32", "64_keys_cut_and_wide_65x9@40",
                     "clip_crossing_in_the_second_chunk@8", "clip_both_pieces_by_the_wave_256x144@8", "stale_moved_outside_both_pieces@8",
                     "two_lists_base_cap@40"):
            case = by_name[name]
            for clear in (False, True):
                assert_equal(f"{name}, one workgroup (clear={clear})", run(torch_mod, engine, case, clear=clear), mirror(case, clear=clear))
    finally:
        engine.set_visibility_grid(0)


# -- 6. two calls, two bases, shared outputs: the second without CLEAR
def test_two_lists_two_calls_into_shared_outputs(torch_mod, engine):
    """A cut triangle's list at base 0 and a wide triangle's list at base 1000 in one buffer drawn with both flags."""
    torch = torch_mod
    w, h = 65, 9
    a = dc.WideCase("shared_a", [dc.poly([dc.ONE_OUT])], width=w, height=h, view_proj=dc.w_from_z_proj(), clip_near=True)
    b = dc.WideCase("shared_b", [dc.poly([dc.wide_sliver(20, 4, w, h)]), dc.poly([dc.pixel_triangle(30, 2, dc.IN, w, h)])], width=w,
                    height=h, view_proj=dc.w_from_z_proj(), clip_near=True, cull_none=True, command_base=1000)
    pa, pb = rc.Packed(a), rc.Packed(b)
    vis = dc.wide.host_vis(pa, wide=True, clip_near=True)[0]
    # (b's triangles at w = 0.4 lie behind a's pieces: give the second list pixels of its own by hand, as a later frame would)
    vis_b = dc.wide.host_vis(pb, wide=True, clip_near=True)[0]
    take = (vis_b != 0) & (np.arange(w)[None, :] % 2 == 0)
    assert take.sum() > 3
    both = np.where(take, vis_b, vis)
    lists = [(pa, 0, True), (pb, 1000, False)]
    want = None
    for pk, base, clear in lists:
        kw, (words, mc, data, vb, vcount, ent, vp, _, _) = pk.args()
        want = raster.host_visibility_surface_drawn(both, words, mc, data, vb, vcount, ent, vp, command_base=base, clear=clear, into=want,
                                                    raster_flags=BOTH, **kw)
    outs = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=PER_PIXEL[k] * w * h) for k in KEYS}
    stats = Guarded(torch, np.zeros(0, np.uint8), nbytes=32)
    d_vis = dev(torch, both)
    for pk, base, clear in lists:
        kw, (words, mc, data, vb, vcount, ent, vp, _, _) = pk.args()
        engine.visibility_surface_drawn(d_vis, w, h, dev(torch, words), mc, dev(torch, data), dev(torch, vb), vcount, dev(torch, ent),
                                        kw["entity_count"], vp, **{k: outs[k].ptr for k in KEYS}, stats=stats.ptr, command_base=base,
                                        clear=clear, meshlet_data_words=kw["meshlet_data_words"], clip_near=True, wide_guard=True)
    torch.cuda.synchronize()
    assert latched(engine) == 0
    got = {k: outs[k].read().view(DTYPE[k]).reshape(h, w, -1) for k in KEYS}
    assert_equal("two lists", dict(got, stats=stats.read().view(L.SURFACE_DRAWN_STATS)[0], status=0), want)
    assert int(want["stats"]["foreign_pixels"]) > 0 and int(want["stats"]["written_pixels"]) == int(take.sum())
    assert (got["triangle"][..., 0] != 0xFFFFFFFF).all()  # every pixel by one list or the other


# -- 7. captured into a graph as the first call of a fresh context, replayed twice on changed buffers
def test_the_first_call_captures_into_a_graph(torch_mod, cases):
    torch = torch_mod
    from orbit_amd.engine import Engine

    picked = [next(c for c in cases if c.name == n) for n in ("one_out_full_65x9@8", "cut_with_a_wide_piece_65x9@40",
                                                              "64_keys_cut_and_wide_65x9@40", "stale_depth_bit_in_piece_1@8")]
    w, h = 65, 9
    assert all(c.visibility.shape == (h, w) for c in picked)
    size = lambda f: max(len(np.ascontiguousarray(f(c)).view(np.uint8).reshape(-1)) for c in picked)  # noqa: E731
    n_words, n_data, n_vb = size(lambda c: c.packed.words), size(lambda c: c.packed.meshlet_data), size(lambda c: c.packed.vertices)
    mc = max(c.packed.max_commands for c in picked)

    def padded(a, nbytes):
        out = np.zeros(nbytes, np.uint8)
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        out[:len(a)] = a
        return out

    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        z = lambda nbytes: torch.full((nbytes,), 5, dtype=torch.uint8, device="cuda")  # noqa: E731
        g_vis, g_words, g_data, g_vb, g_ent = z(8 * w * h), z(max(n_words, 4 + 28 * mc)), z(n_data), z(n_vb), z(128)
        outs = dict(bary=z(8 * w * h), grad=z(16 * w * h), triangle=z(16 * w * h))
        stats = z(32)
        vp = rc.w_from_z_proj()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.visibility_surface_drawn(g_vis, w, h, g_words, mc, g_data, g_vb, n_vb // 12, g_ent, 1, vp, **outs, stats=stats, clear=True,
                                         meshlet_data_words=n_data // 4, clip_near=True, wide_guard=True)
        for c in picked + picked[:1]:  # replayed: new buffers, new lists, the first ones again
            pk = c.packed
            assert pk.entity_count == 1 and (np.asarray(pk.case.view_proj) == vp).all()
            words, data, vb = padded(pk.words, len(g_words)), padded(pk.meshlet_data, n_data), padded(pk.vertices, n_vb)
            for t, a in ((g_vis, c.visibility), (g_words, words), (g_data, data), (g_vb, vb), (g_ent, pk.entities)):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda())
            want = raster.host_visibility_surface_drawn(c.visibility, words, mc, data.view(np.uint32), vb, n_vb // 12, pk.entities, vp,
                                                        raster_flags=BOTH)
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == want["status"], c.name
                for k in KEYS:
                    assert host(outs[k]).tobytes() == want[k].tobytes(), (c.name, k, replay)
                assert host(stats).tobytes() == want["stats"].tobytes(), c.name
        assert want["status"] == 0 and int(want["stats"]["cut_pixels"]) > 50
        assert _lib.RASTER_CLIP_NEAR | _lib.RASTER_WIDE_GUARD == BOTH
    finally:
        eng.close()
