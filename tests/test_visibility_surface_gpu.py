"""orbit_visibility_surface on the MI355X (include/orbit_abi_ext.h S1-S7): every output — bary, grad,
triangle, counters — and the latched status equal the host mirror's (orbit_amd.raster.host_visibility_surface on the same
buffers; tests/test_visibility_surface_cpu.py holds it to the restatement) on every case of
tests/visibility_surface_cases.py, with and without ORBIT_SURFACE_CLEAR; on buffers that orbit_raster_visibility made on
the device, nothing copied to the host in between, for the census, the 100-instance scene and the two-pass frame; each
output NULL in turn, NULL stats; two calls with two bases into shared outputs; the call captured into a graph on a fresh
context's first call.  Every buffer sits between sentinel guards; inputs come back unchanged; what the call must not write
keeps the sentinel.  No test provokes a fault: a stale buffer is ordinary data that the range checks reject."""
import numpy as np
import pytest

import raster_cases as rc
import raster_scene as rs
import visibility_surface_cases as sc
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
    return sc.all_cases()


def run(torch, engine, case, clear=False, want=KEYS, with_stats=True):
    """One orbit_visibility_surface call on guarded copies -> the dict of raster.host_visibility_surface (status: what the
    context latched)."""
    (vis, words, mc, data, vb, vcount, ent, vp), kw = case.args()
    h, w = vis.shape
    g_vis, g_cmd, g_dat, g_vb, g_ent = (Guarded(torch, a) for a in (vis, words, data, vb, ent))
    outs = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=PER_PIXEL[k] * w * h) for k in KEYS}
    stats = Guarded(torch, np.zeros(0, np.uint8), nbytes=32)
    engine.visibility_surface(g_vis.ptr, w, h, g_cmd.ptr, mc, g_dat.ptr, g_vb.ptr, vcount, g_ent.ptr, kw["entity_count"], vp,
                              **{k: outs[k].ptr for k in want}, stats=stats.ptr if with_stats else None,
                              command_base=kw["command_base"], clear=clear, vertex_stride=kw["vertex_stride"],
                              position_offset=kw["position_offset"], meshlet_data_words=kw["meshlet_data_words"])
    torch.cuda.synchronize()
    for g in (g_vis, g_cmd, g_dat, g_vb, g_ent):
        g.unchanged()
    for k in KEYS:
        if k not in want:
            outs[k].unchanged()
    if not with_stats:
        stats.unchanged()
    got = {k: outs[k].read().view(DTYPE[k]).reshape(h, w, -1) if k in want else None for k in KEYS}
    return dict(got, stats=stats.read().view(L.SURFACE_STATS)[0] if with_stats else None, status=latched(engine))


def mirror(case, clear=False, want=KEYS):
    a, kw = case.args(fill=FILL, clear=clear, want=want)
    return raster.host_visibility_surface(*a, **kw)


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
    written = stale = unsupported = degenerate = 0
    for case in cases:
        got = run(torch_mod, engine, case, clear=clear)
        assert_equal(f"{case.name} (clear={clear})", got, mirror(case, clear=clear))
        written, stale = written + int(got["stats"]["written_pixels"]), stale + int(got["stats"]["stale_pixels"])
        unsupported, degenerate = unsupported + int(got["stats"]["unsupported_pixels"]), degenerate + int(got["stats"]["degenerate_pixels"])
    assert written > 10000 and stale >= 9 and unsupported > 1000 and degenerate > 10


# -- 2. each output NULL in turn, alone, and NULL stats
def test_null_outputs_and_null_stats(torch_mod, engine, cases):
    by_name = {c.name: c for c in cases}
    for name in ("w_1_1_4", "foreshortened", "two_lists_base_cap", "stale_depth_bit", "clip_lone_out_vertex_0", "64_keys_in_a_tile"):
        case = by_name[name]
        for clear in (False, True):
            full = mirror(case, clear=clear)
            for k in KEYS:
                rest = tuple(q for q in KEYS if q != k)
                assert_equal(f"{name} without {k}", run(torch_mod, engine, case, clear=clear, want=rest), full)
                assert_equal(f"{name} {k} alone", run(torch_mod, engine, case, clear=clear, want=(k,)), full)
            assert_equal(f"{name} without stats", run(torch_mod, engine, case, clear=clear, with_stats=False), full)


# -- 3. two calls, two bases, shared outputs: the second without CLEAR
def test_two_lists_two_calls_into_shared_outputs(torch_mod, engine, cases):
    torch = torch_mod
    a, b = (next(c for c in cases if c.name == n) for n in ("two_lists_base_0", "two_lists_base_cap"))
    assert a.visibility.tobytes() == b.visibility.tobytes()
    h, w = a.visibility.shape
    want = None
    for c, clear in ((a, True), (b, False)):
        args, kw = c.args(clear=clear, into=want)
        want = raster.host_visibility_surface(*args, **kw)
    outs = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=PER_PIXEL[k] * w * h) for k in KEYS}
    stats = Guarded(torch, np.zeros(0, np.uint8), nbytes=32)
    d_vis = dev(torch, a.visibility)
    for c, clear in ((a, True), (b, False)):
        (_, words, mc, data, vb, vcount, ent, vp), kw = c.args()
        engine.visibility_surface(d_vis, w, h, dev(torch, words), mc, dev(torch, data), dev(torch, vb), vcount, dev(torch, ent),
                                  kw["entity_count"], vp, **{k: outs[k].ptr for k in KEYS}, stats=stats.ptr,
                                  command_base=kw["command_base"], clear=clear, meshlet_data_words=kw["meshlet_data_words"])
    torch.cuda.synchronize()
    assert latched(engine) == 0
    got = {k: outs[k].read().view(DTYPE[k]).reshape(h, w, -1) for k in KEYS}
    assert_equal("two lists", dict(got, stats=stats.read().view(L.SURFACE_STATS)[0], status=0), want)
    covered = a.visibility != 0
    assert int(want["stats"]["foreign_pixels"]) > 0 and (got["triangle"][covered][:, 0] != 0xFFFFFFFF).all()
    assert (got["triangle"][~covered] == 0xFFFFFFFF).all()


# -- 4. buffers made on the device: raster_visibility -> visibility_surface, nothing copied to the host in between
def on_device(torch, engine, lists, data, vertices, vertex_count, entities, entity_count, view_proj, w, h, **raster_kw):
    """lists: [(draw words, max_commands, command_base)], drawn into one buffer and surfaced into shared outputs ->
    (the buffer read back afterwards, outputs dict, stats rows, what the raster calls latched, what the surface calls
    latched).  The status is read between the two groups of calls (a wait, no copy of any buffer) so that each group's
    own latch is seen."""
    d_data, d_vb, d_ent = dev(torch, data), dev(torch, vertices), dev(torch, entities)
    d_lists = [dev(torch, words) for words, _, _ in lists]
    vis = torch.zeros(w * h, dtype=torch.int64, device="cuda")
    outs = dict(bary=torch.zeros(2 * w * h, dtype=torch.float32, device="cuda"), grad=torch.zeros(4 * w * h, dtype=torch.float32, device="cuda"),
                triangle=torch.zeros(4 * w * h, dtype=torch.int32, device="cuda"))
    stats = [torch.zeros(8, dtype=torch.int32, device="cuda") for _ in lists]
    for k, (d, (_, mc, base)) in enumerate(zip(d_lists, lists)):
        engine.raster_visibility(d, mc, d_data, d_vb, vertex_count, d_ent, entity_count, view_proj, vis, w, h, command_base=base,
                                 clear=k == 0, meshlet_data_words=len(data), **raster_kw)
    raster_status = latched(engine)
    for k, (d, (_, mc, base)) in enumerate(zip(d_lists, lists)):
        engine.visibility_surface(vis, w, h, d, mc, d_data, d_vb, vertex_count, d_ent, entity_count, view_proj, **outs,
                                  stats=stats[k], command_base=base, clear=k == 0, meshlet_data_words=len(data))
    surface_status = latched(engine)
    got = {k: host(outs[k], DTYPE[k]).reshape(h, w, -1) for k in KEYS}
    return (host(vis, np.uint64).reshape(h, w), got, [host(s, np.uint32).view(L.SURFACE_STATS)[0] for s in stats], raster_status,
            surface_status)


def mirror_lists(vis, lists, data, vertices, vertex_count, entities, view_proj, entity_count=None):
    want, rows = None, []
    for k, (words, mc, base) in enumerate(lists):
        want = raster.host_visibility_surface(vis, words, mc, data, vertices, vertex_count, entities, view_proj, command_base=base,
                                              clear=k == 0, into=want, entity_count=entity_count)
        rows.append(want["stats"])
    return want, rows


def test_census_buffers_made_on_the_device(torch_mod, engine, cases):
    """The census through the device's own raster — the clip cases with ORBIT_RASTER_CLIP_NEAR, as their buffers were drawn
    — then the surface: the buffer equals the case's host-drawn one, the outputs, the counters and the surface call's own
    latched status equal the mirror's on the buffer read back.  (The raster latches ORBIT_E_RANGE on the R9 and the
    257-triangle cases: that is its own status, read before the surface call.)"""
    assert latched(engine) == 0
    written = unsupported = drawn = 0
    for case in cases:
        pk = case.packed
        if case.stale or case.words is not None or case.name.startswith("two_lists") or \
                case.name in ("range_ends", "base_top_of_24_bits"):  # (tampered with, another count, two calls: test 3 and below)
            continue
        clip_near = case.name.startswith("clip_")
        (_, words, mc, data, vb, vcount, ent, vp), kw = case.args()
        h, w = case.visibility.shape
        vis, got, rows, raster_status, surface_status = on_device(
            torch_mod, engine, [(words, mc, case.command_base)], data, vb, vcount, ent, kw["entity_count"], vp, w, h,
            cull_none=pk.case.cull_none, clip_near=clip_near)
        assert raster_status in (0, _lib.E_RANGE), case.name
        assert vis.tobytes() == case.visibility.tobytes(), case.name
        want, want_rows = mirror_lists(vis, [(words, mc, case.command_base)], data, vb, vcount, ent, vp, kw["entity_count"])
        assert_equal(case.name, dict(got, stats=rows[0], status=surface_status), want)
        assert surface_status == 0 and int(rows[0]["stale_pixels"]) == 0, case.name
        assert clip_near or int(rows[0]["unsupported_pixels"]) == 0, case.name
        written, unsupported, drawn = written + int(rows[0]["written_pixels"]), unsupported + int(rows[0]["unsupported_pixels"]), drawn + 1
    assert written > 10000 and unsupported > 1000 and drawn > 70


def test_the_scene_and_the_two_pass_frame_on_the_device(torch_mod, engine, oracle):
    scene = rs.glb_scene(100)
    w, h, cap = 320, 180, scene.cap_c
    cams = [rs.camera(w, h), rs.camera(w, h, (1.5, 1.2, 5.0))]
    frames = rs.two_pass_frame(scene, oracle, cams[0], cams[1], w, h)
    common = (scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities)
    assert latched(engine) == 0
    for f, cam in enumerate(cams):
        vp = rs.view_proj(cam)
        lists = [(frames[f]["draw1"], cap, 0), (frames[f]["draw2"], cap, cap)]
        for use in (lists[:1], lists):  # the early list alone (the scene), then the frame's two lists
            vis, got, rows, raster_status, surface_status = on_device(torch_mod, engine, use, *common, scene.entity_count, vp, w, h)
            assert raster_status == 0 and surface_status == 0
            want, want_rows = mirror_lists(vis, use, *common, vp)
            for k in range(len(use)):
                assert_equal(f"frame {f}, list {k} of {len(use)}", dict(got, stats=rows[k], status=0), dict(want, stats=want_rows[k], status=0))
                assert int(rows[k]["stale_pixels"]) == int(rows[k]["unsupported_pixels"]) == int(rows[k]["degenerate_pixels"]) == 0
            # (frame 0 starts from empty visibility bits: its early list is empty and the late one draws everything)
            assert sum(int(r["written_pixels"]) for r in rows) == int((vis != 0).sum()) > (w * h // 4 if len(use) == 2 or f == 1 else -1)
        assert (vis >> np.uint64(32)).astype(np.uint32).tobytes() == frames[f]["depth2"].tobytes()


# -- 5. captured into a graph on the first call of a fresh context, replayed on changed buffers
def test_the_first_call_captures_into_a_graph(torch_mod, cases):
    torch = torch_mod
    from orbit_amd.engine import Engine

    picked = [next(c for c in cases if c.name == n) for n in ("wound_front", "stale_moved_word", "64_keys_in_a_tile")]
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
        vp = rc.pixel_proj(w, h)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.visibility_surface(g_vis, w, h, g_words, mc, g_data, g_vb, n_vb // 12, g_ent, 1, vp, **outs, stats=stats, clear=True,
                                   meshlet_data_words=n_data // 4)
        for c in picked + picked[:1]:  # replayed: new buffers, new lists, the first ones again
            pk = c.packed
            assert pk.entity_count == 1 and (np.asarray(pk.case.view_proj) == vp).all()
            words, data, vb = padded(pk.words, len(g_words)), padded(pk.meshlet_data, n_data), padded(pk.vertices, n_vb)
            for t, a in ((g_vis, c.visibility), (g_words, words), (g_data, data), (g_vb, vb), (g_ent, pk.entities)):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda())
            want = raster.host_visibility_surface(c.visibility, words, mc, data.view(np.uint32), vb, n_vb // 12, pk.entities, vp)
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == want["status"], c.name
                for k in KEYS:
                    assert host(outs[k]).tobytes() == want[k].tobytes(), (c.name, k, replay)
                assert host(stats).tobytes() == want["stats"].tobytes(), c.name
        assert want["status"] == 0 and int(want["stats"]["written_pixels"]) > 50
    finally:
        eng.close()
