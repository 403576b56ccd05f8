"""orbit_visibility_compact on the MI355X (include/orbit_abi_ext.h C1-C6): every output — masks, list,
ids, visible_data, counters — and the latched status equal the host mirror's (orbit_amd.raster.host_visibility_compact on
the same buffers; tests/test_visibility_compact_cpu.py holds it to the restatement) on every case of
tests/visibility_compact_cases.py, in both modes and at every capacity; C6 on the device, the output list going through
orbit_raster_visibility and orbit_visibility_resolve without a host copy in between, for the census, the 100-instance
scene and the two-pass frame; NULL stats and ids; the call captured into a graph on a context's first call.  Every buffer
sits between sentinel guards; inputs come back unchanged; what the call must not write keeps the sentinel."""
import numpy as np
import pytest

import raster_cases as rc
import raster_scene as rs
import visibility_compact_cases as cc
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import Guarded, latched

pytestmark = pytest.mark.gpu
SENTINEL = rc.SENTINEL
FILL = 0x01010101 * SENTINEL  # the mirror's outputs start as the guards' bytes do
HAND = cc.hand_cases()
MODES = (False, True)
KEYS = ("masks", "commands", "ids", "data")


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
def rasterised():
    return cc.rasterised_cases()


def blank(torch, words):
    return Guarded(torch, np.zeros(0, np.uint8), nbytes=4 * int(words))


def run(torch, engine, case, triangles, visible_capacity=None, visible_data_words=None, with_stats=True, with_ids=True):
    """One orbit_visibility_compact call on guarded copies -> the dict of raster.host_visibility_compact (status: what
    the context latched)."""
    from orbit_amd.engine import visibility_compact_workspace

    h, w = case.visibility.shape
    mc = case.max_commands
    cap = mc if visible_capacity is None else visible_capacity
    words = (len(case.meshlet_data) if triangles else 0) if visible_data_words is None else visible_data_words
    vis, cmd, dat = Guarded(torch, case.visibility), Guarded(torch, case.words), Guarded(torch, case.meshlet_data)
    masks, out, ids, vdata, stats = blank(torch, 8 * mc), blank(torch, 1 + 7 * cap), blank(torch, cap), blank(torch, words), blank(torch, 8)
    work = Guarded(torch, np.zeros(0, np.uint8), nbytes=visibility_compact_workspace(mc))
    engine.visibility_compact(vis.ptr, w, h, cmd.ptr, mc, masks.ptr, out.ptr, cap, work.ptr, command_base=case.command_base,
                              meshlet_data=dat.ptr, meshlet_data_words=len(case.meshlet_data) if case.meshlet_data_words is None else case.meshlet_data_words,
                              visible_ids=ids.ptr if with_ids else None, visible_data=vdata.ptr if triangles else None,
                              visible_data_words=words, stats=stats.ptr if with_stats else None, triangles=triangles,
                              workspace_bytes=work.n)
    torch.cuda.synchronize()
    for g in (vis, cmd, dat):
        g.unchanged()
    work.read()  # (its guards)
    if not triangles:
        vdata.unchanged()
    if not with_ids:
        ids.unchanged()
    if not with_stats:
        stats.unchanged()
    u32 = lambda g: g.read().view(np.uint32)  # noqa: E731
    return dict(masks=u32(masks), commands=u32(out), ids=u32(ids) if with_ids else None, data=u32(vdata) if triangles else None,
                stats=u32(stats).view(L.VIS_COMPACT_STATS)[0] if with_stats else None, status=latched(engine))


def mirror(case, triangles, **over):
    a, kw = case.args(triangles, fill=FILL, **over)
    return raster.host_visibility_compact(*a, **kw)


def assert_equal(name, got, want):
    if got["stats"] is not None:
        assert got["stats"].tobytes() == want["stats"].tobytes(), f"{name}: device stats {got['stats']} != host {want['stats']}"
    assert got["status"] == want["status"], f"{name}: latched {got['status']}, the mirror says {want['status']}"
    for k in KEYS:
        if got[k] is None or want[k] is None:  # (an output the call was not given)
            continue
        diff = np.flatnonzero(got[k] != want[k])
        assert len(diff) == 0, (f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}: device {int(got[k][diff[0]]):#x}, "
                                f"host {int(want[k][diff[0]]):#x}")


# -- 1. every case, both modes: bytes, counters, latched status
@pytest.mark.parametrize("triangles", MODES)
def test_every_hand_built_case_equals_the_host_mirror(torch_mod, engine, triangles):
    assert latched(engine) == 0
    for case in HAND:
        assert_equal(f"{case.name} (triangles={triangles})", run(torch_mod, engine, case, triangles), mirror(case, triangles))


@pytest.mark.parametrize("triangles", MODES)
def test_every_rasterised_case_equals_the_host_mirror(torch_mod, engine, rasterised, triangles):
    assert latched(engine) == 0
    for case in rasterised:
        assert_equal(f"{case.name} (triangles={triangles})", run(torch_mod, engine, case, triangles), mirror(case, triangles))


# -- 2. capacities: the prefix, the drop count, ORBIT_E_CAPACITY, the fill behind the written regions
@pytest.mark.parametrize("name", cc.CAPACITY_CASES)
def test_capacities_equal_the_host_mirror(torch_mod, engine, name):
    case = next(c for c in HAND if c.name == name)
    full = mirror(case, True)
    assert latched(engine) == 0 and full["status"] == 0
    for what, over, triangles in cc.capacity_variants(full["stats"]):
        want = mirror(case, triangles, **over)
        assert want["status"] == (0 if "exact" in what else _lib.E_CAPACITY), what
        got = run(torch_mod, engine, case, triangles, **over)
        assert_equal(f"{name} {what}", got, want)
        w = int(got["commands"][0])
        assert (got["commands"][1 + 7 * w:] == FILL).all() and (got["ids"][w:] == FILL).all()


# -- 3. NULL stats, NULL ids, no commands
def test_null_stats_null_ids_and_no_commands(torch_mod, engine):
    by_name = {c.name: c for c in HAND}
    for name in ("m_1_2_3_4", "inconsistent", "three_chunks"):
        for triangles in MODES:
            want = mirror(by_name[name], triangles)
            assert_equal(name, run(torch_mod, engine, by_name[name], triangles, with_stats=False), want)
            assert_equal(name, run(torch_mod, engine, by_name[name], triangles, with_ids=False), want)
            assert_equal(name, run(torch_mod, engine, by_name[name], triangles, with_stats=False, with_ids=False), want)
    case = by_name["tiles_65x9"]
    empty = cc.CompactCase("max_commands_0", case.visibility, case.words, 0, case.meshlet_data, case.command_base)
    for triangles in MODES:
        got = run(torch_mod, engine, empty, triangles, visible_capacity=2)
        assert_equal("max_commands_0", got, mirror(empty, triangles, visible_capacity=2))
        assert int(got["commands"][0]) == 0 and int(got["stats"]["foreign_pixels"]) == int(got["stats"]["covered_pixels"]) > 0


# -- 4. C6 on the device: compact -> raster -> resolve, nothing copied to the host in between
class DeviceC6:
    """The device tensors of one list's round trip; everything is enqueued by compact_and_redraw and read afterwards."""

    def __init__(self, torch, engine, max_commands, width, height, data_words):
        from orbit_amd.engine import visibility_compact_workspace

        self.torch, self.engine, self.mc, self.w, self.h, self.data_words = torch, engine, max_commands, width, height, data_words
        z = lambda n, dt=torch.int32: torch.zeros(max(int(n), 1), dtype=dt, device="cuda")  # noqa: E731
        self.masks, self.out, self.ids, self.vdata = z(8 * max_commands), z(1 + 7 * max_commands), z(max_commands), z(data_words)
        self.stats, self.work = z(8), z(visibility_compact_workspace(max_commands) // 8, torch.int64)
        self.vis2, self.rstats, self.pixels, self.vstats = z(width * height, torch.int64), z(8), z(max_commands), z(4)

    def compact(self, vis, draw, base, data, triangles):
        self.engine.visibility_compact(vis, self.w, self.h, draw, self.mc, self.masks, self.out, self.mc, self.work,
                                       command_base=base, meshlet_data=data, meshlet_data_words=self.data_words,
                                       visible_ids=self.ids, visible_data=self.vdata if triangles else None,
                                       visible_data_words=self.data_words if triangles else 0, stats=self.stats,
                                       triangles=triangles)

    def redraw(self, data, triangles, raster_args, target=None, base=0, clear=True, **kw):
        """raster_args: (vertices, vertex_count, entities, entity_count, view_proj)"""
        self.engine.raster_visibility(self.out, self.mc, self.vdata if triangles else data, *raster_args,
                                      self.vis2 if target is None else target, self.w, self.h, command_base=base, clear=clear,
                                      stats=self.rstats, meshlet_data_words=self.data_words, **kw)

    def resolve(self, target=None, base=0):
        self.engine.visibility_resolve(self.vis2 if target is None else target, self.w, self.h, base, self.mc,
                                       command_pixels=self.pixels, stats=self.vstats)

    def read(self):
        u32 = lambda t: host(t, np.uint32)  # noqa: E731
        got = dict(masks=u32(self.masks)[:8 * self.mc], commands=u32(self.out), ids=u32(self.ids), data=u32(self.vdata),
                   stats=u32(self.stats).view(L.VIS_COMPACT_STATS)[0])
        return got, host(self.vis2, np.uint64).reshape(self.h, self.w), u32(self.rstats).view(L.RASTER_STATS)[0], \
            u32(self.pixels), u32(self.vstats).view(L.VIS_STATS)[0]


def test_c6_on_the_device_for_the_census(torch_mod, engine, rasterised):
    torch = torch_mod
    assert latched(engine) == 0
    visible = 0
    for case in rasterised:
        pk = case.packed
        opts, (words, mc, data, vb, vcount, ent, vp, w, h) = pk.args()
        d_vis, d_words, d_data = dev(torch, case.visibility), dev(torch, case.words), dev(torch, data)
        args = (dev(torch, vb), vcount, dev(torch, ent), opts["entity_count"], vp)
        for triangles in MODES:
            c6 = DeviceC6(torch, engine, case.max_commands, w, h, len(data))
            c6.compact(d_vis, d_words, case.command_base, d_data, triangles)
            c6.redraw(d_data, triangles, args, cull_none=pk.case.cull_none)
            c6.resolve()
            torch.cuda.synchronize()
            assert latched(engine) == 0, case.name
            got, vis2, rstats, pixels, vstats = c6.read()
            assert not cc.c6_misses(case.name, case.visibility, case.command_base, got, triangles, vis2, rstats, pixels, vstats,
                                    whole=case.one_clear_call)
            visible += int(got["stats"]["visible_triangles"])
    assert visible > 400


@pytest.fixture(scope="module")
def scene100(oracle):
    scene = rs.glb_scene(100)
    w, h = 256, 144
    cam = rs.camera(w, h)
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    return scene, cam, w, h, draw


def scene_args(torch, scene, cam):
    return dev(torch, scene.meshlet_data), (dev(torch, scene.vertices), len(scene.vertices), dev(torch, scene.entities),
                                            scene.entity_count, rs.view_proj(cam))


def test_c6_on_the_device_for_the_scene_and_the_mirrors_bytes(torch_mod, engine, scene100):
    torch = torch_mod
    scene, cam, w, h, draw = scene100
    d_data, args = scene_args(torch, scene, cam)
    d_draw = dev(torch, draw)
    vis = torch.zeros(w * h, dtype=torch.int64, device="cuda")
    engine.raster_visibility(d_draw, scene.cap_c, d_data, *args, vis, w, h, clear=True, meshlet_data_words=len(scene.meshlet_data))
    assert latched(engine) == 0
    for triangles in MODES:
        c6 = DeviceC6(torch, engine, scene.cap_c, w, h, len(scene.meshlet_data))
        c6.compact(vis, d_draw, 0, d_data, triangles)
        c6.redraw(d_data, triangles, args)
        c6.resolve()
        torch.cuda.synchronize()
        assert latched(engine) == 0
        got, vis2, rstats, pixels, vstats = c6.read()
        h_vis = host(vis, np.uint64).reshape(h, w)
        want = raster.host_visibility_compact(h_vis, draw, scene.cap_c, 0, scene.meshlet_data, triangles)
        want["status"], got["status"] = 0, 0
        n = int(want["commands"][0])
        assert 1000 < n < int(draw[:4].view(np.uint32)[0]) // 4
        assert_equal(f"scene (triangles={triangles})", got, want)
        assert not cc.c6_misses("scene", h_vis, 0, got, triangles, vis2, rstats, pixels, vstats)


def test_c6_on_the_device_for_the_two_pass_frame(torch_mod, engine, oracle):
    """The frame's final buffer holds the early list at base 0 and the late list at base = the capacity: each is
    compacted with its own base, and the two output lists drawn again give the frame's depth and map back list by list."""
    torch = torch_mod
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("count_visible_list", os.path.join(rs.ROOT, "tools", "count_visible_list.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    scene = rs.glb_scene(tool.INSTANCES)
    w, h, cap = tool.WIDTH, tool.HEIGHT, scene.cap_c
    cams = [rs.camera(w, h, p) for p in tool.CAMERAS]
    frame = rs.two_pass_frame(scene, oracle, cams[0], cams[1], w, h)[1]
    d_data, args = scene_args(torch, scene, cams[1])
    draws = [dev(torch, frame["draw1"]), dev(torch, frame["draw2"])]
    vis = torch.zeros(w * h, dtype=torch.int64, device="cuda")
    for k, d in enumerate(draws):
        engine.raster_visibility(d, cap, d_data, *args, vis, w, h, command_base=k * cap, clear=k == 0,
                                 meshlet_data_words=len(scene.meshlet_data))
    torch.cuda.synchronize()
    h_vis = host(vis, np.uint64).reshape(h, w)
    for triangles in MODES:
        lists = [DeviceC6(torch, engine, cap, w, h, len(scene.meshlet_data)) for _ in draws]
        again = torch.zeros(w * h, dtype=torch.int64, device="cuda")
        for k, (c6, d) in enumerate(zip(lists, draws)):
            c6.compact(vis, d, k * cap, d_data, triangles)
            c6.redraw(d_data, triangles, args, target=again, base=k * cap, clear=k == 0)  # (the output's ids keep the gap)
        for k, c6 in enumerate(lists):
            c6.resolve(target=again, base=k * cap)
        torch.cuda.synchronize()
        assert latched(engine) == 0
        h_again = host(again, np.uint64).reshape(h, w)
        assert (h_again >> np.uint64(32)).tobytes() == (h_vis >> np.uint64(32)).tobytes()
        for k, (c6, name) in enumerate(zip(lists, ("draw1", "draw2"))):
            got, _, rstats, pixels, vstats = c6.read()
            want = raster.host_visibility_compact(h_vis, frame[name], cap, k * cap, scene.meshlet_data, triangles)
            want["status"], got["status"] = 0, 0
            assert_equal(f"{name} (triangles={triangles})", got, want)
            assert int(got["commands"][0]) > (1000 if k == 0 else 0)  # (the late list adds a handful: what the early one lost)
            assert not cc.c6_misses(name, h_vis, k * cap, got, triangles, h_again, rstats, pixels, vstats, out_base=k * cap, whole=False)


# -- 5. captured into a graph on the first call of a fresh context, replayed on changed buffers
def test_the_first_call_captures_into_a_graph(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine, visibility_compact_workspace

    by_name = {c.name: c for c in HAND}
    cases = [by_name[k] for k in ("list_257_third", "m_1_2_3_4", "inconsistent")]
    mc, w, h = 300, 64, 11
    nwords = max(len(c.meshlet_data) for c in cases)

    def padded(c):  # the case in the graph's shapes: the buffer in the top-left corner, the list and the data padded
        vis = np.zeros((h, w), np.uint64)
        ch, cw = c.visibility.shape
        assert ch <= h and cw <= w and c.max_commands <= mc
        vis[:ch, :cw] = c.visibility
        words = np.zeros(1 + 7 * mc, np.uint32)
        words[:len(c.words)] = c.words
        data = np.zeros(nwords, np.uint32)
        data[:len(c.meshlet_data)] = c.meshlet_data
        return cc.CompactCase(c.name, vis, words, mc, data, c.command_base)

    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        z = lambda n, dt=torch.int32: torch.full((n,), 5, dtype=dt, device="cuda")  # noqa: E731
        g_vis, g_words, g_data = z(w * h, torch.int64), z(1 + 7 * mc), z(nwords)
        masks, out, ids, vdata, stats = z(8 * mc), z(1 + 7 * mc), z(mc), z(nwords), z(8)
        work = z(visibility_compact_workspace(mc) // 8, torch.int64)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.visibility_compact(g_vis, w, h, g_words, mc, masks, out, mc, work, meshlet_data=g_data, visible_ids=ids,
                                   visible_data=vdata, visible_data_words=nwords, stats=stats, triangles=True)
        for c in cases + cases[:1]:  # replayed: new buffers, new lists, the first ones again
            p = padded(c)
            g_vis.copy_(dev(torch, p.visibility).view(torch.int64))
            g_words.copy_(dev(torch, p.words).view(torch.int32))
            g_data.copy_(dev(torch, p.meshlet_data).view(torch.int32))
            g.replay()
            torch.cuda.synchronize()
            want = raster.host_visibility_compact(p.visibility, p.words, mc, 0, p.meshlet_data, True)
            n, used = int(want["commands"][0]), int(want["stats"]["data_words_needed"])
            assert n > 2 and latched(eng) == want["status"]
            assert host(masks, np.uint32).tobytes() == want["masks"].tobytes(), c.name
            assert host(out, np.uint32)[:1 + 7 * n].tobytes() == want["commands"][:1 + 7 * n].tobytes(), c.name
            assert host(ids, np.uint32)[:n].tobytes() == want["ids"][:n].tobytes(), c.name
            assert host(vdata, np.uint32)[:used].tobytes() == want["data"][:used].tobytes(), c.name
            assert host(stats, np.uint32).tobytes() == want["stats"].tobytes(), c.name
    finally:
        eng.close()
