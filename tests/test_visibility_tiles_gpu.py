"""The three readers of a finished visibility buffer — orbit_visibility_resolve, orbit_visibility_compact,
orbit_visibility_surface — on the MI355X with their tile loop entered MORE THAN ONCE per wave: the tile
programmes of tests/visibility_tile_cases.py on one workgroup, on two and on the resident grid
(orbit_ctx_set_visibility_grid); the sibling suites' hand-built and stale cases on one workgroup; the lists that take the
compaction's totals launch into its second round, and the clears striding from one workgroup; one natural-grid run on a
1921 x 1081 target drawn on the device, where the resident grid itself takes several trips; a capped first call of a fresh
context captured into a graph; the hook.  Bytes, counters and latched status equal the host mirror's on the same buffers
(tests/test_visibility_tiles_cpu.py holds it to the restatements); every buffer sits between sentinel guards, inputs come
back unchanged.  No tolerance anywhere.  No test provokes a fault: a stale word is data that the range checks reject.
The two later readers, orbit_visibility_surface_drawn and orbit_surface_fragments: tests/test_surface_tiles_gpu.py."""
import numpy as np
import pytest

import raster_walk_cases as wk
import test_visibility_compact_gpu as tcg
import test_visibility_surface_gpu as tsg
import visibility_compact_cases as cc
import visibility_surface_cases as sc
import visibility_tile_cases as tc
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import Guarded, latched
from test_raster_wide_gpu import assert_equal as raster_equal
from test_raster_wide_gpu import run_case

pytestmark = pytest.mark.gpu
FILL = tcg.FILL
MODES = (False, True)
PROGS = tc.programmes()
LISTS = tc.second_round_cases()


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
    e.set_visibility_grid(0)
    e.set_raster_grid(0)
    e.close()


def resolve_equals_the_mirror(torch, engine, name, vis, base, n):
    """One orbit_visibility_resolve call on guarded buffers that start as the sentinel, against the mirror."""
    h, w = vis.shape
    g_vis = Guarded(torch, vis)
    depth, pixels, stats = (Guarded(torch, np.zeros(0, np.uint8), nbytes=k) for k in (4 * w * h, 4 * n, 16))
    engine.visibility_resolve(g_vis.ptr, w, h, base, n, depth=depth.ptr, command_pixels=pixels.ptr, stats=stats.ptr)
    torch.cuda.synchronize()
    g_vis.unchanged()
    want_depth, want_pixels, want_stats = raster.host_visibility_resolve(vis, base, n)
    got = stats.read().view(L.VIS_STATS)[0]
    assert got.tobytes() == want_stats.tobytes(), f"{name}: device stats {got} != host {want_stats}"
    diff = np.flatnonzero(pixels.read().view(np.uint32) != want_pixels)
    assert len(diff) == 0, f"{name}: command_pixels: {len(diff)} entries differ, first at {diff[0]}"
    assert depth.read().tobytes() == want_depth.tobytes(), name
    return got, want_pixels


def compact_equals_the_mirror(torch, engine, name, case, triangles, **over):
    want = tcg.mirror(case, triangles, **over)
    got = tcg.run(torch, engine, case, triangles, **over)
    tcg.assert_equal(name, got, want)
    return got


def surface_equals_the_mirror(torch, engine, name, case, clear):
    got = tsg.run(torch, engine, case, clear=clear)
    tsg.assert_equal(name, got, tsg.mirror(case, clear=clear))
    return got


def readers_equal_the_mirrors(torch, engine, prog, tag):
    """All three readers over one programme: resolve, compact plain and cut, surface with and without CLEAR."""
    name = f"{prog.name} ({tag})"
    assert latched(engine) == 0, name
    resolve_equals_the_mirror(torch, engine, name, prog.visibility, tc.BASE, prog.max_commands)
    assert latched(engine) == 0, name
    for triangles in MODES:
        got = compact_equals_the_mirror(torch, engine, f"{name}, triangles={triangles}", prog.compact, triangles)
        assert got["status"] == 0 and int(got["stats"]["visible_commands"]) == prog.max_commands
    for clear in (False, True):
        got = surface_equals_the_mirror(torch, engine, f"{name}, clear={clear}", prog.surface, clear)
        assert got["status"] == (_lib.E_RANGE if prog.surface.stale else 0), name
        for k, v in prog.expect["surface"].items():
            assert int(got["stats"][k]) == v, (name, k)


# -- 1. the programme on one workgroup, on two, and on the resident grid (the control: a tile per wave)
@pytest.mark.parametrize("cap", tc.CAPS)
def test_the_programme_under_a_cap(torch_mod, engine, cap):
    if cap:  # the waves of this grid meet every arrangement the layout is there for
        found = tc.arrangements_of(PROGS, cap)
        assert found == set(tc.ARRANGEMENTS), sorted(set(tc.ARRANGEMENTS) - found)
    else:
        resident = 8 * torch_mod.cuda.get_device_properties(0).multi_processor_count
        assert all(len(w) <= 1 for p in PROGS for w in tc.assignment(p.tiles, 0, resident))
    try:
        engine.set_visibility_grid(cap)
        for prog in PROGS:
            readers_equal_the_mirrors(torch_mod, engine, prog, f"cap {cap}")
    finally:
        engine.set_visibility_grid(0)


# -- 2. the sibling suites' hand-built and stale cases (65 x 9: 18 tiles, four or five per wave) on one workgroup
def test_the_census_of_the_surface_under_a_cap_of_one(torch_mod, engine):
    cases = sc.hand_cases() + sc.stale_cases()
    assert len(cases) > 25 and latched(engine) == 0
    stale = written = 0
    try:
        engine.set_visibility_grid(1)
        for case in cases:
            for clear in (False, True):
                got = surface_equals_the_mirror(torch_mod, engine, f"{case.name} (cap 1, clear={clear})", case, clear)
                stale, written = stale + int(got["stats"]["stale_pixels"]), written + int(got["stats"]["written_pixels"])
    finally:
        engine.set_visibility_grid(0)
    assert stale >= 2 * 9 and written > 2 * 2000  # (both runs of each case; nine stale cases of a pixel or more)


def test_the_census_of_the_compaction_under_a_cap_of_one(torch_mod, engine):
    assert latched(engine) == 0
    visible = 0
    try:
        engine.set_visibility_grid(1)
        for case in tcg.HAND:
            for triangles in MODES:
                got = compact_equals_the_mirror(torch_mod, engine, f"{case.name} (cap 1, triangles={triangles})", case, triangles)
                visible += int(got["stats"]["visible_commands"])
    finally:
        engine.set_visibility_grid(0)
    assert visible > 2 * 2 * cc.CHUNK  # (both modes; three_chunks alone shows 2 * CHUNK + 5 in each)


# -- 3. the totals' second round, and compact_clear_kernel striding over 8 * 65 797 mask words from one workgroup
@pytest.mark.parametrize("cap", (0, 1))
@pytest.mark.parametrize("case", LISTS, ids=[c.name for c in LISTS])
def test_the_second_round_of_the_totals(torch_mod, engine, case, cap):
    assert latched(engine) == 0
    words = case.expect_cut["data_words_needed"]
    try:
        engine.set_visibility_grid(cap)
        for triangles in MODES:
            name = f"{case.name} (cap {cap}, triangles={triangles})"
            got = compact_equals_the_mirror(torch_mod, engine, name, case, triangles, visible_data_words=words if triangles else 0)
            assert got["status"] == 0
            for k, v in {**case.expect, **(case.expect_cut if triangles else {})}.items():
                assert int(got["stats"][k]) == v, (name, k)
            for j, k in case.claims:  # everything in front of j is the carry that reached command k's block
                assert int(got["ids"][j]) == k, (name, j, k)
    finally:
        engine.set_visibility_grid(0)


@pytest.mark.parametrize("cap", (0, 1))
def test_capacities_cut_the_prefix_in_round_two(torch_mod, engine, cap):
    case = next(c for c in LISTS if c.name == "chunks_258")
    full = tcg.mirror(case, True, visible_data_words=case.expect_cut["data_words_needed"])
    assert latched(engine) == 0 and full["status"] == 0
    try:
        engine.set_visibility_grid(cap)
        for what, over, triangles in tc.second_round_capacities(full["stats"]):
            if not triangles:
                over = dict(over, visible_data_words=0)
            got = compact_equals_the_mirror(torch_mod, engine, f"chunks_258 {what} (cap {cap})", case, triangles, **over)
            assert got["status"] == (0 if "exact" in what else _lib.E_CAPACITY), what
            n = int(got["commands"][0])
            assert n == int(full["stats"]["visible_commands"]) - (0 if "exact" in what else 1), what
            assert (got["commands"][1 + 7 * n:] == FILL).all() and (got["ids"][n:] == FILL).all()
    finally:
        engine.set_visibility_grid(0)


# -- 4. resolve_clear_kernel: one workgroup takes five rounds over 5 000 entries that start as the sentinel
@pytest.mark.parametrize("cap", (1, 0))
def test_the_resolves_clear_strides_under_the_cap(torch_mod, engine, cap):
    main, n = PROGS[0], tc.RESOLVE_CLEAR_COMMANDS
    assert n > 4 * 256 * 4 and latched(engine) == 0
    try:
        engine.set_visibility_grid(cap)
        stats, pixels = resolve_equals_the_mirror(torch_mod, engine, f"5000 entries (cap {cap})", main.visibility, tc.BASE, n)
    finally:
        engine.set_visibility_grid(0)
    assert int(stats["visible_commands"]) == main.max_commands + 1 and not pixels[main.max_commands + 1:].any()


# -- 5. the natural grid: no cap, a target on which the resident grid itself takes several trips
def test_the_resident_grid_takes_several_trips(torch_mod, engine):
    """The main programme's meshes four times on a 1921 x 1081 target — the first trip and the partial column, a middle
    trip, the partial row, the last tile of the last trip —, drawn by orbit_raster_visibility on the device; the three
    readers run on that buffer, and the references are the mirrors on the buffer read back."""
    torch = torch_mod
    from orbit_amd.engine import visibility_compact_workspace

    w, h, waves = tc.natural_target(torch.cuda.get_device_properties(0).multi_processor_count)
    pk, where = tc.instanced(PROGS[0], w, h, waves)
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    last_trip = (tiles - 1) // waves
    trips = {name: (first, last) for name, _, _, first, last in where}
    assert last_trip >= 2 and trips["top_right"] == (0, 0) and trips["bottom_right"][1] == last_trip
    assert 0 < trips["middle"][0] <= trips["middle"][1] < last_trip
    opts, (words, mc, data, vb, vcount, ent, vp, _, _) = pk.args()
    assert latched(engine) == 0
    engine.set_visibility_grid(0)
    z = lambda n, dt=torch.int32: torch.full((max(int(n), 1),), 5, dtype=dt, device="cuda")  # noqa: E731
    d_words, d_data, d_vb, d_ent = dev(torch, words), dev(torch, data), dev(torch, vb), dev(torch, ent)
    vis = z(w * h, torch.int64)
    engine.raster_visibility(d_words, mc, d_data, d_vb, vcount, d_ent, opts["entity_count"], vp, vis, w, h, command_base=tc.BASE,
                             clear=True, clip_near=True, meshlet_data_words=len(data))
    depth, pixels, rstats = z(w * h, torch.float32), z(mc), z(4)
    engine.visibility_resolve(vis, w, h, tc.BASE, mc, depth=depth, command_pixels=pixels, stats=rstats)
    compacted = []
    for triangles in MODES:
        c = dict(masks=z(8 * mc), commands=z(1 + 7 * mc), ids=z(mc), data=z(len(data)), stats=z(8),
                 work=z(visibility_compact_workspace(mc) // 8, torch.int64))
        engine.visibility_compact(vis, w, h, d_words, mc, c["masks"], c["commands"], mc, c["work"], command_base=tc.BASE,
                                  meshlet_data=d_data, meshlet_data_words=len(data), visible_ids=c["ids"],
                                  visible_data=c["data"] if triangles else None, visible_data_words=len(data) if triangles else 0,
                                  stats=c["stats"], triangles=triangles)
        compacted.append(c)
    outs = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))
    sstats = z(8)
    engine.visibility_surface(vis, w, h, d_words, mc, d_data, d_vb, vcount, d_ent, opts["entity_count"], vp, **outs, stats=sstats,
                              command_base=tc.BASE, clear=True, meshlet_data_words=len(data))
    torch.cuda.synchronize()
    assert latched(engine) == 0
    h_vis = host(vis, np.uint64).reshape(h, w)
    # the resolve
    want_depth, want_pixels, want_stats = raster.host_visibility_resolve(h_vis, tc.BASE, mc)
    assert host(rstats, np.uint32).tobytes() == want_stats.tobytes()
    assert host(pixels, np.uint32).tobytes() == want_pixels.tobytes() and host(depth, np.float32).tobytes() == want_depth.tobytes()
    assert want_pixels.all()  # every command of every instance won a pixel: no instance was drawn over
    # the compaction
    for triangles, c in zip(MODES, compacted):
        want = raster.host_visibility_compact(h_vis, words, mc, tc.BASE, data, triangles, fill=5)
        got = {k: host(c[k], np.uint32) for k in ("masks", "commands", "ids", "stats")}
        got.update(data=host(c["data"], np.uint32) if triangles else None, stats=got["stats"].view(L.VIS_COMPACT_STATS)[0], status=0)
        tcg.assert_equal(f"natural grid (triangles={triangles})", got, want)
        assert int(got["commands"][0]) == mc
    # the surface
    want = raster.host_visibility_surface(h_vis, words, mc, data, vb, vcount, ent, vp, command_base=tc.BASE, clear=True,
                                          entity_count=opts["entity_count"])
    got = {k: host(outs[k], tsg.DTYPE[k]).reshape(h, w, -1) for k in tsg.KEYS}
    tsg.assert_equal("natural grid", dict(got, stats=host(sstats, np.uint32).view(L.SURFACE_STATS)[0], status=0), want)
    st = want["stats"]
    assert int(st["written_pixels"]) > 100000 and int(st["unsupported_pixels"]) > 0 and int(st["degenerate_pixels"]) > 0
    assert int(st["stale_pixels"]) == 0 and int(st["foreign_pixels"]) == 0
    # the four instances hold the same picture where nothing spills into them: the K tiles' 64 keys each
    tiles_x = (PROGS[0].width + 7) // 8
    k_tile = PROGS[0].kinds.index("K")
    for name, dx, dy, _, _ in where:
        y0, x0 = dy + 8 * (k_tile // tiles_x), dx + 8 * (k_tile % tiles_x)
        assert len(np.unique(h_vis[y0:y0 + 8, x0:x0 + 8] & np.uint64(0xFFFFFFFF))) == 64, name


# -- 6. a capped first call of a fresh context, captured into a graph: the launches carry their grid
def test_a_capped_first_call_captures_into_a_graph(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine, visibility_compact_workspace

    main = PROGS[0]
    h, w = main.visibility.shape
    tile_row = (np.mgrid[0:h, 0:w][0] // 8)
    other = np.where(tile_row % 2 == 1, main.visibility, np.uint64(0))  # the same list, every other tile row empty
    opts, (words, mc, data, vb, vcount, ent, vp, _, _) = main.packed.args()
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran any of the calls
    try:
        z = lambda n, dt=torch.int32: torch.full((max(int(n), 1),), 5, dtype=dt, device="cuda")  # noqa: E731
        d_words, d_data, d_vb, d_ent = dev(torch, words), dev(torch, data), dev(torch, vb), dev(torch, ent)
        vis = z(w * h, torch.int64)
        depth, pixels, rstats = z(w * h, torch.float32), z(mc), z(4)
        c = dict(masks=z(8 * mc), commands=z(1 + 7 * mc), ids=z(mc), data=z(len(data)), stats=z(8),
                 work=z(visibility_compact_workspace(mc) // 8, torch.int64))
        outs = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))
        sstats = z(8)
        eng.set_visibility_grid(1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.visibility_resolve(vis, w, h, tc.BASE, mc, depth=depth, command_pixels=pixels, stats=rstats)
            eng.visibility_compact(vis, w, h, d_words, mc, c["masks"], c["commands"], mc, c["work"], command_base=tc.BASE,
                                   meshlet_data=d_data, meshlet_data_words=len(data), visible_ids=c["ids"], visible_data=c["data"],
                                   visible_data_words=len(data), stats=c["stats"], triangles=True)
            eng.visibility_surface(vis, w, h, d_words, mc, d_data, d_vb, vcount, d_ent, opts["entity_count"], vp, **outs,
                                   stats=sstats, command_base=tc.BASE, clear=True, meshlet_data_words=len(data))
        eng.set_visibility_grid(0)  # (the captured launches carry their grid)
        for name, buffer in (("main", main.visibility), ("other", other), ("main again", main.visibility)):
            vis.copy_(dev(torch, buffer).view(torch.int64))
            g.replay()
            torch.cuda.synchronize()
            want_depth, want_pixels, want_stats = raster.host_visibility_resolve(buffer, tc.BASE, mc)
            assert host(rstats, np.uint32).tobytes() == want_stats.tobytes(), name
            assert host(pixels, np.uint32).tobytes() == want_pixels.tobytes() and host(depth, np.float32).tobytes() == want_depth.tobytes(), name
            want = raster.host_visibility_compact(buffer, words, mc, tc.BASE, data, True, fill=5)
            n, used = int(want["commands"][0]), int(want["stats"]["data_words_needed"])
            assert n > 100 and want["status"] == 0
            assert host(c["masks"], np.uint32).tobytes() == want["masks"].tobytes(), name
            assert host(c["commands"], np.uint32)[:1 + 7 * n].tobytes() == want["commands"][:1 + 7 * n].tobytes(), name
            assert host(c["ids"], np.uint32)[:n].tobytes() == want["ids"][:n].tobytes(), name
            assert host(c["data"], np.uint32)[:used].tobytes() == want["data"][:used].tobytes(), name
            assert host(c["stats"], np.uint32).tobytes() == want["stats"].tobytes(), name
            want = raster.host_visibility_surface(buffer, words, mc, data, vb, vcount, ent, vp, command_base=tc.BASE, clear=True,
                                                  entity_count=opts["entity_count"])
            assert latched(eng) == want["status"] == _lib.E_RANGE, name  # (the S tiles' words: both buffers hold some)
            for k in tsg.KEYS:
                assert host(outs[k]).tobytes() == want[k].tobytes(), (name, k)
            assert host(sstats, np.uint32).tobytes() == want["stats"].tobytes(), name
            assert int(want["stats"]["written_pixels"]) > 300
    finally:
        eng.set_visibility_grid(0)
        eng.close()


# -- 7. the hook itself
def test_the_hook_needs_a_context_and_touches_no_raster_launch(torch_mod, engine):
    assert engine._lib.orbit_ctx_set_visibility_grid(None, 1) == _lib.E_INVALID
    assert latched(engine) == 0
    pk = PROGS[1].packed
    want_vis, want_stats, err = wk.host_vis(pk)
    assert not err.any()
    try:
        engine.set_visibility_grid(1)  # a raster call under the readers' cap ...
        got_vis, got_stats = run_case(torch_mod, engine, "visibility", pk, wide_guard=False)
        raster_equal("raster under set_visibility_grid(1)", got_vis, got_stats, want_vis, want_stats)
        engine.set_visibility_grid(0)
        engine.set_raster_grid(1)      # ... and the readers under the raster's
        for prog in PROGS:
            readers_equal_the_mirrors(torch_mod, engine, prog, "set_raster_grid(1)")
    finally:
        engine.set_visibility_grid(0)
        engine.set_raster_grid(0)
    assert latched(engine) == 0
