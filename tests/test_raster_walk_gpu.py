"""The walker pins on the MI355X (tests/raster_walk_cases.py): on every case both raster calls leave
the host mirror's bytes, counters and latched status (orbit_amd.raster on the same buffers — never a restatement;
tests/test_raster_walk_cpu.py holds the mirror to the restatements), the visibility words' high halves are the depth
call's bytes (V4), and the case's claims hold on the device's output; the cases named for the pieces form give the
unflagged bytes under ORBIT_RASTER_CLIP_NEAR, ORBIT_RASTER_WIDE_GUARD and both; the lists for a capped grid
(orbit_ctx_set_raster_grid) run on one workgroup, on two and on the resident grid, so that one wave takes a good, a
failed and a good command, a small command after a large one, two entities' commands under CLIP_NEAR, and the clamp of
max_commands; the clearing launch strides under the same cap; a capped first call captures into a graph.  Every buffer
sits between sentinel guards; inputs come back unchanged."""
import numpy as np
import pytest

import raster_cases as rc
import raster_walk_cases as wk
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import latched
from test_raster_wide_gpu import assert_equal, high_halves, run_case

pytestmark = pytest.mark.gpu
SENTINEL = rc.SENTINEL
CASES = wk.all_cases()
LISTS = wk.grid_lists()


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
    e.set_raster_grid(0)
    e.close()


def both_calls_equal_the_mirror(torch, engine, pk, clip_near=None, wide=False, claims=True):
    """Both calls on guarded buffers against the mirror: bytes, counters, latched status, V4, the claims
    -> (visibility, its stats, the depth call's command errors)."""
    case = pk.case
    name = f"{case.name} (clip_near={clip_near}, wide={wide})"
    clip_near = case.clip_near if clip_near is None else clip_near
    want_vis, want_vstats, verr = wk.host_vis(pk, clip_near, wide)
    want_depth, want_dstats, derr = wk.host_depth(pk, clip_near, wide)
    assert latched(engine) == 0, name
    got_vis, got_vstats = run_case(torch, engine, "visibility", pk, clip_near=clip_near, wide_guard=wide)
    assert latched(engine) == (_lib.E_RANGE if verr.any() else 0), name
    got_depth, got_dstats = run_case(torch, engine, "depth", pk, clip_near=clip_near, wide_guard=wide)
    assert latched(engine) == (_lib.E_RANGE if derr.any() else 0), name
    assert_equal(name, got_vis, got_vstats, want_vis, want_vstats)
    assert_equal(name, got_depth, got_dstats, want_depth, want_dstats)
    if verr.tobytes() == derr.tobytes():  # (V4 is of lists both calls accept alike: V3's limit is the visibility call's)
        assert high_halves(got_vis).tobytes() == got_depth.view(np.uint32).tobytes(), name
        assert got_vstats.tobytes() == got_dstats.tobytes(), name
    if claims:  # (None: the route to the lane or the wave is claimed on the restatement's extras, on the CPU)
        assert not wk.check_claims(case, got_vis, got_vstats, verr, None), name
    return got_vis, got_vstats, derr


# -- 1. every walker case: both calls, bytes, counters, latched status, V4, claims
@pytest.mark.parametrize("stride,offset", [(12, 0), (32, 20)])
def test_every_case_equals_the_host_mirror(torch_mod, engine, stride, offset):
    engine.set_raster_grid(0)
    for case in CASES:
        both_calls_equal_the_mirror(torch_mod, engine, rc.Packed(case, stride, offset))


# -- 2. the pieces form on shapes that cross neither the near plane nor the band: the unflagged call's bytes and counters
@pytest.mark.parametrize("clip_near,wide", wk.FLAG_SETS[1:])
def test_the_pieces_form_walks_as_the_plain_form(torch_mod, engine, clip_near, wide):
    engine.set_raster_grid(0)
    by_name = {c.name: c for c in CASES}
    for name in wk.PIECES_CASES:
        pk = rc.Packed(by_name[name])
        got_vis, got_stats, _ = both_calls_equal_the_mirror(torch_mod, engine, pk, clip_near, wide)
        plain_vis, plain_stats, _ = wk.host_vis(pk, False, False)
        assert got_vis.tobytes() == plain_vis.tobytes() and got_stats.tobytes() == plain_stats.tobytes(), name


# -- 3. one wave, several commands: the lists on one workgroup, on two, and on the resident grid
@pytest.mark.parametrize("stride,offset", [(12, 0), (32, 20)])
@pytest.mark.parametrize("cap", wk.CAPS)
def test_capped_grids(torch_mod, engine, cap, stride, offset):
    found = set()
    try:
        engine.set_raster_grid(cap)
        for case in LISTS:
            pk = rc.Packed(case, stride, offset)
            _, _, derr = both_calls_equal_the_mirror(torch_mod, engine, pk)
            if cap:
                found |= wk.arrangements(pk, wk.host_vis(pk)[2], cap) | wk.arrangements(pk, derr, cap)
    finally:
        engine.set_raster_grid(0)
    if cap:  # the waves of this grid met every arrangement the lists are there for
        skip = set(wk.NOT_UNDER_TWO_WORKGROUPS) if cap == 2 else set()
        assert found >= set(wk.ARRANGEMENTS) - skip, set(wk.ARRANGEMENTS) - found


def test_the_pieces_form_under_a_cap(torch_mod, engine):
    """The walker cases of the pieces form on one workgroup, under both flags: its four waves stride over the commands
    with the kept mvp and the `best` outcome of each lane."""
    by_name = {c.name: c for c in CASES}
    try:
        engine.set_raster_grid(1)
        for name in wk.PIECES_CASES[::3] + ["two_wave_pieces_beside_a_wave_triangle"]:
            both_calls_equal_the_mirror(torch_mod, engine, rc.Packed(by_name[name]), True, True)
    finally:
        engine.set_raster_grid(0)


# -- 4. the clearing launch shares the cap: one workgroup strides over 57 600 words
def test_the_clear_strides_under_the_cap(torch_mod, engine):
    w, h = 320, 180
    case = wk.WalkCase("full_target_320x180", [rc.tri((-1, -1), (-1, 3 * h), (3 * w, -1), z=0.75)], width=w, height=h,
                       stats=dict(triangles=1, fragments=w * h), covered_count=w * h,
                       winners=lambda won, e, s, err: won == {(0, 0): w * h})
    assert w * h > 1024 * 4  # more words than one workgroup clears in a round
    try:
        for cap in (1, 0):
            engine.set_raster_grid(cap)
            both_calls_equal_the_mirror(torch_mod, engine, rc.Packed(case))
    finally:
        engine.set_raster_grid(0)


# -- 5. a capped first call of a fresh context, captured into a graph
def test_a_capped_first_call_captures_into_a_graph(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine

    by_name = {c.name: c for c in LISTS}
    # (lists whose faults do not depend on the buffers' sizes, which the graph's buffers pad)
    pks = [rc.Packed(by_name[k]) for k in ("grid_9_corner_is_vcount", "grid_9_large_then_small", "grid_8")]
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
        depth = torch.full((48 * 64,), 5.0, dtype=torch.float32, device="cuda")
        vstats, dstats = (torch.full((32,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2))
        eng.set_raster_grid(1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.raster_visibility(g_words, 9, g_data, g_vb, vcount, g_ent, 1, rc.pixel_proj(64, 48), vis, 64, 48, command_base=base,
                                  clear=True, stats=vstats, meshlet_data_words=nb["data"] // 4)
            eng.raster_depth(g_words, 9, g_data, g_vb, vcount, g_ent, 1, rc.pixel_proj(64, 48), depth, 64, 48, clear=True,
                             stats=dstats, meshlet_data_words=nb["data"] // 4)
        eng.set_raster_grid(0)  # (the captured launches carry their grid)
        for pk in pks + pks[:1]:  # replayed: new commands, new geometry, the first ones again
            assert pk.vertex_count <= vcount and len(pk.commands) <= 9
            g_words.copy_(dev(torch, pad(pk.words, nb["words"])))
            g_data.copy_(dev(torch, pad(pk.meshlet_data, nb["data"])))
            g_vb.copy_(dev(torch, pad(pk.vertices, nb["vb"])))
            g_ent.copy_(dev(torch, pad(pk.entities, nb["ent"])))
            g.replay()
            torch.cuda.synchronize()
            args = (pad(pk.words, nb["words"]).view(np.uint32), 9, pad(pk.meshlet_data, nb["data"]).view(np.uint32), pad(pk.vertices, nb["vb"]), vcount,
                    pad(pk.entities, nb["ent"]), rc.pixel_proj(64, 48), 64, 48)
            want_vis, want_vstats, err = raster.host_raster_visibility(*args, command_base=base, entity_count=1)
            want_depth, want_dstats, _ = raster.host_raster_depth(*args, entity_count=1)
            assert [k for k, e in enumerate(err) if e] == sorted(pk.case.faults), pk.case.name
            assert latched(eng) == (_lib.E_RANGE if err.any() else 0), pk.case.name
            assert_equal(pk.case.name, host(vis, np.uint64).reshape(48, 64), host(vstats).view(L.RASTER_STATS)[0], want_vis, want_vstats)
            assert_equal(pk.case.name, host(depth, np.float32).reshape(48, 64), host(dstats).view(L.RASTER_STATS)[0], want_depth, want_dstats)
            assert int(want_vstats["fragments"]) > 0
    finally:
        eng.close()


def test_the_hook_needs_a_context(torch_mod, engine):
    assert engine._lib.orbit_ctx_set_raster_grid(None, 1) == _lib.E_INVALID
    engine.set_raster_grid(3)
    engine.set_raster_grid(0)
    assert latched(engine) == 0
