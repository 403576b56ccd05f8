"""orbit_fragments_shade and orbit_fragments_shade_shadowed on the MI355X with their tile loop entered MORE THAN ONCE per wave
(DESIGN.md §4.29): the tile programmes of tests/shade_tile_cases.py on one workgroup, on two and on the resident grid
(orbit_ctx_set_visibility_grid), in every form of the walk the grid is eligible for, with and without CLEAR, render_mode 8 on
the main programme; one natural-grid run per call on a 1921 x 1081 target, where the resident grid itself takes several
trips; a capped first call of a fresh context captured into a graph, for either call; a cap together with NULL outputs; the
chain shade -> bloom -> post_process on the device under a cap of one workgroup.  Bytes, counters and latched status equal
the host mirrors' (tests/test_shade_tiles_cpu.py holds them to the restatements); every buffer of a single call sits between
sentinel guards, inputs come back unchanged.  No tolerance anywhere.  No test provokes a fault: a stale index, row or
material is ordinary data that the range checks reject."""
import time

import numpy as np
import pytest

import fragments_shade_cases as fc
import fragments_shade_shadowed_cases as sc
import shade_tile_cases as st
import test_fragments_shade_gpu as tsg
import test_fragments_shade_shadowed_gpu as thg
from orbit_amd import _lib, post
from test_gpu_parity import dev, host
from test_raster_depth_gpu import latched

pytestmark = pytest.mark.gpu
OPTIONAL = ("lights_walked", "stats", "shadow_factor", "cascade", "shadow_stats")


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
    e.close()


@pytest.fixture(scope="module")
def progs(oracle):
    return st.programmes(oracle)


@pytest.fixture(scope="module")
def mirrors():
    """the mirrors' results by (call, case name, clear, render_mode): computed once — they do not depend on the grid —, left unchanged"""
    return {}


def mirror_of(mirrors, call, p, clear, render_mode=0):
    key = (call, p.name, clear, render_mode)
    if key not in mirrors:
        mirrors[key] = tsg.mirror(p.case, clear=clear, render_mode=render_mode) if call == "shade" else thg.mirror(p.shadow, clear=clear, render_mode=render_mode)
    return mirrors[key]


def forms_of(p):
    return (None, "per_lane", "staged") if p.case.staged else (None, "per_lane")


def run_call(torch, engine, call, p, **kw):
    return tsg.run(torch, engine, p.case, **kw) if call == "shade" else thg.run(torch, engine, p.shadow, **kw)


def assert_call(call, name, got, want):
    (tsg if call == "shade" else thg).assert_equal(name, got, want)


def assert_counters(name, call, got, expect):
    for k, v in expect[call].items():
        assert int(got["stats"][k]) == v, (name, k, int(got["stats"][k]), v)
    if call == "shadowed":
        for k, v in expect["shadow"].items():
            assert int(got["shadow_stats"][k]) == v, (name, k, int(got["shadow_stats"][k]), v)


# -- 1. the programmes on one workgroup, on two, and on the resident grid (the control: a tile per wave)
def under_the_cap(torch, engine, cap, body):
    if cap:  # the waves of this grid meet every arrangement the layouts are there for
        found = st.arrangements_of(st.LAYOUTS, cap)
        assert found == set(st.ARRANGEMENTS), sorted(set(st.ARRANGEMENTS) - found)
    else:
        resident = 8 * torch.cuda.get_device_properties(0).multi_processor_count
        assert all(len(w) <= 1 for _, tiles in st.LAYOUTS for w in st.assignment(tiles, 0, resident))
    assert latched(engine) == 0
    try:
        engine.set_visibility_grid(cap)
        body()
    finally:
        engine.set_visibility_grid(0)
    assert latched(engine) == 0


@pytest.mark.parametrize("cap", st.CAPS)
@pytest.mark.parametrize("call", ("shade", "shadowed"))
def test_the_programmes_under_a_cap(torch_mod, engine, progs, mirrors, call, cap):
    def body():
        assert [(p.kinds, p.tiles) for p in progs if p.tile != 4] == list(st.LAYOUTS)
        for p in progs:
            for form in forms_of(p):
                for clear in (False, True):
                    name = f"{call} {p.name} (cap {cap}, form={form}, clear={clear})"
                    got = run_call(torch_mod, engine, call, p, clear=clear, form=form)
                    assert_call(call, name, got, mirror_of(mirrors, call, p, clear))
                    assert got["status"] == (_lib.E_RANGE if p.stale(call) else 0), name
                    assert_counters(name, call, got, p.expect)
        main = progs[0]
        for form in forms_of(main):  # the heat map on the main programme
            name = f"{call} {main.name} heat map (cap {cap}, form={form})"
            got = run_call(torch_mod, engine, call, main, clear=True, form=form, render_mode=8)
            assert_call(call, name, got, mirror_of(mirrors, call, main, True, 8))
            assert got["status"] == _lib.E_RANGE, name
            assert_counters(name, call, got, main.expect8)
    under_the_cap(torch_mod, engine, cap, body)


# -- 2. the natural grid: no cap, a target on which the resident grid itself takes several trips
@pytest.mark.parametrize("call", ("shade", "shadowed"))
def test_the_resident_grid_takes_several_trips(torch_mod, engine, oracle, call):
    """shade_tile_cases.natural_programme() four times on a 1921 x 1081 target that is uncovered everywhere else — the first
    trip and the partial column, a middle trip, the partial row, the last tile of the last trip; every list outside the
    copies is empty.  Where it fits, a fifth copy lies one trip behind the first on the same waves: every counter of a wave
    there is fed in two trips."""
    prog = st.natural_programme(oracle)
    w, h, waves = st.natural_target(torch_mod.cuda.get_device_properties(0).multi_processor_count)
    big, shadowed, where = st.instanced(prog, w, h, waves)
    last_trip = (((w + 7) // 8) * ((h + 7) // 8) - 1) // waves
    trips = {name: (first, last) for name, _, _, first, last in where}
    assert last_trip >= 2 and trips["top_right"] == (0, 0) and trips["bottom_right"][1] == last_trip
    assert 0 < trips["middle"][0] <= trips["middle"][1] < last_trip
    assert len(where) == 4 or (trips["same_waves"][0] == 1 and where[4][1] // 8 + (where[4][2] // 8) * ((w + 7) // 8) == (w - prog.width) // 8 + waves)
    assert w % 8 == 1 and h % 8 == 1 and big.visibility[:, w - 1].any() and big.visibility[h - 1, :].any()  # the partial column and row are met
    assert latched(engine) == 0
    engine.set_visibility_grid(0)
    t0 = time.perf_counter()
    want = tsg.mirror(big, clear=True) if call == "shade" else thg.mirror(shadowed, clear=True)
    print(f"natural grid {w} x {h}, {call}: the mirror took {time.perf_counter() - t0:.2f} s")
    got = tsg.run(torch_mod, engine, big, clear=True) if call == "shade" else thg.run(torch_mod, engine, shadowed, clear=True)
    assert_call(call, f"natural grid, {call}", got, want)
    assert got["status"] == (_lib.E_RANGE if prog.stale(call) else 0)
    for k, v in prog.expect[call].items():
        assert int(got["stats"][k]) == len(where) * v, k
    if call == "shadowed":
        for k, v in prog.expect["shadow"].items():
            assert int(got["shadow_stats"][k]) == len(where) * v, k


# -- 3. a capped first call of a fresh context, captured into a graph: the launches carry their grid
def padded(a, nbytes):
    out = np.zeros(nbytes, np.uint8)
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    out[:len(a)] = a
    return out


@pytest.mark.parametrize("call", ("shade", "shadowed"))
def test_a_capped_first_call_captures_into_a_graph(torch_mod, oracle, progs, call):
    torch = torch_mod
    from orbit_amd.engine import Engine

    first, second = progs[0], st.tamper_free_programme(oracle, seed=1)  # one target, one view position, other lists; the first holds the stale kinds
    picked = [first, second, first]
    w, h, cc = first.width, first.height, first.case.cluster_count
    assert (second.width, second.height, second.case.cluster_count, second.case.view_pos) == (w, h, cc, first.case.view_pos)
    args = [p.shadow.args()[0] for p in picked]
    which = list(range(8)) + [15, 16]  # the ten input arrays
    sizes = {k: max(np.ascontiguousarray(a[k]).view(np.uint8).size for a in args) for k in which}
    ic = (np.ascontiguousarray(args[0][7]).view(np.uint8).size - 4) // 4  # the first programme's: its BC list ends one past it
    assert (np.ascontiguousarray(args[1][7]).view(np.uint8).size - 4) // 4 <= ic
    a0 = args[0]
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        z = lambda n: torch.full(((n + 15) // 16 * 16,), 5, dtype=torch.uint8, device="cuda")  # noqa: E731
        g_in = {k: z(n) for k, n in sizes.items()}
        outs = {k: z(n) for k, n in dict(color=16 * w * h, lights_walked=4 * w * h, stats=32, shadow_factor=4 * w * h, cascade=4 * w * h, shadow_stats=16).items()}
        common = (g_in[0], w, h, g_in[1], g_in[2], g_in[3], g_in[4], 12, g_in[5], 40, g_in[6], g_in[7], ic, cc, 8, a0[10], a0[11], a0[12], a0[13], a0[14])
        eng.set_visibility_grid(1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            if call == "shade":
                eng.fragments_shade(*common, outs["color"], lights_walked=outs["lights_walked"], stats=outs["stats"], clear=True)
            else:
                eng.fragments_shade_shadowed(*common, outs["color"], g_in[15], len(a0[15]), g_in[16], len(a0[16]), a0[17], a0[18], a0[19], a0[20],
                                             shadow_index_base=sc.BASE, shadow_factor=outs["shadow_factor"], cascade=outs["cascade"],
                                             shadow_stats=outs["shadow_stats"], lights_walked=outs["lights_walked"], stats=outs["stats"], clear=True)
        eng.set_visibility_grid(0)  # (the captured launches carry their grid)
        for p, a in zip(picked, args):
            for k in which:
                x = padded(a[k], sizes[k])
                g_in[k][:len(x)].copy_(torch.from_numpy(x).cuda())
            full = p.case.copy(p.name)  # (the mirror reads the list behind the same capacity: the buffer padded as the device's is)
            full.index_buffer = padded(a[7], 4 + 4 * ic)
            over = dict(index_capacity=ic, clear=True, fill=0)
            want = fc.mirror(full, **over) if call == "shade" else sc.mirror(sc.ShadowCase(full, p.shadow.rows, p.shadow.maps), **over)
            assert want["status"] == (_lib.E_RANGE if p.stale(call) else 0), p.name
            keys = ("color", "lights_walked", "stats") + (("shadow_factor", "cascade", "shadow_stats") if call == "shadowed" else ())
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == want["status"], p.name
                for k in keys:
                    assert host(outs[k])[:want[k].nbytes].tobytes() == want[k].tobytes(), (p.name, k, replay)
        assert first.stale(call) and not second.stale(call)
    finally:
        eng.set_visibility_grid(0)
        eng.close()


# -- 4. a cap and NULL outputs together: the walk does not depend on which outputs exist
def test_a_cap_of_one_with_null_outputs(torch_mod, engine, progs, mirrors):
    main = progs[0]
    assert latched(engine) == 0
    try:
        engine.set_visibility_grid(1)
        for clear in (False, True):
            for form in forms_of(main):
                want = mirror_of(mirrors, "shade", main, clear)
                for kw in (dict(with_walked=False), dict(with_stats=False), dict(with_walked=False, with_stats=False)):
                    got = tsg.run(torch_mod, engine, main.case, clear=clear, form=form, **kw)
                    tsg.assert_equal(f"{main.name} {kw} (cap 1, clear={clear}, form={form})", got, want)
                    assert got["status"] == _lib.E_RANGE
                want = mirror_of(mirrors, "shadowed", main, clear)
                for without in [(k,) for k in OPTIONAL] + [OPTIONAL]:
                    got = thg.run(torch_mod, engine, main.shadow, clear=clear, form=form, without=without)
                    thg.assert_equal(f"{main.name} without {without} (cap 1, clear={clear}, form={form})", got, want)
                    assert got["status"] == _lib.E_RANGE and all(got[k] is None for k in without)
    finally:
        engine.set_visibility_grid(0)


# -- 5. the chain on the device under a cap of one workgroup: nothing copied to the host in between
def test_the_chain_on_the_device_under_a_cap_of_one(torch_mod, engine, oracle):
    torch = torch_mod
    prog = st.tamper_free_programme(oracle)
    a, kw = prog.shadow.args()
    h, w = a[0].shape
    bufs, outs, _, _ = thg.device_job(torch, prog.shadow)
    ic = (np.ascontiguousarray(a[7]).view(np.uint8).size - 4) // 4
    lay = post.bloom_layout(w, h)
    color = torch.zeros(4 * w * h, dtype=torch.float32, device="cuda")
    mips = torch.zeros(lay["total_texels"], dtype=torch.int32, device="cuda")
    ldr = torch.zeros(4 * w * h, dtype=torch.float32, device="cuda")
    rgba8 = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
    bloom_stats, post_stats = (torch.zeros(4, dtype=torch.int32, device="cuda") for _ in range(2))
    assert latched(engine) == 0
    try:
        engine.set_visibility_grid(1)
        engine.fragments_shade_shadowed(bufs[0], w, h, bufs[1], bufs[2], bufs[3], bufs[4], len(a[4]), bufs[5], len(a[5]), bufs[6], bufs[7], ic, a[8], a[9],
                                        a[10], a[11], a[12], a[13], a[14], color, bufs[8], len(a[15]), bufs[9], len(a[16]), a[17], a[18], a[19], a[20],
                                        shadow_index_base=kw["shadow_index_base"], shadow_stats=outs["shadow_stats"], stats=outs["stats"], clear=True)
        engine.bloom(color, w, h, mips, stats=bloom_stats)
        engine.post_process(color, w, h, bloom=mips, ldr=ldr, rgba8=rgba8, stats=post_stats, exposure=0.1, bloom_intensity=0.4)
        torch.cuda.synchronize()
    finally:
        engine.set_visibility_grid(0)
    assert latched(engine) == 0
    shaded = sc.mirror(prog.shadow, clear=True)
    assert shaded["status"] == 0 and host(color, np.float32).tobytes() == shaded["color"].tobytes()
    assert host(outs["stats"]).tobytes() == shaded["stats"].tobytes() and host(outs["shadow_stats"]).tobytes() == shaded["shadow_stats"].tobytes()
    want_b = post.host_bloom(shaded["color"])
    want_p = post.host_post_process(shaded["color"], want_b["mips"], exposure=0.1, bloom_intensity=0.4)
    assert host(mips, np.uint32).tobytes() == want_b["mips"].tobytes() and host(bloom_stats, np.uint32).tobytes() == want_b["stats"].tobytes()
    assert host(ldr, np.float32).tobytes() == want_p["ldr"].tobytes() and host(rgba8, np.uint8).tobytes() == want_p["rgba8"].tobytes()
    assert host(post_stats, np.uint32).tobytes() == want_p["stats"].tobytes()
    # 73 x 33 pixels are ten blocks of 256: under the cap the pass over the pixels takes ten trips (a degenerate pixel is stored as 0: L8)
    assert int(want_p["stats"]["pixels"]) == w * h == 2409 and prog.expect["shadowed"]["degenerate_pixels"] == 2
    assert int(want_p["stats"]["bloom_pixels"]) > 1000 and len(np.unique(want_p["rgba8"][..., :3])) > 100  # a picture, not a constant
