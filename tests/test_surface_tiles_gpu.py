"""orbit_visibility_surface_drawn and orbit_surface_fragments on the MI355X with their tile loop entered MORE THAN ONCE per
wave: the tile programmes of tests/surface_tile_cases.py — and, for the fragments, those of
tests/visibility_tile_cases.py — on one workgroup, on two and on the resident grid (orbit_ctx_set_visibility_grid), the
drawn reader with flags 40 and with flags 8 on the same buffer, the fragments with and without grad, each with and
without CLEAR; the chain raster -> surface -> fragments on the device under a cap of one workgroup; one natural-grid run
on a 1921 x 1081 target drawn on the device, where the resident grid itself takes several trips; a capped first call of a
fresh context captured into a graph, for either reader; a cap together with NULL outputs.  Bytes, counters and latched
status equal the host mirror's on the same buffers (tests/test_surface_tiles_cpu.py holds it to the restatements); every
buffer of a single call sits between sentinel guards, inputs come back unchanged.  No tolerance anywhere.  No test
provokes a fault: a stale word or record is ordinary data that the range checks reject."""
import time

import numpy as np
import pytest

import surface_drawn_cases as dc
import surface_fragments_cases as fc
import surface_tile_cases as st
import test_surface_drawn_gpu as tdg
import test_surface_fragments_gpu as tfg
import visibility_tile_cases as tc
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import latched

pytestmark = pytest.mark.gpu
NO_GRAD = tuple(k for k in tfg.KEYS if k != "uv_grad")


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
def progs():
    return st.programmes()


@pytest.fixture(scope="module")
def tamper_free():
    return st.tamper_free_programme()


@pytest.fixture(scope="module")
def old_frags():
    return st.old_programmes_as_frag_cases()


@pytest.fixture(scope="module")
def mirrors():
    """the mirror's results by (reader, case name, clear): computed once — they do not depend on the grid —, left unchanged"""
    return {}


def drawn_mirror(mirrors, case, clear):
    key = ("drawn", case.name, clear)
    if key not in mirrors:
        mirrors[key] = tdg.mirror(case, clear=clear)
    return mirrors[key]


def frag_mirror(mirrors, case, clear):
    key = ("frag", case.name, clear)
    if key not in mirrors:
        mirrors[key] = tfg.mirror(case, clear=clear)
    return mirrors[key]


# -- 1. the programmes on one workgroup, on two, and on the resident grid (the control: a tile per wave)
def under_the_cap(torch, engine, cap, body):
    if cap:  # the waves of this grid meet every arrangement the layouts are there for
        found = st.arrangements_of(st.LAYOUTS, cap)
        assert found == set(st.ARRANGEMENTS), sorted(set(st.ARRANGEMENTS) - found)
    else:
        resident = 8 * torch.cuda.get_device_properties(0).multi_processor_count
        assert all(len(w) <= 1 for _, tiles in st.LAYOUTS + ((None, 50),) for w in st.assignment(tiles, 0, resident))
    assert latched(engine) == 0
    try:
        engine.set_visibility_grid(cap)
        body()
    finally:
        engine.set_visibility_grid(0)
    assert latched(engine) == 0


@pytest.mark.parametrize("cap", st.CAPS)
def test_the_drawn_reader_on_the_programmes_under_a_cap(torch_mod, engine, progs, mirrors, cap):
    def body():
        for p in progs:
            assert [p.kinds for p in progs] == [tuple(k) for k, _ in st.LAYOUTS]
            for case, claimed in ((p.surface, p.expect["drawn"]), (p.surface8, p.expect["drawn8"])):
                for clear in (False, True):
                    name = f"{case.name} (cap {cap}, clear={clear})"
                    got = tdg.run(torch_mod, engine, case, clear=clear)
                    tdg.assert_equal(name, got, drawn_mirror(mirrors, case, clear))
                    assert got["status"] == (_lib.E_RANGE if p.stale else 0), name
                    for k, v in claimed.items():
                        assert int(got["stats"][k]) == v, (name, k)
    under_the_cap(torch_mod, engine, cap, body)


@pytest.mark.parametrize("cap", st.CAPS)
def test_the_fragments_reader_on_the_programmes_under_a_cap(torch_mod, engine, progs, old_frags, mirrors, cap):
    def body():
        for case, claimed, stale in [(p.frag, p.expect["frag"], p.frag_stale) for p in progs] + [(c, {}, False) for c in old_frags]:
            for clear in (False, True):
                name = f"{case.name} (cap {cap}, clear={clear})"
                want = frag_mirror(mirrors, case, clear)
                got = tfg.run(torch_mod, engine, case, clear=clear)
                tfg.assert_equal(name, got, want)
                assert got["status"] == (_lib.E_RANGE if stale else 0), name
                for k, v in claimed.items():
                    assert int(got["stats"][k]) == v, (name, k)
                got = tfg.run(torch_mod, engine, case, clear=clear, want=NO_GRAD, with_grad=False)
                tfg.assert_equal(name + ", without grad", got, want)
    assert len(old_frags) == 4
    under_the_cap(torch_mod, engine, cap, body)


# -- 2. the chain on the device under a cap of one workgroup: nothing copied to the host in between
def test_the_chain_on_the_device_under_a_cap_of_one(torch_mod, engine, tamper_free):
    """The tamper-free programme's whole list drawn at once with flags 40 (what the cut triangles spill wins where it lands:
    the buffer is not the programme's, the mirror's chain draws the same one)."""
    src = tamper_free.surface
    (_, words, mc, data, vb, vcount, ent, vp), kw = src.args()
    h, w = src.visibility.shape
    pk = tamper_free.packed
    vis = raster.host_raster_visibility(words, mc, data, vb, vcount, ent, vp, w, h, command_base=st.BASE, cull_none=True, clip_near=True,
                                        wide_guard=True, vertex_stride=kw["vertex_stride"], position_offset=kw["position_offset"],
                                        entity_count=kw["entity_count"], meshlet_data_words=kw["meshlet_data_words"])[0]
    case = fc.of(dc.read(src.name + " at once", vis, pk, st.BASE, dc.BOTH))
    want = tfg.mirror(case, clear=True)
    surface = case.surface["stats"]
    assert int(surface["cut_pixels"]) > 500 and int(surface["wide_pixels"]) > 16 and int(surface["stale_pixels"]) == 0
    assert (vis == tamper_free.visibility).mean() > 0.75  # most tiles hold what the programme gives them
    assert latched(engine) == 0
    try:
        engine.set_visibility_grid(1)
        got, rows, statuses = tfg.on_device(torch_mod, engine, [(words, mc, st.BASE)], data, vb, case.vertices, vcount, case.entities,
                                            kw["entity_count"], case.meshlets, case.kw["meshlet_count"], vp, w, h, dc.BOTH, cull_none=True)
    finally:
        engine.set_visibility_grid(0)
    assert statuses == (0, 0, 0)
    tfg.assert_equal("the chain under a cap of 1", dict(got, stats=rows[0], status=0), want)
    assert int(rows[0]["written_pixels"]) == int(surface["written_pixels"]) == int((vis != 0).sum()) > 1500
    assert int(rows[0]["unshaded_pixels"]) == int(rows[0]["stale_pixels"]) == 0


# -- 3. the natural grid: no cap, a target on which the resident grid itself takes several trips
def test_the_resident_grid_takes_several_trips(torch_mod, engine):
    """surface_tile_cases.natural_programme()'s meshes four times on a 1921 x 1081 target — the first trip and the partial
    column, a middle trip, the partial row, the last tile of the last trip —, drawn by orbit_raster_visibility on the
    device with flags 40; both readers run on that buffer on the resident grid, and the references are the mirrors on the
    buffer read back."""
    torch = torch_mod
    prog = st.natural_programme()
    w, h, waves = tc.natural_target(torch.cuda.get_device_properties(0).multi_processor_count)
    pk, where = st.instanced(prog, w, h, waves)
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    last_trip = (tiles - 1) // waves
    trips = {name: (first, last) for name, _, _, first, last in where}
    assert last_trip >= 2 and trips["top_right"] == (0, 0) and trips["bottom_right"][1] == last_trip
    assert 0 < trips["middle"][0] <= trips["middle"][1] < last_trip
    opts, (words, mc, data, vb, vcount, ent, vp, _, _) = pk.args()
    frag_in = fc.of(dc.read("natural", np.zeros((8, 8), np.uint64), pk, st.BASE, dc.BOTH))  # (the rows, records and entities only)
    assert latched(engine) == 0
    engine.set_visibility_grid(0)
    z = lambda n, dt=torch.int32: torch.full((max(int(n), 1),), 5, dtype=dt, device="cuda")  # noqa: E731
    d_words, d_data, d_vb, d_ent = dev(torch, words), dev(torch, data), dev(torch, vb), dev(torch, frag_in.entities)
    d_rows, d_mlt = dev(torch, frag_in.vertices), dev(torch, frag_in.meshlets)
    vis = z(w * h, torch.int64)
    engine.raster_visibility(d_words, mc, d_data, d_vb, vcount, d_ent, opts["entity_count"], vp, vis, w, h, command_base=st.BASE,
                             clear=True, cull_none=True, clip_near=True, wide_guard=True, meshlet_data_words=len(data))
    surf = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))
    sstats, fstats = z(8), z(8)
    engine.visibility_surface_drawn(vis, w, h, d_words, mc, d_data, d_vb, vcount, d_ent, opts["entity_count"], vp, **surf, stats=sstats,
                                    command_base=st.BASE, clear=True, meshlet_data_words=len(data), clip_near=True, wide_guard=True)
    outs = {k: z(tfg.WORDS[k] * w * h, getattr(torch, tfg.TORCH_KIND.get(k, "float32"))) for k in tfg.KEYS}
    engine.surface_fragments(vis, w, h, d_words, mc, d_mlt, frag_in.kw["meshlet_count"], surf["bary"], surf["triangle"], d_rows, vcount,
                             d_ent, opts["entity_count"], grad=surf["grad"], **outs, stats=fstats, command_base=st.BASE, clear=True)
    torch.cuda.synchronize()
    assert latched(engine) == 0
    h_vis = host(vis, np.uint64).reshape(h, w)
    t0 = time.perf_counter()
    want = raster.host_visibility_surface_drawn(h_vis, words, mc, data, vb, vcount, ent, vp, command_base=st.BASE, clear=True,
                                                entity_count=opts["entity_count"], raster_flags=dc.BOTH)
    got = {k: host(surf[k], tdg.DTYPE[k]).reshape(h, w, -1) for k in tdg.KEYS}
    tdg.assert_equal("natural grid, drawn", dict(got, stats=host(sstats, np.uint32).view(L.SURFACE_DRAWN_STATS)[0], status=0), want)
    s = want["stats"]
    assert int(s["written_pixels"]) == int(s["covered_pixels"]) > 4 * 1500 and int(s["cut_pixels"]) > 4 * 500 and int(s["wide_pixels"]) > 4 * 64
    assert int(s["stale_pixels"]) == int(s["foreign_pixels"]) == int(s["unsupported_pixels"]) == 0
    case = fc.tamper(frag_in, "natural", 0, visibility=h_vis, surface={k: want[k] for k in tdg.KEYS})
    want = tfg.mirror(case, clear=True)
    got = {k: host(outs[k], tfg.DTYPE[k]).reshape(h, w, -1) for k in tfg.KEYS}
    tfg.assert_equal("natural grid, fragments", dict(got, stats=host(fstats, np.uint32).view(L.SURFACE_FRAGMENT_STATS)[0], status=0), want)
    assert int(want["stats"]["written_pixels"]) == int(s["written_pixels"]) and int(want["stats"]["stale_pixels"]) == 0
    print(f"natural grid {w} x {h}: the two mirrors and the comparisons took {time.perf_counter() - t0:.2f} s")
    # every instance holds the keys of most of its 64-key tiles (K, KS, K1, KA: six of them): none was drawn over
    assert sum(prog.kinds.count(k) for k in ("K", "KS", "K1", "KA")) == 6
    for name, dx, dy, _, _ in where:
        keys = np.unique(h_vis[dy:dy + prog.height, dx:dx + prog.width] & np.uint64(0xFFFFFFFF))
        assert len(keys) > 4 * 64, (name, len(keys))


# -- 4. a capped first call of a fresh context, captured into a graph: the launches carry their grid
def padded(a, nbytes):
    out = np.zeros(nbytes, np.uint8)
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    out[:len(a)] = a
    return out


def load(torch, t, a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t[:len(a)].copy_(torch.from_numpy(a.copy()).cuda())


def test_a_capped_first_drawn_call_captures_into_a_graph(torch_mod, progs, tamper_free):
    torch = torch_mod
    from orbit_amd.engine import Engine

    picked = [progs[0].surface, tamper_free.surface]  # two programmes of 73 x 33, two lists; the first holds Sm tiles
    h, w = picked[0].visibility.shape
    assert picked[1].visibility.shape == (h, w)
    size = lambda f: max(len(np.ascontiguousarray(f(c)).view(np.uint8).reshape(-1)) for c in picked)  # noqa: E731
    n_data, n_vb = size(lambda c: c.packed.meshlet_data), size(lambda c: c.packed.vertices)
    mc = max(c.packed.max_commands for c in picked)
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        z = lambda nbytes: torch.full((nbytes,), 5, dtype=torch.uint8, device="cuda")  # noqa: E731
        g_vis, g_words, g_data, g_vb, g_ent = z(8 * w * h), z(4 + 28 * mc), z(n_data), z(n_vb), z(256)
        outs = dict(bary=z(8 * w * h), grad=z(16 * w * h), triangle=z(16 * w * h))
        stats = z(32)
        vp = picked[0].packed.case.view_proj
        eng.set_visibility_grid(1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.visibility_surface_drawn(g_vis, w, h, g_words, mc, g_data, g_vb, n_vb // 12, g_ent, 2, vp, **outs, stats=stats, clear=True,
                                         command_base=st.BASE, meshlet_data_words=n_data // 4, clip_near=True, wide_guard=True)
        eng.set_visibility_grid(0)  # (the captured launches carry their grid)
        for c in picked + picked[:1]:  # replayed: new buffers, new lists, the first ones again
            pk = c.packed
            assert pk.entity_count == 2 and (np.asarray(pk.case.view_proj) == vp).all()
            words, data, vb = padded(pk.words, len(g_words)), padded(pk.meshlet_data, n_data), padded(pk.vertices, n_vb)
            for t, a in ((g_vis, c.visibility), (g_words, words), (g_data, data), (g_vb, vb), (g_ent, pk.entities)):
                load(torch, t, a)
            want = raster.host_visibility_surface_drawn(c.visibility, words, mc, data.view(np.uint32), vb, n_vb // 12, pk.entities, vp,
                                                        command_base=st.BASE, entity_count=2, raster_flags=dc.BOTH)
            assert want["status"] == (_lib.E_RANGE if c.stale else 0) and int(want["stats"]["cut_pixels"]) > 500, c.name
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == want["status"], c.name
                for k in tdg.KEYS:
                    assert host(outs[k]).tobytes() == want[k].tobytes(), (c.name, k, replay)
                assert host(stats).tobytes() == want["stats"].tobytes(), c.name
    finally:
        eng.set_visibility_grid(0)
        eng.close()


def test_a_capped_first_fragments_call_captures_into_a_graph(torch_mod, progs, tamper_free):
    torch = torch_mod
    from orbit_amd.engine import Engine

    picked = [progs[0].frag, tamper_free.frag]  # the first holds T and TU tiles
    h, w = picked[0].visibility.shape
    assert picked[1].visibility.shape == (h, w)
    size = lambda f: max(len(np.ascontiguousarray(f(c)).view(np.uint8).reshape(-1)) for c in picked)  # noqa: E731
    n_mlt, n_vb, n_ent = size(lambda c: c.meshlets), size(lambda c: c.vertices), size(lambda c: c.entities)
    mc = max(c.max_commands for c in picked)
    vcount, mcount = (n_vb + 31) // 32, (n_mlt + 31) // 32
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        z = lambda nbytes: torch.full(((nbytes + 15) // 16 * 16,), 5, dtype=torch.uint8, device="cuda")  # noqa: E731
        g_vis, g_words, g_mlt, g_vb, g_ent = z(8 * w * h), z(4 + 28 * mc), z(32 * mcount), z(32 * vcount), z(n_ent)
        g_surf = dict(bary=z(8 * w * h), grad=z(16 * w * h), triangle=z(16 * w * h))
        outs = {k: z(4 * tfg.WORDS[k] * w * h) for k in tfg.KEYS}
        stats = z(32)
        eng.set_visibility_grid(1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.surface_fragments(g_vis, w, h, g_words, mc, g_mlt, mcount, g_surf["bary"], g_surf["triangle"], g_vb, vcount, g_ent, n_ent // 128,
                                  grad=g_surf["grad"], **outs, stats=stats, command_base=st.BASE, clear=True)
        eng.set_visibility_grid(0)  # (the captured launches carry their grid)
        for c in picked + picked[:1]:  # replayed: new buffers, new lists, new records, the first ones again
            assert c.kw["command_base"] == st.BASE and c.kw["entity_count"] == n_ent // 128 == 2
            words, meshlets = padded(c.words, len(g_words)), padded(c.meshlets, len(g_mlt))
            rows, ent = padded(c.vertices, len(g_vb)), padded(c.entities, len(g_ent))
            for t, a in ((g_vis, c.visibility), (g_words, words), (g_mlt, meshlets), (g_vb, rows), (g_ent, ent), (g_surf["bary"], c.surface["bary"]),
                         (g_surf["grad"], c.surface["grad"]), (g_surf["triangle"], c.surface["triangle"])):
                load(torch, t, a)
            want = raster.host_surface_fragments(c.visibility, words, mc, meshlets, c.surface, rows, vcount, ent, command_base=st.BASE,
                                                 entity_count=2, meshlet_count=mcount)
            assert (want["status"] == _lib.E_RANGE) == (c.stale > 0) and int(want["stats"]["written_pixels"]) > 1500, c.name
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == want["status"], c.name
                for k in tfg.KEYS:
                    assert host(outs[k])[:want[k].nbytes].tobytes() == want[k].tobytes(), (c.name, k, replay)
                assert host(stats)[:32].tobytes() == want["stats"].tobytes(), c.name
    finally:
        eng.set_visibility_grid(0)
        eng.close()


# -- 5. a cap and NULL outputs together: the walk does not depend on which outputs exist
def test_a_cap_of_one_with_null_outputs(torch_mod, engine, progs, mirrors):
    main = progs[0]
    assert latched(engine) == 0
    try:
        engine.set_visibility_grid(1)
        for clear in (False, True):
            for case in (main.surface, main.surface8):
                got = tdg.run(torch_mod, engine, case, clear=clear, want=("triangle",))
                tdg.assert_equal(f"{case.name} triangle alone (cap 1, clear={clear})", got, drawn_mirror(mirrors, case, clear))
                assert got["status"] == _lib.E_RANGE and got["bary"] is None
            want = frag_mirror(mirrors, main.frag, clear)
            got = tfg.run(torch_mod, engine, main.frag, clear=clear, want=("material",), with_grad=False)
            tfg.assert_equal(f"{main.name} material alone (cap 1, clear={clear})", got, want)
            assert got["status"] == _lib.E_RANGE and int(got["stats"]["written_pixels"]) == main.expect["frag"]["written_pixels"]
            got = tfg.run(torch_mod, engine, main.frag, clear=clear, with_stats=False)
            tfg.assert_equal(f"{main.name} without stats (cap 1, clear={clear})", got, want)
            assert got["status"] == _lib.E_RANGE and got["stats"] is None
    finally:
        engine.set_visibility_grid(0)
