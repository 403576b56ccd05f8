"""orbit_cull_stats on the MI355X: the product's counters against the numpy classifier (tests/cull_stats_ref.py) on the
scene set and on the reference binaries' knife-edge vectors; the counters against the real cull that follows on the same
stream (records, commands, capacities cut below the totals); no byte of any other buffer written; the argument checks;
graph capture on the first call; both arithmetic profiles; and the 50 M-meshlet scene once."""
import numpy as np
import pytest

import cull_stats_ref as ref
from orbit_amd import layouts as L
from test_gpu_parity import GpuScene, dev, host, torch_mod  # noqa: F401
from test_spirv_vectors_cpu import CASES as KNIFE_CASES, load_case, load_contracted_case, vectors  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(torch_mod):
    from orbit_amd.engine import Engine

    e = Engine(0, max_entities=4096, max_dispatches=100_000, max_draws=200_000)
    yield e
    e.close()


class Bufs:
    """Device inputs of one case (tests/cull_stats_ref.py make_case), outputs sized for the uncapped cull."""

    def __init__(self, torch, c, disp_cap=None, draw_cap=None):
        s = c["scene"]
        self.c, self.gs = c, GpuScene(torch, s)
        self.gs.draws = dev(torch, s.entity_draw_buffer(c["count"]))
        self.disp_cap = s.max_dispatches() + 8 if disp_cap is None else disp_cap
        self.draw_cap = s.lod0_meshlets + 8 if draw_cap is None else draw_cap  # LOD 0 is every mesh's largest
        self.disp = torch.zeros(L.DISPATCH_HEADER + 16 * self.disp_cap, dtype=torch.uint8, device="cuda")
        self.draw = torch.zeros(L.DRAW_HEADER + 28 * self.draw_cap, dtype=torch.uint8, device="cuda")
        self.evis = None if c["evis"] is None else dev(torch, c["evis"])
        self.mvis = None if c["mvis"] is None else dev(torch, c["mvis"])
        self.pyr = None if c["pyr"] is None else dev(torch, c["pyr"])
        self.stats = torch.full((256,), 0x5A, dtype=torch.uint8, device="cuda")  # overwritten, not added to

    def kw(self, material_count=0):
        return dict(visibility_buffer=self.evis, meshlet_visibility_buffer=self.mvis, depth_pyramid=self.pyr,
                    depth_pyramid_size=self.c["psize"], material_count=material_count)

    def stats_call(self, eng, material_count=0, stream=None, stats=None):
        g, c = self.gs, self.c
        eng.cull_stats(self.stats if stats is None else stats, c["ci"], g.draws, g.mesh_infos, self.disp, g.entities,
                       c["edc"], self.disp_cap, g.meshlets, self.draw, g.materials, self.draw_cap, stream=stream,
                       **self.kw(material_count))

    def cull(self, eng, material_count=0, stream=None):
        g, c, k = self.gs, self.c, self.kw(material_count)
        eng.entity_cull(c["ci"], g.draws, g.mesh_infos, self.disp, g.entities, c["edc"], self.disp_cap,
                        visibility_buffer=k["visibility_buffer"], depth_pyramid=self.pyr,
                        depth_pyramid_size=c["psize"], stream=stream)
        eng.meshlet_cull(c["ci"], self.disp, g.meshlets, self.draw, g.entities, g.materials, self.disp_cap, self.draw_cap,
                         meshlet_visibility_buffer=self.mvis, depth_pyramid=self.pyr, depth_pyramid_size=c["psize"],
                         material_count=material_count, stream=stream)


def got(b):
    from orbit_amd.engine import cull_stats_dict

    return cull_stats_dict(b.stats)


def headers(b):
    return int(host(b.disp)[:4].view(np.uint32)[0]), int(host(b.draw)[:4].view(np.uint32)[0])


@pytest.fixture(scope="module")
def cases(oracle):
    return {name: ref.make_case(name, oracle) for name in ref.CASES}


@pytest.mark.parametrize("material_count", [0, 25], ids=["alpha_gathered", "alpha_table"])
@pytest.mark.parametrize("name", ref.CASES)
def test_counters_equal_the_classifier_then_the_cull_agrees(torch_mod, engine, cases, name, material_count):
    torch = torch_mod
    c = cases[name]
    want = ref.public(ref.classify_case(c))
    b = Bufs(torch, c)
    b.stats_call(engine, material_count)
    b.cull(engine, material_count)  # the cull itself, next on the same stream
    torch.cuda.synchronize()
    engine.status()
    g = got(b)
    assert g == want
    ref.check_invariants(g)
    nrec, ncmd = headers(b)
    assert g["records"] == nrec and g["meshlet_drawn"] == ncmd


def test_totals_stay_uncapped_when_the_capacities_are_cut(torch_mod, cases):
    torch = torch_mod
    from orbit_amd import _lib
    from orbit_amd.engine import Engine

    c = cases["p0_ortho_cascade"]
    want = ref.public(ref.classify_case(c))
    eng = Engine(0, max_entities=4096, max_dispatches=100_000, max_draws=200_000)
    try:
        b = Bufs(torch, c, disp_cap=want["records"] // 2, draw_cap=want["meshlet_drawn"] // 3)
        b.stats_call(eng)
        b.cull(eng)
        torch.cuda.synchronize()
        with pytest.raises(_lib.OrbitError) as e:
            eng.status()
        assert e.value.code == _lib.E_CAPACITY
        g = got(b)
        assert g == want
        nrec, ncmd = headers(b)
        assert nrec == b.disp_cap < g["records"] and ncmd <= b.draw_cap < g["meshlet_drawn"]
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["p1_persp", "p2_persp", "p2_ortho"])
def test_nothing_but_the_counters_is_written(torch_mod, engine, cases, name):
    torch = torch_mod
    b = Bufs(torch, cases[name])
    for i, t in enumerate((b.disp, b.draw)):
        t.copy_(torch.randint(0, 256, t.shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(i)).cuda())
    before = [host(t).copy() for t in (b.disp, b.draw, b.evis, b.mvis)]
    guard = torch.full((512,), 0xC3, dtype=torch.uint8, device="cuda")
    b.stats_call(engine, stats=guard[128:384])
    torch.cuda.synchronize()
    engine.status()  # no latched status either
    for t, h in zip((b.disp, b.draw, b.evis, b.mvis), before):
        assert np.array_equal(host(t), h)
    gh = host(guard)
    assert (gh[:128] == 0xC3).all() and (gh[384:] == 0xC3).all()
    b.stats = guard[128:384]
    assert got(b) == ref.public(ref.classify_case(cases[name]))


def test_argument_checks(torch_mod, engine, cases):
    torch = torch_mod
    from orbit_amd import _lib
    from orbit_amd.engine import Engine

    def code(fn):
        with pytest.raises(_lib.OrbitError) as e:
            fn()
        return e.value.code

    c = cases["p2_persp"]
    b = Bufs(torch, c)
    for ds in (64, 128):
        e2 = Engine(0, max_entities=4096, max_dispatches=100_000, max_draws=200_000, dispatch_size=ds)
        try:
            c0 = dict(cases["p0_persp_lods"])
            b0 = Bufs(torch, c0)
            assert code(lambda: b0.stats_call(e2)) == _lib.E_INVALID
        finally:
            e2.close()
    ci = c["ci"].copy()
    ci["cull_plane_count"] = 13
    bad = Bufs(torch, dict(c, ci=ci))
    assert code(lambda: bad.stats_call(engine)) == _lib.E_PLANES
    ci = c["ci"].copy()
    ci["projection_type"] = 2
    bad = Bufs(torch, dict(c, ci=ci))
    assert code(lambda: bad.stats_call(engine)) == _lib.E_INVALID
    bad = Bufs(torch, c)
    bad.pyr = None
    assert code(lambda: bad.stats_call(engine)) == _lib.E_MISSING
    bad = Bufs(torch, c)
    bad.evis = None
    assert code(lambda: bad.stats_call(engine)) == _lib.E_MISSING
    bad = Bufs(torch, c)
    bad.mvis = None
    assert code(lambda: bad.stats_call(engine)) == _lib.E_MISSING
    raw = torch.zeros(264, dtype=torch.uint8, device="cuda")
    assert code(lambda: b.stats_call(engine, stats=raw[4:260])) == _lib.E_INVALID  # not 8-B aligned
    torch.cuda.synchronize()
    engine.status()


def test_stats_then_cull_capture_into_a_graph_on_the_first_call(torch_mod, cases):
    torch = torch_mod
    from orbit_amd.engine import Engine

    c = cases["p2_persp_noskip"]
    want = ref.public(ref.classify_case(c))
    eng = Engine(0, max_entities=4096, max_dispatches=100_000, max_draws=200_000)  # a context that never ran it
    try:
        b = Bufs(torch, c)
        evis0, mvis0 = b.evis.clone(), b.mvis.clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            b.stats_call(eng)
            b.cull(eng)
        for _ in range(2):
            b.evis.copy_(evis0)  # pass 2 rewrote the words: every replay starts from the same frame
            b.mvis.copy_(mvis0)
            b.stats.fill_(0x77)
            g.replay()
            torch.cuda.synchronize()
            eng.status()
            s = got(b)
            assert s == want
            assert (s["records"], s["meshlet_drawn"]) == headers(b)
    finally:
        eng.close()


def _knife(vectors, name, contracted=False):
    c = load_contracted_case(vectors, name) if contracted else load_case(vectors, name)
    p = int(c["ci"]["occlusion_pass"])
    draws = c["draws"]
    count = int(np.frombuffer(draws[:4].tobytes(), np.uint32)[0])
    scene = ref_scene(draws, c)
    return c, dict(scene=scene, ci=c["ci"], count=count, edc=count, evis=c["evis"] if p else None,
                   mvis=c["mvis"] if p else None, pyr=c["pyr"] if p == 2 else None, psize=c["ps"] if p == 2 else (0, 0))


def ref_scene(draws, c):
    from scenes import Scene

    d = np.frombuffer(draws[L.ENTITY_DRAW_HEADER:].tobytes(), dtype=L.ENTITY_DRAW)
    return Scene(d, c["entities"], c["mesh_infos"], c["meshlets"], c["materials"], len(c["mvis"]), 0)


@pytest.mark.parametrize("name", [n for n in KNIFE_CASES if "knife" in n])
def test_knife_edge_vectors_in_both_profiles(torch_mod, vectors, name):
    """On the reference binaries' knife-edge cases the canonical counters are the classifier's, class for class, and
    each profile's counters are its own cull's: where the profiles draw differently, so do their counts."""
    torch = torch_mod
    from orbit_amd.engine import Engine

    seen = {}
    for profile in (0, 1):
        gold, c = _knife(vectors, name, contracted=profile == 1)
        eng = Engine(0, max_entities=4096, max_dispatches=gold["caps"][0] + 64, max_draws=gold["caps"][1] + 64,
                     arith_profile=profile)
        try:
            b = Bufs(torch, c, disp_cap=gold["caps"][0], draw_cap=gold["caps"][1])
            b.stats_call(eng)
            b.cull(eng)
            torch.cuda.synchronize()
            eng.status()
            s = got(b)
            ref.check_invariants(s)
            assert (s["records"], s["meshlet_drawn"]) == headers(b)
            assert s["meshlet_drawn"] == int(gold["spv_draw"][:4].view(np.uint32)[0])  # that profile's binary run
            if profile == 0:
                assert s == ref.public(ref.classify_case(c))
            seen[profile] = (s, host(b.draw)[:L.DRAW_HEADER + 28 * s["meshlet_drawn"]].tobytes())
        finally:
            eng.close()
    if seen[0][1] != seen[1][1]:  # the profiles decide the knife edge differently: the counts say so
        assert seen[0][0] != seen[1][0]


def test_full_size_scene_once(torch_mod, oracle):
    """BASELINE config 5 at full size (195 313 entities x 256 meshlets): records and meshlet_drawn are the cull's."""
    torch = torch_mod
    from orbit_amd.engine import cull_stats_dict
    from test_gpu_full_size import Frame

    f = Frame(torch, 195_313)
    try:
        ci = f.ci(0)
        stats = torch.zeros(256, dtype=torch.uint8, device="cuda")
        disp = torch.zeros(L.DISPATCH_HEADER + 16 * f.disp_cap, dtype=torch.uint8, device="cuda")
        draw = torch.zeros(L.DRAW_HEADER + 28 * f.draw_cap, dtype=torch.uint8, device="cuda")
        E = f.spec.entities
        f.eng.cull_stats(stats, ci, f.draws, f.mesh, disp, f.ent, E, f.disp_cap, f.meshlets, draw, f.materials, f.draw_cap,
                         material_count=f.spec.materials)
        f.eng.entity_cull(ci, f.draws, f.mesh, disp, f.ent, E, f.disp_cap)
        f.eng.meshlet_cull(ci, disp, f.meshlets, draw, f.ent, f.materials, f.disp_cap, f.draw_cap,
                           material_count=f.spec.materials)
        torch.cuda.synchronize()
        f.eng.status()
        s = cull_stats_dict(stats)
        ref.check_invariants(s)
        nrec, ncmd = int(disp[:4].view(torch.int32).item()), int(draw[:4].view(torch.int32).item())
        assert s["records"] == nrec and s["meshlet_drawn"] == ncmd
        assert s["entities"] == E and s["meshlets"] > 40_000_000 and 0 < ncmd < s["meshlets"]
    finally:
        f.close()
