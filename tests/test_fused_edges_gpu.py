"""The one-launch cull (orbit_amd/csrc/cull_fused.hip, behind orbit_cull_views) at its shape, bisection, tile and look-back
edges, on the device (tests/fused_edges.py; what each case reaches is counted by tests/test_fused_edges_cpu.py): every
case through engines of cull_path = 2, passes 0 / 1 / 2, bit for bit against oracle.entity_cull + oracle.meshlet_cull with
no tolerance anywhere — dispatch header and records, draw header and commands, both bitsets whole.

Every output buffer is pre-filled with a byte pattern: everything behind the counted entries and behind each capacity
must still hold it afterwards (the draw buffer's red zone is a whole trip of 64 commands).  fused_culls() moves by the
number of views, status() is clean or ORBIT_E_CAPACITY exactly when a total exceeds its capacity.  The local and the
tile cases run on a grid capped at 1 and at 2 workgroups (orbit_ctx_set_fused_grid: one wave then runs many tiles in a row
on the same slab, payload and cmd; the last workgroup out is the only one) and on the sized grid."""
import numpy as np
import pytest

import fused_edges as fe
import meshlet_edges as me
from orbit_amd import layouts as L
from test_gpu_parity import dev, host, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

CAPS = dict(max_entities=6000, max_dispatches=4000, max_draws=100_000, max_views=4)
PATTERN = 0xA7
DISPATCH_RED = 512
DRAW_RED = 64 * 28
GRIDS = (1, 2, 0)
PLANTED = {0: (None, None, None), 1: ("ones", "ones", None), 2: ("zero", "zero", "zero")}  # (entity words, meshlet words, pyramid)
SEEDED = {0: (None, None, None), 1: ("random", "random", None), 2: ("random", "random", "zero")}
SEEDED_DEPTH = {2: ("random", "random", "depth")}
REPEATED = (65, 129, 130)  # tile counts whose default-grid run is made three times: which flags a look-back sees is timing


# ------------------------------------------------------------------------------------------------------------ engines
@pytest.fixture(scope="module")
def engines(torch_mod):
    """kind -> an engine of cull_path = 2 ("chain": cull_path = 1; "contracted": arith_profile = 1), made when first asked for."""
    from orbit_amd.engine import Engine

    kw = dict(fused=dict(cull_path=2), chain=dict(cull_path=1), contracted=dict(cull_path=2, arith_profile=1))
    made = {}

    def get(kind="fused"):
        if kind not in made:
            made[kind] = Engine(0, **dict(CAPS, **kw[kind]))
        return made[kind]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture
def grid(engines):
    """set_fused_grid of the fused engine; the sized grid is restored whatever the test does."""
    eng = engines()
    try:
        yield eng.set_fused_grid
    finally:
        eng.set_fused_grid(0)


# ---------------------------------------------------------------------------------------------------- cases on the device
class GpuScene:
    """A scene's inputs on the device: read-only afterwards."""

    def __init__(self, torch, s):
        self.torch, self.s, self._draws = torch, s, {}
        self.mesh_infos = dev(torch, s.mesh_infos)

    def draws(self, header=None):
        if header not in self._draws:
            self._draws[header] = dev(self.torch, self.s.draw_buffer(header))
        return self._draws[header]


_state = {}


def gpu_scene(torch, name):
    if name not in _state:
        _state[name] = GpuScene(torch, fe.scene(name))
    return _state[name]


def shared(torch, oracle):
    if "shared" not in _state:
        _state["shared"] = dict(meshlets=dev(torch, me.meshlet_buffer("scattered")), entities=dev(torch, me.entities()),
                                materials=dev(torch, me.materials()), zero=dev(torch, me.pyramid(oracle, "zero")),
                                depth=dev(torch, me.pyramid(oracle, "depth")))
    return _state["shared"]


_refs = {}


def reference(oracle, s, op, how, header=None, cap_d=None, cap_c=None, profile=0):
    """(dispatch bytes, draw bytes, entity words, meshlet words, records dropped, commands dropped, the input words) of the
    oracle's two stages: computed once per argument set, shared, left unchanged."""
    ewords, mwords, pyr_kind = how[op]
    ex = s.expect(header)
    cap_d = ex.total + 8 if cap_d is None else cap_d
    cap_c = ex.survivors() + 8 if cap_c is None else cap_c
    key = (s.name, op, ewords, mwords, pyr_kind, header, cap_d, cap_c, profile)
    if key not in _refs:
        ci = fe.cull_info(op)
        evis = s.entity_words(ewords, seed=op) if op else None
        mvis = s.meshlet_vis_words(mwords, seed=op) if op else None
        pyr, psize = (me.pyramid(oracle, pyr_kind), fe.PYRAMID) if op == 2 else (None, (0, 0))
        ents = me.entities()
        with oracle.arith_profile(profile):
            od, oev, d1 = oracle.entity_cull(ci, s.draw_buffer(header), s.n, s.mesh_infos, ents, cap_d, evis, pyr, psize)
            oc, omv, d2 = oracle.meshlet_cull(ci, od, me.meshlet_buffer("scattered"), cap_c, ents, me.materials(), mvis, pyr, psize)
        _refs[key] = (od, oc, oev, omv, d1, d2, evis, mvis, cap_d, cap_c)
    return _refs[key]


def make_view(torch, oracle, gs, op, how, ref, header=None):
    """One view's arguments with patterned output buffers -> (the view, its outputs)."""
    sh = shared(torch, oracle)
    evis, mvis, cap_d, cap_c = ref[6:10]
    disp = torch.full((L.DISPATCH_HEADER + 16 * cap_d + DISPATCH_RED,), PATTERN, dtype=torch.uint8, device="cuda")
    draw = torch.full((L.DRAW_HEADER + 28 * cap_c + DRAW_RED,), PATTERN, dtype=torch.uint8, device="cuda")
    e_d, m_d = (dev(torch, evis), dev(torch, mvis)) if op else (None, None)
    pyr = dict(depth_pyramid=sh[how[op][2]], depth_pyramid_size=fe.PYRAMID) if op == 2 else {}
    view = dict(cull_info=fe.cull_info(op), entity_draw_buffer=gs.draws(header), mesh_info_buffer=gs.mesh_infos,
                meshlet_dispatch_buffer=disp, entity_buffer=sh["entities"], entity_draw_count=gs.s.n, dispatch_capacity=cap_d,
                meshlet_buffer=sh["meshlets"], draw_commands_buffer=draw, material_buffer=sh["materials"],
                draw_capacity=cap_c, visibility_buffer=e_d, meshlet_visibility_buffer=m_d, **pyr)
    return view, (disp, draw, e_d, m_d)


def check(out, ref, what):
    """Headers, records and commands == the oracle's; the pattern behind the counted entries and behind each capacity; both
    bitsets whole."""
    disp, draw, e_d, m_d = out
    od, oc, oev, omv = ref[:4]
    h, g = host(disp), host(draw)
    nrec, ncmd = int(od[:4].view(np.uint32)[0]), int(oc[:4].view(np.uint32)[0])
    assert list(h[:12].view(np.uint32)) == list(od[:12].view(np.uint32)), (what, "dispatch header")
    assert np.array_equal(h[12:12 + 16 * nrec], od[12:12 + 16 * nrec]), (what, "dispatch records differ")
    assert bool((h[12 + 16 * nrec:] == PATTERN).all()), (what, "a write behind the counted records or the dispatch capacity")
    assert int(g[:4].view(np.uint32)[0]) == ncmd, (what, "draw header", int(g[:4].view(np.uint32)[0]), ncmd)
    assert np.array_equal(g[4:4 + 28 * ncmd], oc[4:4 + 28 * ncmd]), (what, "draw commands differ")
    assert bool((g[4 + 28 * ncmd:] == PATTERN).all()), (what, "a write behind the counted commands or the draw capacity")
    if oev is not None:
        assert np.array_equal(host(e_d, np.uint32), oev), (what, "entity bitset differs")
        assert np.array_equal(host(m_d, np.uint32), omv), (what, "meshlet bitset differs")
    return nrec, ncmd


def status_is(eng, overflow, what):
    from orbit_amd._lib import E_CAPACITY, OrbitError

    if overflow:
        with pytest.raises(OrbitError) as ei:
            eng.status()
        assert ei.value.code == E_CAPACITY, what
    else:
        eng.status()


def run(torch, oracle, eng, name, op, how=PLANTED, header=None, cap_d=None, cap_c=None, profile=0, fused=True):
    """One orbit_cull_views call of one view, checked.  -> (records, commands) counted."""
    gs = gpu_scene(torch, name)
    ref = reference(oracle, gs.s, op, how, header, cap_d, cap_c, profile)
    view, out = make_view(torch, oracle, gs, op, how, ref, header)
    before = eng.fused_culls()
    eng.cull_views([view])
    torch.cuda.synchronize()
    what = (name, "pass", op, "header", header, "capacities", ref[8], ref[9])
    status_is(eng, ref[4] > 0 or ref[5] > 0, what)
    assert eng.fused_culls() - before == (1 if fused else 0), what
    return check(out, ref, what)


# ------------------------------------------------------------------------------------------------------------ the hook
def test_the_grid_hook(torch_mod, engines, oracle, grid):
    """orbit_ctx_set_fused_grid rejects a NULL context, takes any cap, and is read when the launch is enqueued: a view
    array prepared under the sized grid runs capped, with the same outputs."""
    from orbit_amd import _lib

    torch, eng = torch_mod, engines()
    assert eng._lib.orbit_ctx_set_fused_grid(None, 1) == _lib.E_INVALID
    gs = gpu_scene(torch, "t4_130_steps_full")
    ref = reference(oracle, gs.s, 0, PLANTED)
    view, out = make_view(torch, oracle, gs, 0, PLANTED, ref)
    arr, keep = eng.prepare_views([view])
    for cap in (1, 7, 0):
        grid(cap)
        out[0].fill_(PATTERN), out[1].fill_(PATTERN)
        eng.cull_views_prepared(arr)
        torch.cuda.synchronize()
        eng.status()
        assert check(out, ref, ("prepared", cap)) == (520, gs.s.expect().survivors())
    del keep


# ---------------------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("name", fe.SHAPE_CASES)
def test_every_shape_at_its_sizes(torch_mod, engines, oracle, grid, name):
    """1, 255 .. 257, 767 .. 769 and 4095 .. 4097 draws (at 769 and 4097 the last chunk holds one draw), passes 0 / 1 / 2
    with seeded bitsets, the draw buffer's header saying N, N - 40 and N + 40; at N also on one workgroup, and pass 2
    against the seeded pyramid."""
    torch, eng = torch_mod, engines()
    s = fe.scene(name)
    total = 0
    for header in s.header_counts():
        for op in (0, 1, 2):
            total += run(torch, oracle, eng, name, op, SEEDED, header)[0]
    assert total > 0
    run(torch, oracle, eng, name, 2, SEEDED_DEPTH)
    grid(1)
    for op in (0, 1, 2):
        run(torch, oracle, eng, name, op, SEEDED)


# ------------------------------------------------------------------------------------------------ 2. the local bisection
@pytest.mark.parametrize("name", fe.LOCAL_CASES)
def test_the_local_entity_stage(torch_mod, engines, oracle, grid, name):
    """768 draws in passes 0 and 1 (and, through the chunked 2-row shape, pass 2): the first draw only, the last only, every
    draw a record; runs of 1, 31, 255, 256 and 300 draws without a record at the start, across each chunk boundary and
    at the end, a middle chunk without any; one draw of 41 records at draw 0, 255, 256 and 767; totals of 4 t - 1, 4 t and
    4 t + 1 records — on 1, on 2 and on the sized number of workgroups."""
    torch, eng = torch_mod, engines()
    ex = fe.scene(name).expect()
    for cap in GRIDS:
        grid(cap)
        for op in (0, 1, 2):
            assert run(torch, oracle, eng, name, op) == (ex.total, ex.survivors()), (name, cap, op)


# ----------------------------------------------------------------------------------------------- 3. tiles and look-back
@pytest.mark.parametrize("tag,ntiles", [(tag, T) for tag in ("t4", "t4c", "t16") for T in fe.TILE_COUNTS if fe.tile_cases(tag, T)])
def test_tiles_and_look_back(torch_mod, engines, oracle, grid, tag, ntiles):
    """Tiles of 4 records (the local stage; "t4c": the chunked entity stage) and of 16, 1 .. 130 of them, the last one full,
    of one record and of all but one, every density — on 1, on 2 and on the sized number of workgroups; the sized run of
    65, 129 and 130 tiles three times on the same context."""
    torch, eng = torch_mod, engines()
    for name in fe.tile_cases(tag, ntiles):
        ex = fe.scene(name).expect()
        for cap in GRIDS:
            grid(cap)
            for _ in range(3 if cap == 0 and ntiles in REPEATED else 1):
                for op in (0, 1, 2):
                    assert run(torch, oracle, eng, name, op) == (ex.total, ex.survivors()), (name, cap, op)


# ------------------------------------------------------------------------------------------------------- 4. capacities
@pytest.mark.parametrize("name", fe.CUT_CASES)
def test_capacities_cut_to_the_canonical_prefix(torch_mod, engines, oracle, grid, name):
    """draw_capacity total - 1, total, 1, 0, on a tile boundary, on a trip boundary inside a tile and one to either side;
    dispatch_capacity total - 1, total, 1, 4 t, 4 t +- 1 (passes 0 / 1: the local stage where the case is local; pass 2:
    the chunked one); both short at once.  The canonical prefix, the headers min(total, capacity), ORBIT_E_CAPACITY
    exactly when a total exceeds its capacity, nothing behind a capacity — and a full-capacity call on the same context
    after every cut finds nothing stale and no latch."""
    torch, eng = torch_mod, engines()
    s = fe.scene(name)
    ex = s.expect()
    recs = fe.tile_records_of(name) if name in fe.TILE_CASES else 4
    for cap in (0, 1):
        grid(cap)
        for op in (0, 1, 2):
            for what, cap_d, cap_c in fe.capacities(ex, recs):
                nrec = min(ex.total, cap_d)
                got = run(torch, oracle, eng, name, op, cap_d=cap_d, cap_c=cap_c)
                assert got == (nrec, min(ex.survivors(nrec), cap_c)), (name, what, op)
                assert run(torch, oracle, eng, name, op) == (ex.total, ex.survivors()), (name, "after", what, op)


# ------------------------------------------------------------------------------------------------------ 5. mixed calls
def _views_call(torch, oracle, eng, names, passes, how):
    views, outs, refs = [], [], []
    for k, (name, op) in enumerate(zip(names, passes)):
        gs = gpu_scene(torch, name)
        ref = reference(oracle, gs.s, op, how)
        view, out = make_view(torch, oracle, gs, op, how, ref)
        views.append(view), outs.append(out), refs.append(ref)
    before = eng.fused_culls()
    eng.cull_views(views)
    torch.cuda.synchronize()
    eng.status()
    assert eng.fused_culls() - before == len(names)
    return [check(out, ref, (names, passes, "view", k)) for k, (out, ref) in enumerate(zip(outs, refs))]


@pytest.mark.parametrize("passes", fe.MIXED_PASSES, ids=["pass0", "passes_0_1_2_0"])
def test_views_of_three_shapes_in_one_call(torch_mod, engines, oracle, grid, passes):
    """One orbit_cull_views of [4097, 300, 1000, 768] draws: three launches, views regrouped through ViewGroup::idx with
    idx[slot] != slot (view 3 is slot 1 of the local launch, view 2 slot 0 of the 2-row one, view 0 slot 0 of the 8-row one);
    then with view 1 on pass 1 and view 2 on pass 2.  On the sized grids and on two workgroups a view."""
    torch, eng = torch_mod, engines()
    got = [(s, idx) for s, idx, _ in fe.launches([fe.scene(n).n for n in fe.MIXED_VIEWS], passes, 256)]
    assert got == [(0, [1, 3]), (1, [2]), (2, [0])]
    for cap in (0, 2):
        grid(cap)
        counts = _views_call(torch, oracle, eng, fe.MIXED_VIEWS, passes, SEEDED)
        assert all(r > 0 and c > 0 for r, c in counts)


def test_two_local_views_of_1_and_768_draws(torch_mod, engines, oracle, grid):
    """One group, the grid sized by the larger view: the workgroups of the view of one draw find no tile."""
    torch, eng = torch_mod, engines()
    for cap in GRIDS:
        grid(cap)
        for op in (0, 1):
            _views_call(torch, oracle, eng, fe.LOCAL_PAIR, (op, op), SEEDED)


# ---------------------------------------------------------------------------------------------------- 6. back to back
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_back_to_back_on_one_context(torch_mod, engines, oracle, order):
    """One engine, one stream, no synchronize until the end: 130 tiles of 16, 1 draw, 129 local tiles of 4, 769 draws, 64
    tiles, 4097 draws (and the other way round), passes 0 and 2 in turn, then the other pass each: every launch finds
    ent_flags, tile_flags and the sync words as the last workgroup out of another shape, or of a launch of many more or
    fewer tiles, left them."""
    torch, eng = torch_mod, engines()
    names = fe.BACK_TO_BACK if order == "ascending" else fe.BACK_TO_BACK[::-1]
    jobs = []
    for k, name in enumerate(names * 2):
        op = 2 * (k % 2) if k < len(names) else 2 - 2 * (k % 2)
        how = PLANTED if name in fe.TILE_CASES else SEEDED
        gs = gpu_scene(torch, name)
        ref = reference(oracle, gs.s, op, how)
        jobs.append((name, op, ref) + make_view(torch, oracle, gs, op, how, ref))
    assert {(n, op) for n, op, *_ in jobs} == {(n, op) for n in names for op in (0, 2)}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    before = eng.fused_culls()
    with torch.cuda.stream(stream):
        for name, op, ref, view, out in jobs:
            eng.cull_views([view], stream=stream)
    eng.status(stream=stream)
    assert eng.fused_culls() - before == len(jobs)
    for k, (name, op, ref, view, out) in enumerate(jobs):
        check(out, ref, (k, name, op))


# ------------------------------------------------------------------------------------------- 7. the chain, word for word
@pytest.mark.parametrize("name", ["t4_65_steps_full", "t4_65_full_full", "t16_65_steps_full", "t16_65_full_full",
                                  "t4_130_steps_all_but_one", "t16_130_full_one"])
def test_the_launch_chain_writes_the_same_words(torch_mod, engines, oracle, name):
    """cull_path = 1 (entity launches, evaluation, scan, emit) against the one launch on the steps and the full density:
    every counted word of both buffers and both bitsets."""
    torch = torch_mod
    gs = gpu_scene(torch, name)
    for op in (0, 1, 2):
        ref = reference(oracle, gs.s, op, PLANTED)
        outs = {}
        for kind in ("chain", "fused"):
            eng = engines(kind)
            view, outs[kind] = make_view(torch, oracle, gs, op, PLANTED, ref)
            before = eng.fused_culls()
            eng.cull_views([view])
            torch.cuda.synchronize()
            eng.status()
            assert eng.fused_culls() - before == (1 if kind == "fused" else 0)
        nrec, ncmd = check(outs["fused"], ref, (name, op))
        a, b = outs["chain"], outs["fused"]
        assert torch.equal(a[0][:12 + 16 * nrec], b[0][:12 + 16 * nrec]) and torch.equal(a[1][:4 + 28 * ncmd], b[1][:4 + 28 * ncmd])
        if op:
            assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


# ------------------------------------------------------------------------------------------------- 8. the contracted twin
@pytest.mark.parametrize("name", fe.SHAPE_CASES)
def test_the_contracted_twin_at_every_shape(torch_mod, engines, oracle, name):
    """arith_profile = 1 takes the same three shapes (and the same grid cap) through cull_fused_contracted.hip: against the
    oracle under arith_profile(1)."""
    torch, eng = torch_mod, engines("contracted")
    try:
        for cap in (0, 1):
            eng.set_fused_grid(cap)
            for op in (0, 1, 2):
                run(torch, oracle, eng, name, op, SEEDED, profile=1)
    finally:
        eng.set_fused_grid(0)
