"""The entity stage at its launch-form, chunk and range edges, on every launch form (tests/entity_edges.py; what each
case exercises is counted by tests/test_entity_edges_cpu.py): the one launch with its in-launch look-back, the two
launches above 128 chunks, the entity phase of the one-launch cull, the shard launch, the contracted twins and the
dispatch sizes 64 / 128 — bit for bit against the oracle, with no tolerance anywhere.

Every output buffer is pre-filled with a byte pattern: everything behind the records the header counts, and behind the
capacity, must still hold it afterwards; the visibility words are compared whole, the words past the count included."""
from types import SimpleNamespace

import numpy as np
import pytest

import entity_edges as ee
from orbit_amd import layouts as L
from test_gpu_parity import _expected_visible_records, assert_same, dev, host, torch_mod  # noqa: F401
from test_shard_gpu import _shard

pytestmark = pytest.mark.gpu

CAPS = dict(max_entities=66_000, max_dispatches=140_000, max_draws=400_000)
PATTERN = 0xA7
RED_ZONE = 512
PLAIN = [f"plain_{n}" for n in ee.SIZES]
PLANTED = [f"{p}_{n}" for p in ee.PLANTS for n in ee.PLANT_SIZES]
BACK_TO_BACK = [ee.ONE_LAUNCH + 1, 1, ee.ONE_LAUNCH, ee.CHUNK + 1, ee.SHARD_MAX + 1, ee.FUSED_MAX, ee.ONE_LAUNCH - (ee.CHUNK - 1),
                ee.CHUNK]  # every launch follows one of another form (or of another size of the same form)


# ------------------------------------------------------------------------------------------------------- engines
class _Engines:
    """The engines of this module, made when first asked for: "plain", "side" (a meshlet stream with a mesh side table
    bound: bind_side), "contracted" (arith_profile = 1), "s64" / "s128" (dispatch sizes, pass 0 only)."""
    KW = dict(plain={}, side={}, contracted=dict(arith_profile=1), s64=dict(dispatch_size=64), s128=dict(dispatch_size=128))

    def __init__(self):
        self.made, self.side_of, self.ms = {}, None, None

    def __getitem__(self, kind):
        from orbit_amd.engine import Engine

        if kind not in self.made:
            self.made[kind] = Engine(0, **dict(CAPS, **self.KW[kind]))
        return self.made[kind]

    def bind_side(self, torch, gc):
        """The side engine's stream and mesh side table are this case's (derived once per case, in turn)."""
        eng = self["side"]
        if self.side_of is not gc:
            self.drop_side()
            self.ms = eng.meshlet_stream(gc.meshlets, 0, gc.meshlets.numel() // 32)
            self.ms.update_meshes(gc.mesh_infos, 0, gc.mesh_infos.numel() // 128)
            eng.bind_meshlet_stream(self.ms)
            torch.cuda.synchronize()
            self.side_of = gc
        return eng

    def drop_side(self):
        if self.ms is not None:
            self.made["side"].bind_meshlet_stream(None)
            self.ms.close()
        self.ms = self.side_of = None

    def close(self):
        self.drop_side()
        for e in self.made.values():
            e.close()


@pytest.fixture(scope="module")
def engines(torch_mod):
    e = _Engines()
    yield e
    e.close()


def profile_of(kind):
    return 1 if kind == "contracted" else 0


def size_of(kind):
    return dict(s64=64, s128=128).get(kind, 32)


# ---------------------------------------------------------------------------------------------------- cases on the device
class GpuCase:
    """A case's inputs on the device: read-only afterwards.  draws(header): the draw buffer claiming `header` draws."""

    def __init__(self, torch, case):
        s = case["scene"]
        self.torch, self.case, self._draws = torch, case, {}
        self.mesh_infos, self.entities = dev(torch, s.mesh_infos), dev(torch, s.entities)
        self.meshlets, self.materials = dev(torch, s.meshlets), dev(torch, s.materials)
        self.pyr = dev(torch, case["pyr"])

    def draws(self, header):
        if header not in self._draws:
            self._draws[header] = dev(self.torch, ee.draw_buffer(self.case, header))
        return self._draws[header]


_state = {}


def gpu_case(torch, oracle, name):
    if name not in _state:
        _state[name] = GpuCase(torch, ee.make_case(name, oracle))
    return _state[name]


def pyramid_kw(gc, occlusion_pass):
    return dict(depth_pyramid=gc.pyr, depth_pyramid_size=ee.PYRAMID) if occlusion_pass == 2 else {}


def out_buffer(torch, capacity):
    return torch.full((L.DISPATCH_HEADER + 16 * capacity + RED_ZONE,), PATTERN, dtype=torch.uint8, device="cuda")


def entity_call(torch, eng, gc, occlusion_pass, header, vis, first=None, count=None, capacity=None, stream=None, out=None):
    """orbit_entity_cull (first is None) or orbit_entity_cull_range into a patterned buffer -> (dispatch buffer, words)."""
    c = gc.case
    cap = c["capacity"] if capacity is None else capacity
    disp, vis_d = out if out is not None else (out_buffer(torch, cap), None if vis is None else dev(torch, vis))
    eng.entity_cull(ee.cull_info(c, occlusion_pass), gc.draws(header), gc.mesh_infos, disp, gc.entities,
                    c["n"] if count is None else count, cap, visibility_buffer=vis_d, draw_first=first, stream=stream,
                    **pyramid_kw(gc, occlusion_pass))
    return disp, vis_d


def oracle_call(oracle, gc, occlusion_pass, header, vis, first=None, count=None, capacity=None, kind="plain"):
    c = gc.case
    s = c["scene"]
    with oracle.arith_profile(profile_of(kind)), oracle.dispatch_size(size_of(kind)):
        return oracle.entity_cull(ee.cull_info(c, occlusion_pass), ee.draw_buffer(c, header),
                                  c["n"] if count is None else count, s.mesh_infos, s.entities,
                                  c["capacity"] if capacity is None else capacity, vis, c["pyr"], c["psize"], draw_first=first)


def check(got, ref, what):
    """Header and records == the oracle's; the pattern behind them and behind the capacity; the words whole."""
    (disp, vis_d), (od, ovis, _) = got, ref
    h = host(disp)
    n = int(od[:4].view(np.uint32)[0])
    assert list(h[:12].view(np.uint32)) == list(od[:12].view(np.uint32)), (what, "header")
    assert np.array_equal(h[12:12 + 16 * n], od[12:12 + 16 * n]), (what, "dispatch records differ")
    assert bool((h[12 + 16 * n:] == PATTERN).all()), (what, "a write behind the counted records or the capacity")
    if ovis is not None:
        assert np.array_equal(host(vis_d, np.uint32), ovis), (what, "visibility words differ")
    return n


WORDS = {0: "zero", 1: "random", 2: "random"}


def whole_calls(torch, engines, oracle, gc, kinds=("plain", "side", "contracted"), sized=("s64", "s128")):
    """orbit_entity_cull: passes 0 / 1 / 2 x every header_counts value x the engines; no latch afterwards."""
    c = gc.case
    total = 0
    for header in ee.header_counts(c["n"]):
        for op in (0, 1, 2):
            vis = ee.words(c, WORDS[op], seed=op) if op else None
            for kind in kinds + (sized if op == 0 else ()):
                eng = engines.bind_side(torch, gc) if kind == "side" else engines[kind]
                before = eng.mesh_side_culls()
                got = entity_call(torch, eng, gc, op, header, vis)
                eng.status()
                assert eng.mesh_side_culls() - before == (1 if kind == "side" else 0)
                total += check(got, oracle_call(oracle, gc, op, header, vis, kind=kind), (c["name"], header, op, kind))
    return total


def range_calls(torch, engines, oracle, gc, kinds=("plain", "side", "contracted")):
    """orbit_entity_cull_range over ranges(N), passes 0 and 2, the draw buffer claiming N + 300 draws."""
    c = gc.case
    header = c["n"] + ee.SLACK
    for b, e in ee.ranges(c["n"]):
        for op in (0, 2):
            vis = ee.words(c, "random", seed=b) if op else None
            for kind in kinds:
                eng = engines.bind_side(torch, gc) if kind == "side" else engines[kind]
                got = entity_call(torch, eng, gc, op, header, vis, first=b, count=e - b)
                eng.status()
                check(got, oracle_call(oracle, gc, op, header, vis, first=b, count=e - b, kind=kind),
                      (c["name"], (b, e), op, kind))


# ------------------------------------------------------------------------------------------- 1. every size, whole buffer
@pytest.mark.parametrize("name", PLAIN)
def test_entity_cull_at_every_size(torch_mod, engines, oracle, name):
    """orbit_entity_cull at 1, 31 .. 33, 255 .. 257 and on both sides of 16 384, 32 768 (and 128 chunks whose last one
    holds one draw) and 65 536 entity-draws, passes 0 / 1 / 2, the draw buffer's header saying N, N - 300 and N + 300 (the
    call then processes up to ceil(N / 256) x 256 draws): records, header and bitset."""
    gc = gpu_case(torch_mod, oracle, name)
    total = whole_calls(torch_mod, engines, oracle, gc)
    assert total > 0 or gc.case["n"] == 1


# --------------------------------------------------------------------------------- 2. one context across the thresholds
def test_one_context_across_the_thresholds_back_to_back(torch_mod, engines, oracle):
    """One engine, one stream, no synchronize until the end: 32 769, 1, 32 768, 257, 65 537, 16 384, 32 513, 256 draws,
    twice, passes 0 and 2 alternating — every launch finds ent_flags and sync as it needs them, whatever form left them."""
    torch = torch_mod
    eng = engines["plain"]
    jobs = []
    for k, n in enumerate(BACK_TO_BACK * 2):
        gc = gpu_case(torch, oracle, f"plain_{n}")
        op = 2 * (k % 2) if k < len(BACK_TO_BACK) else 2 - 2 * (k % 2)  # each size meets both passes
        vis = ee.words(gc.case, "random", seed=k) if op else None
        gc.draws(n)
        jobs.append((gc, op, vis, (out_buffer(torch, gc.case["capacity"]), None if vis is None else dev(torch, vis))))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for gc, op, vis, out in jobs:
            entity_call(torch, eng, gc, op, gc.case["n"], vis, stream=stream, out=out)
    eng.status(stream=stream)
    assert {op for _, op, _, _ in jobs} == {0, 2}
    for k, (gc, op, vis, out) in enumerate(jobs):
        check(out, oracle_call(oracle, gc, op, gc.case["n"], vis), (k, gc.case["name"], op))


# ----------------------------------------------------------------------------------------------------------- 3. ranges
@pytest.mark.parametrize("n", ee.RANGE_SIZES)
def test_entity_cull_range(torch_mod, engines, oracle, n):
    """orbit_entity_cull_range: the whole, a word in from both ends, the tail shorter than a word (pass 2 stores a whole
    ballot word whose bits past the end are zero), a start that is no chunk boundary with a length across the one-launch
    threshold, three shards — exactly [first, first + n) although the draw buffer claims more."""
    gc = gpu_case(torch_mod, oracle, f"plain_{n}")
    assert (32 * (n // 32), n) in ee.ranges(n) and n % 32 == 1
    range_calls(torch_mod, engines, oracle, gc)


# ---------------------------------------------------------------------------------------------------- 4. planted cases
@pytest.mark.parametrize("name", PLANTED)
def test_planted_cases(torch_mod, engines, oracle, name):
    """zero_chunk (a chunk that publishes 0 << 2 | kAggregate: it must read as published and the chunks after it take its
    base), fat_chunk (the expansion loop's second trip, within several owners and within one), ragged (the record
    boundaries of dispatch sizes 32 / 64 / 128; through those engines too), lod_far (LODs read from the MeshInfo with a
    side table bound) — whole-buffer calls and ranges."""
    gc = gpu_case(torch_mod, oracle, name)
    sized = ("s64", "s128") if gc.case["plant"] == "ragged" else ()
    assert whole_calls(torch_mod, engines, oracle, gc, sized=sized) > 0
    range_calls(torch_mod, engines, oracle, gc, kinds=("plain", "side"))


# ---------------------------------------------------------------------------------------------------------- 5. capacity
@pytest.mark.parametrize("name", [f"{p}_{n}" for p in ("plain",) + ee.CLAMPED for n in ee.PLANT_SIZES])
def test_capacity_cuts_to_the_canonical_prefix(torch_mod, engines, oracle, name):
    """dispatch_capacity total - 1, total and 1 (and 4 096 against an entity of 65 536 records, in the first, a middle and
    the last chunk: what its chunk publishes is cut to capacity + 1): the canonical prefix, the header min(total,
    capacity), ORBIT_E_CAPACITY latched exactly when total > capacity, nothing written behind the capacity — through
    the whole-buffer call and the range call."""
    from orbit_amd._lib import E_CAPACITY, OrbitError

    torch = torch_mod
    gc = gpu_case(torch, oracle, name)
    c, eng = gc.case, engines["plain"]
    n = c["n"]
    for first, count, header in ((None, n, n), (0, n, n + ee.SLACK), (96, n - 96, n + ee.SLACK)):
        for op in (0, 2):
            vis = ee.words(c, "random", seed=5) if op else None
            probe = oracle_call(oracle, gc, op, header, vis, first=first, count=count, capacity=1)
            total = int(probe[0][:4].view(np.uint32)[0]) + probe[2]
            assert total > 2
            caps = [total - 1, total, 1] + ([ee.CLAMP_CAPACITY] if c["plant"] in ee.CLAMPED else [])
            for cap in caps:
                got = entity_call(torch, eng, gc, op, header, vis, first=first, count=count, capacity=cap)
                if total > cap:
                    with pytest.raises(OrbitError) as ei:
                        eng.status()
                    assert ei.value.code == E_CAPACITY
                else:
                    eng.status()
                ref = oracle_call(oracle, gc, op, header, vis, first=first, count=count, capacity=cap)
                assert int(ref[0][:4].view(np.uint32)[0]) == min(total, cap) and ref[2] == max(total - cap, 0)
                assert check(got, ref, (name, first, op, cap)) == min(total, cap)
    eng.status()  # the latch does not outlive the call that reads it


# ------------------------------------------------------------------------------------------------------------- 6. views
def _view_case(torch, oracle, count):
    """(case on the device, entity_draw_count) of a view of `count` draws: the case of that size, or the first `count`
    draws of the next larger one."""
    name = f"plain_{count}" if count in ee.SIZES else f"plain_{min(n for n in ee.SIZES if n >= count)}"
    return gpu_case(torch, oracle, name), count


VIEW_LISTS = [[n] for n in (ee.FUSED_MAX, ee.FUSED_MAX + 1, ee.ONE_LAUNCH, ee.ONE_LAUNCH + 1)] + \
             [[n, 300, 1] for n in (ee.FUSED_MAX, ee.FUSED_MAX + 1, ee.ONE_LAUNCH, ee.ONE_LAUNCH + 1)] + [[ee.ONE_LAUNCH + 1, 0, 300]]


VIEW_RUNS = [(path, v) for path in (0, 1, 2) for v in VIEW_LISTS if not (path == 2 and 0 in v)]  # (no one-launch cull of no draws)


@pytest.fixture(scope="module")
def view_engines(torch_mod):
    """cull_path -> an engine with scratch for three views, made when first asked for."""
    from orbit_amd.engine import Engine

    made = {}

    def get(cull_path):
        if cull_path not in made:
            made[cull_path] = Engine(0, max_views=3, cull_path=cull_path, **CAPS)
        return made[cull_path]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("cull_path,counts", VIEW_RUNS,
                         ids=[f"{('library_chooses', 'launch_chain', 'one_launch')[p]}-{'_'.join(map(str, v))}" for p, v in VIEW_RUNS])
def test_cull_views_on_both_sides_of_a_threshold(torch_mod, view_engines, oracle, cull_path, counts):
    """orbit_cull_views with views on both sides of the thresholds in one call (the two-launch views form runs the
    largest view's blocks for every view: 129 for a view of 2 chunks, or of none), passes 0 and 2, each view with its own
    bitsets: records, commands and both bitsets == oracle.entity_cull + oracle.meshlet_cull, and fused_culls() moves
    by len(views) exactly where every view is non-empty and (at most 16 384 draws or cull_path = 2)."""
    torch = torch_mod
    eng = view_engines(cull_path)
    fused = cull_path != 1 and all(k != 0 and (cull_path == 2 or k <= ee.FUSED_MAX) for k in counts)
    for op in (0, 2):
        views, outs, refs = [], [], []
        for k, count in enumerate(counts):
            gc, count = _view_case(torch, oracle, count)
            c = gc.case
            s = c["scene"]
            ci = ee.cull_info(c, op)
            evis = ee.words(c, "random", seed=10 + k)
            mvis = np.random.default_rng(20 + k).integers(0, 2 ** 32, s.vis_words, dtype=np.uint32)
            cap_d, cap_c = c["capacity"], s.lod0_meshlets + 8
            disp = out_buffer(torch, cap_d)
            draw = torch.full((L.DRAW_HEADER + 28 * cap_c + RED_ZONE,), PATTERN, dtype=torch.uint8, device="cuda")
            e_d, m_d = dev(torch, evis), dev(torch, mvis)
            views.append(dict(cull_info=ci, entity_draw_buffer=gc.draws(count), mesh_info_buffer=gc.mesh_infos,
                              meshlet_dispatch_buffer=disp, entity_buffer=gc.entities, entity_draw_count=count,
                              dispatch_capacity=cap_d, meshlet_buffer=gc.meshlets, draw_commands_buffer=draw,
                              material_buffer=gc.materials, draw_capacity=cap_c, visibility_buffer=e_d if op else None,
                              meshlet_visibility_buffer=m_d if op else None, **pyramid_kw(gc, op)))
            outs.append((disp, draw, e_d, m_d, cap_d, cap_c))
            od, oev, d1 = oracle.entity_cull(ci, ee.draw_buffer(c, count), count, s.mesh_infos, s.entities, cap_d,
                                             evis if op else None, c["pyr"], c["psize"])
            oc, omv, d2 = oracle.meshlet_cull(ci, od, s.meshlets, cap_c, s.entities, s.materials, mvis if op else None,
                                              c["pyr"], c["psize"])
            assert d1 == 0 and d2 == 0
            refs.append((od, oc, oev, omv))
        before = eng.fused_culls()
        eng.cull_views(views)
        torch.cuda.synchronize()
        eng.status()
        assert eng.fused_culls() - before == (len(counts) if fused else 0)
        for k, ((disp, draw, e_d, m_d, cap_d, cap_c), ref) in enumerate(zip(outs, refs)):
            recs, cmds = assert_same((host(disp), host(draw), host(e_d, np.uint32) if op else None,
                                      host(m_d, np.uint32) if op else None), ref)
            assert (len(recs) > 0 and len(cmds) > 0) or counts[k] <= 1
            assert bool((disp[12 + 16 * len(recs):] == PATTERN).all()), "a write behind the counted records"
            assert bool((draw[4 + 28 * cap_c:] == PATTERN).all()), "a write behind the draw capacity"


# ------------------------------------------------------------------------------------------------------------- 7. shard
_shard_refs = {}


@pytest.mark.parametrize("first,count", [(0, ee.SHARD_MAX), (0, ee.SHARD_MAX + 1), (96, ee.SHARD_MAX)])
@pytest.mark.parametrize("commands", [False, True], ids=["list", "list_and_commands"])
def test_cull_shard_on_both_sides_of_256_chunks(torch_mod, engines, oracle, first, count, commands):
    """orbit_cull_shard over 65 536 and 65 537 draws from draw 0 and over 65 536 draws from draw 96: dispatch records,
    record list and commands == the oracle's and == orbit_entity_cull_range + the record-list call's; the one launch is
    taken exactly for the ranges of at most 256 chunks."""
    torch = torch_mod
    gc = gpu_case(torch, oracle, f"plain_{ee.SHARD_MAX + 1}")
    c, eng = gc.case, engines["plain"]
    s = c["scene"]
    assert first + count <= s.entity_draw_count
    header = s.entity_draw_count
    ci = ee.cull_info(c, 0)
    cap_d, cap_c = c["capacity"], s.lod0_meshlets + 8

    _Scene = SimpleNamespace(draws=gc.draws(header), mesh_infos=gc.mesh_infos, entities=gc.entities, meshlets=gc.meshlets,
                             materials=gc.materials)  # what test_shard_gpu._shard reads
    before = eng.shard_culls()
    disp, rec, cmd = _shard(torch, eng, _Scene, ci, first, first + count, cap_d, cap_c, commands)
    disp2, rec2, cmd2 = _shard(torch, eng, _Scene, ci, first, first + count, cap_d, cap_c, commands, two_calls=True)
    torch.cuda.synchronize()
    eng.status()
    assert eng.shard_culls() - before == (1 if ee.chunks_of(count) <= ee.SHARD_MAX_CHUNKS else 0)
    if (first, count) not in _shard_refs:  # computed once, shared by the two forms, left unchanged
        odisp, _, d1 = oracle.entity_cull(ci, ee.draw_buffer(c, header), count, s.mesh_infos, s.entities, cap_d, draw_first=first)
        odraw, _, d2 = oracle.meshlet_cull(ci, odisp, s.meshlets, cap_c, s.entities, s.materials)
        assert d1 == 0 and d2 == 0
        (n_rec, _, _), orecs = L.dispatch_buffer_records(odisp)
        on, ocmds = L.draw_buffer_commands(odraw)
        _shard_refs[first, count] = (odisp, odraw, int(n_rec), on, _expected_visible_records(orecs, ocmds))
    odisp, odraw, n_rec, on, want = _shard_refs[first, count]
    assert n_rec > 0 and on > 0
    hd, hr = host(disp), host(rec)
    assert np.array_equal(hd[:12 + 16 * n_rec], odisp[:12 + 16 * n_rec]), "dispatch records differ from the oracle's"
    assert bool((hd[12 + 16 * cap_d:] == 0xAB).all())
    assert list(hr[:8].view(np.uint32)) == [n_rec, on]
    assert np.array_equal(hr[8:8 + 12 * n_rec].view(np.uint32), want.view(np.uint32)), "record list differs"
    assert bool((hr[8 + 12 * n_rec:] == 0xCD).all()), "a write behind the record list"
    assert torch.equal(rec, rec2) and torch.equal(disp[:12 + 16 * n_rec], disp2[:12 + 16 * n_rec])
    if commands:
        hc = host(cmd)
        assert np.array_equal(hc[:4 + 28 * on], odraw[:4 + 28 * on]), "commands differ from the oracle's"
        assert bool((hc[4 + 28 * cap_c:] == 0xEF).all()) and torch.equal(cmd[:4 + 28 * on], cmd2[:4 + 28 * on])
