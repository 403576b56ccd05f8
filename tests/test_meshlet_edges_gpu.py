"""The meshlet stage at its tile, group, scan-chunk and ticket edges, on the device (tests/meshlet_edges.py; what each case
exercises is counted by tests/test_meshlet_edges_cpu.py): orbit_meshlet_cull and its three sister outputs fed hand-built
MeshletDispatchBuffers — from the Meshlet buffer (payload emit), from a bound derived stream (chain emit) and from a
stream with alpha classes — bit for bit against the oracle, with no tolerance anywhere.

Every output buffer is pre-filled with a byte pattern: everything behind what the header counts, and behind the capacity,
must still hold it afterwards; the visibility words are compared whole (the words of the full records that lie behind
entry n of every dispatch buffer included: they never show).  Every run reads the context's status: ORBIT_E_CAPACITY
exactly when the reference says the survivors exceed the draw capacity.

Not tried here: the chain emit's `capped` loop (meshlet_emit.hip: a wave that has had kDynGroups ticketed groups while
its pool still holds some).  It needs the waves of a fully resident grid to run at very different speeds, which a test
cannot force and must not try to (no test here loops or stalls to provoke it)."""
import numpy as np
import pytest

import meshlet_edges as me
from orbit_amd import layouts as L
from test_gpu_parity import dev, host, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

PATTERN = 0xA7
RED_ZONE = 512
OUTPUTS = ("commands", "task", "list", "list_and_commands")
LAYOUT = dict(plain="scattered", contracted="scattered", stream="chain", classes="chain")
SMALL_CAPS = dict(max_entities=1024, max_dispatches=4 * (2 * me.CHUNK + 1) + me.TAIL, max_draws=1 << 21)


# ------------------------------------------------------------------------------------------------------------ context
class Ctx:
    """The planted buffers on the device (read-only afterwards) and the engines over them, made when first asked for:
    "plain", "contracted" (arith_profile 1), "stream" (a derived stream of the chain layout bound), "classes" (that stream
    with the alpha classes of the material buffer)."""

    def __init__(self, torch, oracle, **caps):
        self.torch, self.oracle, self.caps = torch, oracle, caps
        self.meshlets = {k: dev(torch, me.meshlet_buffer(k)) for k in ("scattered", "chain")}
        self.entities, self.materials = dev(torch, me.entities()), dev(torch, me.materials())
        self.pyr = {k: dev(torch, me.pyramid(oracle, k)) for k in ("zero", "depth")}
        self.engines, self.streams, self.dispatch = {}, {}, {}

    def engine(self, kind):
        from orbit_amd.engine import Engine

        if kind not in self.engines:
            eng = Engine(0, **dict(self.caps, **(dict(arith_profile=1) if kind == "contracted" else {})))
            if kind in ("stream", "classes"):
                ms = eng.meshlet_stream(self.meshlets["chain"], 0, me.N_MESHLETS)
                if kind == "classes":
                    ms.set_materials(self.materials, me.N_MATERIALS)
                eng.bind_meshlet_stream(ms)
                self.torch.cuda.synchronize()
                self.streams[kind] = ms
            self.engines[kind] = eng
        return self.engines[kind]

    def records(self, c):
        """The case's MeshletDispatchBuffer on the device: the header says n, full records lie behind entry n."""
        if c.name not in self.dispatch:
            self.dispatch[c.name] = dev(self.torch, c.buffer())
        return self.dispatch[c.name]

    def close(self):
        for kind, eng in self.engines.items():
            if kind in self.streams:
                eng.bind_meshlet_stream(None)
                self.streams[kind].close()
            eng.close()


@pytest.fixture(scope="module")
def ctx(torch_mod, oracle):
    c = Ctx(torch_mod, oracle, **SMALL_CAPS)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------- reference
def reference(oracle, c, kind, op, pyr_kind, cap, vis, lists=True):
    """The oracle's commands and visibility words — and, with `lists`, its task records and the record list derived from
    them — of a cull at capacity (dispatch, draw): it is given the records the library is to read, min(header, dispatch
    capacity) of them."""
    cap_d, cap_c = cap
    layout = LAYOUT[kind]
    buf = c.buffer(min(c.n, cap_d))
    pyr = me.pyramid(oracle, pyr_kind) if op == 2 else None
    args = (me.entities(), me.materials(), vis, pyr, me.PYRAMID)
    with oracle.arith_profile(1 if kind == "contracted" else 0):
        out, ovis, dropped = oracle.meshlet_cull(me.cull_info(op), buf, me.meshlet_buffer(layout), cap_c, *args)
        task = oracle.meshlet_task_cull(me.cull_info(op), buf, me.meshlet_buffer(layout), *args)[0] if lists else None
    kept = int(out[:4].view(np.uint32)[0])
    assert kept == min(kept + dropped, cap_c)
    ref = dict(commands=out[:4 + 28 * kept], total=kept + dropped, vis=ovis, records=min(c.n, cap_d))
    if lists:
        ref["task"] = task
        ref["list"], survivors = me.record_list_of(task)
        assert survivors == ref["total"]
    return ref


# ---------------------------------------------------------------------------------------------------------------- runs
def patterned(torch, nbytes):
    return torch.full((nbytes + RED_ZONE,), PATTERN, dtype=torch.uint8, device="cuda")


def prepare(ctx, c, op, output, cap):
    """The buffers of one cull: (visibility words or None, {name: patterned output buffer})."""
    torch = ctx.torch
    cap_d, cap_c = cap
    vis_d = dev(torch, c.words("random")) if op else None
    out = {}
    if output in ("commands", "list_and_commands"):
        out["commands"] = patterned(torch, L.DRAW_HEADER + 28 * cap_c)
    if output in ("list", "list_and_commands"):
        out["list"] = patterned(torch, L.VISIBLE_HEADER + 12 * cap_d)
    if output == "task":
        out["task"] = patterned(torch, 44 * cap_d)
    ctx.records(c)
    return vis_d, out


def launch(ctx, kind, c, op, pyr_kind, output, cap, bufs, stream=None):
    cap_d, cap_c = cap
    vis_d, out = bufs
    eng = ctx.engine(kind)
    kw = dict(meshlet_visibility_buffer=vis_d, stream=stream)
    if op == 2:
        kw.update(depth_pyramid=ctx.pyr[pyr_kind], depth_pyramid_size=me.PYRAMID)
    a = (me.cull_info(op), ctx.records(c), ctx.meshlets[LAYOUT[kind]])
    e = (ctx.entities, ctx.materials)
    before = eng.meshlet_stream_culls(), eng.meshlet_class_culls()
    if output == "commands":
        eng.meshlet_cull(*a, out["commands"], *e, cap_d, cap_c, **kw)
    elif output == "task":
        eng.meshlet_task_cull(*a, out["task"], *e, cap_d, **kw)
    elif output == "list":
        eng.meshlet_cull_visible_records(*a, out["list"], *e, cap_d, cap_d, **kw)
    else:
        eng.meshlet_cull_records_and_commands(*a, out["list"], out["commands"], *e, cap_d, cap_d, cap_c, **kw)
    # the path the run is for was taken: the derived streams serve passes 0 and 2, the classes where they are bound
    streamed = 1 if (kind in ("stream", "classes") and op != 1) else 0
    assert eng.meshlet_stream_culls() - before[0] == streamed
    assert eng.meshlet_class_culls() - before[1] == (streamed if kind == "classes" else 0)


def same(torch, got, want, what):
    """got[:len(want)] == want and the pattern behind it."""
    k = len(want)
    assert torch.equal(got[:k], torch.from_numpy(np.ascontiguousarray(want)).cuda()), what
    assert bool((got[k:] == PATTERN).all()), (what, "a write behind what the header counts or behind the capacity")


def check(ctx, ref, output, cap, bufs, what):
    torch = ctx.torch
    vis_d, out = bufs
    cap_d, cap_c = cap
    if "commands" in out:
        hdr = int(out["commands"][:4].view(torch.int32).item()) & 0xFFFFFFFF
        assert hdr == min(ref["total"], cap_c), (what, "command header", hdr, ref["total"], cap_c)
        same(torch, out["commands"], ref["commands"], (what, "commands differ"))
    if "list" in out:
        hdr = host(out["list"][:8], np.uint32).tolist()
        assert hdr == [ref["records"], ref["total"]], (what, "record-list header", hdr)
        same(torch, out["list"][8:], ref["list"].view(np.uint8), (what, "record list differs"))
    if "task" in out:
        assert len(ref["task"]) == ref["records"]
        same(torch, out["task"], ref["task"].view(np.uint8), (what, "task records differ"))
    if vis_d is not None:
        assert np.array_equal(host(vis_d, np.uint32), ref["vis"]), (what, "visibility words differ")


def status(eng, overflow, what, stream=None):
    from orbit_amd._lib import E_CAPACITY, OrbitError

    if overflow:
        with pytest.raises(OrbitError) as ei:
            eng.status(stream=stream)
        assert ei.value.code == E_CAPACITY, what
    else:
        eng.status(stream=stream)  # raises whatever was latched


def run(ctx, kind, c, op, pyr_kind, output, cap, refs=None):
    """One cull, its status, one comparison."""
    what = (c.name, kind, f"pass {op}", pyr_kind, output, cap)
    bufs = prepare(ctx, c, op, output, cap)
    launch(ctx, kind, c, op, pyr_kind, output, cap, bufs)
    key = (LAYOUT[kind], kind == "contracted", op, pyr_kind, cap)
    lists = output != "commands"  # the task records and the record list only where an output is compared with them
    ref = None if refs is None else refs.get(key)
    if ref is None or (lists and "task" not in ref):
        ref = reference(ctx.oracle, c, kind, op, pyr_kind, cap, c.words("random") if op else None, lists=lists)
        if refs is not None:
            refs[key] = ref
    status(ctx.engine(kind), "commands" in bufs[1] and ref["total"] > cap[1], what)
    check(ctx, ref, output, cap, bufs, what)
    return ref


# ----------------------------------------------------------------------------------- 1. small and chunk cases, every density
@pytest.mark.parametrize("name", list(me.PLAN))
def test_every_density_at_every_small_and_chunk_count(ctx, name):
    """0 .. 65 records and both sides of one and two scan chunks x all zero, all full (512 a tile: the dense rebuild, slow
    groups), tiles of exactly 64 / 65 / 128 / 129 and groups of exactly 128 / 129 survivors, a single survivor in the last
    record, alternating records, an empty tile between full ones, the first tile of chunk 1 alone, the planted chain
    breaks, seeded runs: pass 0 on the plain, stream and alpha-class engines x commands, task records, record list, record
    list + commands; passes 1 and 2 (both pyramids) with commands on the plain and stream engines; the contracted
    arithmetic's pass-0 commands."""
    c = me.case(name)
    cap = (c.n, c.survivors() + 8)
    refs = {}
    for kind in ("plain", "stream", "classes"):
        for output in OUTPUTS:
            ref = run(ctx, kind, c, 0, None, output, cap, refs)
            assert ref["total"] == c.survivors() and ref["records"] == c.n
    for kind in ("plain", "stream"):
        for op, pyr_kind in ((1, None), (2, "zero"), (2, "depth")):
            run(ctx, kind, c, op, pyr_kind, "commands", cap, refs)
    run(ctx, "contracted", c, 0, None, "commands", cap, refs)


# ----------------------------------------------------------------------------------------------------------- 2. capacities
@pytest.mark.parametrize("name", me.CUT_CASES)
def test_capacities_cut_to_the_canonical_prefix(ctx, name):
    """Dispatch capacities n, n + 1, n rounded up to a tile, 4 n (the grid and the first three tiles' prefetch follow the
    capacity) and n - 1 under a header that still says n; draw capacities S + 8, S, S - 1, 0, inside a trip at a multiple of
    64 and at the end of a tile's first trip with both neighbours, on a tile, a group and a chunk boundary: the canonical
    prefix, the header min(total, capacity), ORBIT_E_CAPACITY exactly when total > capacity, nothing behind the capacity."""
    c = me.case(name)
    pairs = me.capacities(c)
    assert len(pairs) >= 8
    for cap in pairs:
        for kind in ("plain", "stream"):  # (two layouts: a reference each)
            ref = run(ctx, kind, c, 0, None, "commands", cap)
            assert ref["total"] == c.survivors(cap[0])
    ctx.engine("plain").status()  # the latch does not outlive the call that reads it


# --------------------------------------------------------------------------------------------------- 3. device-derived cases
class BigCtx(Ctx):
    """A context sized for the device-derived cases of THIS device, its cases and their references (built once)."""

    def __init__(self, torch, oracle):
        self.num_cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.sizes = dict(eval=me.eval_sizes(self.num_cus), chain=me.chain_sizes(self.num_cus))
        largest = max(self.sizes["eval"] + self.sizes["chain"])
        super().__init__(torch, oracle, max_entities=1024, max_dispatches=largest + me.TAIL, max_draws=4 * largest)
        self.refs = {}

    def case(self, kind, index, variant=0):
        return me.device_case(kind, self.sizes[kind][index], self.num_cus, variant)

    def run(self, engine_kind, c, op, pyr_kind, output):
        return run(self, engine_kind, c, op, pyr_kind, output, (c.n, c.survivors() + 8), self.refs.setdefault(c.name, {}))


@pytest.fixture(scope="module")
def big(torch_mod, oracle):
    b = BigCtx(torch_mod, oracle)
    yield b
    b.close()


BIG_RUNS = [("plain", "commands"), ("stream", "commands"), ("plain", "list"), ("plain", "task")]


@pytest.mark.parametrize("engine_kind,output", BIG_RUNS, ids=["-".join(r) for r in BIG_RUNS])
@pytest.mark.parametrize("index", range(4), ids=["3T", "3T+1rec", "4T+17rec", "8T"])
def test_evaluation_around_its_first_ticket(big, index, engine_kind, output):
    """16 x 3 T records (every ticket drawn lies past the end), + 1 (one ticketed tile), 16 x 4 T + 17 (a ticketed round and
    two tiles, the last one of a single record), 16 x 8 T (two ticketed rounds); T = the wave stride in tiles on this
    device.  Short records, every 64th one full."""
    c = big.case("eval", index)
    layout = LAYOUT[engine_kind]
    want = ("eval_tickets_none_taken", "eval_one_ticketed_tile", "eval_ticketed_round", "eval_ticketed_round")[index]
    assert want in me.census(c, (c.n, c.survivors() + 8), layout, big.num_cus)
    ref = big.run(engine_kind, c, 0, None, output)
    assert ref["total"] == c.survivors() > c.n // 4


@pytest.mark.parametrize("engine_kind", ["plain", "stream"])
@pytest.mark.parametrize("op,pyr_kind", [(1, None), (2, "zero"), (2, "depth")], ids=["pass1", "pass2_zero", "pass2_depth"])
def test_the_late_passes_with_a_ticketed_round(big, op, pyr_kind, engine_kind):
    """Passes 1 and 2 at 16 x 4 T + 17 records: pass 2 draws tickets like pass 0 (and writes the visibility words of every
    tile, whoever took it), pass 1 walks its plain grid stride."""
    big.run(engine_kind, big.case("eval", 2), op, pyr_kind, "commands")


@pytest.mark.parametrize("engine_kind,output", BIG_RUNS, ids=["-".join(r) for r in BIG_RUNS])
@pytest.mark.parametrize("index", range(3), ids=["4G", "4G+1", "5G+1+1rec"])
def test_chain_emit_around_its_first_ticket(big, index, engine_kind, output):
    """32 x 4 G records (four static rounds: the tickets drawn lie past the end), + 32 (one ticketed group: the planted
    full one, which the general form finds again through the wave's list of ticketed groups), 32 x 5 G + 33 (a ticketed
    round and two groups, the last one of a single record); G = the chain emit's wave stride in groups on this device.
    The other engines and outputs run the same records through their own launches."""
    c = big.case("chain", index)
    got = me.census(c, (c.n, c.survivors() + 8), LAYOUT[engine_kind], big.num_cus)
    if engine_kind == "stream":
        assert ("emit_slow_group_ticketed" in got) == (index > 0) and ("emit_ticketed_groups" in got) == (index > 0)
    ref = big.run(engine_kind, c, 0, None, output)
    assert ref["total"] == c.survivors() > c.n // 4


# ------------------------------------------------------------------------------------------------------- 4. back to back
def _reference_of(big, c, engine_kind, cap):
    refs = big.refs.setdefault(c.name, {})
    key = (LAYOUT[engine_kind], False, 0, None, cap)
    if "task" not in refs.get(key, {}):
        refs[key] = reference(big.oracle, c, engine_kind, 0, None, cap, None)
    return refs[key]


def _in_a_row(big, engine_kind, jobs):
    """jobs = [(case, output)]: launched on one stream with nothing in between, compared after the last one."""
    torch = big.torch
    runs = []
    for c, output in jobs:
        cap = (c.n, c.survivors() + 8)
        runs.append((c, output, cap, prepare(big, c, 0, output, cap)))
    eng = big.engine(engine_kind)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for c, output, cap, bufs in runs:
            launch(big, engine_kind, c, 0, None, output, cap, bufs, stream=stream)
    eng.status(stream=stream)
    for k, (c, output, cap, bufs) in enumerate(runs):
        check(big, _reference_of(big, c, engine_kind, cap), output, cap, bufs, (k, c.name, output, engine_kind))


@pytest.mark.parametrize("engine_kind", ["plain", "stream"])
def test_output_kinds_back_to_back_where_tickets_are_drawn(big, engine_kind):
    """One context, one stream, no synchronisation in between: commands -> record list -> task records -> record list +
    commands -> commands at 16 x 4 T + 17 records.  Every output kind zeroes the tile tickets for the next evaluation in a
    place of its own (the emit launch or the scan launch, the evaluation's last workgroup, the task-record launch): a
    counter left standing drops or repeats tiles of the NEXT cull.  Consecutive culls read two variants of the case that
    differ in every record, so a tile the next evaluation skips is not saved by what the last one left in the scratch."""
    order = ("commands", "list", "task", "list_and_commands", "commands")
    _in_a_row(big, engine_kind, [(big.case("eval", 2, variant=k % 2), output) for k, output in enumerate(order)])


def test_a_shrinking_cull_behind_ticketed_groups(big):
    """The same context and stream, the derived stream bound: the chain emit with ticketed groups (32 x 4 G + 32 records),
    then 17 records, then none — each with its own capacity, so the grids shrink — and the other variant of the ticketed
    size: the group tickets and chunk_sums are the evaluation's to zero, the tile tickets the emit's."""
    seq = [big.case("chain", 1), me.case("mixed_17"), me.case("zero_0"), big.case("chain", 1, variant=1),
           big.case("chain", 2)]
    _in_a_row(big, "stream", [(c, "commands") for c in seq])
