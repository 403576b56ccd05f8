"""orbit_expand_visible_records and orbit_compact_segments (orbit_amd/csrc/meshlet_lists.hip) on lists chosen for them:
the hand-made lists of tests/record_lists.py at every one of their capacities, from the Meshlet buffer and from a bound
derived stream; list after list on one context; one captured call replayed on other lists; compaction around the trips of
its copy loop and with every way a capacity can cut it; and, end to end, sparse culled scenes — most of whose records are
empty, the command buffer sized for what survives — through cull, compaction and expansion against the oracle.

Every buffer the library writes lies inside a larger tensor of 0xCD; what it must not touch is compared after every call.
What each (list, capacity) pair exercises is counted by tests/test_record_lists_cpu.py."""
import numpy as np
import pytest

import record_lists as rl
from orbit_amd import layouts as L
from test_gpu_parity import GpuScene, dev, engine, host, torch_mod  # noqa: F401
from test_record_lists_cpu import culled  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 256
PATHS = ["meshlet_buffer", "meshlet_stream"]


class Guarded:
    """`nbytes` for the library to write (`buf`), 0xCD like the guards on either side of it."""

    def __init__(self, torch, nbytes):
        self.torch, self.nbytes = torch, nbytes
        self.all = torch.full((GUARD + nbytes + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
        self.buf = self.all[GUARD:GUARD + nbytes]

    def check(self, written, what):
        """Only buf[:written] may differ from 0xCD."""
        assert bool((self.all[:GUARD] == 0xCD).all()), f"{what}: the guard in front was written"
        assert bool((self.all[GUARD + written:] == 0xCD).all()), f"{what}: written behind byte {written} of {self.nbytes}"


def check_status(eng, overflow, what):
    from orbit_amd._lib import E_CAPACITY, OrbitError

    if overflow:
        with pytest.raises(OrbitError) as ei:
            eng.status()
        assert ei.value.code == E_CAPACITY, what
    else:
        eng.status()  # raises whatever was latched


def expand_and_check(torch, eng, rec_d, meshlets_d, S, ref_d, cap, what):
    """One orbit_expand_visible_records at capacity `cap` of a list with S survivors whose commands' bytes are ref_d."""
    out = Guarded(torch, L.DRAW_HEADER + 28 * cap)
    eng.expand_visible_records(rec_d, meshlets_d, out.buf, cap)
    torch.cuda.synchronize()
    k = min(S, cap)
    got = int(out.buf[:4].view(torch.int32).item())
    assert got == k, f"{what}: header {got}, {S} survivors at capacity {cap}"
    assert torch.equal(out.buf[4:4 + 28 * k], ref_d[:28 * k]), f"{what}: commands differ at capacity {cap}"
    out.check(4 + 28 * k, f"{what} at capacity {cap}")
    check_status(eng, S > cap, f"{what} at capacity {cap}")


class _Lists:
    """The meshlet buffer of the hand-made lists on the device, and an engine per path: the `meshlet_stream` one has a
    derived stream bound that covers the buffer (expand_gather<true>)."""

    def __init__(self, torch):
        from orbit_amd.engine import Engine

        self.torch = torch
        self.meshlets = rl.meshlet_buffer()
        self.meshlets_d = dev(torch, self.meshlets)
        self.engines = {p: Engine(0, max_entities=1024, max_dispatches=8192, max_draws=65536) for p in PATHS}
        self.ms = self.engines["meshlet_stream"].meshlet_stream(self.meshlets_d, 0, rl.N_MESHLETS)
        self.engines["meshlet_stream"].bind_meshlet_stream(self.ms)
        torch.cuda.synchronize()
        self.refs = {}

    def ref(self, case):
        """(record buffer on the device, all the list's commands as bytes on the device), made once per list."""
        if case.name not in self.refs:
            S, cmds, _ = rl.expand_ref(case.records, case.n, self.meshlets, case.S)
            assert S == case.S == len(cmds)
            self.refs[case.name] = (dev(self.torch, case.buffer), dev(self.torch, cmds) if S else
                                    self.torch.zeros(0, dtype=self.torch.uint8, device="cuda"))
        return self.refs[case.name]

    def close(self):
        self.engines["meshlet_stream"].bind_meshlet_stream(None)
        self.ms.close()
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def lists(torch_mod):
    ctx = _Lists(torch_mod)
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------------- expansion
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(rl.LISTS))
def test_expansion_of_a_hand_made_list_at_each_of_its_capacities(torch_mod, lists, name, path):
    """Header min(S, capacity), the commands of expand_ref, nothing behind them, E_CAPACITY if and only if S > capacity."""
    case, eng = rl.LISTS[name], lists.engines[path]
    rec_d, ref_d = lists.ref(case)
    before = eng.meshlet_stream_culls()
    caps = rl.capacities(case)
    for cap in caps:
        expand_and_check(torch_mod, eng, rec_d, lists.meshlets_d, case.S, ref_d, cap, f"{name} from the {path}")
    assert eng.meshlet_stream_culls() - before == (len(caps) if path == "meshlet_stream" else 0), "the wrong gather ran"


@pytest.mark.parametrize("path", PATHS)
def test_lists_of_different_lengths_on_one_context(torch_mod, lists, path):
    """The survivor counts per block of a longer list stay in the context's scratch: a shorter list must not sum them."""
    from orbit_amd.engine import Engine

    torch = torch_mod
    eng = Engine(0, max_entities=1024, max_dispatches=8192, max_draws=65536)
    if path == "meshlet_stream":
        eng.bind_meshlet_stream(lists.ms)
    for name in ("p64_4097", "full_1", "alternating_2049", "zero_0", "p64_1025", "full_64", "bit0_4097", "last_only_1025"):
        case = rl.LISTS[name]
        rec_d, ref_d = lists.ref(case)
        for cap in (case.S + 8, case.S):
            expand_and_check(torch, eng, rec_d, lists.meshlets_d, case.S, ref_d, cap, f"{name} in a row, {path}")
    eng.bind_meshlet_stream(None)
    eng.close()


@pytest.mark.parametrize("path", PATHS)
def test_one_captured_expansion_replayed_on_other_lists(torch_mod, lists, path):
    """The list's length and its survivors are read on the device: a call captured over one list expands whatever list
    lies in the same buffer at replay — longer, shorter, sparser, or one that overflows the capacity it was captured with."""
    torch = torch_mod
    eng = lists.engines[path]
    cap = 2100
    rec = torch.zeros(L.VISIBLE_HEADER + 12 * (4097 + rl.TAIL), dtype=torch.uint8, device="cuda")
    out = Guarded(torch, L.DRAW_HEADER + 28 * cap)
    first = rl.LISTS["alternating_63"]
    rec[:len(first.buffer)].copy_(lists.ref(first)[0])
    st, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        eng.expand_visible_records(rec, lists.meshlets_d, out.buf, cap, stream=st)  # warm
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            eng.expand_visible_records(rec, lists.meshlets_d, out.buf, cap, stream=st)
    torch.cuda.synchronize()
    eng.status()
    for name in ("p64_4097", "alternating_65", "last_only_2049", "bit0_4097", "zero_1025"):
        case = rl.LISTS[name]
        rec_d, ref_d = lists.ref(case)
        rec.zero_()
        rec[:len(case.buffer)].copy_(rec_d)
        out.all.fill_(0xCD)
        g.replay()
        torch.cuda.synchronize()
        k = min(case.S, cap)
        assert int(out.buf[:4].view(torch.int32).item()) == k, name
        assert torch.equal(out.buf[4:4 + 28 * k], ref_d[:28 * k]), f"{name}: the replayed expansion differs"
        out.check(4 + 28 * k, f"{name} replayed")
        check_status(eng, case.S > cap, f"{name} replayed")


# ------------------------------------------------------------------------------------------------------ end to end
def _tail(torch, n_meshlets):
    """TAIL full entries over valid meshlets, to lie behind a compacted list on the device (tests/record_lists.py)."""
    return dev(torch, rl.with_tail("tail", [], [], [], n_meshlets).records)


@pytest.fixture(scope="module")
def gpu_scenes(torch_mod, culled):  # noqa: F811
    return {keep: GpuScene(torch_mod, culled[keep][0]) for keep in rl.KEEPS}


@pytest.mark.parametrize("world", [1, 3, 8])
@pytest.mark.parametrize("keep", rl.KEEPS)
def test_sparse_scene_through_cull_compaction_and_expansion(torch_mod, engine, culled, gpu_scenes, keep, world):  # noqa: F811
    """Every rank's record list (orbit_meshlet_cull_visible_records, then orbit_cull_shard), the ranks' whole list
    buffers side by side as the segments of an all-gather, orbit_compact_segments, orbit_expand_visible_records with the
    command buffer sized for what survives: the oracle's records and the oracle's commands, and no status latched — most
    records are empty, so the list has more 1024-record blocks than the commands have 1024-command blocks.
    (keep = 0.05 before the expansion walked the list with the stride of its grid: 2318 records, 760 survivors, 350 of
    them in the first 1024 records; at a capacity of 760 or 761 the header was 350 and ORBIT_E_CAPACITY was latched.)"""
    from orbit_amd.dist import shard_ranges

    torch = torch_mod
    scene, case, ocmds = culled[keep]
    gs, ci = gpu_scenes[keep], rl.scene_cull_info()
    S, n = len(ocmds), case.n
    ref_d, tail_d = dev(torch, ocmds), _tail(torch, len(scene.meshlets))
    want = torch.from_numpy(case.buffer[8:8 + 12 * n].copy()).cuda()
    cap_d = scene.max_dispatches() + 8  # a segment's capacity, the same on every rank
    for shard_call in (False, True):
        what = f"keep {keep}, world {world}, {'orbit_cull_shard' if shard_call else 'orbit_meshlet_cull_visible_records'}"
        ranks = []
        for b, e in shard_ranges(scene.entity_draw_count, world):
            disp = torch.zeros(L.DISPATCH_HEADER + 16 * cap_d, dtype=torch.uint8, device="cuda")
            rec = Guarded(torch, L.VISIBLE_HEADER + 12 * cap_d)
            if shard_call:
                engine.cull_shard(ci, gs.draws, gs.mesh_infos, disp, gs.entities, b, e - b, cap_d, gs.meshlets, gs.materials,
                                  rec.buf, cap_d)
            else:
                engine.entity_cull(ci, gs.draws, gs.mesh_infos, disp, gs.entities, e - b, cap_d, draw_first=b)
                engine.meshlet_cull_visible_records(ci, disp, gs.meshlets, rec.buf, gs.entities, gs.materials, cap_d, cap_d)
            torch.cuda.synchronize()
            engine.status()
            rec.check(8 + 12 * int(rec.buf[:4].view(torch.int32).item()), f"{what}, ranks' lists")
            ranks.append(rec.buf)
        segments = torch.cat(ranks)  # slack (0xCD) included, as an all-gather of the whole buffers leaves them
        gathered = Guarded(torch, L.VISIBLE_HEADER + 12 * n)
        engine.compact_segments(segments, world, cap_d, gathered.buf, n, L.VISIBLE_HEADER, 12)
        torch.cuda.synchronize()
        engine.status()
        assert host(gathered.buf[:8], np.uint32).tolist() == [n, 0], what
        assert torch.equal(gathered.buf[8:], want), f"{what}: the gathered list is not the oracle's"
        gathered.check(8 + 12 * n, f"{what}, compaction")
        rec_d = torch.cat([gathered.buf, tail_d])
        for cap in (S, S + 1, scene.lod0_meshlets + 8, S - 1):
            expand_and_check(torch, engine, rec_d, gs.meshlets, S, ref_d, cap, what)


# ------------------------------------------------------------------------------------------------------- compaction
SEGMENT_CAPACITY = 6000  # several workgroups per segment
COUNTS = (0, 1, 85, 86, 341, 342, 5999, 6000)  # x 3 words: around the 256- and the 1024-dword trips of the copy


def _segments(rng, world, header, stride, counts):
    seg_bytes = header + stride * SEGMENT_CAPACITY
    seg = rng.integers(0, 256, world * seg_bytes, dtype=np.uint8)  # slack and further header words: garbage
    for r in range(world):
        seg[seg_bytes * r:seg_bytes * r + 4].view(np.uint32)[0] = counts[r]
    return seg


def _compact_and_check(torch, eng, seg, seg_d, world, header, stride, out_capacity, what):
    ref, overflow = rl.compact_ref(seg, world, SEGMENT_CAPACITY, out_capacity, header, stride)
    out = Guarded(torch, header + stride * out_capacity)
    eng.compact_segments(seg_d, world, SEGMENT_CAPACITY, out.buf, out_capacity, header, stride)
    torch.cuda.synchronize()
    assert host(out.buf[:header], np.uint32).tolist() == ref[:header].view(np.uint32).tolist(), what
    assert torch.equal(out.buf[:len(ref)].cpu(), torch.from_numpy(ref)), f"{what}: the list differs"
    out.check(len(ref), what)
    check_status(eng, overflow, what)
    return overflow


@pytest.mark.parametrize("header,stride", [(8, 12), (4, 28)])
@pytest.mark.parametrize("world", [1, 2, 3, 8, 64])
def test_compaction_against_the_reference(torch_mod, world, header, stride):
    """Both layouts the library's callers exchange (record lists: header 8 / stride 12; command lists: 4 / 28)."""
    from orbit_amd.engine import Engine

    torch = torch_mod
    eng = Engine(0, max_entities=1024, max_dispatches=8192, max_draws=65536)
    rng = np.random.default_rng(1000 * world + stride)
    what = f"world {world}, header {header}, stride {stride}"
    # every count of COUNTS in turn (a world of 64 holds them all at once), everything fits
    for trial in range(2 if world >= 8 else 4):
        counts = [COUNTS[(trial * world + r + int(rng.integers(0, 2)) * 4) % len(COUNTS)] for r in range(world)]
        seg = _segments(rng, world, header, stride, counts)
        assert not _compact_and_check(torch, eng, seg, dev(torch, seg), world, header, stride, sum(counts) + 3, f"{what}, {counts}")
    counts = [int(c) for c in rng.choice(COUNTS, world)]
    k = world // 2
    counts[k] = 342
    seg = _segments(rng, world, header, stride, counts)
    seg_d = dev(torch, seg)
    first = sum(counts[:k])
    # out_capacity inside segment k: the later segments write nothing, the overflow is latched; exactly at its ends; 0
    for out_capacity in (first + 171, first + 1, first + 341, first, first + 342, sum(counts), 0):
        overflow = _compact_and_check(torch, eng, seg, seg_d, world, header, stride, out_capacity, f"{what}, cut at {out_capacity}")
        assert overflow == (sum(counts) > out_capacity)
    # one rank states more than a segment holds (its own overflow, latched where it happened): cut there, nothing
    # latched here, and the slack behind the others' items is garbage
    stated = list(counts)
    stated[k] = SEGMENT_CAPACITY + 77
    seg = _segments(rng, world, header, stride, stated)
    total = sum(min(c, SEGMENT_CAPACITY) for c in stated)
    assert not _compact_and_check(torch, eng, seg, dev(torch, seg), world, header, stride, total, f"{what}, overstated")
    # all segments empty
    seg = _segments(rng, world, header, stride, [0] * world)
    for out_capacity in (5, 0):
        assert not _compact_and_check(torch, eng, seg, dev(torch, seg), world, header, stride, out_capacity, f"{what}, empty")
    eng.close()
