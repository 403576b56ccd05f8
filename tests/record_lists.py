"""Record lists chosen by hand, plain references of what the library makes of them, and a census of what they exercise.

The record list — {records, survivors} + 12-B {entity_index, meshlet_offset, should-draw mask} per dispatch record — is
the only product of a cull that leaves the GPU that made it; orbit_compact_segments (the segments of an all-gather -> one
list) and orbit_expand_visible_records (a list -> MeshletDrawCommands) are what every frame of more than one rank passes
through (orbit_amd/csrc/meshlet_lists.hip).  Shared by tests/test_record_lists_cpu.py (the references against the oracle,
census floors), tests/test_record_lists_gpu.py (the kernels against the references) and tests/test_dist_cpu.py.  Nothing
of the product is asked: only the layouts.

`LISTS` lie over `meshlet_buffer()`, 4096 seeded meshlets: the lists' lengths sit around the 64-record chunk a wave takes
and the 1024-record block a workgroup takes, their masks run from all empty to all full; `capacities` cuts a list's
commands where the expansion's windows end; `sparse_scene` is a culled scene most of whose records are empty; `census`
names what a (list, capacity) pair exercises.  The floors tests/test_record_lists_cpu.py holds them to are a condition
on these INPUTS.
"""
import zlib

import numpy as np

import scenes as sc
from orbit_amd import layouts as L

CHUNK, BLOCK = 64, 1024  # records a wave / a workgroup of the expansion takes at a time
N_MESHLETS = 4096
TAIL = 96  # entries with a full mask behind entry n of every list: a read past n shows up as extra commands
SEED = 97
CLASSES = ("empty_records", "full_chunk_2048", "multi_block", "partial_last_block", "cut_inside_chunk",
           "cut_on_chunk_boundary", "cut_on_block_boundary", "capacity_zero",
           "fits_but_fewer_grid_blocks_than_record_blocks", "single_survivor_in_last_record", "first_index_wraps")


def _u32(seed, stream, idx):
    return (sc.rnd_u64(seed, stream, idx) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def meshlet_buffer():
    """4096 meshlets with arbitrary command words: vertex and triangle counts up to 255 (a quarter of them 255 each),
    one data_offset in eight within 1000 of 2^32, so that data_offset + vertex_count — and with it cmd_first_index —
    wraps."""
    i = np.arange(N_MESHLETS)
    m = np.zeros(N_MESHLETS, dtype=L.MESHLET)
    for a in range(4):
        m["bounding_sphere"][:, a] = sc.rnd_range(SEED, 1 + a, i, -50.0, 50.0)
    m["cone_axis"] = _u32(SEED, 5, i).view(np.int8).reshape(-1, 4)[:, :3]
    m["cone_cutoff"] = sc.rnd_int(SEED, 6, i, -128, 127).astype(np.int8)
    m["vertex_offset"] = _u32(SEED, 7, i)
    near = (np.uint64(1 << 32) - np.uint64(1) - sc.rnd_int(SEED, 9, i, 0, 999).astype(np.uint64)).astype(np.uint32)
    m["data_offset"] = np.where(i % 8 == 3, near, _u32(SEED, 8, i))
    m["material_index"] = sc.rnd_int(SEED, 10, i, 0, 65535).astype(np.uint16)
    m["vertex_count"] = np.where(i % 4 == 1, 255, sc.rnd_int(SEED, 11, i, 0, 255)).astype(np.uint8)
    m["triangle_count"] = np.where(i % 4 == 2, 255, sc.rnd_int(SEED, 12, i, 0, 255)).astype(np.uint8)
    return m


# ------------------------------------------------------------------------------------------------------ references
def mask_bits(masks):
    """(entry, bit) of every set bit of `masks`, entries in order, the bits of an entry ascending."""
    bits = np.unpackbits(np.ascontiguousarray(masks, dtype="<u4").view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")
    return np.nonzero(bits)


def expand_ref(records, n, meshlets, capacity):
    """orbit_expand_visible_records of records[:n] over `meshlets`: (S, commands[:min(S, capacity)], overflow) — the
    set bits of every mask in list order, ascending within an entry, each as the MeshletDrawCommand of meshlet
    meshlet_offset + bit for the entry's entity (shaders/meshlet_cull.comp:216-230); S counts all of them."""
    recs = np.ascontiguousarray(records[:n], dtype=L.VISIBLE_RECORD)
    entry, bit = mask_bits(recs["mask"])
    S = len(entry)
    entry, bit = entry[:min(S, capacity)], bit[:min(S, capacity)]
    index = recs["meshlet_offset"][entry].astype(np.int64) + bit
    assert len(index) == 0 or int(index.max()) < len(meshlets), "a list names a meshlet outside its buffer"
    m = meshlets[index]
    cmds = np.zeros(len(index), dtype=L.MESHLET_DRAW_COMMAND)
    cmds["cmd_index_count"] = m["triangle_count"].astype(np.uint32) * 3
    cmds["cmd_instance_count"] = 1
    cmds["cmd_first_index"] = ((m["data_offset"].astype(np.uint64) + m["vertex_count"]) * 4 & 0xFFFFFFFF).astype(np.uint32)
    cmds["cmd_vertex_offset"] = m["data_offset"].view(np.int32)
    cmds["cmd_first_instance"] = recs["entity_index"][entry]
    cmds["meshlet_vertex_offset"] = m["vertex_offset"]
    cmds["meshlet_index"] = index
    return S, cmds, S > capacity


def compact_ref(segments, world, segment_capacity, out_capacity, header_bytes, stride):
    """orbit_compact_segments of `world` segments {count | header | segment_capacity items} (bytes): (list, overflow),
    the list being {min(total, out_capacity), 0 ..} and the ranks' first min(count, segment_capacity) items in rank
    order, cut at out_capacity; overflow = the items do not all fit."""
    seg = np.ascontiguousarray(segments).view(np.uint8).reshape(-1)
    seg_bytes = header_bytes + stride * segment_capacity
    counts = [min(int(seg[seg_bytes * r:seg_bytes * r + 4].view("<u4")[0]), segment_capacity) for r in range(world)]
    items = [seg[seg_bytes * r + header_bytes:seg_bytes * r + header_bytes + stride * counts[r]] for r in range(world)]
    kept = min(sum(counts), out_capacity)
    out = np.zeros(header_bytes + stride * kept, dtype=np.uint8)
    out[:4].view("<u4")[0] = kept
    out[header_bytes:] = np.concatenate(items)[:stride * kept]
    return out, sum(counts) > out_capacity


def compact_segments_numpy(segments, world, segment_capacity, out, out_capacity, header, stride, stream=None):
    """compact_ref with orbit_compact_segments' arguments, on host tensors or arrays: writes the list into `out` and
    nothing behind it (what orbit_amd.dist.AllGatherExchange takes as `compact`)."""
    as_np = lambda t: t.numpy() if hasattr(t, "numpy") else t  # noqa: E731
    got, _ = compact_ref(as_np(segments), world, segment_capacity, out_capacity, header, stride)
    as_np(out)[:len(got)] = got


# ------------------------------------------------------------------------------------------------------------ lists
class Case:
    """A record list of `n` entries in the bytes of a record buffer: header {n, garbage}, the entries, and TAIL entries
    with a full mask behind them."""

    def __init__(self, name, records, n):
        self.name, self.n = name, n
        self.records = np.ascontiguousarray(records, dtype=L.VISIBLE_RECORD)
        assert len(self.records) == n + TAIL and bool((self.records["mask"][n:] == 0xFFFFFFFF).all())
        self.buffer = np.zeros(L.VISIBLE_HEADER + 12 * len(self.records), dtype=np.uint8)
        self.buffer[:8].view("<u4")[:] = (n, 0xDEADBEEF)  # the second word is not maintained by the exchanges
        self.buffer[8:] = self.records.view(np.uint8)
        self.pops = np.unpackbits(np.ascontiguousarray(self.records["mask"][:n]).view(np.uint8)).reshape(-1, 32).sum(axis=1)
        self.S = int(self.pops.sum())
        self.before = np.concatenate([[0], np.cumsum(self.pops)]).astype(np.int64)  # survivors in front of entry i

    def __repr__(self):
        return self.name


def with_tail(name, entity_index, meshlet_offset, mask, n_meshlets):
    """The Case of these entries: a tail of full entries over valid meshlets is appended."""
    n = len(mask)
    seed = zlib.crc32(name.encode()) & 0xFFFF
    recs = np.zeros(n + TAIL, dtype=L.VISIBLE_RECORD)
    recs["entity_index"][:n], recs["meshlet_offset"][:n], recs["mask"][:n] = entity_index, meshlet_offset, mask
    t = np.arange(TAIL)
    recs["entity_index"][n:] = _u32(seed, 31, t)
    recs["meshlet_offset"][n:] = sc.rnd_int(seed, 32, t, 0, n_meshlets - 32)
    recs["mask"][n:] = 0xFFFFFFFF
    return Case(name, recs, n)


MASKS = {
    "zero": lambda seed, i: np.zeros(len(i), np.uint32),
    "full": lambda seed, i: np.full(len(i), 0xFFFFFFFF, np.uint32),  # 2048 codes per chunk, 32 768 survivors per block
    "bit0": lambda seed, i: np.full(len(i), 1, np.uint32),
    "bit31": lambda seed, i: np.full(len(i), 0x80000000, np.uint32),
    "alternating": lambda seed, i: np.where(i % 2 == 0, 0xFFFFFFFF, 0).astype(np.uint32),
    "p64": lambda seed, i: _u32(seed, 21, i) & _u32(seed, 22, i) & _u32(seed, 23, i) & _u32(seed, 24, i)
                           & _u32(seed, 25, i) & _u32(seed, 26, i),  # every bit with probability 2^-6
    "last_only": lambda seed, i: np.where(i == len(i) - 1, 1 << 17, 0).astype(np.uint32),
    "first_only": lambda seed, i: np.where(i == 0, 1 << 5, 0).astype(np.uint32),
}

# not the full product: every count and every pattern occurs, the full masks at a chunk, a block and a block and one
# record, the sparse ones with every count of more than a block
_PLAN = {
    0: ("zero",),
    1: ("full", "bit31", "zero"),
    63: ("alternating", "p64"),
    64: ("full", "bit0", "first_only"),
    65: ("bit31", "alternating", "last_only"),
    1023: ("alternating", "p64", "bit0"),
    1024: ("full", "zero", "last_only"),
    1025: ("full", "zero", "p64", "last_only", "first_only", "alternating"),
    2049: ("zero", "p64", "last_only", "first_only", "bit31", "alternating"),
    4097: ("zero", "p64", "last_only", "first_only", "bit0"),
}
COUNTS = tuple(_PLAN)


def _hand_made(n, pattern):
    name = f"{pattern}_{n}"
    seed = zlib.crc32(name.encode()) & 0xFFFF
    i = np.arange(n)
    entity = _u32(seed, 1, i)
    entity[i % 7 == 3] = 0xFFFFFFFF
    offset = sc.rnd_int(seed, 2, i, 0, N_MESHLETS - 32)  # offset + 31 < 4096: no case reads outside the buffer
    return with_tail(name, entity, offset, MASKS[pattern](seed, i), N_MESHLETS)


LISTS = {c.name: c for c in (_hand_made(n, p) for n, ps in _PLAN.items() for p in ps)}


def _chunks_with_survivors(case):
    """(survivors in front of the chunk, survivors of the chunk) of the 64-record chunks that hold any."""
    starts = np.arange(0, case.n, CHUNK)
    ends = np.minimum(starts + CHUNK, case.n)
    return [(int(case.before[a]), int(case.before[b] - case.before[a])) for a, b in zip(starts, ends)
            if case.before[b] > case.before[a]]


def capacities(case):
    """Command capacities to expand `case` at: S + 8, S, S - 1 and 0; inside the first and the last chunk that has
    survivors a cut at a multiple of 64 with its two neighbours, the same 64 commands behind the chunk's first (where the
    chunk's first window of commands ends), its middle and its two ends; and the survivors of the first 1024-record block.
    (The smallest capacity >= S that has fewer 1024-command blocks than the list has 1024-record blocks is S itself,
    where there is one: the census names the pairs.)"""
    S = case.S
    out = {S + 8, S, S - 1, 0, int(case.before[min(BLOCK, case.n)])}
    chunks = _chunks_with_survivors(case)
    for base, cnt in chunks[:1] + chunks[-1:]:
        m = (base // CHUNK + 1) * CHUNK
        if m < base + cnt:
            out |= {m - 1, m, m + 1}
        if cnt > CHUNK:
            out |= {base + CHUNK - 1, base + CHUNK, base + CHUNK + 1}
        out |= {base, base + cnt // 2, base + cnt}
    return sorted(c for c in out if c >= 0)


def census(case, capacity, meshlets):
    """The classes of CLASSES that expanding `case` at `capacity` exercises."""
    n, S, masks = case.n, case.S, case.records["mask"][:case.n]
    blocks = lambda x: (x + BLOCK - 1) // BLOCK  # noqa: E731
    chunks = _chunks_with_survivors(case)
    cut = 0 < capacity < S
    out = set()
    if n and bool((masks == 0).any()):
        out.add("empty_records")
    if any(cnt == 32 * CHUNK and base < capacity for base, cnt in chunks):
        out.add("full_chunk_2048")
    if n > BLOCK:
        out.add("multi_block")
    if n % BLOCK:
        out.add("partial_last_block")
    if cut and any(base < capacity < base + cnt for base, cnt in chunks):
        out.add("cut_inside_chunk")
    if cut and any(base == capacity for base, cnt in chunks):
        out.add("cut_on_chunk_boundary")
    if cut and capacity in {int(case.before[b]) for b in range(BLOCK, n, BLOCK)}:
        out.add("cut_on_block_boundary")
    if capacity == 0:
        out.add("capacity_zero")
    if S <= capacity and max(blocks(capacity), 1) < blocks(n):  # (a launch has at least one workgroup)
        out.add("fits_but_fewer_grid_blocks_than_record_blocks")
    if S == 1 and capacity >= 1 and masks[-1] != 0:
        out.add("single_survivor_in_last_record")
    entry, bit = mask_bits(masks)
    m = meshlets[(case.records["meshlet_offset"][entry].astype(np.int64) + bit)[:min(S, capacity)]]
    if bool((m["data_offset"].astype(np.uint64) + m["vertex_count"] >= np.uint64(1 << 32)).any()):
        out.add("first_index_wraps")
    return out


# ----------------------------------------------------------------------------------------------------------- scenes
KEEPS = (0.05, 0.02)


def dense_scene():
    """The scene of test_visible_record_lists_expand_to_the_canonical_list: about 1.8 survivors per record."""
    return sc.make_scene(31, 2600, meshlets_per_mesh=(1, 70), lods=2)


def sparse_scene(keep):
    """dense_scene with all meshlets but a share of `keep` moved out of every view: most records of a cull of it are
    empty, and a command buffer sized for what survives has fewer 1024-command blocks than the list has record blocks."""
    scene = dense_scene()
    away = sc.rnd_f32(7, 1, np.arange(len(scene.meshlets))) >= np.float32(keep)
    scene.meshlets["bounding_sphere"][away, :3] += np.float32(1e6)
    return scene


def scene_cull_info():
    cam = sc.default_camera(rot=(0.2, 0.4))
    return sc.make_cull_info(cam.view, cam.planes, alpha_mode_flag=L.ALPHA_ALL)


def scene_case(name, want, n_meshlets):
    """The Case of a record list `want` (VISIBLE_RECORD entries) that came out of a cull."""
    return with_tail(name, want["entity_index"], want["meshlet_offset"], want["mask"], n_meshlets)
