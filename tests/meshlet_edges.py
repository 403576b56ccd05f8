"""The meshlet stage at its tile, group, scan-chunk and ticket edges: the cases.

orbit_meshlet_cull is evaluation (orbit_amd/csrc/meshlet_eval.hip) -> scan -> emit (meshlet_emit.hip) or the list launches
(meshlet_lists.hip), and everything between them is launch arithmetic over the RECORD COUNT: wave tiles of 16 records,
chain-emit groups of 2 tiles, scan chunks of 1024 tiles, a static grid-stride share and atomic tickets behind it.  The
scenes of the other suites reach it with whatever record counts and survivor densities their entity stage leaves; here
the MeshletDispatchBuffer is built by hand.  Every size is derived from ONE table (`K`) that
tests/test_meshlet_edges_cpu.py holds against the constants in the source text; that module holds the reference side to
account (the planting, the census floors, oracle == numpy restatement), tests/test_meshlet_edges_gpu.py runs the cases.

The planting.  4096 meshlets, each either a KEEP meshlet (a small sphere in front of scenes.default_camera(), cone_axis 0,
cone_cutoff 127: it survives pass 0) or an AWAY meshlet (the same sphere moved by 1e6: culled), laid out in regions —
all keep, all away, the boundaries between them, seeded densities.  Records alias this one buffer: a record of 32 that
begins k meshlets in front of a keep -> away boundary has exactly k survivors, so per-tile and per-group totals are exact
and a case of 700 000 records needs no more meshlets than one of 17.  One table of identity entities, ALPHA_ALL.

Two layouts of the same meshlets: "scattered" (arbitrary vertex_offset / data_offset, some within 1000 of 2^32: what the
payload emit copies) and "chain" (data_offset / vertex_offset follow the upload chain whose link bits the derived streams
keep, kernels.h MeshletStreamView, with breaks planted where the chain emit's cases meet: tests/test_meshlet_stream_gpu.py
_relayout is the precedent).
"""
import numpy as np

import scenes as sc
from orbit_amd import layouts as L

# ------------------------------------------------------------------------------------------------------- the table
K = dict(
    kTileRecords=16,       # kernels.h: dispatch records per wave tile
    kGroupTiles=2,         # meshlet_emit.hip: tiles per group of the chain emit
    kScanChunk=1024,       # kernels.h: tiles per scan chunk
    kPayloadCap=128,       # meshlet_common.h: survivors per tile whose payload the evaluation keeps
    kTicketPools=8,        # kernels.h: tile-ticket counters of the evaluation
    kEmitTicketPools=16,   # kernels.h: group-ticket counters of the chain emit
    kDynGroups=16,         # meshlet_emit.hip: ticketed groups a wave takes inside its pipelined loop
    kSlowWords=16,         # meshlet_emit.hip: 32 iterations each a wave can mark as slow
    kEvWaves=4,            # meshlet_eval.hip: waves per evaluation workgroup
    kEvWavesPerSimd=4,     # meshlet_eval.hip: resident waves per SIMD of the evaluation ...
    ORBIT_EV_WPS0=5,       # ... and of pass 0 from the derived streams on a long launch
    kChainWavesPerSimd=4,  # meshlet_emit.hip: resident waves per SIMD of the chain emit (4 waves a workgroup)
)
TRIP = 64               # commands a wave of either emit writes per trip (a lane a command)
CHAIN_FAST_MAX = 128    # meshlet_emit.hip `slow = n > 128u`: the FAST loop's two trips; a fuller group is redone (!FAST)
TILE = K["kTileRecords"]
GROUP = K["kGroupTiles"] * TILE
CHUNK = K["kScanChunk"] * TILE  # records per scan chunk
LANES = 32                      # MESHLET_DISPATCH_SIZE
NUM_CUS = (256, 304, 64)        # the MI355X and two other parts: a table written for one must not hide a class on another


def ceil_div(a, b):
    return (a + b - 1) // b


def tiles_of(records):
    return ceil_div(records, TILE)


def eval_grid(num_cus, dispatch_capacity, occlusion_pass, stream):
    """Workgroups of the evaluation launch (meshlet_eval.hip eval_grid): sized from the CAPACITY, not the count."""
    max_tiles = tiles_of(dispatch_capacity)
    wps = K["ORBIT_EV_WPS0"] if (occlusion_pass == 0 and stream) else K["kEvWavesPerSimd"]
    if wps > K["kEvWavesPerSimd"] and max_tiles < 8 * num_cus * wps * K["kEvWaves"]:
        wps = K["kEvWavesPerSimd"]
    return max(min(num_cus * wps, ceil_div(max_tiles, K["kEvWaves"])), 1)


def eval_stride(num_cus, dispatch_capacity, occlusion_pass, stream):
    """T: the evaluation's wave stride in tiles."""
    return eval_grid(num_cus, dispatch_capacity, occlusion_pass, stream) * K["kEvWaves"]


def eval_n_static(ntiles, stride):
    """Claims of a wave that are static tiles (claim k -> tile k * stride + wave); None: all of them (no ticket drawn)."""
    if ntiles <= stride:
        return None
    full_rounds = ntiles // stride
    dyn_rounds = min(max(full_rounds // 4, 1), 3)
    return max(full_rounds - dyn_rounds if full_rounds >= dyn_rounds else 0, 3)


def chain_grid(num_cus, dispatch_capacity):
    """Workgroups of the chain emit (meshlet_emit.hip launch_meshlet_emit, stream = true)."""
    eneed = ceil_div(tiles_of(dispatch_capacity), 4)
    gneed = ceil_div(eneed, K["kGroupTiles"])
    per_wave = 32 * K["kSlowWords"] - K["kDynGroups"]
    return max(min(num_cus * K["kChainWavesPerSimd"], gneed), ceil_div(gneed, per_wave), 1)


def chain_stride(num_cus, dispatch_capacity):
    """G: the chain emit's wave stride in groups."""
    return chain_grid(num_cus, dispatch_capacity) * 4


def chain_n_static(ngroups, stride):
    """Iterations of a wave that are static groups; None: all of them."""
    full_rounds = ngroups // stride
    if full_rounds < 4:
        return None
    return max(full_rounds - min(max(full_rounds // 4, 1), 3), 4)


# --------------------------------------------------------------------------------------------------- the meshlet buffer
N_MESHLETS = 4096
N_ENTITIES = 5
N_MATERIALS = 7
SEED = 131
# regions [begin, end): what a record reads depends only on where it begins
KEEP_A = (0, 1024)      # all keep; the chain layout's planted breaks lie here
AWAY = (1024, 2048)     # all away: a record of 32 at 1024 - k has its k survivors in lanes 0 .. k - 1
KEEP_C = (2048, 3072)   # all keep: a record of 32 at 2016 + k has its k survivors in lanes 32 - k .. 31
HALF = (3072, 3584)     # seeded, a keep with probability 1 / 2
SPARSE = (3584, 4096)   # seeded, a keep with probability 1 / 16
# chain breaks inside records that begin on a multiple of 32 in KEEP_A (meshlet index: the record at 32 has one at its
# lane 1, the one at 64 at lane 31, the one at 128 in the middle, the one at 160 two — keep meshlets behind the second)
BREAKS_IN_RECORD = {32: (1,), 64: (31,), 128: (16,), 160: (10, 20)}
BREAK_EVERY = 256       # ... and an allocation boundary on every 256th meshlet: +32 runs continue up to there

_cache = {}


def keep_flags():
    """bool[4096]: the keep meshlets."""
    i = np.arange(N_MESHLETS)
    keep = np.zeros(N_MESHLETS, bool)
    keep[KEEP_A[0]:KEEP_A[1]] = keep[KEEP_C[0]:KEEP_C[1]] = True
    keep[HALF[0]:HALF[1]] = sc.rnd_f32(SEED, 1, i[HALF[0]:HALF[1]]) < np.float32(0.5)
    keep[SPARSE[0]:SPARSE[1]] = sc.rnd_f32(SEED, 2, i[SPARSE[0]:SPARSE[1]]) < np.float32(1.0 / 16.0)
    return keep


def chain_breaks():
    """bool[4096]: meshlet i does NOT continue meshlet i - 1's chain (the chain layout)."""
    brk = np.zeros(N_MESHLETS, bool)
    brk[::BREAK_EVERY] = True
    for rec, lanes in BREAKS_IN_RECORD.items():
        for region in (KEEP_A[0], HALF[0]):
            brk[[region + rec + l for l in lanes]] = True
    return brk


def meshlet_buffer(layout):
    """The 4096 planted meshlets; layout "scattered" or "chain" (their bounds, cones, materials and counts are the same)."""
    if ("meshlets", layout) in _cache:
        return _cache["meshlets", layout]
    i = np.arange(N_MESHLETS)
    m = np.zeros(N_MESHLETS, dtype=L.MESHLET)
    # in front of the camera at (0, 2, 0) looking down -z, 90 degrees: |x| <= 4, |y - 2| <= 2 at a distance of 6 .. 30
    m["bounding_sphere"][:, 0] = sc.rnd_range(SEED, 3, i, -4.0, 4.0)
    m["bounding_sphere"][:, 1] = sc.rnd_range(SEED, 4, i, 0.0, 4.0)
    m["bounding_sphere"][:, 2] = sc.rnd_range(SEED, 5, i, -30.0, -6.0)
    m["bounding_sphere"][:, 3] = sc.rnd_range(SEED, 6, i, 0.2, 0.6)
    m["bounding_sphere"][~keep_flags(), 0] += np.float32(1e6)
    m["cone_axis"] = 0
    m["cone_cutoff"] = 127
    m["material_index"] = sc.rnd_int(SEED, 7, i, 0, N_MATERIALS - 1).astype(np.uint16)
    m["vertex_count"] = np.where(i % 4 == 1, 255, sc.rnd_int(SEED, 8, i, 0, 255)).astype(np.uint8)
    m["triangle_count"] = np.where(i % 4 == 2, 255, sc.rnd_int(SEED, 9, i, 0, 255)).astype(np.uint8)
    if layout == "scattered":
        m["vertex_offset"] = (sc.rnd_u64(SEED, 10, i) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        near = (np.uint64(1 << 32) - np.uint64(1) - sc.rnd_int(SEED, 11, i, 0, 999).astype(np.uint64)).astype(np.uint32)
        m["data_offset"] = np.where(i % 8 == 3, near, (sc.rnd_u64(SEED, 12, i) & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    elif layout == "chain":
        # meshlet_data_words (kernels.h): the vertex indices, then the triangle bytes rounded up to words
        size = m["vertex_count"].astype(np.int64) + (m["triangle_count"].astype(np.int64) * 3 + 3) // 4
        brk = chain_breaks()
        gap = np.where(brk, sc.rnd_int(SEED, 13, i, 1, 5000), 0)
        data = np.cumsum(gap) + np.concatenate([[0], np.cumsum(size)[:-1]]) + 0xFFFF0000  # wraps past 2^32 on the way
        m["data_offset"] = (data & 0xFFFFFFFF).astype(np.uint32)
        m["vertex_offset"] = (sc.rnd_u64(SEED, 14, np.cumsum(brk)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    else:
        raise ValueError(layout)
    _cache["meshlets", layout] = m
    return m


def link_bits():
    """bool[4096] of the chain layout, as kernels.h defines the link bit: this meshlet's vertex_offset equals its
    predecessor's and its data_offset is the predecessor's plus the predecessor's data size."""
    m = meshlet_buffer("chain")
    size = m["vertex_count"].astype(np.uint32) + (m["triangle_count"].astype(np.uint32) * 3 + 3) // 4
    link = np.zeros(N_MESHLETS, bool)
    link[1:] = (m["vertex_offset"][1:] == m["vertex_offset"][:-1]) & \
               (m["data_offset"][1:] == m["data_offset"][:-1] + size[:-1])
    return link


def entities():
    e = np.zeros(N_ENTITIES, dtype=L.ENTITY_DATA)
    e["model_matrix"] = e["normal_matrix"] = np.eye(4, dtype=np.float32).reshape(-1)
    return e


def materials():
    """Seven materials, all three alpha modes: with ALPHA_ALL every one of them is drawn, and a stream's alpha classes
    (orbit_meshlet_stream_set_materials) hold no class 3."""
    m = np.zeros(N_MATERIALS, dtype=L.MATERIAL)
    m["alpha_mode"] = np.arange(N_MATERIALS) % 3
    return m


def camera():
    return sc.default_camera()


SCREEN = (128, 72)    # -> a 64 x 64 pyramid
PYRAMID = (64, 64)


def pyramid(oracle, kind):
    """"zero": nothing occludes (reverse Z: 0 is the far plane); "depth": oracle.depth_reduce of scenes.make_depth."""
    if ("pyr", kind) not in _cache:
        W, H = SCREEN
        depth = sc.make_depth(217, W, H, camera(), n_occluders=192)
        pyr, d = oracle.depth_reduce(depth, W, H)
        assert (d.width, d.height) == PYRAMID
        _cache["pyr", "depth"] = pyr
        _cache["pyr", "zero"] = np.zeros_like(pyr)
    return _cache["pyr", kind]


def cull_info(occlusion_pass):
    cam = camera()
    return sc.make_cull_info(cam.view, cam.planes, occlusion_pass=occlusion_pass, alpha_mode_flag=L.ALPHA_ALL,
                             p00=cam.p00, p11=cam.p11, z_near=cam.z_near)


# ------------------------------------------------------------------------------------------------------------ records
TAIL = 48  # full records over keep meshlets behind entry n (and up to the capacity): a read past n shows up as commands
SMALL = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
CHUNKS = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
# survivors of consecutive tiles of the "steps" density: one trip, the second trip by one, the payload's cap, the dense
# rebuild by one — and behind them a group of exactly 128 and one of 129
STEPS = (64, 65, 128, 129, 64, 64, 64, 65)


def _u(seed, stream, idx, lo, hi):
    return sc.rnd_int(seed, stream, idx, lo, hi)


def _boundary(i, k):
    """A record of 32 with exactly k survivors: even records in front of keep -> away (survivors in the low lanes), odd
    ones in front of away -> keep (in the high lanes)."""
    return np.where(i % 2 == 0, AWAY[0] - k, KEEP_C[0] - LANES + k)


def _density(name, n):
    """(meshlet_offset, meshlet_count) of the n records of a planted density."""
    i = np.arange(n)
    away = AWAY[0] + (i * 7) % (AWAY[1] - AWAY[0] - LANES)  # unaligned offsets, all culled
    full = KEEP_A[0] + LANES * (i % 32)                       # aligned, + 32 runs of 32 records, every break planted
    c32 = np.full(n, LANES)
    if name == "zero":      # no survivor anywhere; every count from 0 to 32
        return away, i % 33
    if name == "full":      # 512 per tile, 1024 per group: the dense rebuild, every group slow
        return full, c32
    if name == "steps":     # tiles of exactly 64, 65, 128, 129 survivors; groups of exactly 128 and 129
        per_tile = np.array(STEPS)[(i // TILE) % len(STEPS)]
        k = per_tile // TILE + ((i % TILE) == TILE - 1) * (per_tile % TILE)
        return _boundary(i, k), c32
    if name == "last_only":  # a single survivor, in the last record
        return np.where(i == n - 1, AWAY[0] - 1, away), np.where(i == n - 1, LANES, 1 + i % 32)
    if name == "alternating":  # full and empty records in turn
        return np.where(i % 2 == 0, KEEP_A[0] + LANES * ((i // 2) % 32), away), c32
    if name == "empty_tile":   # an empty tile between full ones
        return np.where((i // TILE) % 3 == 1, away, full), c32
    if name == "chunk1_first":  # the first tile of chunk 1 holds the only survivors
        inside = (i >= CHUNK) & (i < CHUNK + TILE)
        return np.where(inside, KEEP_C[0] + LANES * (i % TILE), away), np.where(inside, LANES, i % 33)
    if name == "breaks":  # four full records a group (exactly 128) over the planted breaks; the rest empty
        return np.where(i % 8 == 0, KEEP_A[0] + LANES * ((i // 8) % 8), away), np.where(i % 8 == 0, LANES, i % 33)
    if name == "mixed":   # seeded: runs of + 32 from aligned and unaligned starts anywhere, short and empty records
        run = i // 6
        start = _u(SEED, 20, run, 0, N_MESHLETS - 7 * LANES)
        start = np.where(_u(SEED, 21, run, 0, 1) == 0, start & ~31, start)
        cnt = np.where(_u(SEED, 22, i, 0, 7) == 0, _u(SEED, 23, i, 0, 31), LANES)
        return start + LANES * (i % 6), cnt
    raise ValueError(name)


DENSITIES = ("zero", "full", "steps", "last_only", "alternating", "empty_tile", "chunk1_first", "breaks", "mixed")


def _short(n, variant=0):
    """The large cases: records of 0 .. 4 meshlets anywhere, every 64th one full — under two million lanes.  Two
    variants differ in every record: what one cull leaves in the context's scratch is wrong for the other."""
    i = np.arange(n)
    off = _u(SEED, 30 + variant, i, 0, N_MESHLETS - LANES)
    cnt = (i + 2 * variant) % 5
    big = i % 64 == 63
    return np.where(big, KEEP_A[0] + LANES * ((i // 64) % 32), off), np.where(big, LANES, cnt)


class Case:
    """n hand-built MESHLET_DISPATCH records and, behind them, full records over keep meshlets up to `room` records:
    entity indices vary, visibility_offset = the record's index (one word each: no two records share a word)."""

    def __init__(self, name, offset, count, room=None, kind="small"):
        n = len(offset)
        self.name, self.n, self.kind = name, n, kind
        self.room = max(n + TAIL, room or 0)
        i = np.arange(self.room)
        r = np.zeros(self.room, dtype=L.MESHLET_DISPATCH)
        r["entity_index"] = _u(SEED, 40, i, 0, N_ENTITIES - 1)
        r["meshlet_offset"] = KEEP_C[0] + LANES * (i % 31)
        r["meshlet_count"] = LANES
        r["meshlet_offset"][:n], r["meshlet_count"][:n] = offset, count
        r["visibility_offset"] = i
        assert int((r["meshlet_offset"].astype(np.int64) + LANES).max()) <= N_MESHLETS
        self.records = r
        keep = keep_flags()
        lane = np.arange(LANES)
        bits = keep[r["meshlet_offset"][:n, None].astype(np.int64) + lane] & (lane < r["meshlet_count"][:n, None])
        self.masks = (bits.astype(np.uint64) << lane.astype(np.uint64)).sum(axis=1).astype(np.uint32)  # pass 0, planted
        self.pops = bits.sum(axis=1).astype(np.int64)
        self.before = np.concatenate([[0], np.cumsum(self.pops)]).astype(np.int64)  # survivors in front of record i

    def __repr__(self):
        return self.name

    def survivors(self, records=None):
        return int(self.before[self.n if records is None else min(records, self.n)])

    def buffer(self, header=None):
        """The MeshletDispatchBuffer's bytes: all `room` records, the header claiming `header` of them (default n)."""
        buf = L.make_dispatch_buffer(self.records)
        buf[:4].view("<u4")[0] = self.n if header is None else header
        return buf

    def words(self, how):
        """The meshlet visibility words, one per record of the buffer and three more: zero or seeded."""
        if how == "zero":
            return np.zeros(self.room + 3, np.uint32)
        return (sc.rnd_u64(SEED, 50 + self.n % 7, np.arange(self.room + 3)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def small_case(density, n):
    key = f"{density}_{n}"
    if key not in _cache:
        off, cnt = _density(density, n)
        _cache[key] = Case(key, off, cnt, room=4 * n, kind="chunk" if n >= CHUNK - 1 else "small")
    return _cache[key]


def plan():
    """{name: (density, n)} of the small and chunk cases: every density at every count it can show at (the first tile of
    chunk 1 needs more than a chunk)."""
    out = {}
    for n in SMALL + CHUNKS:
        for d in DENSITIES:
            if d == "chunk1_first" and n <= CHUNK:
                continue
            if n == 0 and d != "zero":
                continue
            out[f"{d}_{n}"] = (d, n)
    return out


PLAN = plan()
# the cases every capacities() pair is run at: between them they carry every cut class
CUT_CASES = ("steps_65", "full_33", "mixed_64", "breaks_64", "steps_16385", "alternating_32769")


def case(name):
    return small_case(*PLAN[name])


def eval_sizes(num_cus):
    """Record counts around the evaluation's first ticket, T = its wave stride in tiles on this part (capacity = count:
    a launch this long runs kEvWavesPerSimd waves per SIMD whatever its pass and source — 8 T tiles stay below the
    8 x CUs x 5 x 4 tiles at which pass 0 from the streams takes the fifth)."""
    T = num_cus * K["kEvWavesPerSimd"] * K["kEvWaves"]
    sizes = (TILE * 3 * T, TILE * 3 * T + 1, TILE * 4 * T + 17, TILE * 8 * T)
    assert all(eval_stride(num_cus, n, 0, s) == T for n in sizes for s in (False, True))
    return sizes


def chain_sizes(num_cus):
    """Record counts around the chain emit's first ticket, G = its wave stride in groups on this part."""
    G = num_cus * K["kChainWavesPerSimd"] * 4
    sizes = (GROUP * 4 * G, GROUP * 4 * G + GROUP, GROUP * 5 * G + GROUP + 1)
    assert all(chain_stride(num_cus, n) == G for n in sizes)
    return sizes


def device_case(kind, n, num_cus, variant=0):
    """A device-derived case of short records.  The chain-emit cases carry one full group (1024 survivors, every planted
    break: slow) at the first ticketed group — or, where no group is ticketed, at the last one."""
    key = f"{kind}_{n}_cus{num_cus}_v{variant}"
    if key not in _cache:
        off, cnt = _short(n, variant)
        if kind == "chain":
            G = chain_stride(num_cus, n)
            g = min(4 * G, ceil_div(n, GROUP) - 1)
            at = np.arange(g * GROUP, min((g + 1) * GROUP, n))
            off[at], cnt[at] = KEEP_A[0] + LANES * (at % 32), LANES
        c = Case(key, off, cnt, kind=kind)
        c.full_group = g if kind == "chain" else None
        _cache[key] = c
    return _cache[key]


# ------------------------------------------------------------------------------------------- outputs from one set of masks
def masks_of_task_records(task):
    """The should-draw ballot of every MESH_TASK_RECORD: its first task_mesh_count lane indices."""
    idx, cnt = task["meshlet_indices"].astype(np.uint64), task["task_mesh_count"]
    live = np.arange(LANES)[None, :] < cnt[:, None]
    return ((np.uint64(1) << idx) * live).sum(axis=1).astype(np.uint32)


def record_list_of(task):
    """(12-B entries, survivors) of the record list of a cull whose task records are `task`."""
    out = np.zeros(len(task), dtype=L.VISIBLE_RECORD)
    out["entity_index"], out["meshlet_offset"] = task["entity_index"], task["meshlet_offset"]
    out["mask"] = masks_of_task_records(task)
    return out, int(task["task_mesh_count"].sum())


# ---------------------------------------------------------------------------------------------------------- capacities
def _tile_sums(c, records):
    pops = np.zeros(tiles_of(records) * TILE, np.int64)
    pops[:records] = c.pops[:records]
    cnt = pops.reshape(-1, TILE).sum(axis=1)
    return cnt, np.concatenate([[0], np.cumsum(cnt)])[:-1]


def dispatch_capacities(c):
    """n, n + 1, n rounded up to a tile, 4 n, and n - 1 with the header still saying n."""
    n = c.n
    return sorted({n, n + 1, tiles_of(n) * TILE, 4 * n, max(n - 1, 0)})


def draw_capacities(c, records=None):
    """S + 8, S, S - 1 and 0; in the first and the last tile with survivors a cut at a multiple of 64 with its two
    neighbours and the end of the tile's first trip with its; a cut on the first tile boundary, on the first group
    boundary, and the survivors in front of chunk 1."""
    records = c.n if records is None else min(records, c.n)
    S = c.survivors(records)
    out = {S + 8, S, S - 1, 0}
    cnt, base = _tile_sums(c, records)
    have = np.flatnonzero(cnt)
    for t in list(have[:1]) + list(have[-1:]):
        b, k = int(base[t]), int(cnt[t])
        m = (b // TRIP + 1) * TRIP
        if m < b + k:
            out |= {m - 1, m, m + 1}
        if k > TRIP:
            out |= {b + TRIP - 1, b + TRIP, b + TRIP + 1}
    later = [int(t) for t in have if base[t] > 0]
    on_tile = [t for t in later if t % K["kGroupTiles"]]
    on_group = [t for t in later if t % K["kGroupTiles"] == 0 and t % K["kScanChunk"]]
    out |= {int(base[t]) for t in on_tile[:1] + on_group[:1]}
    if records > CHUNK:
        out.add(int(c.before[CHUNK]))
    return sorted(x for x in out if x >= 0)


def capacities(c):
    """(dispatch capacity, draw capacity) pairs: every dispatch capacity with room for all its survivors, every draw
    capacity at dispatch capacity n."""
    pairs = [(d, c.survivors(d) + 8) for d in dispatch_capacities(c)]
    pairs += [(c.n, k) for k in draw_capacities(c)]
    return sorted(set(pairs))


# -------------------------------------------------------------------------------------------------------------- census
PAYLOAD_CLASSES = ("one_trip", "two_trips", "dense_rebuild", "full_tile_512", "empty_tile")
CHAIN_CLASSES = ("group_128", "group_129_slow", "second_break_slow", "chain_continues", "chain_starts_unaligned",
                 "chain_starts_aligned")
RECORD_CLASSES = ("count_zero_record", "partial_record", "partial_last_tile", "odd_tile_count", "header_above_capacity")
SCAN_CLASSES = ("two_chunks", "three_chunks")
CUT_CLASSES = ("cut_inside_trip", "cut_on_tile", "cut_on_group", "cut_on_chunk", "capacity_zero")
TICKET_CLASSES = ("eval_tickets_none_taken", "eval_one_ticketed_tile", "eval_ticketed_round", "emit_ticketed_groups",
                  "emit_slow_group_ticketed")
CLASSES = PAYLOAD_CLASSES + CHAIN_CLASSES + RECORD_CLASSES + SCAN_CLASSES + CUT_CLASSES + TICKET_CLASSES


def chain_flags(c, records):
    """Per record of the first `records`, as meshlet_emit.hip chain_stage decides them from the chain layout's link bits
    and the reference's masks: (has survivors, continues its predecessor's chain, a survivor lies behind a second broken
    link of its record)."""
    r, masks = c.records[:records], c.masks[:records]
    link = link_bits()
    lane = np.arange(LANES)
    lk = link[r["meshlet_offset"][:, None].astype(np.int64) + lane]  # [record, lane]
    has = (masks != 0) & (r["meshlet_count"] != 0)
    full = has & (r["meshlet_count"] == LANES) & lk[:, 1:].all(axis=1)
    first = np.arange(records) % GROUP == 0
    prev_full = np.concatenate([[False], full[:-1]])
    prev_y = np.concatenate([[0], r["meshlet_offset"][:-1].astype(np.int64)])
    cont = has & ~first & prev_full & (r["meshlet_offset"] == prev_y + LANES) & lk[:, 0]
    broken = ~lk
    broken[:, 0] = False
    nbreaks = np.cumsum(broken, axis=1)  # broken links among lanes 1 .. l
    bits = ((masks[:, None] >> lane.astype(np.uint32)) & 1).astype(bool)
    second = (bits & (nbreaks >= 2)).any(axis=1)
    return has, cont, second


def census(c, capacity, layout, num_cus, occlusion_pass=0):
    """The classes of CLASSES that a pass-0 cull of `c` at capacity = (dispatch capacity, draw capacity) exercises — from the
    reference's masks alone (Case.masks: the planting, which tests/test_meshlet_edges_cpu.py holds against the oracle's
    task records).  layout "chain": the derived streams are bound (the chain emit writes the commands), else the payload
    emit does; the ticket classes are those of a part with `num_cus` compute units."""
    cap_d, cap_c = capacity
    records = min(c.n, cap_d)
    ntiles = tiles_of(records)
    out = set()
    cnt, base = _tile_sums(c, records) if records else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    stream = layout == "chain"
    if not stream:
        for name, sel in (("one_trip", (cnt >= 1) & (cnt <= TRIP)), ("two_trips", (cnt > TRIP) & (cnt <= K["kPayloadCap"])),
                          ("dense_rebuild", cnt > K["kPayloadCap"]), ("full_tile_512", cnt == TILE * LANES),
                          ("empty_tile", cnt == 0)):
            if bool(sel.any()):
                out.add(name)
    ngroups = ceil_div(ntiles, K["kGroupTiles"])
    gcnt = np.zeros(ngroups * K["kGroupTiles"], np.int64)
    gcnt[:ntiles] = cnt
    gcnt = gcnt.reshape(-1, K["kGroupTiles"]).sum(axis=1)
    slow = np.zeros(ngroups, bool)
    if stream and records:
        has, cont, second = chain_flags(c, records)
        sec = np.zeros(ngroups * GROUP, bool)
        sec[:records] = second
        sec = sec.reshape(-1, GROUP).any(axis=1)
        slow = (gcnt > CHAIN_FAST_MAX) | sec
        start = has & ~cont
        aligned = c.records["meshlet_offset"][:records] % 32 == 0
        for name, sel in (("group_128", gcnt == CHAIN_FAST_MAX), ("group_129_slow", gcnt == CHAIN_FAST_MAX + 1),
                          ("second_break_slow", sec & (gcnt <= CHAIN_FAST_MAX)),
                          ("chain_continues", cont), ("chain_starts_unaligned", start & ~aligned),
                          ("chain_starts_aligned", start & aligned)):
            if bool(sel.any()):
                out.add(name)
    counts = c.records["meshlet_count"][:records]
    if bool((counts == 0).any()):
        out.add("count_zero_record")
    if bool(((counts > 0) & (counts < LANES)).any()):
        out.add("partial_record")
    if records % TILE:
        out.add("partial_last_tile")
    if ntiles % K["kGroupTiles"]:
        out.add("odd_tile_count")
    if c.n > cap_d:
        out.add("header_above_capacity")
    nchunks = ceil_div(ntiles, K["kScanChunk"])
    if nchunks in (2, 3):
        out.add("two_chunks" if nchunks == 2 else "three_chunks")
    S = int(cnt.sum())
    if 0 < cap_c < S:
        if bool(((base < cap_c) & (cap_c < base + cnt)).any()):
            out.add("cut_inside_trip")
        t = np.flatnonzero((base == cap_c) & (cnt > 0))
        if len(t) and t[0] % K["kGroupTiles"]:
            out.add("cut_on_tile")
        if len(t) and t[0] % K["kGroupTiles"] == 0 and t[0] % K["kScanChunk"]:
            out.add("cut_on_group")
        if len(t) and t[0] and t[0] % K["kScanChunk"] == 0:
            out.add("cut_on_chunk")
    if cap_c == 0:
        out.add("capacity_zero")
    # ---- tickets (passes 0 and 2: pass 1 walks a plain grid stride)
    if occlusion_pass != 1 and records:
        stride = eval_stride(num_cus, cap_d, occlusion_pass, stream)
        n_static = eval_n_static(ntiles, stride)
        if n_static is not None:
            ticketed = ntiles - n_static * stride
            if ticketed <= 0:
                out.add("eval_tickets_none_taken")  # every ticket drawn lies past the end
            elif ticketed == 1:
                out.add("eval_one_ticketed_tile")
            elif ticketed >= stride:
                out.add("eval_ticketed_round")
        if stream:
            gstride = chain_stride(num_cus, cap_d)
            g_static = chain_n_static(ngroups, gstride)
            if g_static is not None and ngroups > g_static * gstride:
                out.add("emit_ticketed_groups")
                if bool(slow[g_static * gstride:].any()):
                    out.add("emit_slow_group_ticketed")
    return out
