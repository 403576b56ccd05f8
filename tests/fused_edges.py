"""The one-launch cull at its shape, bisection, tile and look-back edges: the cases.

orbit_cull_views sends every view of at most 16 384 entity-draws through ONE launch (orbit_amd/csrc/cull_fused.hip) that
makes its own dispatch records, so a case here is a SCENE, not a dispatch buffer: entity-draws over meshes whose LOD 0 is
a (meshlet_offset, meshlet_count) range aliased into the 4096 planted keep / away meshlets of tests/meshlet_edges.py.  A
"drawn" mesh has a bounding sphere in front of the camera (it passes every plane and an all-zero pyramid), a "culled"
one has it moved by 1e6 and yields no record, an "empty" one is drawn with meshlet_count 0 and yields none either.  A
drawn mesh of count 32 at AWAY[0] - k yields one record of exactly k survivors; one of count 32 m + j yields m + 1
records, the last of j lanes.  Records, per-record survivors, per-tile totals and prefix sums are derived on the host
from meshlet_edges.keep_flags(); tests/test_fused_edges_cpu.py holds them against the oracle, holds the table below
against the source text, restates the launcher's shape selection and counts what every case reaches;
tests/test_fused_edges_gpu.py runs the cases.
"""
import numpy as np

import meshlet_edges as me
import scenes as sc
from orbit_amd import layouts as L

# ------------------------------------------------------------------------------------------------------- the table
K = dict(
    kEntityBlock=256,             # kernels.h: entity-draws per chunk, threads per workgroup
    kFusedWaves=4,                # cull_fused.hip: waves per workgroup
    kFusedLocalChunks=3,          # cull_fused.hip: views of at most this many chunks, passes 0 / 1: the local entity stage
    kFusedSmallEntityDraws=4096,  # cull_fused.hip: views of at most this many draws take the 2-row tiles
    kFusedMaxEntityDraws=16384,   # kernels.h: larger views leave the one-launch cull (unless cull_path = 2)
    kFusedSyncWords=160,          # kernels.h: the sync words the last workgroup out zeroes
)
TILE_RECORDS = {2: 4, 8: 16}      # fused_tile_records(rows) = 2 x rows: records per tile of the 2-row and the 8-row shape
LOOK_BACK = 64                    # tiles_before: tiles a look-back step reads (a lane a tile)
TRIP = 64                         # commands a wave writes per trip (a lane a command)
LOCAL_OFFSETS = 1024              # LocalEntityLds::off: ten bisection steps
CHUNK = K["kEntityBlock"]
LOCAL_MAX = K["kFusedLocalChunks"] * CHUNK
SMALL_MAX = K["kFusedSmallEntityDraws"]
LANES = 32
SLACK = 40                        # drawn entity-draws behind N in every scene's array: the header can claim them
PAD_WORDS = 3                     # words behind both bitsets: compared too, never written
SEED = 977
DRAWN, CULLED = 0, 1
PYRAMID = me.PYRAMID


def ceil_div(a, b):
    return (a + b - 1) // b


def chunks_of(n):
    return ceil_div(n, CHUNK)


def shape_of(n, occlusion_pass):
    """`want` of launch_cull_fused_views: 0 = the local entity stage (2-row tiles), 1 = 2-row tiles, 2 = 8-row tiles."""
    if chunks_of(n) <= K["kFusedLocalChunks"] and occlusion_pass != 2:
        return 0
    return 1 if n <= K["kFusedSmallEntityDraws"] else 2


def rows_of(shape):
    return 8 if shape == 2 else 2


def fused_grid(entity_draw_count, rows, num_cus, views):
    """fused_grid of cull_fused.hip: workgroups per view of a launch whose largest view has `entity_draw_count` draws."""
    chunks = chunks_of(entity_draw_count)
    waves = ceil_div(entity_draw_count, 2 * rows)
    cap = max(num_cus * (3 if rows == 2 else 2) // max(views, 1), 1)
    return max(min(max(chunks, ceil_div(waves, K["kFusedWaves"])), cap), 1)


def launches(counts, passes, num_cus, grid_cap=0):
    """[(shape, view indices in slot order, grid x)] of one orbit_cull_views call, as launch_cull_fused_views groups it."""
    out = []
    for shape in range(3):
        idx = [j for j, (n, op) in enumerate(zip(counts, passes)) if shape_of(n, op) == shape]
        if idx:
            sized = fused_grid(max(counts[j] for j in idx), rows_of(shape), num_cus, len(idx))
            out.append((shape, idx, min(sized, grid_cap) if grid_cap else sized))
    return out


# ------------------------------------------------------------------------------------------------------------ scenes
def boundary(i, k):
    """meshlet_offset of a record of 32 with exactly k survivors: even ones in front of keep -> away (survivors in the low
    lanes), odd ones in front of away -> keep (in the high lanes)."""
    return np.where(np.asarray(i) % 2 == 0, me.AWAY[0] - k, me.KEEP_C[0] - LANES + k)


class Expect:
    """What a cull of the first `end` draws makes, from the planting alone: the dispatch records in canonical order, each
    record's survivors (pass 0; pass 2 against an all-zero pyramid and zero bitsets) and their prefix sums."""

    def __init__(self, scene, end):
        idx = np.flatnonzero((scene.kind[:end] == DRAWN) & (scene.cnt[:end] > 0))
        per = (scene.cnt[idx] + LANES - 1) // LANES
        own = np.repeat(idx, per)
        j = np.arange(int(per.sum())) - np.repeat(np.cumsum(per) - per, per)
        r = np.zeros(len(own), dtype=L.MESHLET_DISPATCH)
        r["entity_index"] = scene.draws["entity_index"][own]
        r["meshlet_offset"] = scene.off[own] + LANES * j
        r["meshlet_count"] = np.minimum(scene.cnt[own] - LANES * j, LANES)
        r["visibility_offset"] = scene.draws["visibility_offset"][own] + j
        self.records, self.owner, self.end = r, own, end
        lane = np.arange(LANES)
        at = np.minimum(r["meshlet_offset"][:, None].astype(np.int64) + lane, me.N_MESHLETS - 1)
        bits = me.keep_flags()[at] & (lane < r["meshlet_count"][:, None])
        self.masks = (bits.astype(np.uint64) << lane.astype(np.uint64)).sum(axis=1).astype(np.uint32)
        self.pops = bits.sum(axis=1).astype(np.int64)
        self.before = np.concatenate([[0], np.cumsum(self.pops)]).astype(np.int64)
        self.per_draw = np.zeros(end, np.int64)
        self.per_draw[idx] = per

    @property
    def total(self):
        return len(self.records)

    def survivors(self, records=None):
        return int(self.before[self.total if records is None else min(records, self.total)])

    def tiles(self, recs, records=None):
        """(survivors per tile, survivors in front of each tile) for tiles of `recs` records over the first `records`."""
        n = self.total if records is None else min(records, self.total)
        pops = np.zeros(ceil_div(n, recs) * recs, np.int64)
        pops[:n] = self.pops[:n]
        cnt = pops.reshape(-1, recs).sum(axis=1)
        return cnt, np.concatenate([[0], np.cumsum(cnt)])[:-1]


class Scene:
    """N + SLACK entity-draws (kind, meshlet_offset, meshlet_count each; the SLACK ones behind N are drawn records of 7
    survivors), one MeshInfo per distinct triple, the five identity entities of meshlet_edges, each draw's
    visibility_offset on words of its own.  n: the entity_draw_count a call is given."""

    def __init__(self, name, kind, off, cnt):
        n = len(kind)
        i = np.arange(n + SLACK)
        self.name, self.n = name, n
        self.kind = np.concatenate([kind, np.full(SLACK, DRAWN)]).astype(np.int64)
        self.off = np.concatenate([off, np.full(SLACK, me.AWAY[0] - 7)]).astype(np.int64)
        self.cnt = np.concatenate([cnt, np.full(SLACK, LANES)]).astype(np.int64)
        self.off[(self.kind == CULLED) & (self.cnt == 0)] = 0
        assert int((self.off + self.cnt).max()) <= me.N_MESHLETS and int(self.off.min()) >= 0
        rows, inverse = np.unique(np.stack([self.kind, self.off, self.cnt], axis=1), axis=0, return_inverse=True)
        mi = np.zeros(len(rows), dtype=L.MESH_INFO)
        mi["bounding_sphere"] = (0.0, 2.0, -15.0, 1.0)  # in front of meshlet_edges.camera(): inside every plane
        mi["bounding_sphere"][rows[:, 0] == CULLED, 0] += np.float32(1e6)
        mi["aabb_min"][:, :3], mi["aabb_max"][:, :3] = -1.0, 1.0
        mi["lod_count"] = 1
        mi["mesh_lods"][:, 0, 0], mi["mesh_lods"][:, 0, 1] = rows[:, 1], rows[:, 2]
        self.mesh_infos = mi
        words = (self.cnt + LANES - 1) // LANES
        d = np.zeros(n + SLACK, dtype=L.ENTITY_DRAW)
        d["entity_index"] = sc.rnd_int(SEED, 1, i, 0, me.N_ENTITIES - 1)
        d["mesh_index"] = inverse.reshape(-1)
        d["visibility_offset"] = np.concatenate([[0], np.cumsum(words)])[:-1]
        self.draws = d
        self.meshlet_words = int(words.sum())
        self._expect = {}

    def __repr__(self):
        return self.name

    def draw_end(self, header=None):
        """draw_end of the kernels: min(the buffer's count, entity_draw_count rounded up to a chunk)."""
        return min(self.n if header is None else header, chunks_of(self.n) * CHUNK, self.n + SLACK)

    def expect(self, header=None):
        end = self.draw_end(header)
        if end not in self._expect:
            self._expect[end] = Expect(self, end)
        return self._expect[end]

    def draw_buffer(self, header=None):
        return L.entity_draw_buffer(self.draws, self.n if header is None else header)

    def entity_words(self, how, seed=0):
        count = (self.n + SLACK + 31) // 32 + PAD_WORDS
        return _words(count, how, 60 + seed)

    def meshlet_vis_words(self, how, seed=0):
        return _words(self.meshlet_words + PAD_WORDS, how, 70 + seed)

    def header_counts(self):
        return sorted({self.n, max(self.n - SLACK, 0), self.n + SLACK})


def _words(count, how, stream):
    if how == "zero":
        return np.zeros(count, np.uint32)
    if how == "ones":
        return np.full(count, 0xFFFFFFFF, np.uint32)
    return (sc.rnd_u64(SEED, stream, np.arange(count)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def cull_info(occlusion_pass):
    return me.cull_info(occlusion_pass)


# --------------------------------------------------------------------------------------------------- scene builders
def _singles(n, k=None):
    """n drawn draws of one record each, k[i] survivors (default i % 33)."""
    i = np.arange(n)
    k = i % 33 if k is None else np.asarray(k)
    return np.full(n, DRAWN), boundary(i, k), np.full(n, LANES)


def _no_record(kind, off, cnt, at):
    """The draws `at` yield no record: culled and empty ones in turn."""
    at = np.asarray(at)
    kind[at] = np.where(at % 2 == 0, CULLED, DRAWN)
    cnt[at] = np.where(at % 2 == 0, LANES, 0)
    off[at] = np.where(at % 2 == 0, me.KEEP_A[0], 0)


def seeded(n, stream):
    """Drawn (one record of 0 .. 32 survivors, a partial record, or 2 .. 4 records), culled and empty draws by seed: about
    min(0.75, 1800 / n) of them drawn.  The last draw is a drawn record of 5."""
    i = np.arange(n)
    u, v = sc.rnd_f32(SEED, 10 + stream, i), sc.rnd_f32(SEED, 20 + stream, i)
    p = np.float32(min(0.75, 1800.0 / n))
    kind = np.where(u < p + np.float32(0.1), DRAWN, CULLED)
    empty = (u >= p) & (u < p + np.float32(0.1))
    off = boundary(i, sc.rnd_int(SEED, 30 + stream, i, 0, 32))
    cnt = np.full(n, LANES)
    multi, part = v < np.float32(0.15), (v >= np.float32(0.15)) & (v < np.float32(0.25))
    off = np.where(multi | part, me.HALF[0] + sc.rnd_int(SEED, 40 + stream, i, 0, 380), off)
    cnt = np.where(multi, sc.rnd_int(SEED, 50 + stream, i, 33, 100), np.where(part, sc.rnd_int(SEED, 55 + stream, i, 1, 31), cnt))
    cnt = np.where(empty, 0, cnt)
    kind[n - 1], off[n - 1], cnt[n - 1] = DRAWN, me.AWAY[0] - 5, LANES
    return kind, off, cnt


SHAPE_SIZES = (1, 255, 256, 257, 767, 768, 769, 4095, 4096, 4097)
RUNS = (1, 31, 255, 256, 300)
RUN_AT = ("start", "b256", "b512", "end")
FAT_RECORDS = 41                       # meshlet_count 32 x 40 + 7
FAT_COUNT = LANES * 40 + 7
FAT_OFFSET = 1000                      # 24 keep, the 1024 away, then keep: its records differ
FAT_AT = (0, 255, 256, 767)
TOTALS = tuple(4 * t + d for t in (1, 64, 65) for d in (-1, 0, 1))
TILE_COUNTS = (1, 2, 63, 64, 65, 66, 127, 128, 129, 130)
LAST = ("full", "one", "all_but_one")
STEPS = {4: (63, 64, 65, 127, 128), 16: (64, 65, 128, 129, 511, 512)}
DENSITIES = ("zero", "full", "steps", "first_tile_only", "last_tile_only", "tile_64_only", "alternating")
BIG_N = 4097


def _run_range(length, where):
    if where == "start":
        return 0, length
    if where == "end":
        return LOCAL_MAX - length, LOCAL_MAX
    b = 256 if where == "b256" else 512
    lo = max(b - (length + 1) // 2, 1) if length > 1 else b - 1  # (a run of one: the draw in front of the boundary)
    lo = min(lo, LOCAL_MAX - 1 - length)
    return lo, lo + length


def _local(name):
    """The local bisection's scenes: 768 draws (fewer where the name says so)."""
    part = name.split("_")
    if part[1] == "first":
        kind, off, cnt = _singles(LOCAL_MAX)
        _no_record(kind, off, cnt, np.arange(1, LOCAL_MAX))
    elif part[1] == "last":
        kind, off, cnt = _singles(LOCAL_MAX)
        _no_record(kind, off, cnt, np.arange(0, LOCAL_MAX - 1))
    elif part[1] == "every":
        kind, off, cnt = _singles(LOCAL_MAX)
    elif part[1] == "run":
        kind, off, cnt = _singles(LOCAL_MAX)
        _no_record(kind, off, cnt, np.arange(*_run_range(int(part[2]), part[3])))
    elif part[1] == "middle":
        kind, off, cnt = _singles(LOCAL_MAX)
        _no_record(kind, off, cnt, np.arange(CHUNK, 2 * CHUNK))
    elif part[1] == "fat":
        kind, off, cnt = _singles(LOCAL_MAX)
        off[int(part[2])], cnt[int(part[2])] = FAT_OFFSET, FAT_COUNT
    elif part[1] == "total":
        total = int(part[2])
        kind, off, cnt = _singles(LOCAL_MAX)
        drawn = np.zeros(LOCAL_MAX, bool)
        drawn[np.arange(total) * LOCAL_MAX // total] = True
        _no_record(kind, off, cnt, np.flatnonzero(~drawn))
    else:
        raise ValueError(name)
    return kind, off, cnt


def tile_survivors(recs, ntiles, density):
    """Survivors per tile of a density (a full tile has recs x 32)."""
    t = np.arange(ntiles)
    full = recs * LANES
    if density == "zero":
        return np.zeros(ntiles, np.int64)
    if density == "full":
        return np.full(ntiles, full)
    if density == "steps":
        return np.array(STEPS[recs])[t % len(STEPS[recs])]
    if density == "first_tile_only":
        return np.where(t == 0, full, 0)
    if density == "last_tile_only":
        return np.where(t == ntiles - 1, full, 0)
    if density == "tile_64_only":
        return np.where(t == 64, full, 0)
    if density == "alternating":
        return np.where(t % 2 == 0, full, 0)
    raise ValueError(density)


def _tiles(recs, ntiles, density, last, pad):
    """ntiles tiles of `recs` records (the last one full, of one record, or of all but one), one drawn draw a record.
    pad = 0: the draws alone (at most 768: the local stage in passes 0 / 1, the chunked 2-row shape in pass 2); else `pad`
    draws in all, the records' draws spread evenly among culled ones (every chunk holds some)."""
    in_last = dict(full=recs, one=1, all_but_one=recs - 1)[last]
    nrec = (ntiles - 1) * recs + in_last
    r = np.arange(nrec)
    tile, slot = r // recs, r % recs
    in_tile = np.where(tile == ntiles - 1, in_last, recs)
    want = np.minimum(tile_survivors(recs, ntiles, density)[tile], in_tile * LANES)
    k = want // in_tile + (slot < want % in_tile)  # spread evenly over the tile's records
    kind, off, cnt = _singles(nrec, k)
    if density == "zero":  # records of 1 .. 32 lanes over away meshlets
        off, cnt = me.AWAY[0] + (r * 7) % (me.AWAY[1] - me.AWAY[0] - LANES), 1 + r % LANES
    if not pad:
        return kind, off, cnt
    at = r * pad // nrec
    all_kind, all_off, all_cnt = np.full(pad, CULLED), np.full(pad, me.KEEP_A[0]), np.full(pad, LANES)
    all_kind[at], all_off[at], all_cnt[at] = kind, off, cnt
    return all_kind, all_off, all_cnt


def _tile_names():
    out = {}
    for recs, pad, tag in ((4, 0, "t4"), (4, 800, "t4c"), (16, BIG_N, "t16")):
        for T in TILE_COUNTS:
            for d in DENSITIES:
                if d == "tile_64_only" and T <= 64:
                    continue
                if tag == "t4c" and (T not in (65, 130) or d not in ("steps", "full")):
                    continue
                for last in (LAST if d in ("full", "steps") and tag != "t4c" else LAST[:1]):
                    out[f"{tag}_{T}_{d}_{last}"] = (recs, T, d, last, pad)
    return out


TILE_CASES = _tile_names()
SHAPE_CASES = [f"shape_{n}" for n in SHAPE_SIZES]
LOCAL_CASES = (["local_first_only", "local_last_only", "local_every_one", "local_middle_chunk"] +
               [f"local_run_{n}_{w}" for n in RUNS for w in RUN_AT] + [f"local_fat_{g}" for g in FAT_AT] +
               [f"local_total_{n}" for n in TOTALS])
MIXED_CASES = ["mixed_300", "mixed_1000"]
ALL_CASES = SHAPE_CASES + LOCAL_CASES + MIXED_CASES + list(TILE_CASES)
_cache = {}


def scene(name):
    """Built once per process and shared: nobody writes into it."""
    if name not in _cache:
        if name in TILE_CASES:
            arrays = _tiles(*TILE_CASES[name])
        elif name.startswith("local_"):
            arrays = _local(name)
        elif name.startswith(("shape_", "mixed_")):
            n = int(name.split("_")[1])
            arrays = seeded(n, (SHAPE_SIZES + (300, 1000)).index(n) % 9)
        else:
            raise KeyError(name)
        _cache[name] = Scene(name, *arrays)
    return _cache[name]


def tile_records_of(name):
    """Records per tile of the shape a tile case is for."""
    return TILE_CASES[name][0]


def tile_cases(tag, ntiles):
    return [k for k, v in TILE_CASES.items() if k.startswith(tag + "_") and v[1] == ntiles]


# ---------------------------------------------------------------------------------------------------------- capacities
CUT_CASES = ("t4_65_steps_full", "t4c_65_steps_full", "t16_65_steps_full", "local_fat_255")
DISPATCH_T = 16  # the t of the 4 t and 4 t +- 1 dispatch capacities


def draw_capacities(ex, recs):
    """{name: draw_capacity} against the uncut total: total - 1, total, 1, 0, the prefix at a tile boundary, the prefix at a
    trip boundary inside a tile and that prefix +- 1."""
    S = ex.survivors()
    cnt, base = ex.tiles(recs)
    out = dict(draw_total_minus_1=S - 1, draw_total=S, draw_1=1, draw_0=0)
    later = np.flatnonzero((base > 0) & (cnt > 0))
    if len(later):
        out["draw_on_tile"] = int(base[later[0]])
    two = np.flatnonzero((cnt > TRIP) & (base > 0))
    if len(two):
        b = int(base[two[0]]) + TRIP
        out.update(draw_on_trip=b, draw_on_trip_minus_1=b - 1, draw_on_trip_plus_1=b + 1)
    return {k: v for k, v in out.items() if v >= 0}


def dispatch_capacities(ex):
    t = 4 * DISPATCH_T
    out = dict(disp_total_minus_1=ex.total - 1, disp_total=ex.total, disp_1=1, disp_4t=t, disp_4t_minus_1=t - 1,
               disp_4t_plus_1=t + 1)
    return {k: v for k, v in out.items() if 0 < v <= ex.total}


def capacities(ex, recs):
    """[(what, dispatch capacity, draw capacity)]: every dispatch capacity with room for all its survivors, every draw
    capacity with room for all records, and both short at once."""
    room_d, room_c = ex.total + 8, ex.survivors() + 8
    out = [(k, v, room_c) for k, v in dispatch_capacities(ex).items()]
    out += [(k, room_d, v) for k, v in draw_capacities(ex, recs).items()]
    half = ex.total // 2
    out.append(("both_short", half, max(ex.survivors(half) - 3, 1)))
    return out


# -------------------------------------------------------------------------------------------------------------- census
def run_classes(sc_):
    """{(length, where)} of the maximal runs of draws without a record in a local scene."""
    none = (sc_.kind[:sc_.n] == CULLED) | (sc_.cnt[:sc_.n] == 0)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], none.astype(np.int8), [0]])))
    out = set()
    for lo, hi in zip(edges[::2], edges[1::2]):
        if lo == 0:
            out.add((hi - lo, "start"))
        if hi == sc_.n:
            out.add((hi - lo, "end"))
        for b, w in ((256, "b256"), (512, "b512")):
            if lo < b <= hi - (1 if hi - lo > 1 else 0) or (hi - lo == 1 and hi == b):
                out.add((hi - lo, w))
    return out


def arrangements(name, records, pops):
    """What a case reaches, from the records and per-record survivors of a cull of it (the CPU module passes the
    oracle's): a set of names, REQUIRED lists those that must occur somewhere."""
    s = scene(name)
    out = set()
    total = len(records)
    if name in SHAPE_CASES:
        for op in (0, 1, 2):
            out.add(f"shape{shape_of(s.n, op)}_at_{s.n}_pass{op}")
        if s.n % CHUNK == 1 and s.n > 1 and s.kind[s.n - 1] == DRAWN and s.cnt[s.n - 1] > 0:
            out.add(f"last_chunk_one_drawn_draw_{s.n}")
        for h in s.header_counts():
            out.add("header_" + ("equal" if h == s.n else "below" if h < s.n else "above"))
            if h > s.n and s.draw_end(h) > s.n:
                out.add("header_above_reaches_draws_past_n")
    if name in LOCAL_CASES:
        assert s.n == LOCAL_MAX
        owners = np.unique(s.expect().owner)
        if total and list(owners) == [0]:
            out.add("first_draw_only")
        if total and list(owners) == [LOCAL_MAX - 1]:
            out.add("last_draw_only")
        if len(owners) == LOCAL_MAX and total == LOCAL_MAX:
            out.add("every_draw_one_record")
        for length, where in run_classes(s):
            out.add(f"run_{length}_{where}")
        per_chunk = [int(s.expect().per_draw[c * CHUNK:(c + 1) * CHUNK].sum()) for c in range(3)]
        if per_chunk[1] == 0 and per_chunk[0] and per_chunk[2]:
            out.add("middle_chunk_no_record")
        fat = np.flatnonzero(s.expect().per_draw >= FAT_RECORDS)
        for g in fat:
            first = int(s.expect().per_draw[:g].sum())
            tiles = (first + FAT_RECORDS - 1) // 4 - first // 4 + 1
            if tiles > 10 and total > FAT_RECORDS:
                out.add(f"fat_draw_at_{g}")
        if total in TOTALS:
            out.add(f"local_total_{total}")
    if name in TILE_CASES:
        recs, T, density, last, pad = TILE_CASES[name]
        tag = name.split("_")[0]
        for op in (0, 2):
            assert rows_of(shape_of(s.n, op)) * 2 == recs
        ntiles = ceil_div(total, recs)
        p = np.zeros(ntiles * recs, np.int64)
        p[:total] = pops
        cnt = p.reshape(-1, recs).sum(axis=1)
        full = recs * LANES
        out.add(f"{tag}_tiles_{ntiles}")
        in_last = total - (ntiles - 1) * recs
        out.add(f"{tag}_last_" + ("full" if in_last == recs else "one" if in_last == 1 else
                                   "all_but_one" if in_last == recs - 1 else "other"))
        if total and not cnt.any():
            out.add(f"{tag}_zero")
        if in_last == recs and bool((cnt == full).all()):
            out.add(f"{tag}_full")
        for v in STEPS[recs]:
            at = np.flatnonzero(cnt == v)
            if len(at) and not (v == full and bool((cnt == full).all())):
                out.add(f"{tag}_step_{v}")
        others = lambda t: not np.delete(cnt, t).any()  # noqa: E731
        if ntiles > 1 and cnt[0] == full and others(0):
            out.add(f"{tag}_first_tile_only")
        if ntiles > 1 and cnt[-1] == full and others(ntiles - 1):
            out.add(f"{tag}_last_tile_only")
        if ntiles > 65 and cnt[64] == full and others(64):
            out.add(f"{tag}_tile_64_only")
        if ntiles > 2 and bool((cnt[::2] == full).all()) and not cnt[1::2].any():
            out.add(f"{tag}_alternating")
        if bool(((cnt > TRIP) & (cnt % TRIP != 0)).any()):
            out.add(f"{tag}_partial_second_trip")
    return out


def cut_arrangements(name, records, pops):
    """The capacity arrangements a cut case reaches, from the uncut oracle's records and survivors."""
    s = scene(name)
    ex = s.expect()
    recs = tile_records_of(name) if name in TILE_CASES else 4
    form = "local" if shape_of(s.n, 0) == 0 else "chunked"
    total, S = len(records), int(pops.sum())
    p = np.zeros(ceil_div(total, recs) * recs, np.int64)
    p[:total] = pops
    cnt = p.reshape(-1, recs).sum(axis=1)
    base = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    out = set()
    for what, cap_d, cap_c in capacities(ex, recs):
        if what.startswith("disp_") and cap_d <= total:
            out.add(f"{what}_{form}")
            out.add(f"{what}_pass2_chunked")
        if what == "draw_total_minus_1" and cap_c == S - 1:
            out.add(what)
        if what == "draw_total" and cap_c == S:
            out.add(what)
        if what in ("draw_1", "draw_0") and cap_c < S:
            out.add(what)
        if what == "draw_on_tile" and bool(((base == cap_c) & (cnt > 0) & (base > 0)).any()):
            out.add(what)
        if what.startswith("draw_on_trip"):
            d = dict(draw_on_trip=0, draw_on_trip_minus_1=-1, draw_on_trip_plus_1=1)[what]
            inside = (base + TRIP < base + cnt) & (base + TRIP + d == cap_c)
            if bool(inside.any()):
                out.add(what)
        if what == "both_short" and cap_d < total and cap_c < int(pops[:cap_d].sum()):
            out.add(what)
    return out


REQUIRED = (
    [f"shape0_at_{n}_pass{op}" for n in (1, 255, 256, 257, 767, 768) for op in (0, 1)] +
    [f"shape1_at_{n}_pass2" for n in (1, 255, 256, 257, 767, 768)] +
    [f"shape1_at_{n}_pass{op}" for n in (769, 4095, 4096) for op in (0, 1, 2)] +
    [f"shape2_at_4097_pass{op}" for op in (0, 1, 2)] +
    ["last_chunk_one_drawn_draw_769", "last_chunk_one_drawn_draw_4097", "header_equal", "header_below", "header_above",
     "header_above_reaches_draws_past_n"] +
    ["first_draw_only", "last_draw_only", "every_draw_one_record", "middle_chunk_no_record"] +
    [f"run_{n}_{w}" for n in RUNS for w in RUN_AT] + [f"fat_draw_at_{g}" for g in FAT_AT] +
    [f"local_total_{n}" for n in TOTALS] +
    [f"{tag}_tiles_{T}" for tag in ("t4", "t16") for T in TILE_COUNTS] +
    [f"{tag}_last_{w}" for tag in ("t4", "t16") for w in LAST] +
    [f"{tag}_{d}" for tag in ("t4", "t16") for d in DENSITIES if d != "steps"] +
    [f"{tag}_step_{v}" for tag, recs in (("t4", 4), ("t16", 16)) for v in STEPS[recs]] +
    ["t4c_tiles_65", "t4c_tiles_130", "t4c_full", "t4c_step_127"]
)
REQUIRED_CUTS = (
    ["draw_total_minus_1", "draw_total", "draw_1", "draw_0", "draw_on_tile", "draw_on_trip", "draw_on_trip_minus_1",
     "draw_on_trip_plus_1", "both_short"] +
    [f"disp_{w}_{form}" for w in ("total_minus_1", "total", "1", "4t", "4t_minus_1", "4t_plus_1") for form in ("local", "chunked")]
)

# ------------------------------------------------------------------------------------------------------- mixed calls
MIXED_VIEWS = ("shape_4097", "mixed_300", "mixed_1000", "shape_768")   # [4097, 300, 1000, 768] draws
MIXED_PASSES = ((0, 0, 0, 0), (0, 1, 2, 0))
LOCAL_PAIR = ("shape_1", "shape_768")
# every launch follows one of another shape or of a very different tile count
BACK_TO_BACK = ("t16_130_full_full", "shape_1", "t4_129_steps_full", "shape_769", "t4_64_full_full", "shape_4097")
