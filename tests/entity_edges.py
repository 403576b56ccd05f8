"""The entity stage at its launch-form, chunk and range edges: the cases.

The shader body (orbit_amd/csrc/entity_common.h entity_eval_one) is wrapped in five launch protocols chosen from the
entity-draw count alone; the sizes here are the smallest at which each form switches, derived from ONE table that
tests/test_entity_edges_cpu.py holds against the constants in the source text.  That module holds the reference side
to them (census floors, oracle == numpy restatement, range algebra); a GPU module that runs every case through every
form (tests/test_entity_edges_gpu.py) reads the same cases and helpers.

A case is a scenes.make_scene scene of N + SLACK entity-draws (the draw array is longer than any count a call is given,
so that the draw buffer's header can claim more), a 64 x 64 pyramid, and — the planted cases — edits of `mesh_infos`
and `entity_draws` alone.  A planted case's counts no longer match its meshlet array: it is `entity_only` and never
handed to a meshlet stage.
"""
import numpy as np

import hiz_edges as hz
import scenes as sc
from orbit_amd import dist

# ------------------------------------------------------------------------------------------------------- the table
CHUNK = 256              # kEntityBlock: entity-draws per workgroup of every entity launch
EXPAND_TRIP = 1024       # records per trip of entity_expand_records (4 x kEntityBlock)
ONE_LAUNCH_CHUNKS = 128  # kEntityOneLaunchChunks: more chunks take eval + emit
FUSED_MAX = 16384        # kFusedMaxEntityDraws: larger views leave the one-launch cull
SHARD_MAX_CHUNKS = 256   # kShardMaxChunks: larger shards leave the shard launch

ONE_LAUNCH = ONE_LAUNCH_CHUNKS * CHUNK
SHARD_MAX = SHARD_MAX_CHUNKS * CHUNK
SIZES = [1, 31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, FUSED_MAX - 1, FUSED_MAX, FUSED_MAX + 1,
         ONE_LAUNCH - (CHUNK - 1),  # 128 chunks, the last one holding a single draw
         ONE_LAUNCH, ONE_LAUNCH + 1, SHARD_MAX, SHARD_MAX + 1]
# the active draws of a size's last chunk: what the sizes one past a chunk boundary are for
LAST_CHUNK_DRAWS = {1: 1, 31: 31, 32: 32, 33: 33, 255: 255, 256: 256, 257: 1, 16383: 255, 16384: 256, 16385: 1, 32513: 1,
                    32768: 256, 32769: 1, 65536: 256, 65537: 1}
PLANT_SIZES = [CHUNK + 1, ONE_LAUNCH, ONE_LAUNCH + 1]
RANGE_SIZES = [CHUNK + 1, ONE_LAUNCH + 1, SHARD_MAX + 1]
SLACK = 300              # draws behind N in every case's draw array (header_counts)
PAD_WORDS = 3            # entity visibility words behind those of N + SLACK draws: compared too, never written
PYRAMID = (64, 64)
CLAMP_MESHLETS = 1 << 21  # 65 536 records.  No higher: the two-launch emit loops once per 1 024 records of a block
CLAMP_CAPACITY = 4096
RAGGED = (31, 32, 33, 63, 64, 65, 127, 128, 129)  # the record boundaries of dispatch sizes 32, 64 and 128
RAGGED_AT = CHUNK - 8    # ... next to each other across the first chunk boundary
FAT_MANY, FAT_ONE = 9001, 40_003  # 282 records an entity (four of them in a chunk); 1 251 records in ONE entity
PLANTS = ("zero_chunk", "fat_chunk", "ragged", "lod_far")
CLAMPED = ("clamped_first", "clamped_middle", "clamped_last")

CASES = {f"plain_{n}": dict(plant=None, n=n) for n in SIZES}
for _p in PLANTS + CLAMPED:
    for _n in PLANT_SIZES:
        CASES[f"{_p}_{_n}"] = dict(plant=_p, n=_n)
WHOLE = [k for k, v in CASES.items() if v["plant"] not in CLAMPED]  # (the clamped cases are for capacity runs)

_cache = {}


def chunks_of(n):
    return (n + CHUNK - 1) // CHUNK


def header_counts(n):
    """What the draw buffer's header says against a call given `n`: the same, fewer, more."""
    return sorted({n, max(n - SLACK, 0), n + SLACK})


def ranges(n):
    """[begin, end) of the range calls over `n` draws: the whole, a word in from both ends, the tail shorter than a word,
    a start that is no chunk boundary with a length that crosses the one-launch threshold, and three shards."""
    out = [(0, n), (32, n - 32), (32 * (n // 32), n), (96, min(n, 96 + ONE_LAUNCH + 1))] + list(dist.shard_ranges(n, 3))
    seen = []
    for b, e in out:
        if b < e and (b, e) not in seen:
            seen.append((b, e))
    return seen


def _pyramid(oracle):
    if "pyr" not in _cache:
        cam = hz.camera()
        W, H = hz.screen_of(*PYRAMID)
        depth = sc.make_depth(211, W, H, cam, n_occluders=192)
        pyr, d = oracle.depth_reduce(depth, W, H)
        assert (d.width, d.height) == PYRAMID
        _cache["pyr"] = (cam, pyr)
    return _cache["pyr"]


def cull_info(case, occlusion_pass, **kw):
    cam = case["cam"]
    if case["plant"] == "lod_far":  # far enough that the LOD clamps at the last one of the chain for (nearly) every draw
        kw.setdefault("lod_target", (0.0, 0.0, 4000.0))
    return sc.make_cull_info(cam.view, cam.planes, occlusion_pass=occlusion_pass, p00=cam.p00, p11=cam.p11,
                             z_near=cam.z_near, **kw)


def _clone_mesh(scene, src, meshlets):
    """A mesh with mesh `src`'s bounds (the same verdict for the same entity) and `meshlets` meshlets at every LOD."""
    mi = scene.mesh_infos[src:src + 1].copy()
    mi["mesh_lods"][0, :, 0] = 0
    mi["mesh_lods"][0, :int(mi["lod_count"][0]), 1] = meshlets
    scene.mesh_infos = np.concatenate([scene.mesh_infos, mi])
    return len(scene.mesh_infos) - 1


def _plant(oracle, case):
    """Edits mesh_infos and entity_draws of the finished scene; what was planted where goes into case["planted"]."""
    scene, n, plant = case["scene"], case["n"], case["plant"]
    draws, nch = scene.entity_draws, chunks_of(n)
    # a draw that passes the frustum and the pyramid: the planted draws are its entity with its mesh's bounds
    _, evis, _ = oracle.entity_cull(cull_info(case, 2), scene.entity_draw_buffer(n), n, scene.mesh_infos, scene.entities,
                                    n + 8, np.zeros((n + 31) // 32, np.uint32), case["pyr"], PYRAMID)
    good = int(np.flatnonzero(np.unpackbits(evis.view(np.uint8), bitorder="little")[:n])[0])
    entity, src = int(draws["entity_index"][good]), int(draws["mesh_index"][good])

    def put(g, meshlets):
        draws["entity_index"][g], draws["mesh_index"][g] = entity, _clone_mesh(scene, src, meshlets)

    planted = {}
    if plant == "zero_chunk":
        empty = _clone_mesh(scene, src, 0)
        zero = [0] + ([nch // 2] if nch >= 3 else [])
        for c in zero:
            draws["mesh_index"][c * CHUNK:(c + 1) * CHUNK] = empty
        for c in zero:  # (behind the loop above: chunk 0's successor is not overwritten)
            for g in (c * CHUNK - 1, (c + 1) * CHUNK):
                if 0 <= g < n:
                    put(g, 5)
        planted["zero_chunks"] = zero
    elif plant == "fat_chunk":
        many, one = (0, nch - 1) if nch <= 2 else (77, 101)
        for o in (3, 100, 200, 255):
            put(many * CHUNK + o, FAT_MANY)
        put(one * CHUNK, FAT_ONE)
        planted.update(fat_many=many, fat_one=one)
    elif plant == "ragged":
        for o, m in enumerate(RAGGED):
            put(RAGGED_AT + o, m)
    elif plant in CLAMPED:
        g = dict(clamped_first=5, clamped_middle=n // 2, clamped_last=n - 1)[plant]
        put(g, CLAMP_MESHLETS)
        planted["clamped_draw"] = g
    case["planted"] = planted


def make_case(name, oracle):
    """-> dict(name, n, plant, scene, cam, pyr, psize, capacity, entity_only, planted); built once per process and
    shared: nobody writes into it."""
    if name in _cache:
        return _cache[name]
    spec = CASES[name]
    n = spec["n"]
    cam, pyr = _pyramid(oracle)
    scene = sc.make_scene(300 + SIZES.index(n) if n in SIZES else 299, n + SLACK, n_meshes=400, meshlets_per_mesh=(0, 6),
                          lods=3, extent=(60.0, 20.0, 60.0))
    case = dict(name=name, n=n, plant=spec["plant"], scene=scene, cam=cam, pyr=pyr, psize=PYRAMID, planted={},
                entity_only=spec["plant"] not in (None, "lod_far"))
    if case["entity_only"]:
        _plant(oracle, case)
    lods = scene.mesh_infos["mesh_lods"][scene.entity_draws["mesh_index"], :, 1].astype(np.int64).max(axis=1)
    case["capacity"] = CLAMP_CAPACITY if spec["plant"] in CLAMPED else int(((lods + 31) // 32).sum()) + 8
    _cache[name] = case
    return case


def draw_buffer(case, header=None):
    """The EntityDrawBuffer's bytes: all N + SLACK draws, the header claiming `header` of them (default N)."""
    return case["scene"].entity_draw_buffer(case["n"] if header is None else header)


def words(case, how, seed=0):
    """The entity bitset over N + SLACK draws and PAD_WORDS more: all zero, all ones, or random."""
    count = (case["n"] + SLACK + 31) // 32 + PAD_WORDS
    if how == "zero":
        return np.zeros(count, np.uint32)
    if how == "ones":
        return np.full(count, 0xFFFFFFFF, np.uint32)
    return np.random.default_rng(2000 + seed).integers(0, 2 ** 32, count, dtype=np.uint32)


def excused(case):
    """{floor: reason} of the census floors a case cannot meet."""
    out = {}
    if case["n"] < 128:
        out["frustum"] = "fewer than 128 draws cannot have 64 culled by the frustum and 64 drawn"
    if case["plant"] == "zero_chunk" and chunks_of(case["n"]) < 3:
        out["interior_zero_chunk"] = "two chunks have no interior one: this size covers the zero chunk 0 and its successor only"
    if case["n"] < 64:
        out["occlusion"] = "of fewer than 64 draws about a third pass the frustum: not 16 removed and 16 kept"
    return out
