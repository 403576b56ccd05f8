"""GPU tests of the per-block evaluation's tile-to-tile pipeline (orbit_amd/csrc/meshlet_eval_blocks.hip): a wave hands
its registers over from tile to tile in one of two forms — eight cone words of an all-sparse tile, or the first two rows of
a tile with a dense row — and every hand-over between the two, from the ramp and past a wave's last tile, is reached here
with a few hundred records by capping the launch's grid (orbit_ctx_set_block_cull_grid): under a cap of c workgroups wave
w of 4 c takes tiles w, w + 4 c, w + 8 c, ...  Every case is culled with the path on and off and compared byte for byte
with the oracle (both_ways), and the path must have been taken."""
import numpy as np
import pytest

import scenes as sc
from orbit_amd import _lib, layouts as L
from test_block_cull_gpu import _cone_scene, both_ways, engine, far_camera, info, sparse_share  # noqa: F401
from test_gpu_parity import GpuScene, run_gpu, run_oracle, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

RECS = 16  # records per tile, two per row


@pytest.fixture()
def capped(engine):  # noqa: F811
    """-> set(cap); the cap is taken off again behind the test."""
    yield engine.set_block_cull_grid
    engine.set_block_cull_grid(0)


def record_sparse_flags(scene, cam, recs, stream_count=None, stream_first=0):
    """The sparse flag blk_setup derives for each dispatched record, from the host pre-test (orbit_host_block_pretest): a
    record that does not start a block or is not inside the stream [stream_first, stream_first + stream_count) reads no
    bound and is dense; the others are what the pre-test says of their view x model matrix, their block's bound and the
    planes."""
    from test_block_pretest_cpu import F, _host, bounds_of, slab_scale

    h = _host()
    model = scene.entities["model_matrix"].reshape(-1, 4, 4).transpose(0, 2, 1).astype(F)
    view = np.asarray(cam.view, dtype=F)
    vm = np.zeros_like(model)
    for k in range(4):  # mat4_mul_col: term by term in binary32
        vm = (vm + view[None, :, k, None] * model[:, None, k, :]).astype(F)
    cols = np.ascontiguousarray(vm.transpose(0, 2, 1)).reshape(-1, 16)
    scale = slab_scale(cols)
    m = scene.meshlets
    bnd = bounds_of(m["bounding_sphere"])
    cones = (m["cone_axis"].view(np.uint8).astype(np.uint32) << np.array([0, 8, 16], dtype=np.uint32)).sum(1).astype(np.uint32) \
        | m["cone_cutoff"].view(np.uint8).astype(np.uint32) << 24
    planes = np.ascontiguousarray(cam.planes, dtype=F).reshape(-1, 4)
    n_ms = len(m) - stream_first if stream_count is None else stream_count
    flags = np.zeros(len(recs), dtype=bool)
    out = np.zeros(32, dtype=np.uint8)
    for i, (ent, off, cnt, _) in enumerate(recs.tolist()):
        rel = off - stream_first
        if cnt == 0 or off % 32 != 0 or rel < 0 or rel >= n_ms or cnt > n_ms - rel:
            continue
        c = cols[ent]
        with np.errstate(invalid="ignore"):
            affine = bool(c[3] == 0 and c[7] == 0 and c[11] == 0 and c[15] == 1 and (c[12:15] * F(0) == 0).all())
        lane_cones = np.ascontiguousarray(cones[off:off + cnt])
        f = h.orbit_host_block_pretest(c.ctypes.data, int(affine), float(scale[ent]), bnd[off // 32:off // 32 + 1].ctypes.data,
                                       planes.ctypes.data, len(planes), -1.0, lane_cones.ctypes.data, cnt, out.ctypes.data)
        flags[i] = (f & 1) != 0
    return flags


def tile_kinds(flags):
    """'S' every row sparse (records the list does not hold count as sparse), 'D' none, 'M' some — per tile of 16 records."""
    n = (len(flags) + RECS - 1) // RECS
    padded = np.ones(n * RECS, dtype=bool)
    padded[:len(flags)] = flags
    rows = padded.reshape(n, RECS // 2, 2).all(2)
    return "".join("S" if r.all() else "D" if not r.any() else "M" for r in rows)


def wave_sequences(kinds, cap):
    stride = 4 * cap
    return [kinds[w::stride] for w in range(stride) if kinds[w::stride]]


def dispatched(oracle, scene, ci):
    return L.dispatch_buffer_records(run_oracle(oracle, scene, ci)[0])[1]


def handover_scene(oracle):
    """The 600-entity, 64-meshlet scene of test_camera_inside_and_blocks_across_the_planes from a camera at its edge (the
    records near the camera are dense, the others sparse: 75 tiles, all-sparse and mixed ones in turn), with the entities
    of tiles 4 and 19 under a slightly projective matrix: their records are dense wherever they are, so these two tiles are
    wholly dense — one between two all-sparse tiles of a wave under a cap of 1, the other under a cap of 2."""
    scene = sc.make_scene(7, 600, meshlets_per_mesh=(64, 64), n_materials=3)
    cam = sc.default_camera(position=(0.0, 2.0, 60.0), rot=(1.0, 0.0))
    recs = dispatched(oracle, scene, info(cam))
    for t in (4, 19):
        for e in set(recs["entity_index"][RECS * t:RECS * t + RECS].tolist()):
            scene.entities["model_matrix"][e][3] = 1e-3  # w = 1 + x / 1000
    assert np.array_equal(dispatched(oracle, scene, info(cam)), recs), "the entity stage must dispatch the same records"
    return scene, cam


HANDOVERS = ("SS", "SM", "MS", "MM", "SDS")


@pytest.mark.parametrize("cap", [1, 2])
def test_mixed_handovers(torch_mod, engine, capped, oracle, cap):  # noqa: F811
    """4 and 8 waves over 75 tiles: some wave's sequence of tiles goes from an all-sparse tile to an all-sparse one, from
    an all-sparse to a mixed one and back, from mixed to mixed, through a wholly dense tile between two all-sparse ones, and
    waves begin and end on either kind — asserted on the host from the pre-test's flags before the GPU runs."""
    scene, cam = handover_scene(oracle)
    ci = info(cam)
    kinds = tile_kinds(record_sparse_flags(scene, cam, dispatched(oracle, scene, ci)))
    assert len(kinds) >= 40
    seqs = wave_sequences(kinds, cap)
    for h in HANDOVERS:
        assert any(h in s for s in seqs), f"no wave passes through {h} under a cap of {cap}: {seqs}"
    assert any(s[0] in "MD" for s in seqs) and any(s[-1] in "MD" for s in seqs), seqs
    assert any(s[0] == "S" for s in seqs) and any(s[-1] == "S" for s in seqs), seqs
    capped(cap)
    both_ways(torch_mod, engine, oracle, scene, ci)


@pytest.mark.parametrize("records", [1, 15, 16, 17, 65, 81])
def test_short_launches(torch_mod, engine, capped, oracle, records):  # noqa: F811
    """One workgroup of four waves over 1 / 1 / 1 / 2 / 5 / 6 tiles: a wave with exactly one tile, waves with none, waves
    with two, and (17, 65, 81) a last tile that holds one record — its fifteen empty records count as sparse, so it is an
    all-sparse tile whose eight loads must read nothing."""
    scene = sc.make_scene(300 + records, records, meshlets_per_mesh=(32, 32), n_materials=3, shuffle=False)
    cam = far_camera()
    ci = info(cam)
    recs = dispatched(oracle, scene, ci)
    assert len(recs) == records
    kinds = tile_kinds(record_sparse_flags(scene, cam, recs))
    assert kinds == "S" * ((records + RECS - 1) // RECS), "these scenes are meant to take the whole-tile path"
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


def _spread(total):
    """`total` open lanes over the 16 records of a tile, from its first record on."""
    return [min(32, max(0, total - 32 * r)) for r in range(RECS)]


# candidates per tile; under a cap of 1 wave w takes tiles w, w + 4, ...: the columns below
_WAVE_TILES = [[0, 1, 63, 64, 65, 128, 512, 0],      # wave 0: every count next to another one, last tile without any
               [512, 128, 65, 64, 63, 1, 0, 39],     # wave 1: the other way round, last tile with the common 39
               [64, 0, 512, 1, 128, 63, 65, 512],    # wave 2: last tile with every lane
               [39, 39, 39, 39, 39, 39, 39, 39]]     # wave 3: the benchmark's share throughout


def test_candidate_counts_across_tiles(torch_mod, engine, capped, oracle):  # noqa: F811
    """Consecutive tiles of one wave queue 0, 1, 63, 64, 65, 128 and 512 candidates in two orders (the ring's head and count
    start over with each tile, the end-of-tile gather of one tile is evaluated around the next slab's setup), and a wave's
    last tile queues 0, 39 and 512."""
    per_tile = [_WAVE_TILES[t % 4][t // 4] for t in range(32)]
    open_lanes = [k for total in per_tile for k in _spread(total)]
    scene = _cone_scene(open_lanes)
    cam = sc.default_camera(position=(0.0, 0.0, 900.0))
    share, counts = sparse_share(scene, cam)
    assert share == 1.0 and list(counts) == open_lanes, "the scene must queue exactly these candidates"
    ci = info(cam)
    assert len(dispatched(oracle, scene, ci)) == 32 * RECS
    assert [int(counts[RECS * t:RECS * t + RECS].sum()) for t in range(0, 32, 4)] == _WAVE_TILES[0]
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


def test_knife_edges(torch_mod, engine, capped, oracle):  # noqa: F811
    """The cone knife-edge generator (cone quantities within rounding of zero) on a scene whose records all start blocks,
    from far away: 38 tiles on four waves."""
    import make_spirv_vectors as gen

    rng = np.random.default_rng(31)
    scene = sc.make_scene(31, 300, meshlets_per_mesh=(64, 64), lods=1, shuffle=False)
    gen.quantise(scene, rng)
    cam = sc.default_camera(position=(0.0, 0.0, 400.0), rot=(1.0, 0.0))
    gen.cone_knife_edge(scene, cam, False)
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, sc.make_cull_info(cam.view, cam.planes))


def test_range_status(torch_mod, engine, capped, oracle):  # noqa: F811
    """A stream over the first part of the buffer only, one workgroup: the tiles before the stream's end are all-sparse
    and raise nothing, the records behind it are dense and raise ORBIT_E_RANGE from their row loads; lists and status
    text are the same with the path on and off.  The whole stream under the same cap raises nothing (both_ways)."""
    torch = torch_mod
    scene = sc.make_scene(33, 200, meshlets_per_mesh=(32, 32), n_materials=3, shuffle=False)
    cam = far_camera()
    ci = info(cam)
    short = len(scene.meshlets) - 200
    kinds = tile_kinds(record_sparse_flags(scene, cam, dispatched(oracle, scene, ci), stream_count=short))
    assert "S" in kinds and ("M" in kinds or "D" in kinds)
    capped(1)
    both_ways(torch, engine, oracle, scene, ci)
    gs = GpuScene(torch, scene)
    ms = engine.meshlet_stream(gs.meshlets, 0, short)
    ms.set_materials(gs.materials, len(scene.materials))
    engine.bind_meshlet_stream(ms)
    torch.cuda.synchronize()
    out = []
    for on in (True, False):
        engine.set_block_cull(on)
        before = engine.block_culls()
        got = run_gpu(torch, engine, gs, ci)
        assert engine.block_culls() == before + (1 if on else 0)
        with pytest.raises(_lib.OrbitError) as err:
            engine.status()
        out.append((got[1], str(err.value)))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    engine.set_block_cull(True)
    engine.bind_meshlet_stream(None)
    ms.close()


def test_the_cap_changes_nothing(torch_mod, engine, capped, oracle):  # noqa: F811
    """Caps of 0 (none), 1, 3 and one above the grid the library would take: the same bytes."""
    scene, cam = handover_scene(oracle)
    ci = info(cam)
    lists = []
    for cap in (0, 1, 3, 1 << 20):
        capped(cap)
        lists.append(both_ways(torch_mod, engine, oracle, scene, ci))
    assert all(np.array_equal(lists[0], x) for x in lists[1:])
