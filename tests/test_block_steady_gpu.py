"""GPU tests of the per-block evaluation's steady state (orbit_amd/csrc/meshlet_eval_blocks.hip): all-sparse tiles behind
one another, each with the next tile's eight cone words in flight, and at each tile's end the gather of the candidates still
queued issued AHEAD of the set-up of the slab two tiles on and evaluated behind it.  A wave enters that state from the
ramp, from a tile with a dense row and by ticket, and leaves it at its end or in front of a tile with a dense row, after an
odd and after an even number of tiles (a form of the loop that runs two tiles per turn with two register sets was built
and measured with these cases; profiles/block_steady_notes.md).  Every case is a few hundred records on ONE workgroup
(orbit_ctx_set_block_cull_grid(1): wave w takes tiles w, w + 4, ..., the first n_static of them by position and the others
by ticket), culled with the path on and off and compared byte for byte with the oracle (both_ways), and the path must
have been taken.  What a case is meant to reach — which tiles are all-sparse, how many a wave takes, which come from
tickets, how many candidates a tile queues — is asserted on the host first, from the BlockRecords the host derives
(orbit_host_block_record) and the host pre-test."""
import numpy as np
import pytest

import scenes as sc
from test_block_cull_gpu import _cone_scene, both_ways, engine, far_camera, info, sparse_share  # noqa: F401
from test_block_pipeline_gpu import RECS, capped, dispatched  # noqa: F401
from test_block_pretest_cpu import F, bounds_of, slab_scale
from test_block_setup_quad_cpu import records
from test_gpu_parity import torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

SPARSE = 1
WAVES = 4  # of the one workgroup


def tile_kinds(scene, cam, recs):
    """'S' every row sparse, 'D' none, 'M' some, per tile of 16 dispatched records of up to 32 meshlets — the row word
    blk_setup derives, from orbit_host_block_record: a record is dense if it does not start a block or does not lie inside
    the stream with all its meshlets (it reads no bound), or if the host's record says so; the slab's affine flag is
    row-wide, so a record beside a projective one or beside none is not affine; records the list does not hold are sparse."""
    model = scene.entities["model_matrix"].reshape(-1, 4, 4).transpose(0, 2, 1).astype(F)
    view = np.asarray(cam.view, dtype=F)
    vm = np.zeros_like(model)
    for k in range(4):  # mat4_mul_col: term by term in binary32
        vm = (vm + view[None, :, k, None] * model[:, None, k, :]).astype(F)
    n = len(recs)
    ent, off, cnt = recs["entity_index"], recs["meshlet_offset"].astype(np.int64), recs["meshlet_count"].astype(np.int64)
    assert ((cnt >= 1) & (cnt <= 32)).all()
    covered = (off % 32 == 0) & (off + cnt <= len(scene.meshlets))
    cols = np.ascontiguousarray(vm.transpose(0, 2, 1)).reshape(-1, 16)[ent]
    with np.errstate(invalid="ignore"):
        own = (cols[:, 3] == 0) & (cols[:, 7] == 0) & (cols[:, 11] == 0) & (cols[:, 15] == 1) & (cols[:, 12:15] * F(0) == 0).all(1)
    padded = np.zeros(n + (n & 1), dtype=bool)  # (a last record without a partner: beside no record)
    padded[:n] = own
    affine = np.repeat(padded.reshape(-1, 2).all(1), 2)[:n]
    bnd = bounds_of(scene.meshlets["bounding_sphere"])[np.where(covered, off // 32, 0)]
    planes = np.ascontiguousarray(cam.planes, dtype=F).reshape(-1, 4)
    flags = records(cols, affine, slab_scale(cols), bnd, planes, -1.0, 1)["flags"] if n else np.zeros(0, dtype=np.uint32)
    sparse = ((flags & SPARSE) != 0) & covered
    tiles = (n + RECS - 1) // RECS
    full = np.ones(tiles * RECS, dtype=bool)
    full[:n] = sparse
    rows = full.reshape(tiles, RECS // 2, 2).all(2)
    return "".join("S" if r.all() else "D" if not r.any() else "M" for r in rows)


def static_rounds(ntiles):
    """How many of a wave's tiles it takes by position under a cap of one workgroup (the kernel's n_static); the tiles
    behind them are handed out by ticket."""
    if ntiles <= WAVES:
        return 1
    full = ntiles // WAVES
    dyn = min(max(full // 4, 1), 3)
    return max(full - dyn, 3)


def sparse_scene(seed, ntiles, partial=True):
    """`ntiles` tiles of records of one 32-meshlet mesh each, in draw order (record r is entity r's), every one sparse
    from far_camera().  partial: the last tile holds six records and the last of them 17 meshlets."""
    n = RECS * ntiles - (RECS - 6 if partial else 0)
    scene = sc.make_scene(seed, n, meshlets_per_mesh=(32, 32), n_materials=3, shuffle=False, unit_scale=True,
                          mesh_radius=(0.5, 1.0))
    if partial:
        scene.mesh_infos["mesh_lods"][-1, 0, 1] = 17
    return scene


@pytest.mark.parametrize("ntiles", range(0, 28))
def test_tiles_per_wave(torch_mod, engine, capped, oracle, ntiles):  # noqa: F811
    """4 k + j all-sparse tiles on four waves, k = 0 ... 6 and j = 0 ... 3: j waves take k + 1 tiles and the others k, so
    waves take 0 to 7 tiles — none, an odd number and an even one (a loop of two tiles per turn is left behind its first
    and behind its second half), by position up to n_static and by ticket behind that; every tile's end-of-tile gather is
    in flight across the set-up of a slab that, behind the wave's last tiles, holds no record.  The last tile holds six
    records, the last of them 17 meshlets.  No tiles at all: the camera looks away, the entity stage dispatches nothing."""
    if ntiles == 0:
        scene = sparse_scene(700, 1)
        cam = far_camera(rot=(-1.0, 0.0))
    else:
        scene = sparse_scene(700 + ntiles, ntiles)
        cam = far_camera()
    ci = info(cam)
    recs = dispatched(oracle, scene, ci)
    assert len(recs) == (RECS * ntiles - 10 if ntiles else 0)
    if ntiles:
        assert recs["meshlet_count"][-1] == 17 and (recs["meshlet_count"][:-1] == 32).all()
    assert tile_kinds(scene, cam, recs) == "S" * ntiles, "every tile is meant to be all-sparse"
    per_wave = sorted(len(range(w, ntiles, WAVES)) for w in range(WAVES))
    k, j = divmod(ntiles, WAVES)
    assert per_wave == [k] * (WAVES - j) + [k + 1] * j
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


def test_ticketed_tiles_in_the_steady_state(torch_mod, engine, capped, oracle):  # noqa: F811
    """42 all-sparse tiles on four waves: ten whole rounds, of which a wave takes the first eight by position — an even
    number, so its first ticketed tile is an even one of its sequence and its second an odd one — and ten tiles are
    handed out by ticket: more than two per wave on average, so some wave takes two ticketed tiles in a row."""
    ntiles = 42
    n_static = static_rounds(ntiles)
    assert n_static == 8 and n_static < ntiles // WAVES
    assert ntiles - n_static * WAVES > 2 * WAVES
    scene = sparse_scene(760, ntiles)
    cam = far_camera()
    ci = info(cam)
    recs = dispatched(oracle, scene, ci)
    assert len(recs) == RECS * ntiles - 10
    assert tile_kinds(scene, cam, recs) == "S" * ntiles
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


@pytest.mark.parametrize("ntiles,dense", [(24, (4,)), (24, (8,)), (24, (12,)), (24, (16,)), (24, (4, 8)), (24, (12, 16)), (12, (8,)),
                                          (12, (4, 8))],
                         ids=["1", "2", "3", "4", "1-2", "3-4", "last", "last-two"])
def test_one_tile_with_a_dense_row(torch_mod, engine, capped, oracle, ntiles, dense):  # noqa: F811
    """Six tiles per wave (three in the last two cases, where a wave's last tile is the dense one), all by position where
    it matters (n_static = 5 and 3), every tile all-sparse except wave 0's tile 1, 2, 3 or 4 — tile 4, 8, 12, 16 of the
    list —, in which one entity stands two units in front of the camera: too near for its size, its record and with it one
    row of the tile is dense.  Wave 0 leaves the steady state after an odd number of tiles (in front of its tiles 2 and
    4) and after an even one (1 and 3): the tile before the dense one loads two rows instead of eight cone words, the
    dense one runs row by row with the candidates of its sparse rows gathered ahead at its end like any other's, and the
    steady state is entered again from the dense tile's own whole-tile loads; two dense tiles in a row; a dense tile
    last."""
    scene = sparse_scene(800 + ntiles, ntiles, partial=False)
    cam = far_camera()
    ci = info(cam)
    for t in dense:
        scene.entities["model_matrix"][RECS * t + 5, 12:15] = (0.0, 2.0, 598.0)
    recs = dispatched(oracle, scene, ci)
    assert np.array_equal(recs["entity_index"], np.arange(RECS * ntiles)), "the entity stage must dispatch every record in order"
    kinds = tile_kinds(scene, cam, recs)
    assert kinds == "".join("M" if t in dense else "S" for t in range(ntiles))
    assert all(t % WAVES == 0 and t // WAVES < static_rounds(ntiles) for t in dense), "wave 0's, by position"
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


def _tile(rows01, rows23, rest=0):
    """Open lanes of a tile's 16 records: `rows01` over records 0-3 (rows 0 and 1), `rows23` over records 4-7, `rest` over
    the other eight, each filled from its first record on."""
    fill = lambda total, n: [min(32, max(0, total - 32 * r)) for r in range(n)]  # noqa: E731
    return fill(rows01, 4) + fill(rows23, 4) + fill(rest, 8)


# under a cap of 1 wave w takes tiles w, w + 4, w + 8 (all by position): the columns
_FLUSH_TILES = [_tile(96, 40, 30), _tile(128, 128, 256), _tile(20, 19), _tile(0, 0),     # tiles 0-3: a wave's first tile
                _tile(100, 70), _tile(70, 0, 3), _tile(65, 64, 1), _tile(20, 19),        # tiles 4-7: its second
                _tile(128, 30, 100), _tile(0, 0), _tile(127, 1, 130), _tile(20, 19)]     # tiles 8-11: its third


def test_mid_tile_flushes_in_both_halves(torch_mod, engine, capped, oracle):  # noqa: F811
    """Twelve all-sparse tiles, three per wave, the even and the odd tiles of a wave's sequence.  Waves 0 and 1 queue more than 64 candidates in front of row 2 of an even and of an odd
    tile (96 and 100; 128 and 70) and wave 2 of an odd one (65, then 64 more in front of row 4); tiles 1, 8 and 10 queue
    more than 256 in all (512, 258, 258), so that behind the 64 gathered ahead at the tile's end further flushes follow in order and the
    ring goes round inside the tile; a tile without candidates (the gather ahead reads nothing and nothing is evaluated)
    stands behind flushing ones.  The counts are set cone by cone
    (test_block_cull_gpu._cone_scene) and asserted through the host pre-test."""
    open_lanes = [k for t in _FLUSH_TILES for k in t]
    scene = _cone_scene(open_lanes)
    cam = sc.default_camera(position=(0.0, 0.0, 900.0))
    share, counts = sparse_share(scene, cam)
    assert share == 1.0 and list(counts) == open_lanes, "the scene must queue exactly these candidates"
    per = counts.reshape(12, RECS)
    first = per[:, :4].sum(1)
    for w in (0, 1):
        assert first[w] > 64 and first[w + 4] > 64, "an even and an odd tile of the wave"
    assert first[6] > 64 and first[8] > 64
    assert (per.sum(1)[[1, 8, 10]] > 256).all() and (per.sum(1)[[3, 9]] == 0).all()
    ci = info(cam)
    recs = dispatched(oracle, scene, ci)
    assert len(recs) == 12 * RECS and tile_kinds(scene, cam, recs) == "S" * 12 and static_rounds(12) == 3
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)


# (x, y, z, cutoff) of a cone whose lane is a candidate from a camera on +z looking down -z at a sphere at the origin: the
# cone quantity is within the band when z = -cutoff, whatever x and y are (the view-space centre has neither)
_EDGE_CONES = [(-128, 127, 0, 0), (127, -128, 0, 0), (-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, 0, 0), (-128, -128, 1, -1),
               (127, 127, -1, 1), (-1, -1, 127, -127), (0, 127, -127, 127), (-128, 0, -1, 1), (127, -1, 1, -1)]


def test_cone_words_at_the_edges_of_their_bytes(torch_mod, engine, capped, oracle):  # noqa: F811
    """Candidates whose cone words hold the bytes -128, -1, 0 and 127 in the axis and a cutoff byte of either sign, in the
    first and in the last lane of their records — the lanes at the two ends of a half-wave — in an even and in an odd tile
    of wave 0: the word a candidate is evaluated from (sign extension byte by byte) is the word its row read."""
    ntiles = 8
    scene = _cone_scene([0] * (RECS * ntiles))
    m = scene.meshlets
    put = []
    for t in (0, 4):  # wave 0's first and second tile
        for i, cone in enumerate(_EDGE_CONES):
            r = RECS * t + i
            for lane in (0, 31):
                m["cone_axis"][32 * r + lane] = cone[:3]
                m["cone_cutoff"][32 * r + lane] = cone[3]
                put.append((r, lane))
    cam = sc.default_camera(position=(0.0, 0.0, 900.0))
    share, counts = sparse_share(scene, cam)
    assert share == 1.0
    want = np.zeros(RECS * ntiles, dtype=np.int64)
    for r, _ in put:
        want[r] += 1
    assert np.array_equal(counts, want), "exactly the lanes with these cones are candidates"
    axes = m["cone_axis"][[32 * r + lane for r, lane in put]]
    cuts = m["cone_cutoff"][[32 * r + lane for r, lane in put]]
    assert {-128, -1, 0, 127} <= set(axes.reshape(-1).tolist()) and (cuts < 0).any() and (cuts > 0).any()
    ci = info(cam)
    recs = dispatched(oracle, scene, ci)
    assert len(recs) == RECS * ntiles and tile_kinds(scene, cam, recs) == "S" * ntiles
    capped(1)
    both_ways(torch_mod, engine, oracle, scene, ci)
