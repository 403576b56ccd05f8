"""The one-launch cull at its shape, bisection, tile and look-back edges, CPU side (tests/fused_edges.py): the table the
case sizes are derived from is the source text's, the restated shape selection and grid give the values worked out by hand
below and put every case on the shape it is for, the planting gives the oracle exactly the records and survivors it was
planted for (and the numpy restatement the same records), and every arrangement the cases are there for is shown by at
least one of them — counted from the oracle's outputs, not from the cases' names."""
import os
import re

import numpy as np
import pytest

import fused_edges as fe
import meshlet_edges as me
import np_restatement as npr
from orbit_amd import layouts as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orbit_amd", "csrc")


def _text(source):
    with open(os.path.join(CSRC, source)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("constant,source", [
    ("kEntityBlock", "entity_common.h"), ("kFusedWaves", "cull_fused.hip"), ("kFusedLocalChunks", "cull_fused.hip"),
    ("kFusedSmallEntityDraws", "cull_fused.hip"), ("kFusedMaxEntityDraws", "kernels.h"), ("kFusedSyncWords", "kernels.h"),
])
def test_the_table_is_the_codes(constant, source):
    found = re.findall(r"constexpr\s+(?:uint32_t|int)\s+%s\s*=\s*(\d+)u?\s*[;,]" % constant, _text(source))
    assert found == [str(fe.K[constant])], (constant, found)


def test_the_literals_next_to_the_table_are_the_codes():
    """Records per tile of the two tile shapes, the look-back's step, the command trip, the offsets the local stage keeps and
    the bisection's first step, the launcher's choice of rows."""
    text = _text("cull_fused.hip")
    assert len(re.findall(r"fused_tile_records\(int rows\) \{ return 2u \* \(uint32_t\)rows; \}", text)) == 1
    assert re.findall(r"const uint32_t rows = shape == 2u \? (\d+)u : (\d+)u;", text) == [("8", "2")]
    assert fe.TILE_RECORDS == {2: 4, 8: 16}
    assert re.findall(r"pos -= (\d+)u;", text) == [str(fe.LOOK_BACK)]
    assert re.findall(r"for \(uint32_t j0 = 0; j0 < n; j0 \+= (\d+)u\)", text) == [str(fe.TRIP)]
    assert re.findall(r"uint32_t off\[(\d+)\];", text) == [str(fe.LOCAL_OFFSETS)]
    assert re.findall(r"for \(uint32_t step = (\d+)u; step >= 1u; step >>= 1\)", text) == [str(fe.LOCAL_OFFSETS // 2)] * 2
    assert fe.LOCAL_MAX == 768 <= fe.LOCAL_OFFSETS and fe.SMALL_MAX == 4096 and fe.CHUNK == 256
    assert fe.LANES == L.MESHLET_DISPATCH_SIZE
    # a payload slab holds a tile of all survivors
    assert re.findall(r"constexpr uint32_t kFusedCap = kRecs \* (\d+)u;", text) == ["32"]


# ------------------------------------------------------------------------------------------------- the shape selection
def test_the_shape_selection_is_the_launchers():
    """`want` and fused_grid as the source states them, and by hand."""
    text = _text("cull_fused.hip")
    want = re.search(r"const uint32_t want = \(chunks <= local_max && all\.v\[j\]\.m\.ci\.occlusion_pass != 2u\) \? 0u\s*"
                     r": entity_draw_counts\[j\] <= kFusedSmallEntityDraws\s*\? 1u\s*: 2u;", text)
    assert want is not None
    assert "const uint32_t local_max = kFusedLocalChunks;" in text
    assert "const uint32_t cap = max(num_cus * (rows == 2u ? 3u : 2u) / max(views, 1u), 1u);" in text
    assert "return max(min(max(chunks, (waves + kFusedWaves - 1u) / kFusedWaves), cap), 1u);" in text
    for n, shapes in ((1, (0, 0, 1)), (768, (0, 0, 1)), (769, (1, 1, 1)), (4096, (1, 1, 1)), (4097, (2, 2, 2)),
                      (16384, (2, 2, 2))):
        assert tuple(fe.shape_of(n, op) for op in (0, 1, 2)) == shapes, n
    # 768 draws, 2 rows: 3 chunks, 192 waves -> 48 workgroups; 4097 draws, 8 rows: 17 chunks, 257 waves -> 65 workgroups
    assert fe.fused_grid(768, 2, 256, 1) == 48 and fe.fused_grid(1, 2, 256, 1) == 1 and fe.fused_grid(4097, 8, 256, 1) == 65
    assert fe.fused_grid(16384, 8, 256, 4) == 128 and fe.fused_grid(4096, 2, 256, 1) == 256 and fe.fused_grid(4096, 2, 2, 16) == 1
    # the mixed call: view 0 alone on the 8-row shape, views 1 .. 3 regrouped; with passes (0, 1, 2, 0) slot 1 of the local
    # launch is view 3 — idx[slot] != slot in every launch but the first
    assert fe.launches((4097, 300, 1000, 768), (0, 0, 0, 0), 256) == [(0, [1, 3], 48), (1, [2], 63), (2, [0], 65)]
    assert fe.launches((4097, 300, 1000, 768), (0, 1, 2, 0), 256) == [(0, [1, 3], 48), (1, [2], 63), (2, [0], 65)]
    assert fe.launches((1, 768), (0, 0), 256) == [(0, [0, 1], 48)]  # the grid is the larger view's
    assert fe.launches((1, 768), (0, 0), 256, grid_cap=2) == [(0, [0, 1], 2)]


def test_every_case_takes_the_shape_it_is_for():
    for name in fe.SHAPE_CASES:
        n = fe.scene(name).n
        assert fe.shape_of(n, 0) == (0 if n <= 768 else 1 if n <= 4096 else 2)
    for name in fe.LOCAL_CASES:
        assert fe.shape_of(fe.scene(name).n, 0) == fe.shape_of(fe.scene(name).n, 1) == 0
    for name, (recs, T, d, last, pad) in fe.TILE_CASES.items():
        s = fe.scene(name)
        want = {"t4": (0, 0, 1), "t4c": (1, 1, 1), "t16": (2, 2, 2)}[name.split("_")[0]]
        assert tuple(fe.shape_of(s.n, op) for op in (0, 1, 2)) == want, name
        assert s.n <= 5000 and s.expect().total <= 2500, name
    for name in fe.ALL_CASES:
        s = fe.scene(name)
        assert s.n <= 5000 and s.expect(s.n + fe.SLACK).total <= 2500, (name, s.expect().total)
    # the back-to-back order: every launch follows one of another shape or of a very different tile count
    order = [(fe.shape_of(fe.scene(n).n, 0), fe.scene(n).expect().total) for n in fe.BACK_TO_BACK]
    for (s0, r0), (s1, r1) in zip(order, order[1:]):
        assert s0 != s1 or max(r0, r1) > 8 * min(r0, r1), order
    assert {s for s, _ in order} == {0, 1, 2}


# ------------------------------------------------------------------------------------------------------ reference side
_refs = {}


def reference(oracle, name):
    """(oracle records, per-record survivors from the oracle's pass-2 words against an all-zero pyramid) of a case."""
    if name not in _refs:
        s = fe.scene(name)
        ex = s.expect()
        ents, mats, meshlets = me.entities(), me.materials(), me.meshlet_buffer("scattered")
        cap_d, cap_c = ex.total + 8, ex.survivors() + 8
        od, _, d1 = oracle.entity_cull(fe.cull_info(0), s.draw_buffer(), s.n, s.mesh_infos, ents, cap_d)
        oc, _, d2 = oracle.meshlet_cull(fe.cull_info(0), od, meshlets, cap_c, ents, mats)
        assert d1 == 0 and d2 == 0
        _, recs = L.dispatch_buffer_records(od)
        n_cmd, _ = L.draw_buffer_commands(oc)
        pyr = me.pyramid(oracle, "zero")
        od2, ev2, _ = oracle.entity_cull(fe.cull_info(2), s.draw_buffer(), s.n, s.mesh_infos, ents, cap_d,
                                         s.entity_words("zero"), pyr, fe.PYRAMID)
        oc2, mv2, _ = oracle.meshlet_cull(fe.cull_info(2), od2, meshlets, cap_c, ents, mats, s.meshlet_vis_words("zero"), pyr,
                                          fe.PYRAMID)
        assert np.array_equal(od2, od) and np.array_equal(oc2, oc), (name, "pass 2 with nothing drawn before, nothing hidden")
        masks = mv2[recs["visibility_offset"]]
        pops = np.array([bin(int(m)).count("1") for m in masks], np.int64)
        assert int(pops.sum()) == n_cmd
        _refs[name] = (recs, pops, masks, ev2)
    return _refs[name]


@pytest.mark.parametrize("name", fe.SHAPE_CASES + fe.LOCAL_CASES + fe.MIXED_CASES + [k for k in fe.TILE_CASES if "_steps_" in k])
def test_the_oracle_makes_what_was_planted(oracle, name):
    """oracle.entity_cull + oracle.meshlet_cull == the planted expectation: the records byte for byte, each record's
    survivors (the ballot words of pass 2) and so every prefix sum; the numpy restatement makes the same records and
    the same entity bitset."""
    s = fe.scene(name)
    ex = s.expect()
    recs, pops, masks, ev2 = reference(oracle, name)
    assert np.array_equal(recs.view(np.uint32), ex.records.view(np.uint32)), (name, "records")
    assert np.array_equal(masks, ex.masks) and np.array_equal(pops, ex.pops), (name, "survivors")
    assert np.array_equal(np.concatenate([[0], np.cumsum(pops)]), ex.before)
    for header in s.header_counts():
        exh = s.expect(header)
        od, _, _ = oracle.entity_cull(fe.cull_info(0), s.draw_buffer(header), s.n, s.mesh_infos, me.entities(), exh.total + 8)
        assert np.array_equal(L.dispatch_buffer_records(od)[1].view(np.uint32), exh.records.view(np.uint32)), (name, header)
        visible, should, rrecs, words = npr.entity_cull(fe.cull_info(2), s.draws, header, s.n, s.mesh_infos, me.entities(),
                                                        s.entity_words("zero"), me.pyramid(oracle, "zero"), fe.PYRAMID)
        assert np.array_equal(rrecs.view(np.uint32), exh.records.view(np.uint32)), (name, header, "restatement")
        if header == s.n:
            assert np.array_equal(words, ev2), (name, "entity bitset")


def test_the_planted_densities():
    """The steps density gives tiles of exactly the survivors it names, the full one fills every payload slab."""
    for tag, recs in (("t4", 4), ("t16", 16)):
        cnt, base = fe.scene(f"{tag}_66_steps_full").expect().tiles(recs)
        assert tuple(cnt[:len(fe.STEPS[recs])]) == fe.STEPS[recs]
        cnt, _ = fe.scene(f"{tag}_2_full_one").expect().tiles(recs)
        assert tuple(cnt) == (recs * 32, 32)
    assert fe.STEPS[4] == (63, 64, 65, 127, 128) and fe.STEPS[16] == (64, 65, 128, 129, 511, 512)
    s = fe.scene("local_fat_255")
    assert s.expect().per_draw[255] == fe.FAT_RECORDS == 41 and s.expect().total == 767 + 41
    assert fe.TOTALS == (3, 4, 5, 255, 256, 257, 259, 260, 261)
    assert fe.run_classes(fe.scene("local_run_300_b512")) == {(300, "b512")}
    assert fe.run_classes(fe.scene("local_run_1_b256")) == {(1, "b256")}


# -------------------------------------------------------------------------------------------------------------- census
def test_every_arrangement_occurs(oracle):
    """Each arrangement the cases are there for is reached by at least one case — decided from the oracle's records and
    survivors."""
    seen = set()
    for name in fe.ALL_CASES:
        recs, pops, _, _ = reference(oracle, name)
        seen |= fe.arrangements(name, recs, pops)
    missing = [a for a in fe.REQUIRED if a not in seen]
    assert not missing, missing
    cuts = set()
    for name in fe.CUT_CASES:
        recs, pops, _, _ = reference(oracle, name)
        cuts |= fe.cut_arrangements(name, recs, pops)
    missing = [a for a in fe.REQUIRED_CUTS if a not in cuts]
    assert not missing, missing


@pytest.mark.parametrize("name", fe.CUT_CASES)
def test_the_oracle_cuts_to_the_canonical_prefix(oracle, name):
    """Against every capacity pair the oracle's outputs are the uncut ones' prefix and its dropped counts the planted
    overflow: what the GPU module compares to is itself held to the planting."""
    s = fe.scene(name)
    ex = s.expect()
    ents, mats, meshlets = me.entities(), me.materials(), me.meshlet_buffer("scattered")
    recs = fe.tile_records_of(name) if name in fe.TILE_CASES else 4
    full_d, _, _ = oracle.entity_cull(fe.cull_info(0), s.draw_buffer(), s.n, s.mesh_infos, ents, ex.total)
    full_c, _, _ = oracle.meshlet_cull(fe.cull_info(0), full_d, meshlets, ex.survivors(), ents, mats)
    for what, cap_d, cap_c in fe.capacities(ex, recs):
        od, _, d1 = oracle.entity_cull(fe.cull_info(0), s.draw_buffer(), s.n, s.mesh_infos, ents, cap_d)
        oc, _, d2 = oracle.meshlet_cull(fe.cull_info(0), od, meshlets, cap_c, ents, mats)
        nrec = min(ex.total, cap_d)
        ncmd = min(ex.survivors(nrec), cap_c)
        assert d1 == ex.total - nrec and d2 == ex.survivors(nrec) - ncmd, (name, what)
        assert int(od[:4].view(np.uint32)[0]) == nrec and int(oc[:4].view(np.uint32)[0]) == ncmd, (name, what)
        assert np.array_equal(od[12:12 + 16 * nrec], full_d[12:12 + 16 * nrec]), (name, what)
        assert np.array_equal(oc[4:4 + 28 * ncmd], full_c[4:4 + 28 * ncmd]), (name, what)
