"""The meshlet stage at its tile, group, scan-chunk and ticket edges, CPU side (tests/meshlet_edges.py): the table the case
sizes are derived from is the source text's, the restated launch arithmetic gives the values worked out by hand below,
the planting gives the oracle exactly the survivors it was planted for, every census class is shown by at least one
(case, capacity) pair — the ticket classes on parts of 256, 304 and 64 compute units —, and the C oracle equals the numpy
restatement bit for bit on every small and chunk case, in passes 0, 1 and 2."""
import os
import re

import numpy as np
import pytest

import meshlet_edges as me
import np_restatement as npr
from orbit_amd import layouts as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orbit_amd", "csrc")


# ------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("constant,source", [
    ("kTileRecords", "kernels.h"), ("kScanChunk", "kernels.h"), ("kTicketPools", "kernels.h"),
    ("kEmitTicketPools", "kernels.h"), ("kPayloadCap", "meshlet_common.h"), ("kGroupTiles", "meshlet_emit.hip"),
    ("kDynGroups", "meshlet_emit.hip"), ("kSlowWords", "meshlet_emit.hip"), ("kChainWavesPerSimd", "meshlet_emit.hip"),
    ("kEvWaves", "meshlet_eval.hip"), ("kEvWavesPerSimd", "meshlet_eval.hip"), ("ORBIT_EV_WPS0", "meshlet_eval.hip"),
])
def test_the_table_is_the_codes(constant, source):
    """The constants the case sizes are derived from, read out of the source text: whoever retunes one moves the cases
    with it."""
    with open(os.path.join(CSRC, source)) as f:
        text = f.read()
    if constant.startswith("ORBIT_"):
        found = re.findall(r"#define\s+%s\s+(\d+)\s*$" % constant, text, re.M)
    else:
        found = re.findall(r"constexpr\s+(?:uint32_t|int)\s+%s\s*=\s*(\d+)u?\s*[;,]" % constant, text)
    assert found == [str(me.K[constant])], (constant, found)


def test_the_rules_the_census_restates_are_the_codes():
    """The literals next to the table: a chain group is redone by the general form above 128 survivors, the chain emit's
    workgroups have four waves, a record has 32 lanes."""
    with open(os.path.join(CSRC, "meshlet_emit.hip")) as f:
        text = f.read()
    assert re.findall(r"slow\s*=\s*n\s*>\s*(\d+)u?\s*\|\|", text) == [str(me.CHAIN_FAST_MAX)]
    assert me.TRIP == 64 and me.CHAIN_FAST_MAX == 2 * me.TRIP  # trip(0u) and trip(64u) of the FAST loop
    assert len(re.findall(r"const uint32_t stride = gridDim\.x \* 4;", text)) == 2  # both emit bodies
    assert me.LANES == L.MESHLET_DISPATCH_SIZE and me.GROUP == 32 and me.CHUNK == 16384


def test_the_launch_arithmetic_by_hand():
    """eval_grid, the chain emit's grid and the two n_static rules against values worked out by hand."""
    # evaluation: 4 waves a workgroup, 4 workgroups a CU; 196 609 records = 12 289 tiles need 3 073 workgroups, 256 CUs
    # give 1 024 -> T = 4 096 tiles.  17 records = 2 tiles: one workgroup.  No record at all: still one.
    assert me.eval_grid(256, 196_609, 0, False) == 1024 and me.eval_stride(256, 196_609, 0, False) == 4096
    assert me.eval_grid(256, 17, 0, False) == 1 and me.eval_grid(256, 0, 2, True) == 1
    assert me.eval_grid(256, 4092 * 16, 0, True) == 1023 and me.eval_grid(256, 4092 * 16 + 1, 0, True) == 1024  # 4 092 tiles
    # the fifth wave per SIMD: pass 0 from the streams at 8 x 256 x 5 x 4 = 40 960 tiles = 655 360 records and more
    assert me.eval_grid(256, 655_344, 0, True) == 1024   # 40 959 tiles
    assert me.eval_grid(256, 655_345, 0, True) == 1280   # 40 960 tiles
    assert me.eval_grid(256, 655_393, 2, True) == 1024 and me.eval_grid(256, 655_393, 0, False) == 1024
    assert me.eval_grid(304, 1 << 20, 0, True) == 1520 and me.eval_grid(64, 1 << 20, 1, True) == 256
    # n_static = max(full_rounds - dyn_rounds, 3), dyn_rounds = min(max(full_rounds / 4, 1), 3); none up to one round
    T = 4096
    assert me.eval_n_static(T, T) is None and me.eval_n_static(0, T) is None
    assert me.eval_n_static(T + 1, T) == 3       # 1 - 1 = 0 -> 3: the three tiles of a wave's ramp are never ticketed
    assert me.eval_n_static(3 * T, T) == 3       # 3 - 1 = 2 -> 3: tickets are drawn, all of them past the end
    assert me.eval_n_static(3 * T + 1, T) == 3   # ... and tile 3 T is the first ticketed one
    assert me.eval_n_static(4 * T + 2, T) == 3   # 4 - 1
    assert me.eval_n_static(8 * T, T) == 6       # 8 - 2
    assert me.eval_n_static(12 * T + 5, T) == 9  # 12 - 3
    assert me.eval_n_static(40 * T, T) == 37     # 40 - min(10, 3)
    # chain emit: a wave per group of 2 tiles, 4 workgroups a CU; 524 288 records = 32 768 tiles = 16 384 groups need 4 096
    # workgroups, 256 CUs give 1 024 -> G = 4 096 groups.  Never more than 32 x 16 - 16 = 496 groups a wave: 4 000 000
    # records on 8 CUs = 250 000 tiles -> 62 500 -> 31 250 wave quads, / 496 = 63.004 -> 64 workgroups, not 32.
    assert me.chain_grid(256, 524_288) == 1024 and me.chain_stride(256, 524_288) == 4096
    assert me.chain_grid(256, 33) == 1 and me.chain_grid(256, 129) == 2 and me.chain_grid(256, 0) == 1
    assert me.chain_grid(8, 4_000_000) == 64 and me.chain_grid(64, 10_000_000) == 256
    # n_static = all below four rounds, else max(full_rounds - min(max(full_rounds / 4, 1), 3), 4)
    G = 4096
    assert me.chain_n_static(4 * G - 1, G) is None
    assert me.chain_n_static(4 * G, G) == 4 and me.chain_n_static(4 * G + 1, G) == 4  # 4 - 1 = 3 -> 4
    assert me.chain_n_static(5 * G + 2, G) == 4    # 5 - 1
    assert me.chain_n_static(8 * G, G) == 6        # 8 - 2
    assert me.chain_n_static(16 * G + 7, G) == 13  # 16 - 3
    # the sizes the issue names for the MI355X: the evaluation's first ticket at 196 608 + 1 records, the chain emit's at
    # 524 288 + 32
    assert me.eval_sizes(256) == (196_608, 196_609, 262_161, 524_288)
    assert me.chain_sizes(256) == (524_288, 524_320, 655_393)
    assert me.SMALL == (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65) and me.CHUNKS == (16383, 16384, 16385, 32769)


# --------------------------------------------------------------------------------------------------------- the planting
def test_the_planted_buffer():
    """Regions, boundaries and the chain layout's links are what the cases' arithmetic assumes."""
    keep = me.keep_flags()
    assert keep[:1024].all() and not keep[1024:2048].any() and keep[2048:3072].all()
    assert 200 < int(keep[3072:3584].sum()) < 312 and 12 < int(keep[3584:].sum()) < 56
    link, brk = me.link_bits(), me.chain_breaks()
    assert np.array_equal(link, ~brk), "the chain layout's link bits are not the planted breaks"
    for rec, lanes in me.BREAKS_IN_RECORD.items():  # exactly these lanes of that record, no other
        assert tuple(np.flatnonzero(~link[rec:rec + 32])) == lanes
    assert link[1:32].all() and not link[0] and not link[256]  # no break in the record at 0; allocation boundaries
    a, b = me.meshlet_buffer("scattered"), me.meshlet_buffer("chain")
    for f in ("bounding_sphere", "cone_axis", "cone_cutoff", "material_index", "vertex_count", "triangle_count"):
        assert np.array_equal(a[f], b[f])
    assert int(a["vertex_count"].max()) == int(a["triangle_count"].max()) == 255
    wraps = lambda m: int((m["data_offset"].astype(np.uint64) + m["vertex_count"] >= np.uint64(1 << 32)).sum())  # noqa: E731
    assert wraps(a) > 0 and int((np.diff(b["data_offset"].astype(np.int64)) < 0).sum()) == 1  # the chain wraps once
    assert set(me.materials()["alpha_mode"]) == {0, 1, 2} and len(set(a["material_index"])) == me.N_MATERIALS


def test_the_steps_density():
    """Tiles of exactly 64, 65, 128 and 129 survivors, groups of exactly 128 and 129."""
    c = me.case("steps_16384")
    per_tile = c.pops.reshape(-1, me.TILE).sum(axis=1)
    assert tuple(per_tile[:8]) == me.STEPS == (64, 65, 128, 129, 64, 64, 64, 65)
    per_group = per_tile.reshape(-1, 2).sum(axis=1)
    assert tuple(per_group[:4]) == (129, 257, 128, 129)
    assert me.case("last_only_65").survivors() == 1 and me.case("last_only_65").pops[-1] == 1
    assert me.case("full_33").survivors() == 33 * 32 and me.case("zero_16385").survivors() == 0
    c = me.case("chunk1_first_32769")
    assert c.survivors() == 512 and c.survivors(me.CHUNK) == 0 and c.survivors(me.CHUNK + me.TILE) == 512


# ---------------------------------------------------------------------------------------------------------- references
def _restated(c, layout, op, vis, pyr):
    d = {}
    cmds, words = npr.meshlet_cull(me.cull_info(op), c.records[:c.n], me.meshlet_buffer(layout), me.entities(),
                                   me.materials(), vis, pyr, me.PYRAMID, detail=d)
    masks = np.zeros(c.n, np.uint32)
    np.bitwise_or.at(masks, d["record"][d["should_draw"]], np.uint32(1) << d["lane"][d["should_draw"]].astype(np.uint32))
    return cmds, words, masks


@pytest.mark.parametrize("name", list(me.PLAN))
def test_oracle_equals_numpy_restatement(oracle, name):
    """Two restatements by different means agree bit for bit — commands, header, visibility words, task records and the
    record list derived from the same masks — in pass 0, pass 1 (seeded bitsets) and pass 2 (an all-zero pyramid and a
    pyramid from oracle.depth_reduce of scenes.make_depth), on the chain layout; the scattered layout's commands are the
    chain layout's with the other buffer's command words; and in pass 0 the masks are the planted ones."""
    c = me.case(name)
    ents, mats = me.entities(), me.materials()
    runs = [("chain", 0, None, None), ("chain", 1, "random", None), ("chain", 2, "random", "zero"),
            ("chain", 2, "random", "depth")]
    # the scattered layout differs in the command words alone: the chain layout's commands with the other buffer's words
    chain, _, _ = oracle.meshlet_cull(me.cull_info(0), c.buffer(), me.meshlet_buffer("chain"), c.survivors(), ents, mats)
    scattered, _, _ = oracle.meshlet_cull(me.cull_info(0), c.buffer(), me.meshlet_buffer("scattered"), c.survivors(), ents, mats)
    want = L.draw_buffer_commands(chain)[1]
    m = me.meshlet_buffer("scattered")[want["meshlet_index"]]
    want["cmd_first_index"] = (m["data_offset"] + m["vertex_count"].astype(np.uint32)) * np.uint32(4)
    want["cmd_vertex_offset"], want["meshlet_vertex_offset"] = m["data_offset"].view(np.int32), m["vertex_offset"]
    assert np.array_equal(L.draw_buffer_commands(scattered)[1].view(np.uint32), want.view(np.uint32)), (name, "scattered")
    for layout, op, how, kind in runs:
        vis = c.words(how) if how else None
        pyr = me.pyramid(oracle, kind) if kind else None
        cmds, words, masks = _restated(c, layout, op, vis, pyr)
        cap = len(cmds) + 8
        out, ovis, dropped = oracle.meshlet_cull(me.cull_info(op), c.buffer(), me.meshlet_buffer(layout), cap, ents, mats,
                                                 vis, pyr, me.PYRAMID)
        n, ocmds = L.draw_buffer_commands(out)
        assert n == len(cmds) and dropped == 0, (name, layout, op, kind)
        assert np.array_equal(ocmds.view(np.uint32), cmds.view(np.uint32)), (name, layout, op, kind, "commands differ")
        if op == 2:
            assert np.array_equal(ovis, words), (name, op, kind, "visibility words differ")
        elif op == 1:
            assert np.array_equal(ovis, vis)
        task, tvis = oracle.meshlet_task_cull(me.cull_info(op), c.buffer(), me.meshlet_buffer(layout), ents, mats, vis, pyr,
                                              me.PYRAMID)
        assert len(task) == c.n and np.array_equal(me.masks_of_task_records(task), masks), (name, layout, op, kind, "masks")
        assert np.array_equal(task["entity_index"], c.records["entity_index"][:c.n])
        assert np.array_equal(task["meshlet_offset"], c.records["meshlet_offset"][:c.n])
        if op == 2:  # the task shader's lanes past a record's count vote "visible" (forward_depth_prepass.task:124)
            past = ~((np.uint64(1) << c.records["meshlet_count"][:c.n].astype(np.uint64)) - np.uint64(1)) & np.uint64(0xFFFFFFFF)
            assert np.array_equal(tvis[:c.n], ovis[:c.n] | past.astype(np.uint32)) and np.array_equal(tvis[c.n:], ovis[c.n:])
        recs, survivors = me.record_list_of(task)
        assert survivors == n and np.array_equal(recs["mask"], masks)
        if op == 0:
            assert np.array_equal(masks, c.masks) and n == c.survivors(), (name, layout, "the planting")
        elif op == 2:
            live = c.records["meshlet_count"][:c.n] > 0
            if kind == "zero":  # nothing occludes: visible = planted; drawn = visible and not drawn by the early pass
                assert np.array_equal(ovis[:c.n][live], c.masks[live]) and np.array_equal(masks, c.masks & ~vis[:c.n])
            elif name == "full_64":  # the other pyramid hides some of the planted meshlets and leaves some
                hidden = int(np.unpackbits((c.masks & ~ovis[:c.n]).view(np.uint8)).sum())
                assert 64 <= hidden <= c.survivors() - 64


def test_the_planting_at_full_size(oracle):
    """660 000 hand-built short records: the oracle's command count is the planted one, its masks are the planted masks."""
    c = me.device_case("chain", me.chain_sizes(256)[2], 256)
    assert int(c.records["meshlet_count"][:c.n].sum()) < 2_000_000
    out, _, dropped = oracle.meshlet_cull(me.cull_info(0), c.buffer(), me.meshlet_buffer("chain"), c.survivors() + 8,
                                          me.entities(), me.materials())
    assert L.draw_buffer_commands(out)[0] == c.survivors() and dropped == 0
    task, _ = oracle.meshlet_task_cull(me.cull_info(0), c.buffer(), me.meshlet_buffer("chain"), me.entities(), me.materials())
    assert np.array_equal(me.masks_of_task_records(task), c.masks)


# -------------------------------------------------------------------------------------------------------------- census
def _small_and_chunk_classes():
    found = {}
    for name in me.PLAN:
        c = me.case(name)
        pairs = me.capacities(c) if name in me.CUT_CASES else [(c.n, c.survivors() + 8)]
        for cap in pairs:
            for layout in ("scattered", "chain"):
                for k in me.census(c, cap, layout, 256):
                    found.setdefault(k, (name, cap, layout))
    return found


def test_every_class_below_the_tickets_is_shown():
    """A condition on the INPUTS, decided by the reference side alone: every payload, chain, record, scan and cut class is
    exercised by at least one (case, capacity) pair the GPU module runs — and no small or chunk case draws a ticket."""
    found = _small_and_chunk_classes()
    want = me.PAYLOAD_CLASSES + me.CHAIN_CLASSES + me.RECORD_CLASSES + me.SCAN_CLASSES + me.CUT_CLASSES
    assert [k for k in want if k not in found] == []
    assert [k for k in me.TICKET_CLASSES if k in found] == []
    # the pairs are where they are meant to be
    assert "cut_on_chunk" in me.census(me.case("steps_16385"), (16385, me.case("steps_16385").survivors(me.CHUNK)), "chain", 256)
    assert "header_above_capacity" in me.census(me.case("mixed_65"), (64, 4000), "scattered", 256)


@pytest.mark.parametrize("num_cus", me.NUM_CUS)
def test_every_ticket_class_is_shown_on_this_part(num_cus):
    """The device-derived sizes draw the tickets they are for on a part of 256 (the MI355X), 304 and 64 compute units."""
    ev = [me.device_case("eval", n, num_cus) for n in me.eval_sizes(num_cus)]
    ch = [me.device_case("chain", n, num_cus) for n in me.chain_sizes(num_cus)]

    def classes(c, layout):
        return me.census(c, (c.n, c.survivors() + 8), layout, num_cus) & set(me.TICKET_CLASSES)

    for layout in ("scattered", "chain"):
        got = [classes(c, layout) - {"emit_ticketed_groups", "emit_slow_group_ticketed"} for c in ev]
        assert got == [{"eval_tickets_none_taken"}, {"eval_one_ticketed_tile"}, {"eval_ticketed_round"},
                       {"eval_ticketed_round"}], (layout, got)
    assert all(classes(c, "scattered") & {"emit_ticketed_groups", "emit_slow_group_ticketed"} == set() for c in ev + ch)
    got = [classes(c, "chain") & {"emit_ticketed_groups", "emit_slow_group_ticketed"} for c in ch]
    assert got == [set(), {"emit_ticketed_groups", "emit_slow_group_ticketed"},
                   {"emit_ticketed_groups", "emit_slow_group_ticketed"}], got
    # the planted full group is the first ticketed one (or the last static one), and it is the general form's
    G = me.chain_stride(num_cus, ch[1].n)
    assert [c.full_group for c in ch] == [4 * G - 1, 4 * G, 4 * G]
    for c in ch:
        g = c.full_group
        assert int(c.pops[g * me.GROUP:(g + 1) * me.GROUP].sum()) == me.GROUP * me.LANES > 128
    # pass 1 walks a plain grid stride: no ticket class, whatever the size
    assert me.census(ev[3], (ev[3].n, 8), "scattered", num_cus, occlusion_pass=1) & set(me.TICKET_CLASSES) == set()
