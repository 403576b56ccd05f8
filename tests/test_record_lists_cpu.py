"""The references of tests/record_lists.py against the oracle, and the floors on its inputs (no GPU).

expand_ref is what tests/test_record_lists_gpu.py holds orbit_expand_visible_records to; here it is tied to the oracle —
and through it to the reference's binaries (tests/test_spirv_vectors_cpu.py) — on culled scenes: the record list the
oracle's outputs imply, expanded, is the oracle's MeshletDrawCommandBuffer word for word.  The census floors make sure
the hand-made lists and the sparse scenes keep exercising what they were written for."""
import numpy as np
import pytest

import record_lists as rl
from orbit_amd import layouts as L
from test_gpu_parity import _expected_visible_records, run_oracle

SCENES = [None] + list(rl.KEEPS)  # None: the dense scene


@pytest.fixture(scope="module")
def culled(oracle):
    """keep -> (scene, the oracle's record list as a Case, the oracle's commands), computed once."""
    out = {}
    for keep in SCENES:
        scene = rl.dense_scene() if keep is None else rl.sparse_scene(keep)
        ref = run_oracle(oracle, scene, rl.scene_cull_info())
        _, orecs = L.dispatch_buffer_records(ref[0])
        on, ocmds = L.draw_buffer_commands(ref[1])
        want = _expected_visible_records(orecs, ocmds)
        out[keep] = (scene, rl.scene_case(f"scene_{keep}", want, len(scene.meshlets)), ocmds)
    return out


@pytest.mark.parametrize("keep", SCENES)
def test_expand_ref_is_the_oracles_command_list(culled, keep):
    scene, case, ocmds = culled[keep]
    assert case.S == len(ocmds) > 0
    for cap in rl.capacities(case) + [scene.lod0_meshlets + 8]:
        S, cmds, overflow = rl.expand_ref(case.records, case.n, scene.meshlets, cap)
        assert S == len(ocmds) and overflow == (len(ocmds) > cap) and len(cmds) == min(S, cap)
        assert np.array_equal(cmds.view(np.uint32), ocmds[:cap].view(np.uint32)), f"capacity {cap}"


def test_expand_ref_walks_entries_and_bits_in_order():
    """The vectorised walk against the loop it stands for, on a hand-made list with every kind of entry."""
    meshlets = rl.meshlet_buffer()
    case = rl.LISTS["p64_1025"]
    want = []
    for ent, off, mask in case.records[:case.n].tolist():
        for bit in range(32):
            if mask >> bit & 1:
                m = meshlets[off + bit]
                want.append((int(m["triangle_count"]) * 3, 1, (int(m["data_offset"]) + int(m["vertex_count"])) * 4 % 2 ** 32,
                             int(m["data_offset"]), ent, int(m["vertex_offset"]), off + bit))
    S, cmds, overflow = rl.expand_ref(case.records, case.n, meshlets, len(want) - 3)
    assert S == len(want) == case.S and overflow
    assert np.array_equal(cmds.view(np.uint32).reshape(-1, 7), np.array(want[:-3], dtype=np.uint64).astype(np.uint32))


def test_lists_are_what_they_claim():
    meshlets = rl.meshlet_buffer()
    assert int((meshlets["vertex_count"] == 255).sum()) > 0 and int((meshlets["triangle_count"] == 255).sum()) > 0
    assert int((meshlets["data_offset"] >= 2 ** 32 - 1000).sum()) > 0
    assert sorted({c.n for c in rl.LISTS.values()}) == sorted(rl.COUNTS) == [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097]
    assert {c.name.rsplit("_", 1)[0] for c in rl.LISTS.values()} == set(rl.MASKS)
    for n in (64, 1024, 1025):
        assert rl.LISTS[f"full_{n}"].S == 32 * n
    for n in (1025, 2049, 4097):
        for sparse in ("zero", "p64", "last_only", "first_only"):
            assert f"{sparse}_{n}" in rl.LISTS
    ents = np.concatenate([c.records["entity_index"][:c.n] for c in rl.LISTS.values()])
    assert int((ents == 0xFFFFFFFF).sum()) > 0 and len(np.unique(ents >> 28)) == 16
    for c in rl.LISTS.values():
        assert int(c.records["meshlet_offset"].max(initial=0)) + 31 < rl.N_MESHLETS, "a case reads outside the buffer"
        assert int(c.buffer[4:8].view(np.uint32)[0]) not in (0, c.S)
        p = rl.LISTS.get(f"p64_{c.n}")
        if p is c:  # every bit with probability 1/64: half a survivor per record
            assert 0.3 * c.n < c.S < 0.7 * c.n


def test_census_floors_of_the_lists():
    meshlets = rl.meshlet_buffer()
    seen = {}
    for case in rl.LISTS.values():
        caps = rl.capacities(case)
        assert {case.S + 8, case.S, 0} <= set(caps) and (case.S == 0 or case.S - 1 in caps)
        for cap in caps:
            for cls in rl.census(case, cap, meshlets):
                seen.setdefault(cls, []).append((case.name, cap))
    for cls in rl.CLASSES:
        assert seen.get(cls), f"no (list, capacity) pair exercises {cls}"


@pytest.mark.parametrize("keep", rl.KEEPS)
def test_census_floors_of_the_sparse_scenes(culled, keep):
    """A sparse frame whose command buffer is sized for what survives: more blocks of records than blocks of commands."""
    scene, case, ocmds = culled[keep]
    empty = int((case.records["mask"][:case.n] == 0).sum())
    assert empty >= 0.75 * case.n, "too few empty records"
    assert 0 < case.S < case.n / 2, "too many survivors"
    assert -(-case.S // rl.BLOCK) < -(-case.n // rl.BLOCK)
    for cap in (case.S, case.S + 1):
        assert "fits_but_fewer_grid_blocks_than_record_blocks" in rl.census(case, cap, scene.meshlets)
    assert int(case.before[rl.BLOCK]) < case.S, "every survivor is in the first block of records"
    if keep == 0.05:  # the numbers the defect was found with
        assert (case.n, empty, case.S, int(case.before[rl.BLOCK])) == (2318, 1783, 760, 350)


@pytest.mark.parametrize("world,header,stride", [(1, 8, 12), (3, 8, 12), (8, 4, 28), (5, 16, 8)])
def test_compact_ref_is_the_rank_ordered_concatenation(world, header, stride):
    rng = np.random.default_rng(world)
    cap = 50
    seg_bytes = header + stride * cap
    seg = rng.integers(0, 256, world * seg_bytes, dtype=np.uint8)
    counts = [int(c) for c in rng.integers(0, cap + 1, world)]
    counts[0] = cap + 9 if world > 1 else 7  # a sender's overflow: cut at the segment's capacity
    for r in range(world):
        seg[seg_bytes * r:seg_bytes * r + 4].view(np.uint32)[0] = counts[r]
    items = b""
    for r in range(world):
        items += seg[seg_bytes * r + header:seg_bytes * r + header + stride * min(counts[r], cap)].tobytes()
    total = len(items) // stride
    for out_cap in (total + 5, total, total - 1, total // 2, 0):
        got, overflow = rl.compact_ref(seg, world, cap, out_cap, header, stride)
        kept = min(total, out_cap)
        assert overflow == (total > out_cap) and len(got) == header + stride * kept
        assert list(got[:header].view(np.uint32)) == [kept] + [0] * (header // 4 - 1)
        assert got[header:].tobytes() == items[:stride * kept]
