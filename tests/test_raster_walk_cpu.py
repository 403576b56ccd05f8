"""CPU checks of the walker pins (tests/raster_walk_cases.py): on every case and every capped-grid
list the host mirror — the GPU tests' reference — equals the numpy restatement the flags need (raster_ref,
raster_vis_ref, raster_clip_ref, raster_wide_ref) byte for byte and counter for counter, on both raster calls; every
case reaches what it claims, the route to the lane or the wave included; the cases named for the pieces form give the
unflagged bytes under either flag and both; and the arrangements of commands on the waves of a capped grid, computed
from the assignment alone, all occur.  No GPU: this is the check that the reference stays within every claim."""
import numpy as np
import pytest

import raster_cases as rc
import raster_ref as ref
import raster_walk_cases as wk

CASES = wk.all_cases()
LISTS = wk.grid_lists()


def assert_same(name, got, want, view=np.uint64):
    buf, stats, err = got
    wbuf, wstats, werr, _ = want
    for k in ref.STAT_NAMES:
        assert int(stats[k]) == wstats[k], f"{name}: {k} = {int(stats[k])}, restated {wstats[k]}"
    assert list(err) == werr, name
    diff = np.argwhere(buf.view(view) != np.asarray(wbuf).view(view))
    assert len(diff) == 0, f"{name}: {len(diff)} pixels differ, first at (y, x) = {diff[0]}"


def mirror_against_restatement(case, clip_near=None, wide=False):
    """both calls of the mirror against the restatement -> (mirror's visibility result, depth result, extras)"""
    pk = rc.Packed(case)
    vis, depth = wk.host_vis(pk, clip_near, wide), wk.host_depth(pk, clip_near, wide)
    want = wk.restated_vis(pk, clip_near, wide)
    assert_same(case.name, vis, want)
    assert_same(case.name, depth, wk.restated_depth(pk, clip_near, wide), np.uint32)
    return vis, depth, want[3]


def test_the_case_set_reaches_what_it_claims(capsys):
    missed = {k: v for k, v in wk.census(CASES + LISTS).items() if v}
    assert not missed, missed
    assert len(capsys.readouterr().out.splitlines()) == len(CASES) + len(LISTS)
    names = [c.name for c in CASES + LISTS]
    assert len(set(names)) == len(names)


def test_the_ladder_holds_every_box_at_every_origin_both_ways():
    for r in wk.RESIDUES:
        pages = wk.pack(wk.LADDER, r)
        assert sorted((w, h) for p in pages for _, _, w, h in p) == sorted(wk.LADDER)
        assert all(x % 8 == r and y % 8 == r for p in pages for x, y, _, _ in p)
        for kind in ("rects", "corners"):
            assert sum(c.name.startswith(f"ladder_{kind}_origin_{r}_") for c in CASES) == len(pages)
    assert sum(w * h <= 16 for w, h in wk.LADDER) == 5 and min(w * h for w, h in wk.LADDER if w * h > 16) == 17
    first = next(c for c in CASES if c.name == "ladder_rects_origin_0_page_0")
    assert 0 < first.routes[0] < first.routes[0] + first.routes[1]  # lane-walked and wave-walked in one chunk


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_mirror_equals_the_restatement(case):
    vis, depth, extras = mirror_against_restatement(case)
    assert not wk.check_claims(case, vis[0], vis[1], vis[2], extras)  # the claims hold on the mirror's own output
    assert (vis[0] >> np.uint64(32)).astype(np.uint32).tobytes() == depth[0].view(np.uint32).tobytes()  # V4
    assert vis[1].tobytes() == depth[1].tobytes()


@pytest.mark.parametrize("name", wk.PIECES_CASES)
def test_the_flags_change_nothing_on_walker_shapes(name):
    """Nothing of these cases crosses the near plane or the band: under either flag the mirror still equals the
    restatement that flag needs, and its bytes and counters are the unflagged call's."""
    case = next(c for c in CASES if c.name == name)
    plain_vis, plain_depth, _ = mirror_against_restatement(case)
    assert int(plain_vis[1]["clip_skipped"]) == int(plain_vis[1]["guard_skipped"]) == 0
    for clip_near, wide in wk.FLAG_SETS[1:]:
        vis, depth, extras = mirror_against_restatement(case, clip_near, wide)
        assert wk.routes_of(extras) == tuple(case.routes), (name, clip_near, wide)
        assert vis[0].tobytes() == plain_vis[0].tobytes() and vis[1].tobytes() == plain_vis[1].tobytes(), (name, clip_near, wide)
        assert depth[0].tobytes() == plain_depth[0].tobytes() and depth[1].tobytes() == plain_depth[1].tobytes(), (name, clip_near, wide)


def test_the_pieces_subset_names_the_ladder_lane_0_the_sliver_and_the_chunks():
    for prefix in ("ladder_rects", "ladder_corners", "lane_0_owns_nothing", "empty_sliver", "chunks_nt"):
        assert any(n.startswith(prefix) for n in wk.PIECES_CASES), prefix
    own = next(c for c in CASES if c.name == "two_wave_pieces_beside_a_wave_triangle")
    assert own.clip_near and not own.pieces


@pytest.mark.parametrize("case", LISTS, ids=[c.name for c in LISTS])
def test_host_mirror_equals_the_restatement_on_the_capped_lists(case):
    vis, depth, extras = mirror_against_restatement(case)
    assert not wk.check_claims(case, vis[0], vis[1], vis[2], extras)
    # the visibility call fails exactly the commands the list names; the depth call draws the one of 257 triangles
    count = min(int(rc.Packed(case).words[0]), rc.Packed(case).max_commands)
    named = {k: v for k, v in case.faults.items() if k < count}
    assert [k for k, e in enumerate(vis[2]) if e] == sorted(named), case.name
    assert [k for k, e in enumerate(depth[2]) if e] == sorted(k for k, v in named.items() if v != "nt_257"), case.name


def test_every_arrangement_occurs_under_the_caps():
    """(a)-(f) of raster_walk_cases.arrangements, from the host-side assignment of commands to waves alone."""
    sizes = sorted({len(c.meshlets) for c in LISTS})
    assert sizes == [1, 2, 3, 4, 5, 8, 9, 33]
    found = {1: set(), 2: set()}
    for case in LISTS:
        pk = rc.Packed(case)
        _, _, errors = wk.host_vis(pk)
        for cap in found:
            found[cap] |= wk.arrangements(pk, errors, cap)
    assert found[1] >= set(wk.ARRANGEMENTS), set(wk.ARRANGEMENTS) - found[1]
    assert found[2] >= set(wk.ARRANGEMENTS) - set(wk.NOT_UNDER_TWO_WORKGROUPS), set(wk.ARRANGEMENTS) - found[2]
    # the depth call, which has no triangle limit, still meets every other way to fail
    depth_found = set()
    for case in LISTS:
        pk = rc.Packed(case)
        depth_found |= wk.arrangements(pk, wk.host_depth(pk)[2], 1)
    assert depth_found >= set(wk.ARRANGEMENTS) - {"b:nt_257"}
    # the assignment itself: wave k of c workgroups takes k, k + 4 c, ...
    assert wk.assignment(9, 1) == [[0, 4, 8], [1, 5], [2, 6], [3, 7]]
    assert wk.assignment(3, 2) == [[0], [1], [2], [], [], [], [], []]


def test_a_vertex_word_fault_lies_behind_vertices_already_transformed():
    """The command whose only fault is one index word: the word is the command's last, so the lanes in front of it have
    written their vertices to LDS by the time the wave learns that the command is skipped."""
    case = next(c for c in LISTS if c.name == "grid_9_vertex_word")
    pk = rc.Packed(case)
    cmd = pk.commands[4]
    first, nv = int(cmd["cmd_vertex_offset"]), int(cmd["cmd_first_index"]) // 4 - int(cmd["cmd_vertex_offset"])
    sums = int(cmd["meshlet_vertex_offset"]) + pk.meshlet_data[first:first + nv].astype(np.int64)
    assert nv > 1 and (sums[:-1] < pk.vertex_count).all() and sums[-1] == pk.vertex_count


def test_the_wrapping_sum_is_a_range_error_on_all_three_sides():
    """R9 compares vertex_base + word with vertex_count: the sum is >= 2^32, whatever its low 32 bits name."""
    case = next(c for c in CASES if c.name == "r9_wrapping_sum")
    pk = rc.Packed(case)
    cmd = pk.commands[1]
    words = pk.meshlet_data[int(cmd["cmd_vertex_offset"]):int(cmd["cmd_first_index"]) // 4].astype(np.int64)
    sums = int(cmd["meshlet_vertex_offset"]) + words
    assert sums.max() >= 1 << 32 and ((sums & 0xFFFFFFFF) < pk.vertex_count).all()
    for result in (wk.host_vis(pk), wk.host_depth(pk)):
        assert list(result[2]) == [0, 1, 0]
    for clip_near, wide in wk.FLAG_SETS:
        assert wk.restated_vis(pk, clip_near, wide)[2] == [0, 1, 0] and wk.restated_depth(pk, clip_near, wide)[2] == [0, 1, 0]
