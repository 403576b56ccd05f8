"""tests/visibility_tile_cases.py on the CPU: every programme and every second-round list through the
host mirrors — host_visibility_resolve, host_visibility_compact in both modes, host_visibility_surface with and without
CLEAR —, whose outputs, counters and status equal the numpy restatements' byte for byte; each case's closed-form claims
hold on the restatement; the table of which kind of tile feeds which counter is what the restatements count on that tile
alone; and arrangements(), from the assignment alone, returns everything under a cap of 1 and of 2 workgroups and the
reduced set when every wave takes one tile.  No GPU."""
import numpy as np
import pytest

import raster_vis_ref as vref
import visibility_compact_ref as cref
import visibility_surface_ref as sref
import visibility_tile_cases as tc
from orbit_amd import raster

FILL = 0xA5A5A5A5  # what an output holds before the call
MODES = (False, True)
KEYS = ("bary", "grad", "triangle")
PROGS = tc.programmes()
LISTS = tc.second_round_cases()


def resolve_same(name, vis, base, n):
    depth, pixels, stats = raster.host_visibility_resolve(vis, base, n)
    want_depth, want_pixels, want = vref.resolve(vis, base, n)
    assert depth.tobytes() == want_depth.tobytes() and pixels.tobytes() == want_pixels.tobytes(), name
    assert {k: int(stats[k]) for k in want} == want, name
    return want, want_pixels


def compact_same(name, case, triangles, **over):
    a, kw = case.args(triangles, fill=FILL, **over)
    got, want = raster.host_visibility_compact(*a, **kw), cref.compact(*a, **kw)
    assert {k: int(got["stats"][k]) for k in cref.STAT_NAMES} == want["stats"], name
    assert got["status"] == want["status"], name
    for k in ("masks", "commands", "ids", "data"):
        assert (got[k] is None) == (want[k] is None), (name, k)
        if got[k] is not None:
            diff = np.flatnonzero(got[k] != want[k])
            assert len(diff) == 0, f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}"
    return want


def surface_same(name, case, clear):
    a, kw = case.args(fill=FILL, clear=clear)
    got, want = raster.host_visibility_surface(*a, **kw), sref.surface(*a, **kw)
    assert {k: int(got["stats"][k]) for k in sref.STAT_NAMES} == want["stats"], name
    assert got["status"] == want["status"] == (sref.E_RANGE if want["stats"]["stale_pixels"] else 0), name
    for k in KEYS:
        diff = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(diff) == 0, f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}"
    return want


def holds(name, claimed, stats):
    for k, v in claimed.items():
        assert stats[k] == v, f"{name}: {k} = {stats[k]}, claimed {v}"


# -- 1. the programmes: mirror == restatement, and the claims
@pytest.mark.parametrize("prog", PROGS, ids=[p.name for p in PROGS])
def test_the_three_mirrors_equal_the_restatements_on_a_programme(prog):
    n = prog.max_commands
    stats, pixels = resolve_same(prog.name, prog.visibility, tc.BASE, n)
    holds(prog.name + " resolve", prog.expect["resolve"], stats)
    assert pixels.all()  # every command owns a pixel, the ones the raster skipped by hand
    for triangles in MODES:
        want = compact_same(f"{prog.name} (triangles={triangles})", prog.compact, triangles)
        holds(f"{prog.name} compact (triangles={triangles})", prog.expect["compact"], want["stats"])
        assert want["status"] == 0
    for clear in (False, True):
        want = surface_same(f"{prog.name} (clear={clear})", prog.surface, clear)
        holds(prog.name + " surface", prog.expect["surface"], want["stats"])
    # the stale pixels are the ones written by hand, and nothing else is left unwritten but the foreign and the cut ones
    untouched = (want["triangle"] == 0xFFFFFFFF).all(axis=2)
    assert all(untouched[y, x] for y, x in prog.surface.stale)
    st = want["stats"]
    assert int((~untouched).sum()) == st["written_pixels"]
    assert st["covered_pixels"] == st["written_pixels"] + st["foreign_pixels"] + st["unsupported_pixels"] + st["stale_pixels"]


def test_the_main_programme_has_the_shape_the_edges_need():
    main = PROGS[0]
    assert (main.width, main.height) == (tc.MAIN_W, tc.MAIN_H) and main.width <= 80 and main.height <= 40
    tiles_x, tiles_y = (main.width + 7) // 8, (main.height + 7) // 8
    assert main.width % 8 == 1 and main.height % 8 == 1 and tiles_y >= 4  # a partial tile on both edges, of one pixel
    for t, kind in enumerate(main.kinds):
        assert (kind == "Py") == (t // tiles_x == tiles_y - 1) and (kind == "Px") == (t % tiles_x == tiles_x - 1 and t // tiles_x < tiles_y - 1)
    assert {tc.base_kind(k) for k in main.kinds} == set(tc.SHARES) - {"W"}  # (W: the one-row target's)
    assert {k for k in main.kinds if k.startswith("S:")} == {f"S:{w}" for w in tc.S_WAYS}
    assert main.max_commands > tc.CHUNK  # (the programme's list also crosses a block of the scan)
    # the ring: triangles 0, 32 and 33 of ONE command own a whole tile each
    k = ((main.visibility >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64) - tc.BASE
    t = (main.visibility & np.uint64(255)).astype(np.int64)
    assert sorted(np.unique(t[(k == 0) & (main.visibility != 0)])) == [0, 32, 33]
    assert all(int(((k == 0) & (t == q) & (main.visibility != 0)).sum()) == 64 for q in (0, 32, 33))


def test_a_tile_of_each_kind_feeds_the_counters_the_table_says():
    """SHARES is what arrangements() derives (i) from: each kind's first tile alone in the buffer, through the restatements"""
    seen = set()
    for main in (PROGS[0], PROGS[3]):
        feeds_what_the_table_says(main, seen)
    assert {tc.base_kind(k) for k in seen} == set(tc.SHARES)


def feeds_what_the_table_says(main, seen):
    tiles_x = (main.width + 7) // 8
    ys, xs = np.mgrid[0:main.height, 0:main.width]
    tile_of_pixel = (ys // 8) * tiles_x + xs // 8
    for tile, kind in enumerate(main.kinds):
        b = tc.base_kind(kind)
        if kind in seen:
            continue
        seen.add(kind)
        vis = np.where(tile_of_pixel == tile, main.visibility, np.uint64(0))
        _, _, r = vref.resolve(vis, tc.BASE, main.max_commands)
        a, kw = main.compact.args(False)
        c = cref.compact(vis, *a[1:], **kw)["stats"]
        a, kw = main.surface.args()
        s = sref.surface(vis, *a[1:], **kw)["stats"]
        fed = {f"resolve.{k}" for k, v in r.items() if v} | {f"compact.{k}" for k in ("covered_pixels", "foreign_pixels") if c[k]} | \
            {f"surface.{k}" for k, v in s.items() if v}
        assert fed == set(tc.SHARES[b]), (tile, kind, fed)
        if b == "K":
            assert c["visible_triangles"] == c["visible_commands"] == 64
        if b == "O":
            assert c["visible_triangles"] == c["visible_commands"] == 1 and s["written_pixels"] == 64
        if b == "M":
            assert (c["visible_commands"], c["visible_triangles"], s["foreign_pixels"], s["covered_pixels"]) == (2, 3, 3, 25)
        if b == "F":
            ids = np.unique(((vis[vis != 0] >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64))
            assert list(ids) == [tc.BASE - 1, tc.BASE + main.max_commands]  # both sides of the range
        if b == "W":
            assert (c["visible_commands"], c["visible_triangles"], s["written_pixels"]) == (1, 1, 8)


# -- 2. the arrangements, from the assignment alone
@pytest.mark.parametrize("cap", (1, 2))
def test_every_arrangement_occurs_under_the_cap(cap):
    found = tc.arrangements_of(PROGS, cap)
    assert found == set(tc.ARRANGEMENTS), sorted(set(tc.ARRANGEMENTS) - found)
    main = tc.arrangements(PROGS[0].kinds, PROGS[0].tiles, cap)
    assert set(tc.ARRANGEMENTS) - main == {"c:F_alone", "g:own_bit", "h:idle_wave"}  # what the small targets are there for
    assert "g:own_bit" in tc.arrangements(PROGS[3].kinds, PROGS[3].tiles, cap)
    assert "c:F_alone" in tc.arrangements(PROGS[1].kinds, PROGS[1].tiles, cap)
    assert "h:idle_wave" in tc.arrangements(PROGS[2].kinds, PROGS[2].tiles, cap)


def test_the_ring_and_the_shared_key_fall_to_one_wave_under_both_caps():
    """(g) spelled out, not only through arrangements(): triangles 0 and 32 of the ring — bit 0 of two mask words — in two
    trips of one wave, triangle 33 in another wave; the W key in two (cap 2) and three (cap 1) trips of one wave"""
    main, row = PROGS[0], PROGS[3]
    tile_of = {k: t for t, k in enumerate(main.kinds) if k.startswith("O:r")}
    assert sorted(tile_of) == ["O:r0", "O:r32", "O:r33"]
    for cap in (1, 2):
        wave_of = {t: g for g, w in enumerate(tc.assignment(main.tiles, cap)) for t in w}
        assert wave_of[tile_of["O:r0"]] == wave_of[tile_of["O:r32"]] != wave_of[tile_of["O:r33"]], cap
        shared = [t for t, k in enumerate(row.kinds) if k == "W"]
        waves = [set(w) & set(shared) for w in tc.assignment(row.tiles, cap)]
        assert max(len(w) for w in waves) == (3 if cap == 1 else 2), cap
    k = ((row.visibility >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64) - tc.BASE
    own = (row.visibility != 0) & (k == 0)  # the W triangle is command 0, triangle 0
    assert (row.visibility[own] & np.uint64(255) == 0).all()
    assert sorted(np.flatnonzero(own[0])) == list(range(0, 8)) + list(range(32, 40)) + [64] and not own[1:].any()
    # ... and with g:two_words asking for t and t + 32, the layout as it was before (r33 where r32 is) would not pass
    swapped = tuple({"O:r32": "O:r33", "O:r33": "O:r32"}.get(q, q) for q in main.kinds)
    assert all("g:two_words" not in tc.arrangements(swapped, main.tiles, cap) for cap in (1, 2))


def test_the_uncapped_grid_gives_every_wave_one_tile():
    for p in PROGS:
        waves = tc.assignment(p.tiles, 0, 2048)
        assert all(len(w) <= 1 for w in waves) and sorted(t for w in waves for t in w) == list(range(p.tiles))
    assert tc.arrangements_of(PROGS, 0, 2048) == set(tc.UNCAPPED)


def test_the_assignment_is_the_kernels_formula():
    assert tc.assignment(50, 1) == [list(range(g, 50, 4)) for g in range(4)]
    assert tc.assignment(50, 2) == [list(range(g, 50, 8)) for g in range(8)]
    assert tc.assignment(1, 2) == [[0], [], [], []]           # need = 1 workgroup: the cap does not add one
    assert tc.assignment(50, 0, 2048) == [[g] for g in range(50)] + [[], []]  # 13 workgroups
    assert tc.assignment(50, 0, 3)[0] == list(range(0, 50, 12))  # (a 3-workgroup device: the resident grid caps too)


# -- 3. the totals' second round
@pytest.mark.parametrize("case", LISTS, ids=[c.name for c in LISTS])
def test_the_mirror_equals_the_restatement_on_a_second_round_list(case):
    listed = int(case.words[0])
    assert (min(listed, case.max_commands) + tc.CHUNK - 1) // tc.CHUNK > tc.ROUND  # more block totals than one round takes
    words = case.expect_cut["data_words_needed"]
    for triangles in MODES:
        want = compact_same(f"{case.name} (triangles={triangles})", case, triangles, visible_data_words=words if triangles else 0)
        holds(case.name, {**case.expect, **(case.expect_cut if triangles else {})}, want["stats"])
        assert want["status"] == 0
        for j, k in case.claims:  # everything in front of j is the carry that reached command k's block
            assert int(want["ids"][j]) == k, (case.name, j, k)
        n = want["stats"]["written_commands"]
        assert (want["commands"][1 + 7 * n:] == FILL).all() and (want["ids"][n:] == FILL).all()
        if triangles:
            rows = want["commands"][1:1 + 7 * n].reshape(n, 7)
            sizes = np.diff(np.append(rows[:, 3], words))
            assert set(sizes.tolist()) <= {4, 5, 6} and (rows[:, 2] == 4 * (rows[:, 3] + 3)).all()
            assert case.name != "chunks_258" or set(sizes.tolist()) == {4, 5, 6}  # regions of unequal size
    if case.name == "chunks_258":  # the carry that crosses the round: 3 + CHUNK commands in front of chunk 256's first
        assert case.claims[0] == (3 + tc.CHUNK, 256 * tc.CHUNK)


def test_capacities_cut_the_prefix_in_round_two():
    case = next(c for c in LISTS if c.name == "chunks_258")
    a, kw = case.args(True, visible_data_words=case.expect_cut["data_words_needed"])
    full = cref.compact(*a, **kw)["stats"]
    variants = tc.second_round_capacities(full)
    assert [v[0] for v in variants] == ["capacity_exact", "capacity_one_less", "data_words_one_less", "plain_capacity_exact",
                                         "plain_capacity_one_less"]
    for what, over, triangles in variants:
        if not triangles:
            over = dict(over, visible_data_words=0)
        want = compact_same(f"chunks_258 {what}", case, triangles, **over)
        exact = "exact" in what
        assert want["status"] == (0 if exact else cref.E_CAPACITY), what
        assert want["stats"]["dropped_commands"] == (0 if exact else 1), what  # the last command, of block 257
        n = want["stats"]["written_commands"]
        assert int(want["ids"][n - 1]) == int(case.words[0]) - (1 if exact else 2)


# -- 4. the resolve's clear
def test_the_resolve_names_what_the_pixels_name_among_5000_entries():
    main = PROGS[0]
    n = tc.RESOLVE_CLEAR_COMMANDS
    stats, pixels = resolve_same("5000 entries", main.visibility, tc.BASE, n)
    assert n > 4 * 1024 and np.count_nonzero(pixels) == main.max_commands + 1 and not pixels[main.max_commands + 1:].any()
