"""tests/surface_tile_cases.py on the CPU: arrangements(), from the layouts and the assignment formula
alone, returns everything under a cap of 1 and of 2 workgroups, before anything is rasterised; every programme, read with
flags 40 and with flags 8, through the host mirror orbit_amd.raster.host_visibility_surface_drawn, whose outputs, counters
and status equal the restatement tests/surface_drawn_ref.py's byte for byte, with and without CLEAR; every programme's
FragCase, and visibility_tile_cases' programmes as FragCases, through host_surface_fragments against
tests/surface_fragments_ref.py, stats and status included; each programme's closed-form claims hold; every kind of tile
holds what its description says (which candidate owns its pixels, how many keys, which verdict under which flags); and
the table of which kind feeds which counter is what the restatements count on that tile alone.  No GPU."""
import numpy as np
import pytest

import surface_drawn_ref as dref
import surface_fragments_ref as fref
import surface_tile_cases as st
import test_surface_fragments_cpu as tfc
from orbit_amd import raster

FILL = 0xA5A5A5A5  # what an output holds before the call
KEYS = ("bary", "grad", "triangle")


# -- 1. the arrangements, from the layouts and the assignment alone: nothing is rasterised before this has passed
@pytest.mark.parametrize("cap", (1, 2))
def test_every_arrangement_occurs_under_the_cap(cap):
    found = st.arrangements_of(st.LAYOUTS, cap)
    assert found == set(st.ARRANGEMENTS), f"missing under a cap of {cap}: {sorted(set(st.ARRANGEMENTS) - found)}"
    main = st.arrangements(st.MAIN_KINDS, 50, cap)
    assert "h:idle_wave" not in main and "h:idle_wave" in st.arrangements(("C2",), 1, cap)  # what the 7 x 5 target is there for
    assert "CPy_last" in main and "partial_slow>full" in main  # (the partial tiles are the main target's)


def test_the_layouts_have_the_shape_the_edges_need():
    assert (st.MAIN_W, st.MAIN_H) == (73, 33) and len(st.MAIN_KINDS) == 50 and len(st.SECOND_KINDS) == 32
    assert all(max(w, h) <= 80 and min(w, h) <= 40 for w, h in ((st.MAIN_W, st.MAIN_H), (st.SECOND_W, st.SECOND_H)))
    assert st.MAIN_W % 8 == 1 and st.MAIN_H % 8 == 1  # a one-pixel last column and a one-pixel last row
    for t, kind in enumerate(st.MAIN_KINDS):
        assert (kind in ("Py", "CPy")) == (t // 10 == 4) and (kind in ("Px", "CPx")) == (t % 10 == 9 and t // 10 < 4), (t, kind)
    assert set(st.MAIN_KINDS) == set(st.KINDS)  # every kind in the main target
    assert st.MAIN_KINDS[49] == "CPy"  # the corner tile, one pixel: a cut key on one lane
    assert len(st.ARRANGEMENTS) == len(set(st.ARRANGEMENTS)) == len(st.RULES) + 2 + 8 + 6


def test_the_uncapped_grid_gives_every_wave_one_tile():
    for kinds, tiles in st.LAYOUTS:
        waves = st.assignment(tiles, 0, 2048)
        assert all(len(w) <= 1 for w in waves) and sorted(t for w in waves for t in w) == list(range(tiles))
    assert st.arrangements_of(st.LAYOUTS, 0, 2048) == set(st.UNCAPPED)


def test_the_rule_table_reads_consecutive_trips_of_one_wave():
    kinds = ("C2", "E", "E", "E", "O", "E", "E", "E", "C2", "E", "E", "E")  # wave 0 of one workgroup: C2, O, C2
    assert "slow>fast>slow" in st.arrangements(kinds, 12, 1) and "slow>fast>slow" not in st.arrangements(kinds, 12, 2)
    kinds = ("C2",) + ("E",) * 7 + ("C1",) + ("E",) * 7 + ("C2",) + ("E",) * 7  # wave 0 of two workgroups
    assert "cand1>no_cand1>cand1" in st.arrangements(kinds, 24, 2) and "cand1>no_cand1>cand1" not in st.arrangements(kinds, 24, 1)
    assert "fast>slow" in st.arrangements(("O", "E", "E", "E", "Sm"), 5, 1) and "fast>slow" not in st.arrangements(("O", "Sm"), 2, 1)
    # a counter needs two trips of one wave AND a second wave
    assert "i:drawn.stale_pixels" not in st.arrangements(("Sm", "E", "E", "E", "Sm"), 5, 1)
    assert "i:drawn.stale_pixels" in st.arrangements(("Sm", "Sm", "E", "E", "Sm"), 5, 1)


# -- 2. the programmes
@pytest.fixture(scope="module")
def progs():
    return st.programmes() + [st.tamper_free_programme()]


@pytest.fixture(scope="module")
def restated(progs):
    """{(name, flags): the drawn restatement's outputs and detail, without CLEAR}; computed once, shared, left unchanged"""
    out = {}
    for p in progs:
        for case in (p.surface, p.surface8):
            a, kw = case.args(fill=FILL, clear=False)
            out[p.name, case.raster_flags] = dref.surface(*a, **kw, keep_detail=True)
    return out


def drawn_same(name, case, want, clear):
    a, kw = case.args(fill=FILL, clear=clear)
    got = raster.host_visibility_surface_drawn(*a, **kw)
    assert {k: int(got["stats"][k]) for k in dref.STAT_NAMES} == want["stats"], name
    assert got["status"] == want["status"] == (dref.E_RANGE if want["stats"]["stale_pixels"] else 0), name
    for k in KEYS:
        diff = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(diff) == 0, f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}"


def holds(name, claimed, stats):
    for k, v in claimed.items():
        assert int(stats[k]) == v, f"{name}: {k} = {int(stats[k])}, claimed {v}"


def test_the_programmes_are_the_layouts(progs):
    assert [(p.kinds, p.tiles) for p in progs[:3]] == [(tuple(k), t) for k, t in st.LAYOUTS]
    assert [p.tamper_free for p in progs] == [False, False, True, True]
    assert (progs[0].stale, progs[0].frag_stale, progs[1].stale, progs[1].frag_stale) == (True, True, True, True)
    assert not progs[2].stale and not progs[3].stale and not progs[3].frag_stale
    assert set(progs[3].kinds) == set(st.KINDS) - set(st.AT_ONCE)


@pytest.mark.parametrize("flags", (40, 8))
def test_the_drawn_mirror_equals_the_restatement_on_a_programme(progs, restated, flags):
    for p in progs:
        case = p.surface if flags == 40 else p.surface8
        want = restated[p.name, flags]
        drawn_same(f"{case.name}", case, want, False)
        a, kw = case.args(fill=FILL, clear=True)
        drawn_same(f"{case.name} (clear)", case, dref.surface(*a, **kw), True)
        st_ = want["stats"]
        holds(case.name, case.expect, st_)
        assert want["status"] == (dref.E_RANGE if p.stale else 0), case.name
        assert st_["covered_pixels"] == st_["written_pixels"] + st_["foreign_pixels"] + st_["unsupported_pixels"] + st_["stale_pixels"]
        assert want["detail"]["owned_by_two"] == 0, case.name
        untouched = (want["triangle"] == FILL).all(axis=2)
        assert all(untouched[y, x] for y, x in case.stale) and int((~untouched).sum()) == st_["written_pixels"], case.name
        if flags == 40:
            assert st_["unsupported_pixels"] == 0 and st_["cut_pixels"] > 0, case.name


def tile_slice(p, tile):
    tiles_x = (p.width + 7) // 8
    return slice(8 * (tile // tiles_x), 8 * (tile // tiles_x) + 8), slice(8 * (tile % tiles_x), 8 * (tile % tiles_x) + 8)


def test_every_tile_holds_what_its_kind_says(progs, restated):
    seen = set()
    for p in progs:
        both, clip = restated[p.name, 40], restated[p.name, 8]
        owner, setups = both["detail"]["owner"], both["detail"]["setups"]
        for tile, kind in enumerate(p.kinds):
            at = tile_slice(p, tile)
            own = owner[at]
            owners = sorted(set(own.reshape(-1).tolist()) - {-1})
            keys = np.unique(p.visibility[at][p.visibility[at] != 0] & np.uint64(0xFFFFFFFF))
            what = (p.name, tile, kind)
            seen.add(kind)
            is_new = lambda v: v["t"] is not None  # noqa: E731
            if kind in ("O", "T", "U", "TU", "N"):
                assert len(keys) == len(owners) == 1 and (own >= 0).all() and not setups[owners[0]][1] and not setups[owners[0]][0]["wide"], what
            elif kind == "C1":  # one piece, both its later vertices new: (a, N(a, b), N(a, c))
                s, cut, _ = setups[owners[0]]
                assert len(keys) == len(owners) == 1 and (own >= 0).all() and cut and not is_new(s["verts"][0]) and is_new(s["verts"][1]) and \
                    is_new(s["verts"][2]), what
                assert own.size == 64, what
            elif kind in ("CPx", "CPy"):  # C2's key on the lanes of one column or one row
                assert len(keys) == 1 and 1 <= len(owners) <= 2 and (own >= 0).all() and all(setups[q][1] for q in owners), what
                assert own.shape == ((min(8, p.height - at[0].start), 1) if kind == "CPx" else (1, min(8, p.width - at[1].start))), what
            elif kind == "C2":   # piece 0 = (b, c, Q) and piece 1 = (b, Q, P) of ONE key
                verts = [setups[q][0]["verts"] for q in owners]
                assert len(keys) == 1 and len(owners) == 2 and (own >= 0).all() and all(setups[q][1] for q in owners), what
                assert [[is_new(v) for v in vs] for vs in verts] == [[False, False, True], [False, True, True]], what
                assert min(int((own == q).sum()) for q in owners) >= (24 if own.size == 64 else 8), what
            elif kind == "C2a":  # piece 0 of a one-out cut alone: the key has two candidates and nobody asks the second
                s, cut, _ = setups[owners[0]]
                assert len(keys) == len(owners) == 1 and (own >= 0).all() and cut and [is_new(v) for v in s["verts"]] == [False, False, True], what
            elif kind == "Wd":
                s, cut, _ = setups[owners[0]]
                assert len(keys) == len(owners) == 1 and (own >= 0).all() and not cut and s["wide"], what
                assert (clip["detail"]["owner"][at] == -1).all(), what  # with flags 8: unsupported, all of them
            elif kind == "Un":   # the wide piece (b, Q, P) owns the tile
                s, cut, _ = setups[owners[0]]
                assert len(keys) == len(owners) == 1 and (own >= 0).all() and cut and s["wide"], what
                assert [is_new(v) for v in s["verts"]] == [False, True, True] and (clip["detail"]["owner"][at] == -1).all(), what
            elif kind in ("K", "KS", "K1", "KA"):
                slow = [q for q in owners if setups[q][1] or setups[q][0]["wide"]]
                assert len(keys) == len(owners) == 64 and (own >= 0).all(), what
                assert len(slow) == dict(K=0, KS=40, K1=1, KA=64)[kind], what
                if kind == "KS":
                    assert sum(1 for q in slow if setups[q][0]["wide"]) == 8 and sum(1 for q in slow if setups[q][1]) == 32, what
            elif kind == "Sm":   # the tile's first pixel names the cut key and neither piece owns it
                assert len(keys) == 1 and own[0, 0] == -1 and 0 < len(owners) <= 2 and all(setups[q][1] for q in owners), what
                assert p.visibility[at][0, 0] != 0 and (p.visibility[at][0, 0] & np.uint64(0xFFFFFFFF)) == keys[0], what
                assert int((own >= 0).sum()) == int((p.visibility[at] != 0).sum()) - 1 >= 12, what
            elif kind == "Big":  # triangles 0 and 23 of one command of 70 vertices and 72 corner bytes
                k = int(keys[0] >> np.uint64(8)) - st.BASE
                cmd = p.packed.commands[k]
                assert sorted((keys & np.uint64(255)).tolist()) == [0, 23] and len(set((keys >> np.uint64(8)).tolist())) == 1, what
                assert int(cmd["cmd_index_count"]) == 72 > 64 and len(p.packed.case.meshlets[k].positions) == 70 > 64 and (own >= 0).all(), what
            elif kind == "Px":
                assert len(keys) == len(owners) == own.shape[0] and (own[:, 0] >= 0).all() and (own[:, 1:] == -1).all(), what
            elif kind == "Py":
                assert len(keys) == len(owners) == 1 and (own >= 0).all(), what
            else:
                assert kind in ("E", "F") and not owners and (p.visibility[at] != 0).all() == (kind == "F"), what
    assert seen == set(st.KINDS)


def test_a_tile_of_each_kind_feeds_the_counters_the_table_says(progs):
    """SHARES is what arrangements() derives (i) from: each kind's first tile alone in the buffer, through the restatements
    (drawn with flags 40; drawn.unsupported_pixels with flags 8; the fragments over the programme's surface records)"""
    seen = set()
    for p in progs[:2]:
        ys, xs = np.mgrid[0:p.height, 0:p.width]
        tile_of_pixel = (ys // 8) * ((p.width + 7) // 8) + xs // 8
        for tile, kind in enumerate(p.kinds):
            if kind in seen:
                continue
            seen.add(kind)
            vis = np.where(tile_of_pixel == tile, p.visibility, np.uint64(0))
            a, kw = p.surface.args()
            d40 = dref.surface(vis, *a[1:], **kw)["stats"]
            a, kw = p.surface8.args()
            d8 = dref.surface(vis, *a[1:], **kw)["stats"]
            a, kw = p.frag.args()
            f = fref.fragments(vis, *a[1:], **kw)["stats"]
            fed = {f"drawn.{k}" for k, v in d40.items() if v} | ({"drawn.unsupported_pixels"} if d8["unsupported_pixels"] else set()) | \
                {f"frag.{k}" for k in st.FRAG_COUNTERS if f[k]}
            assert fed == set(st.SHARES[kind]), (p.name, tile, kind, sorted(fed))
            assert d40["unsupported_pixels"] == 0
            if kind in ("Wd", "Un"):
                assert d8["unsupported_pixels"] == d40["written_pixels"] == d40["wide_pixels"] == 64 and d8["written_pixels"] == 0
            if kind in ("KS", "KA"):
                assert d8["unsupported_pixels"] == d40["wide_pixels"] == 8
            if kind == "TU":
                assert (f["written_pixels"], f["unshaded_pixels"], f["stale_pixels"]) == (24, 16, 24)
            if kind == "Sm":
                assert d40["stale_pixels"] == d8["stale_pixels"] == 1 and f["unshaded_pixels"] == 1 and f["stale_pixels"] == 0
    assert seen == set(st.KINDS)


# -- 3. the fragments
@pytest.fixture(scope="module")
def frag_cases(progs):
    return [p.frag for p in progs] + st.old_programmes_as_frag_cases()


@pytest.mark.parametrize("clear", (False, True))
def test_the_fragments_mirror_equals_the_restatement(progs, frag_cases, clear):
    assert len(frag_cases) == len(progs) + 4
    unshaded = 0
    for c in frag_cases:
        want = tfc.restate(c, clear=clear)
        tfc.assert_equal(f"{c.name} (clear={clear})", tfc.guarded_mirror(c, clear=clear), want)  # (bytes, the six counters, the status)
        a, kw = c.args(fill=FILL, clear=clear)
        tfc.assert_equal(f"{c.name} (clear={clear}), the Python form", raster.host_surface_fragments(*a, **kw), want)
        s = want["stats"]
        assert s["covered_pixels"] == s["written_pixels"] + s["foreign_pixels"] + s["unshaded_pixels"] + s["stale_pixels"], c.name
        assert want["status"] == (dref.E_RANGE if s["stale_pixels"] else 0), c.name
        unshaded += s["unshaded_pixels"]
    for p in progs:
        want = tfc.restate(p.frag, clear=clear)
        holds(p.name + " fragments", p.expect["frag"], want["stats"])
        assert want["status"] == (dref.E_RANGE if p.frag_stale else 0) and p.frag.stale == want["stats"]["stale_pixels"], p.name
    old = frag_cases[len(progs)]  # tiles_73x33: its S:* and X tiles are unshaded, nothing is fragment-stale
    s = tfc.restate(old, clear=clear)["stats"]
    assert old.name.startswith("tiles_73x33") and s["unshaded_pixels"] > 5 * 64 and s["stale_pixels"] == 0
    assert unshaded > 5 * 64 + 64 * sum(p.kinds.count("U") for p in progs)
