"""The tile programmes of tests/shade_tile_cases.py on the host: which arrangements the layouts hold under
caps of 1 and 2 workgroups, from the kinds and visibility_tile_cases.assignment alone; the two host mirrors
(orbit_amd.raster.host_fragments_shade, host_fragments_shade_shadowed: the references of tests/test_shade_tiles_gpu.py)
against the numpy restatements, byte for byte as tests/test_fragments_shade_cpu.py and test_fragments_shade_shadowed_cpu.py
compare them; the programmes' closed-form counters against the mirrors'; and every kind's defining property on the mirrors'
output, tile by tile.  No GPU."""
import numpy as np
import pytest

import fragments_shade_cases as fc
import fragments_shade_shadowed_cases as sc
import shade_tile_cases as st
import test_fragments_shade_cpu as base_cpu
import test_fragments_shade_shadowed_cpu as shadow_cpu
from orbit_amd import _lib

FILL = base_cpu.FILL


@pytest.fixture(scope="module")
def progs(oracle):
    return st.programmes(oracle) + [st.tamper_free_programme(oracle), st.natural_programme(oracle)]


# -- 1. the arrangements: a condition on the layouts, not a measurement
@pytest.mark.parametrize("cap", (1, 2))
def test_the_layouts_hold_every_arrangement_under_a_cap(cap):
    found = st.arrangements_of(st.LAYOUTS, cap)
    assert found == set(st.ARRANGEMENTS), sorted(set(st.ARRANGEMENTS) - found)
    assert len(st.ARRANGEMENTS) == len(st.RULES) + 1 + 2 * len(st.SHADE_COUNTERS) + len(st.SHADOW_COUNTERS)


def test_uncapped_every_wave_takes_at_most_one_tile(progs):
    for kinds, tiles in st.LAYOUTS:
        assert all(len(w) <= 1 for w in st.assignment(tiles, 0, st.RESIDENT))
        assert st.arrangements(kinds, tiles, 0) <= set(st.UNCAPPED)
    assert st.arrangements_of(st.LAYOUTS, 0) == set(st.UNCAPPED)
    assert [(p.kinds, p.tiles) for p in progs[:3]] == list(st.LAYOUTS[:3]) and progs[3].kinds == st.MAIN_KINDS
    assert [(p.kinds, p.tiles) for p in progs[4:6]] == list(st.LAYOUTS[3:])
    held = set().union(*(set(k) for k, _ in st.LAYOUTS))
    assert held == set(st.KINDS), sorted(set(st.KINDS) - held)  # every kind lies somewhere
    assert set(st.SECOND_KINDS) >= {"S32", "B63", "SH", "MU", "L256", "L1"}  # the staged walk under tile_size_px 16 meets them


# -- 2. mirror = restatement, byte for byte, with the comparison of the two calls' own CPU suites
@pytest.mark.parametrize("render_mode", (0, 8))
@pytest.mark.parametrize("clear", (False, True))
def test_the_mirrors_equal_the_restatements(oracle, progs, clear, render_mode):
    for p in progs:
        name = f"{p.name} (clear={clear}, mode {render_mode})"
        kw = dict(clear=clear, render_mode=render_mode, fill=FILL)
        base_cpu.assert_equal(name, fc.mirror(p.case, **kw), fc.restated(p.case, oracle, **kw))
        shadow_cpu.assert_equal(name + ", shadowed", sc.mirror(p.shadow, **kw), sc.restated(p.shadow, oracle, **kw))


# -- 3. the closed forms
@pytest.mark.parametrize("render_mode", (0, 8))
def test_the_closed_form_counters_are_the_mirrors(progs, render_mode):
    for p in progs:
        expect = p.expect if render_mode == 0 else p.expect8
        a, b = fc.mirror(p.case, clear=True, render_mode=render_mode), sc.mirror(p.shadow, clear=True, render_mode=render_mode)
        for call, got in (("shade", a["stats"]), ("shadowed", b["stats"]), ("shadow", b["shadow_stats"])):
            assert {k: int(got[k]) for k in expect[call]} == expect[call], (p.name, call)
        assert a["status"] == (_lib.E_RANGE if p.stale("shade") else 0) and b["status"] == (_lib.E_RANGE if p.stale("shadowed") else 0), p.name
    main, tamper_free, natural = progs[0], progs[6], progs[7]
    assert main.stale("shade") and main.stale("shadowed") and not tamper_free.stale("shadowed") and not natural.stale("shade")
    assert "BC" not in natural.kinds and natural.stale("shadowed")  # (its SHb tile)


# -- 4. every kind's defining property, on the mirrors' output
def only(case, rows, cols):
    """the case with every word outside the box uncovered"""
    c = case.copy(case.name)
    vis = np.zeros_like(c.visibility)
    vis[rows, cols] = c.visibility[rows, cols]
    c.visibility = vis
    return c


def test_every_tile_gives_what_its_kind_says(progs):
    seen = set()
    for p in progs[:6]:
        whole = fc.mirror(p.case, clear=True)
        shadowed = sc.mirror(p.shadow, clear=True)
        covered = p.case.visibility != 0
        for call, got in (("shade", whole), ("shadowed", shadowed)):
            written = got["color"][..., 3] == 1.0
            unshaded = covered & (p.case.material == st.NONE)
            assert ((covered & ~written & ~unshaded) == p.stale_mask[call]).all(), (p.name, call)  # exactly the pixels the kinds name
        first_d = True
        for t, kind in enumerate(p.kinds):
            rows, cols = p.tile_box(t)
            area = (rows.stop - rows.start) * (cols.stop - cols.start)
            want = st.tile_counts(kind, area, first_d and kind == "D")
            first_d = first_d and kind != "D"
            alone = only(p.case, rows, cols)
            a = fc.mirror(alone, clear=True)
            b = sc.mirror(sc.ShadowCase(alone, p.shadow.rows, p.shadow.maps), clear=True)
            for call, got in (("shade", a["stats"]), ("shadowed", b["stats"]), ("shadow", b["shadow_stats"])):
                assert {k: int(got[k]) for k in want[call]} == want[call], (p.name, t, kind, call)
            walked, factor, cascade = whole["lights_walked"][rows, cols], shadowed["shadow_factor"][rows, cols], shadowed["cascade"][rows, cols]
            if kind in st.L_KINDS or kind in ("PxL65",):
                assert (walked == min({"PxL65": 65}.get(kind) or st.LENGTH[kind], 256)).all(), (p.name, t, kind)
            if kind == "L300":
                assert (walked == 256).all() and (p.case.image[:, 1] == 300).any()
            if kind == "S2":
                assert sorted(np.unique(walked)) == [1, 129]
            if kind == "S32":
                assert set(np.unique(walked)) == {0, 1, 2, 3, 63, 64, 65, 129} and len(np.unique(p.case.visibility[rows, cols] >> np.uint64(32))) == 32
            if kind in st.B_KINDS:
                assert (walked[:4] == 0).all() and (walked[4:] == 5).all() and not whole["color"][rows, cols][:4].any()
            if kind in ("O", "Oz"):
                assert (walked == 0).all() and (whole["color"][rows, cols][..., 3] == 1.0).all()  # written, counted outside above
            if kind == "SH":
                assert (cascade == 0).all() and ((factor > 0) & (factor < 1)).any() and int(b["shadow_stats"]["early_out_pixels"]) == 0
            if kind in ("SH0", "SH12"):
                assert (factor == (1.0 if kind == "SH0" else 0.0)).all() and (cascade == 0).all()
                assert int(b["shadow_stats"]["early_out_pixels"]) == int(b["shadow_stats"]["shadowed_pixels"]) == 64
            if kind == "SHn":
                assert (cascade == 4).all() and (factor == 1.0).all()
            if kind == "SHb":
                assert (cascade == 0xFFFFFFFF).all() and not shadowed["color"][rows, cols].any() and (walked == 68).all()
            if kind == "SHm":
                assert (cascade[:4] == 0).all() and (cascade[4:] == 0xFFFFFFFF).all()
            if kind in st.NO_SHADOW:
                assert (cascade == 0xFFFFFFFF).all() and (factor == 1.0).all()
            seen.add(kind)
    assert seen == set(st.KINDS)


def test_the_natural_target_holds_the_copies_where_the_trips_are(oracle, progs):
    for num_cus in (256, 304, 64):
        w, h, waves = st.natural_target(num_cus)
        big, shadowed, where = st.instanced(progs[7], w, h, waves)
        last_trip = (((w + 7) // 8) * ((h + 7) // 8) - 1) // waves
        trips = {name: (first, last) for name, _, _, first, last in where}
        assert last_trip >= 2 and trips["top_right"] == (0, 0) and trips["bottom_right"][1] == last_trip
        assert 0 < trips["middle"][0] <= trips["middle"][1] < last_trip
        assert w % 8 == 1 and h % 8 == 1 and big.visibility[:, w - 1].any() and big.visibility[h - 1, :].any()  # the partial column and row are met
        assert len(where) == (5 if num_cus == 256 else len(where)) and where[0][0] == "top_right"
        if len(where) == 5:  # tile for tile one trip behind the first copy, on the same waves
            assert where[4][1] // 8 + (where[4][2] // 8) * ((w + 7) // 8) == (w - progs[7].width) // 8 + waves and where[4][3] == 1
    got = fc.mirror(big, clear=True)
    assert {k: int(got["stats"][k]) for k in progs[7].expect["shade"]} == {k: len(where) * v for k, v in progs[7].expect["shade"].items()}
    assert int(sc.mirror(shadowed, clear=True)["stats"]["written_pixels"]) == len(where) * progs[7].expect["shadowed"]["written_pixels"]
