"""CPU checks of orbit_visibility_compact (include/orbit_abi_ext.h C1-C6): the host mirror that is the
GPU tests' reference equals the independent numpy restatement (tests/visibility_compact_ref.py) on every output of every
case of tests/visibility_compact_cases.py, in both modes and at every capacity; the cases reach what they claim; C6
(a)-(d) hold on every rasterised case and on the 100-instance scene's two frames through the mirror's own raster; the
layouts match the header; the device library's argument checks answer ORBIT_E_INVALID for each reason the header lists
(they run in front of the context, so without a GPU); tools/count_visible_list.py agrees with the committed result."""
import ctypes as C
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import raster_scene as rs
import visibility_compact_cases as cc
import visibility_compact_ref as ref
from orbit_amd import _lib, raster
from orbit_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5A5A5A5  # what an output holds before the call: what the call does not write keeps it
MODES = (False, True)


@pytest.fixture(scope="module")
def rasterised():
    return cc.rasterised_cases()


HAND = cc.hand_cases()


def assert_same(name, got, want):
    for k in ref.STAT_NAMES:
        assert int(got["stats"][k]) == want["stats"][k], f"{name}: {k} = {int(got['stats'][k])}, restated {want['stats'][k]}"
    assert got["status"] == want["status"], f"{name}: status {got['status']}, restated {want['status']}"
    for k in ("masks", "commands", "ids", "data"):
        assert (got[k] is None) == (want[k] is None), (name, k)
        if got[k] is not None:
            diff = np.flatnonzero(got[k] != want[k])
            assert len(diff) == 0, (f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}: mirror "
                                    f"{int(got[k][diff[0]]):#x}, restated {int(want[k][diff[0]]):#x}")


def both(case, triangles, **over):
    a, kw = case.args(triangles, fill=FILL, **over)
    return raster.host_visibility_compact(*a, **kw), ref.compact(*a, **kw)


def check_case(case):
    for triangles in MODES:
        got, want = both(case, triangles)
        assert_same(f"{case.name} (triangles={triangles})", got, want)
        for k, v in {**case.expect, **(case.expect_cut if triangles else case.expect_plain)}.items():
            assert want["stats"][k] == v, f"{case.name} (triangles={triangles}): {k} = {want['stats'][k]}, claimed {v}"
        yield triangles, got


@pytest.mark.parametrize("case", HAND, ids=[c.name for c in HAND])
def test_host_mirror_equals_the_restatement_on_hand_built_cases(case):
    for triangles, got in check_case(case):
        n = int(got["commands"][0])
        assert (got["commands"][1 + 7 * n:] == FILL).all() and (got["ids"][n:] == FILL).all()
        if triangles:
            assert (got["data"][int(got["stats"]["data_words_needed"]):] == FILL).all()


def test_host_mirror_equals_the_restatement_on_rasterised_cases(rasterised):
    assert len(rasterised) >= 43
    seen = 0
    for case in rasterised:
        for _, got in check_case(case):
            seen += int(got["stats"]["visible_commands"])
    assert seen > 90  # (both modes)


def test_the_cases_hold_what_the_census_says():
    by_name = {c.name: c for c in HAND}
    got = raster.host_visibility_compact(*by_name["three_chunks"].args(True)[0], **by_name["three_chunks"].args(True)[1])
    assert int(got["commands"][0]) == 2 * cc.CHUNK + 5 and int(got["ids"][0]) == cc.CHUNK
    got = raster.host_visibility_compact(*by_name["inconsistent"].args(False)[0], **by_name["inconsistent"].args(False)[1])
    assert got["status"] == _lib.E_RANGE and list(got["ids"][:3]) == [0, 2, 4]
    case = by_name["m_1_2_3_4"]
    assert [int(c) % 4 for c in case.words[1:].reshape(-1, 7)[:, 2]] == [0, 1, 2, 3]
    got = raster.host_visibility_compact(*case.args(True)[0], **case.args(True, fill=FILL)[1])
    rows =got["commands"][1:].reshape(-1, 7)
    assert list(rows[:, 0]) == [3, 6, 9, 12] and list(rows[:, 3]) == [0, 4, 9, 15] and list(rows[:, 2]) == [12, 28, 48, 72]
    tail = got["data"].view(np.uint8).reshape(-1, 4)  # the pad bytes of each region's last word are 0
    assert list(tail[3][3:]) == [0] and list(tail[8][2:]) == [0, 0] and list(tail[14][1:]) == [0, 0, 0]


@pytest.mark.parametrize("name", cc.CAPACITY_CASES)
def test_capacities_give_the_prefix_and_leave_the_rest(name):
    case = next(c for c in HAND if c.name == name)
    full = both(case, True)[0]
    n, words = int(full["stats"]["visible_commands"]), int(full["stats"]["data_words_needed"])
    assert n > 3 and full["status"] == 0
    for what, over, triangles in cc.capacity_variants(full["stats"]):
        got, want = both(case, triangles, **over)
        assert_same(f"{name} {what}", got, want)
        w = int(got["commands"][0])
        exact = "exact" in what
        assert (w == n) == exact and got["status"] == (0 if exact else _lib.E_CAPACITY), what
        assert int(got["stats"]["dropped_commands"]) == n - w and int(got["stats"]["visible_commands"]) == n
        assert int(got["stats"]["data_words_needed"]) == (words if triangles else 0)
        # the prefix: the uncapped call's first w commands, ids and regions
        assert got["commands"][1:1 + 7 * w].tobytes() == (full if triangles else both(case, False)[0])["commands"][1:1 + 7 * w].tobytes()
        assert got["ids"][:w].tobytes() == full["ids"][:w].tobytes() and (got["ids"][w:] == FILL).all()
        if triangles:
            rows = got["commands"][1:1 + 7 * w].reshape(-1, 7)
            end = int(rows[-1, 3] + (rows[-1, 2] // 4 - rows[-1, 3]) + (rows[-1, 0] + 3) // 4) if w else 0
            assert got["data"][:end].tobytes() == full["data"][:end].tobytes() and (got["data"][end:] == FILL).all(), what
        if what == "data_words_one_less":
            assert w == n - 1


# -------------------------------------------------------------------------------------------------- C6
def c6_of_packed(case, triangles):
    pk = case.packed
    opts, (words, mc, data, vb, vcount, ent, vp, w, h) = pk.args()
    a, kw = case.args(triangles)
    got = raster.host_visibility_compact(*a, **kw)
    written = int(got["commands"][0])
    out_data = got["data"] if triangles else data
    vis2, st2, err2 = raster.host_raster_visibility(got["commands"], written, out_data, vb, vcount, ent, vp, w, h,
                                                    cull_none=pk.case.cull_none, vertex_stride=pk.stride,
                                                    position_offset=pk.offset, entity_count=opts["entity_count"],
                                                    meshlet_data_words=len(out_data) if triangles else opts["meshlet_data_words"])
    assert not err2.any()
    _, pixels2, rst2 = raster.host_visibility_resolve(vis2, 0, written)
    return cc.c6_misses(case.name, case.visibility, case.command_base, got, triangles, vis2, st2, pixels2, rst2,
                        whole=case.one_clear_call), got


def test_c6_holds_on_every_rasterised_case(rasterised):
    visible = 0
    for case in rasterised:
        for triangles in MODES:
            missed, got = c6_of_packed(case, triangles)
            assert not missed, missed
            visible += int(got["stats"]["visible_triangles"])
    assert visible > 400


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("count_visible_list", os.path.join(ROOT, "tools", "count_visible_list.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_c6_holds_on_the_scenes_two_frames_and_the_committed_count_stands(tool, oracle):
    """Each frame's early list (ONE CLEAR call at base 0): mirror against restatement, C6 in both modes; the tool's
    counts, which come from the same calls, equal profiles/visible_list_cpu.json."""
    result = tool.count(oracle, check=lambda name, case, triangles, got: assert_same(
        name, got, ref.compact(*case.args(triangles)[0], **case.args(triangles)[1])))
    with open(os.path.join(ROOT, "profiles", "visible_list_cpu.json")) as fh:
        assert result == json.load(fh)
    for fr in result["frames"]:
        assert fr["c6_missed"] == [] and 0 < fr["commands_out"] < fr["commands_in"] // 4
        assert fr["triangles_out"] < fr["triangles_in"] and fr["data_words_needed"] < fr["input_meshlet_words"]


# -------------------------------------------------------------------------------------------------- layouts, arguments
def test_layouts_match_the_header():
    header = open(os.path.join(ROOT, "include", "orbit_abi_ext.h")).read()
    asserts = dict(re.findall(r"offsetof\(OrbitVisibilityCompact, (\w+)\) == (\d+)", header))
    assert asserts == {"meshlet_data_words": "72", "width": "88"}
    assert "sizeof(OrbitVisibilityCompact) == 120" in header and "sizeof(OrbitVisibilityCompactStats) == 32" in header
    assert C.sizeof(_lib.VisibilityCompact) == 120 and L.VIS_COMPACT_STATS.itemsize == 32
    for name, at in asserts.items():
        assert getattr(_lib.VisibilityCompact, name).offset == int(at)
    fields = re.search(r"typedef struct OrbitVisibilityCompactStats \{[^\n]*\n(.*?);\s*\} OrbitVisibilityCompactStats", header, re.S).group(1)
    assert [f.strip() for f in fields.replace("uint32_t", "").split(",")] == list(L.VIS_COMPACT_STATS.names) == list(ref.STAT_NAMES)
    assert _lib.COMPACT_TRIANGLES == 1 and "#define ORBIT_COMPACT_TRIANGLES 1u" in header
    lib = _lib.load()
    assert [lib.orbit_visibility_compact_workspace(n) for n in (0, 1, cc.CHUNK, cc.CHUNK + 1, 1 << 24)] == \
           [16, 32, 32, 48, 16 * ((1 << 24) // cc.CHUNK + 1)]


def test_every_invalid_argument_is_named_before_the_context_is_looked_at():
    """No GPU here, so no context: a job that passes every check ends at 'ctx is NULL'; each broken one at its own reason."""
    lib = _lib.load()
    buf = np.zeros(64, np.uint64)
    at = buf.ctypes.data
    assert at % 8 == 0

    def call(**over):
        j = _lib.VisibilityCompact()
        kw = dict(visibility=at, draw_commands=at, meshlet_data=at, triangle_masks=at, visible_commands=at, visible_ids=at,
                  visible_data=at, stats=at, workspace=at, meshlet_data_words=16, workspace_bytes=32, width=8, height=8,
                  command_base=0, max_commands=4, visible_capacity=4, visible_data_words=16, flags=_lib.COMPACT_TRIANGLES)
        kw.update(over)
        for k, v in kw.items():
            setattr(j, k, v)
        rc = lib.orbit_visibility_compact(None, C.byref(j), None)
        return rc, lib.orbit_last_error(None).decode()

    assert lib.orbit_visibility_compact(None, None, None) == _lib.E_INVALID and "job is NULL" in lib.orbit_last_error(None).decode()
    for over in (dict(), dict(flags=0, meshlet_data=None, visible_data=None), dict(visible_ids=None, stats=None),
                 dict(max_commands=0, workspace_bytes=16), dict(visible_data_words=1 << 30),
                 dict(command_base=_lib.VIS_MAX_COMMANDS - 4), dict(width=_lib.RASTER_MAX_DIM, height=1)):
        assert call(**over) == (_lib.E_INVALID, "visibility_compact: ctx is NULL"), over
    top = _lib.VIS_MAX_COMMANDS
    for over, reason in (
            [(dict([(k, None)]), "NULL buffer") for k in ("visibility", "draw_commands", "triangle_masks", "visible_commands", "workspace")]
            + [(dict([(k, None)]), "needs meshlet_data and visible_data") for k in ("meshlet_data", "visible_data")]
            + [(dict([(k, at + 4)]), "aligned") for k in ("visibility", "workspace")]
            + [(dict([(k, at + 2)]), "aligned") for k in ("draw_commands", "meshlet_data", "triangle_masks", "visible_commands",
                                                            "visible_ids", "visible_data", "stats")]
            + [(dict(workspace_bytes=31), "workspace of 31 bytes, 32 needed"), (dict(max_commands=257), "48 needed"),
               (dict(width=0), "target"), (dict(height=0), "target"), (dict(width=_lib.RASTER_MAX_DIM + 1), "target"),
               (dict(height=_lib.RASTER_MAX_DIM + 1), "target"), (dict(command_base=top - 3), "24 bits"),
               (dict(command_base=top, max_commands=1), "24 bits"), (dict(max_commands=top + 1, workspace_bytes=1 << 30), "24 bits"),
               (dict(visible_data_words=(1 << 30) + 1), "2^30"), (dict(flags=2), "flags"), (dict(flags=3), "flags"),
               (dict(flags=1 << 31), "flags")]):
        rc, text = call(**over)
        assert rc == _lib.E_INVALID and reason in text and "ctx is NULL" not in text, (over, text)
    assert not buf.any()  # nothing was written
