"""CPU checks of orbit_raster_visibility and orbit_visibility_resolve (include/orbit_abi_ext.h V1-V4):
the host mirror that is the GPU tests' reference equals an independent numpy restatement (tests/raster_vis_ref.py) word
for word, its high halves and counters are the depth call's (V4), the new cases of tests/raster_vis_cases.py reach what
they claim, the resolve's outputs obey their invariants, the layouts match the header, and the false-occlusion count of
tools/count_false_occlusion.py runs and agrees with the committed result."""
import ctypes as C
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

import raster_cases as rc
import raster_scene as rs
import raster_vis_cases as vc
import raster_vis_ref as vref
from orbit_amd import _lib, passes, raster
from orbit_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = vc.all_cases()
NEW = vc.new_cases()


def high_halves(vis):
    return (np.asarray(vis, np.uint64) >> np.uint64(32)).astype(np.uint32)


def assert_same(name, got, want):
    vis, stats, err = got
    wvis, wstats, werr, _ = want
    for k in vref.STAT_NAMES:
        assert int(stats[k]) == wstats[k], f"{name}: {k} = {int(stats[k])}, restated {wstats[k]}"
    assert list(err) == werr, name
    diff = np.argwhere(vis != wvis)
    assert len(diff) == 0, (f"{name}: {len(diff)} words differ, first at (y, x) = {diff[0]}: mirror "
                            f"{int(vis[tuple(diff[0])]):#018x}, restated {int(wvis[tuple(diff[0])]):#018x}")


def more_than_256_triangles(pk):
    return bool((pk.commands["cmd_index_count"][:min(int(pk.words[0]), pk.max_commands)] // 3 > 256).any())


def test_the_new_cases_reach_what_they_claim(capsys):
    missed = {k: v for k, v in vc.census(NEW).items() if v}
    assert not missed, missed
    assert len(capsys.readouterr().out.splitlines()) == len(NEW)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_mirror_equals_the_restatement(case):
    pk = rc.Packed(case)
    got, want = vc.host(pk), vc.restated(pk)
    assert_same(case.name, got, want)
    mirror_extras = dict(want[3], won=vref.winners(got[0], case.command_base, pk.max_commands))
    assert not vc.check_claims(case, got[0], got[1], got[2], mirror_extras)  # the claims hold on the mirror's own output


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_high_halves_and_stats_are_the_depth_calls(case):
    """V4"""
    pk = rc.Packed(case)
    vis, stats, err = vc.host(pk)
    depth, dstats, derr = pk.host()
    if more_than_256_triangles(pk):  # V3: the depth call draws the command that this one skips
        assert int(stats["range_errors"]) == int(dstats["range_errors"]) + 1 and list(err) != list(derr)
        assert (high_halves(vis) <= depth.view(np.uint32)).all() and (high_halves(vis) < depth.view(np.uint32)).any()
        return
    assert high_halves(vis).tobytes() == depth.view(np.uint32).tobytes(), case.name
    assert stats.tobytes() == dstats.tobytes() and list(err) == list(derr), case.name
    assert ((vis == 0) == (depth == 0)).all()  # a word of 0 is an uncovered pixel, and only that


def test_one_case_has_more_than_256_triangles():
    assert [c.name for c in CASES if more_than_256_triangles(rc.Packed(c))] == ["nt_257_between_neighbours"]


@pytest.mark.parametrize("stride,offset", [(32, 0), (32, 20)])
def test_host_mirror_reads_strided_vertices(stride, offset):
    for case in NEW:
        want = vc.host(rc.Packed(case))
        got = vc.host(rc.Packed(case, stride, offset))
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], case.name


@pytest.fixture(scope="module")
def scene100(oracle):
    scene = rs.glb_scene(100)
    w, h = 256, 144
    cam = rs.camera(w, h)
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    return scene, cam, w, h, draw


def test_host_mirror_equals_the_restatement_on_the_scene(scene100):
    scene, cam, w, h, draw = scene100
    n = int(draw[:4].view(np.uint32)[0])
    assert n > 8000
    args = (scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, rs.view_proj(cam), w, h)
    base = 12345
    got = raster.host_raster_visibility(draw, n, *args, command_base=base)
    want = vref.raster(draw, n, *args, command_base=base)
    assert_same("glb scene", got, want)
    depth, dstats, _ = scene.host_raster(draw, cam, w, h)
    assert high_halves(got[0]).tobytes() == depth.view(np.uint32).tobytes() and got[1].tobytes() == dstats.tobytes()
    assert want[3]["lane_triangles"] > 0 and want[3]["wave_triangles"] > 0 and len(want[3]["won"]) > 1000
    # and the resolve of it, mirror against counting
    rdepth, pixels, stats = raster.host_visibility_resolve(got[0], base, n)
    wdepth, wpixels, wstats = vref.resolve(got[0], base, n)
    assert rdepth.tobytes() == wdepth.tobytes() == depth.tobytes() and np.array_equal(pixels, wpixels)
    assert {k: int(stats[k]) for k in wstats} == wstats and wstats["foreign_pixels"] == 0 < wstats["visible_commands"]


def test_two_lists_share_a_buffer():
    a, b, cap = vc.two_lists()
    pa, pb = rc.Packed(a), rc.Packed(b)
    va = vc.host(pa)[0]
    got = vc.host(pb, visibility=va, clear=False)
    assert_same("list b over list a", got, vc.restated(pb, visibility=va, clear=False))
    vab = got[0]
    alone = vc.host(pb)[0]
    assert vab.tobytes() == np.maximum(va, alone).tobytes() and vab.tobytes() not in (va.tobytes(), alone.tobytes())
    _, pix_a, st_a = raster.host_visibility_resolve(vab, 0, cap)
    _, pix_b, st_b = raster.host_visibility_resolve(vab, cap, len(pb.commands))
    assert int(st_a["foreign_pixels"]) == int(pix_b.sum()) > 0 and int(st_b["foreign_pixels"]) == int(pix_a.sum()) > 0
    assert int(st_a["covered_pixels"]) == int(st_b["covered_pixels"]) == int(pix_a.sum() + pix_b.sum())
    assert int(pix_a[len(pa.commands):].sum()) == 0  # the gap between the lists' ids owns nothing
    # B is nearer where the lists overlap: A's first rectangle lost exactly the 8 x 8 samples they share
    assert int(pix_a[0]) == 256 - 64 and int(pix_b[0]) == 256


RESOLVE = vc.resolve_buffers()


@pytest.mark.parametrize("name,vis,base,count", RESOLVE, ids=[r[0] for r in RESOLVE])
def test_host_resolve_equals_counting_and_keeps_its_invariants(name, vis, base, count):
    depth, pixels, stats = raster.host_visibility_resolve(vis, base, count)
    wdepth, wpixels, wstats = vref.resolve(vis, base, count)
    assert depth.tobytes() == wdepth.tobytes() and np.array_equal(pixels, wpixels)
    assert {k: int(stats[k]) for k in wstats} == wstats and int(stats["_pad"]) == 0
    assert int(pixels.sum()) == int(stats["covered_pixels"]) - int(stats["foreign_pixels"])
    assert int(stats["visible_commands"]) == np.count_nonzero(pixels)
    assert depth.view(np.uint32).tobytes() == high_halves(vis).tobytes()
    _, none, no_pixels = raster.host_visibility_resolve(vis, base, count, want_command_pixels=False)
    assert none is None and int(no_pixels["visible_commands"]) == 0
    assert (int(no_pixels["covered_pixels"]), int(no_pixels["foreign_pixels"])) == (wstats["covered_pixels"], wstats["foreign_pixels"])


def test_the_resolve_buffers_reach_their_shapes():
    by_name = {r[0]: vref.resolve(*r[1:])[2] for r in RESOLVE}
    for w, h in vc.RESOLVE_SIZES:
        n = w * h
        assert by_name[f"one_command_{w}x{h}"] == dict(covered_pixels=n, visible_commands=1, foreign_pixels=0)
        assert by_name[f"all_distinct_{w}x{h}"] == dict(covered_pixels=n, visible_commands=n, foreign_pixels=0)
        assert by_name[f"uncovered_{w}x{h}"] == dict(covered_pixels=0, visible_commands=0, foreign_pixels=0)
        assert by_name[f"all_foreign_{w}x{h}"] == dict(covered_pixels=n, visible_commands=0, foreign_pixels=n)
        ends = by_name[f"range_ends_{w}x{h}"]
        assert ends["visible_commands"] <= 2 and (n < 8 or (ends["visible_commands"] == 2 and 0 < ends["foreign_pixels"] < ends["covered_pixels"] < n))
    assert by_name["top_of_24_bits"]["visible_commands"] == 2 and by_name["top_of_24_bits"]["foreign_pixels"] == 65 * 9 // 3
    assert by_name["no_commands"] == dict(covered_pixels=65 * 9, visible_commands=0, foreign_pixels=65 * 9)


def test_layouts_match_the_header(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "orbit_abi_ext.h"\nint main(void){return sizeof(OrbitRasterVisibility)==160'
                   " && offsetof(OrbitRasterVisibility,entity_data)==24 && offsetof(OrbitRasterVisibility,visibility)==32"
                   " && offsetof(OrbitRasterVisibility,stats)==40 && offsetof(OrbitRasterVisibility,vertex_count)==56"
                   " && offsetof(OrbitRasterVisibility,entity_count)==68 && offsetof(OrbitRasterVisibility,width)==80"
                   " && offsetof(OrbitRasterVisibility,flags)==88 && offsetof(OrbitRasterVisibility,command_base)==92"
                   " && offsetof(OrbitRasterVisibility,view_proj)==96 && sizeof(OrbitVisibilityStats)==16"
                   " && offsetof(OrbitVisibilityStats,foreign_pixels)==8 && sizeof(OrbitVisibilityResolve)==48"
                   " && offsetof(OrbitVisibilityResolve,command_pixels)==16 && offsetof(OrbitVisibilityResolve,stats)==24"
                   " && offsetof(OrbitVisibilityResolve,width)==32 && offsetof(OrbitVisibilityResolve,command_base)==40"
                   " && offsetof(OrbitVisibilityResolve,max_commands)==44 && ORBIT_VIS_MAX_COMMANDS==16777216?0:1;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    j, d = _lib.RasterVisibility, _lib.RasterDepth
    assert C.sizeof(j) == 160 and j.visibility.offset == d.depth.offset == 32 and j.command_base.offset == d._pad.offset == 92
    assert [(n, getattr(j, n).offset) for n, _ in j._fields_ if n not in ("visibility", "command_base")] == \
           [(n, getattr(d, n).offset) for n, _ in d._fields_ if n not in ("depth", "_pad")]
    r = _lib.VisibilityResolve
    assert C.sizeof(r) == 48 and (r.depth.offset, r.command_pixels.offset, r.stats.offset, r.width.offset, r.height.offset,
                                  r.command_base.offset, r.max_commands.offset) == (8, 16, 24, 32, 36, 40, 44)
    assert L.VIS_STATS.itemsize == 16 and L.VIS_STATS.names == ("covered_pixels", "visible_commands", "foreign_pixels", "_pad")
    assert _lib.VIS_MAX_COMMANDS == vref.MAX_COMMANDS == 1 << 24


def test_the_library_exports_the_calls_and_rejects_without_a_device():
    """Without a device only the NULL context and the NULL job can be reached: the other ORBIT_E_INVALID paths lie behind
    a live context (tests/test_raster_visibility_gpu.py::test_argument_errors_and_the_empty_call); the host mirror's
    Panic paths below stand in for them on the CPU."""
    lib = _lib.load()
    assert lib.orbit_raster_visibility(None, C.byref(_lib.RasterVisibility()), None) == _lib.E_INVALID
    assert lib.orbit_raster_visibility(None, None, None) == _lib.E_INVALID
    assert lib.orbit_visibility_resolve(None, C.byref(_lib.VisibilityResolve()), None) == _lib.E_INVALID
    assert lib.orbit_visibility_resolve(None, None, None) == _lib.E_INVALID
    assert lib.orbit_abi_version() == 6  # additive


def test_host_mirror_rejects_what_the_device_calls_reject():
    pk = rc.Packed(NEW[0])
    kw, (words, mc, data, vb, vcount, ent, vp, w, h) = pk.args()
    top = vref.MAX_COMMANDS - mc
    assert raster.host_raster_visibility(words, mc, data, vb, vcount, ent, vp, w, h, command_base=top, **kw)[1]["fragments"] > 0
    with pytest.raises(passes.Panic):  # command_base + max_commands = 2^24 + 1
        raster.host_raster_visibility(words, mc, data, vb, vcount, ent, vp, w, h, command_base=top + 1, **kw)
    for over in (dict(vertex_stride=8), dict(vertex_stride=32, position_offset=6)):
        with pytest.raises(passes.Panic):
            raster.host_raster_visibility(words, mc, data, np.zeros(4096, np.uint8), vcount, ent, vp, w, h, **{**kw, **over})
    for size in ((0, 48), (64, 0), (32769, 1)):
        with pytest.raises(passes.Panic):
            raster.host_raster_visibility(words, mc, data, vb, vcount, ent, vp, *size, **kw)
    h_lib = passes.lib()
    vis = np.zeros((h, w), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = [p(words), C.c_uint32(mc), p(data), C.c_uint64(len(data)), p(vb), C.c_uint64(vcount), C.c_uint32(12), C.c_uint32(0),
            p(ent), C.c_uint32(1), (C.c_float * 16)(*vp), p(vis), C.c_uint32(w), C.c_uint32(h), C.c_uint32(1), C.c_uint32(0), None, None]
    assert h_lib.orbit_host_raster_visibility(*args) == 0 and vis.any()
    for k in (0, 2, 4, 8, 10, 11):  # each NULL pointer
        bad = list(args)
        bad[k] = None
        assert h_lib.orbit_host_raster_visibility(*bad) == passes.HOST_PANIC, k
    bad = list(args)
    bad[14] = C.c_uint32(4)  # an unknown flag
    assert h_lib.orbit_host_raster_visibility(*bad) == passes.HOST_PANIC
    # the resolve: no visibility, no output, a size of 0, a range beyond 24 bits
    depth = np.zeros((h, w), np.float32)
    ok = [p(vis), C.c_uint32(w), C.c_uint32(h), C.c_uint32(0), C.c_uint32(0), p(depth), None, None]
    assert h_lib.orbit_host_visibility_resolve(*ok) == 0
    for k, v in ((0, None), (5, None), (1, C.c_uint32(0)), (2, C.c_uint32(32769)), (3, C.c_uint32(vref.MAX_COMMANDS)), ):
        bad = list(ok)
        bad[k] = v
        if k == 3:
            bad[4] = C.c_uint32(1)
        assert h_lib.orbit_host_visibility_resolve(*bad) == passes.HOST_PANIC, k


def test_false_occlusion_count_runs_and_is_the_committed_one(oracle):
    spec = importlib.util.spec_from_file_location("count_false_occlusion", os.path.join(ROOT, "tools", "count_false_occlusion.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    result = tool.count(oracle)
    assert len(result["frames"]) == 2
    for fr in result["frames"]:
        print(fr)
        drawn = fr["early_commands"] + fr["late_commands"]
        assert 0 <= fr["overdraw_commands"] <= drawn and fr["overdraw_commands"] == drawn - fr["early_visible"] - fr["late_visible"]
        assert 0 <= fr["missing_visible_commands"] <= fr["unculled_visible"] <= fr["unculled_commands"]
        assert 0 <= fr["false_occlusion_pixels"] <= fr["covered_pixels"] <= result["width"] * result["height"]
        assert (fr["missing_visible_commands"] == 0) == (fr["missing_visible_pixels"] == 0)
        assert fr["unculled_visible"] > 0 and drawn > 0
    with open(os.path.join(ROOT, "profiles", "false_occlusion_cpu.json")) as fh:
        assert json.load(fh) == result, "profiles/false_occlusion_cpu.json is stale: run tools/count_false_occlusion.py"
