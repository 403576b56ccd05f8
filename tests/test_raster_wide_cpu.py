"""CPU checks of ORBIT_RASTER_WIDE_GUARD (include/orbit_abi_ext.h R4w): the host mirror that is the GPU
tests' reference equals the independent restatement tests/raster_wide_ref.py byte for byte and counter for counter on
every case of tests/raster_wide_cases.py, for both raster calls, and V4 holds between them; the cases reach what they
claim and the census of routes is complete; on the three earlier case sets the flag changes nothing where no vertex is
wide and lowers no pixel anywhere; the camera inside the glTF scene loses no triangle to the guard band any more, and
its two-pass frame loses nothing to occlusion; a wide triangle's depth against exact rationals; the flag word."""
import importlib.util
import os

import numpy as np
import pytest

import raster_cases as rc
import raster_clip_cases as cc
import raster_scene as rs
import raster_vis_cases as vc
import raster_wide_cases as wc
import raster_wide_ref as wref
from orbit_amd import _lib, passes, raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = wc.all_cases()


def assert_same(name, got, want, view=np.uint64):
    buf, stats, err = got
    wbuf, wstats, werr, _ = want
    for k in wref.STAT_NAMES:
        assert int(stats[k]) == wstats[k], f"{name}: {k} = {int(stats[k])}, restated {wstats[k]}"
    assert list(err) == werr, name
    diff = np.argwhere(buf.view(view) != wbuf.view(view))
    assert len(diff) == 0, f"{name}: {len(diff)} pixels differ, first at (y, x) = {diff[0]}"


def high(vis):
    return np.asarray(vis, np.uint64) >> np.uint64(32)


def test_the_case_set_reaches_what_it_claims_and_every_route(capsys):
    missed, reached = wc.census(CASES)
    assert not {k: v for k, v in missed.items() if v}
    assert reached == set(wc.ROUTES), set(wc.ROUTES) - reached
    assert len(capsys.readouterr().out.splitlines()) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_mirror_equals_the_restatement(case):
    pk = rc.Packed(case)
    vis, depth = wc.host_vis(pk), wc.host_depth(pk)
    want = wc.restated_vis(pk, check_wrap=True)
    assert_same(case.name, vis, want)
    assert_same(case.name, depth, wc.restated_depth(pk), np.uint32)
    assert not wc.check_claims(case, vis[0], vis[1], vis[2], want[3])  # the claims hold on the mirror's own output
    # V4 with the flag on both calls
    assert wref.depth_of(vis[0]).tobytes() == depth[0].tobytes() and vis[1].tobytes() == depth[1].tobytes()
    # without the flag every wide triangle is guard_skipped, as before the flag existed; the flag only adds depth
    off = wc.host_vis(pk, wide=False)
    assert_same(case.name, off, wc.restated_vis(pk, wide=False))
    assert (high(vis[0]) >= high(off[0])).all()
    assert int(off[1]["guard_skipped"]) >= int(vis[1]["guard_skipped"])
    if want[3]["wide_pieces"] == 0:
        assert off[0].tobytes() == vis[0].tobytes() and off[1].tobytes() == vis[1].tobytes()


@pytest.mark.parametrize("stride,offset", [(32, 20)])
def test_host_mirror_reads_strided_vertices(stride, offset):
    for case in CASES:
        want = wc.host_vis(rc.Packed(case))
        got = wc.host_vis(rc.Packed(case, stride, offset, vertex_base=1, data_base=0))
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], case.name


def test_the_earlier_census_with_the_flag_added():
    """raster_cases, raster_vis_cases and raster_clip_cases with 32 added to their flags: the mirror still equals the
    restatement; bytes and stats are identical wherever no vertex is wide; nowhere does a pixel go lower."""
    wide_cases = set()
    for case, clip_near in [(c, False) for c in vc.all_cases()] + [(c, True) for c in cc.all_cases()]:
        pk = rc.Packed(case)
        for host, restated, view in ((wc.host_vis, wc.restated_vis, np.uint64), (wc.host_depth, wc.restated_depth, np.uint32)):
            on, off = host(pk, clip_near=clip_near), host(pk, wide=False, clip_near=clip_near)
            want = restated(pk, clip_near=clip_near)
            if view is np.uint64 or int(want[1]["range_errors"]) == 0:  # (nt_257: the depth call has no triangle limit)
                assert_same(case.name, on, want, view)
            bits = (lambda r: high(r[0])) if view is np.uint64 else (lambda r: r[0].view(np.uint32))
            assert (bits(on) >= bits(off)).all(), case.name
            if want[3]["wide_pieces"] == 0:
                assert on[0].tobytes() == off[0].tobytes() and on[1].tobytes() == off[1].tobytes(), case.name
                assert list(on[2]) == list(off[2])
            else:
                wide_cases.add(case.name)
    # the earlier cases with a vertex in R4w's band: the guard band's own case and the two clip cases that leave it
    assert wide_cases == {"guard_band", "guard_piece_other_draws", "guard_piece_none_draws"}, wide_cases


def test_load_without_clear_into_what_an_unflagged_call_left():
    by_name = {c.name: c for c in CASES}
    pk = rc.Packed(by_name["fan_of_wide_triangles"])
    left = rc.Packed(by_name["strip_of_narrow_and_wide"])
    left_d, left_v = wc.host_depth(left, wide=False)[0], wc.host_vis(left, wide=False)[0]
    assert left_d.any() and left_v.any()
    got_d = wc.host_depth(pk, depth=left_d, clear=False)
    assert_same("load depth", got_d, wc.restated_depth(pk, depth=left_d, clear=False), np.uint32)
    got_v = wc.host_vis(pk, visibility=left_v, clear=False)
    assert_same("load visibility", got_v, wc.restated_vis(pk, visibility=left_v, clear=False))
    assert got_d[0].tobytes() == np.maximum(left_d, wc.host_depth(pk)[0]).tobytes() != left_d.tobytes()
    assert wref.depth_of(got_v[0]).tobytes() == got_d[0].tobytes()


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("count_near_clip", os.path.join(ROOT, "tools", "count_near_clip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def inside(oracle, tool):
    """the pass-0 list of the inside camera at 256 x 144, restated once with flags 8 | 32 (exact depth errors included)"""
    scene = rs.glb_scene(tool.INSTANCES)
    w, h = 256, 144
    cam = rs.camera(w, h, tool.CAMERAS[1])
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    n = int(draw[:4].view(np.uint32)[0])
    args = (draw, n, scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, rs.view_proj(cam), w, h)
    want = wref.raster(*args, flags=wref.CLEAR | wref.CLIP_NEAR | wref.WIDE_GUARD, exact=True)
    return scene, cam, args, want


def test_inside_camera_scene_loses_no_triangle_to_the_guard_band(inside):
    scene, cam, args, want = inside
    # the restatement first: every vertex that fails R4's guard is finite and below 2^28, whatever the target's size
    assert want[1]["guard_skipped"] == 0 and want[3]["out_of_band_pieces"] == 0
    assert want[3]["wide_pieces"] >= 100 and want[3]["max_coord_bits"] <= 32
    got = raster.host_raster_visibility(*args, clip_near=True, wide_guard=True)
    assert_same("inside camera", got, want)
    assert int(got[1]["guard_skipped"]) == 0
    clip = raster.host_raster_visibility(*args, clip_near=True)
    print(f"flags 8: {clip[1]}; flags 8 | 32: {got[1]}; {want[3]}")
    assert int(clip[1]["guard_skipped"]) >= want[3]["wide_triangles"] > 0
    assert (high(got[0]) >= high(clip[0])).all()
    depth = raster.host_raster_depth(*args, clip_near=True, wide_guard=True)
    assert wref.depth_of(got[0]).tobytes() == depth[0].tobytes() and got[1].tobytes() == depth[1].tobytes()
    # What the guard band hid on this camera covers no sample: the meshlets' triangles are small against their distance,
    # so one whose cut reaches 2^15 pixels to the side lies beside the target as a whole (or is a back face of the
    # terrain the camera sits in).  Every one of them is now counted as what it is, and no pixel changes
    assert want[3]["wide_drawn"] == 0 and got[0].tobytes() == clip[0].tobytes()
    assert int(got[1]["no_coverage"]) + int(got[1]["back_facing"]) == \
        int(clip[1]["no_coverage"]) + int(clip[1]["back_facing"]) + int(clip[1]["guard_skipped"])


def test_inside_camera_unculled_list_draws_no_wide_triangle_either(oracle, inside):
    """The unculled list with CULL_NONE, on the mirror (which the tests above hold to the restatement): 1 665 triangles
    leave the guard band at 256 x 144, none of them covers a sample."""
    scene, cam, args, _ = inside
    words = scene.all_commands(oracle, cam)
    clip = raster.host_raster_visibility(words, int(words[0]), *args[2:], clip_near=True, cull_none=True)
    both = raster.host_raster_visibility(words, int(words[0]), *args[2:], clip_near=True, cull_none=True, wide_guard=True)
    print(f"unculled, CULL_NONE: flags 8 {clip[1]}; flags 8 | 32 {both[1]}")
    assert int(clip[1]["guard_skipped"]) > 1000 and int(both[1]["guard_skipped"]) == 0
    assert int(both[1]["no_coverage"]) == int(clip[1]["no_coverage"]) + int(clip[1]["guard_skipped"])
    assert both[0].tobytes() == clip[0].tobytes()


def test_inside_camera_two_pass_frame_loses_nothing_to_occlusion_with_the_flag(oracle, tool):
    scene = rs.glb_scene(tool.INSTANCES)
    w, h = 256, 144
    cams = [rs.camera(w, h, p) for p in tool.CAMERAS]
    counts, _, _ = tool.frame_counts(scene, oracle, cams, w, h, True, wide_guard=True)
    print(counts)
    assert counts["missing_by_occlusion"] == 0 and counts["false_occlusion_pixels_vs_pass0"] == 0
    assert counts["guard_skipped"] == 0 and counts["guard_skipped_early"] == 0 and counts["guard_skipped_late"] == 0
    assert counts["early_commands"] > 1000 and counts["covered_pixels"] == w * h


def test_wide_depth_against_exact_rationals(inside):
    """d - d_exact over every pixel a wide triangle writes on the cases, in ulps of d (d_exact: the plane through the
    three fp32 vertex depths in exact rationals, clamped to 1).  No threshold was fixed in advance; the figure is printed
    and recorded in DESIGN.md §4.15.  What is asserted follows from the formats alone: the final rounding to fp32 is
    half an ulp, and the double plane's own error (a handful of 2^-53 relative roundings of products that may exceed d
    by the ratio of the far vertex's distance to the target's, below 2^37 in band) has to stay below the other half
    for the cases' coordinates (below 2^31, except the band-top and 64-bit cases, whose planes are nearly flat on the
    target).  The scene contributes no pixel: none of its wide triangles covers a sample (see above)."""
    worst, where = -np.inf, None
    for case in CASES:
        e = wc.restated_vis(rc.Packed(case), exact=True)[3]
        if e["wide_drawn"]:
            assert e["max_ulp_error"] > -np.inf, case.name
        if e["max_ulp_error"] > worst:
            worst, where = e["max_ulp_error"], case.name
    print(f"largest d - d_exact of a wide triangle: {worst} ulp ({where})")
    assert inside[3][3]["wide_drawn"] == 0 and inside[3][3]["max_ulp_error"] == -np.inf
    assert 0 < worst <= 1.0


def test_flag_validation_and_the_version_stays():
    import ctypes as C

    pk = rc.Packed(CASES[0])
    _, (words, mc, data, vb, vcount, ent, vp, w, h) = pk.args()
    lib = passes.lib()
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    vpc = (C.c_float * 16)(*vp)
    for call, out, extra in ((lib.orbit_host_raster_depth, np.zeros(w * h, np.float32), []),
                             (lib.orbit_host_raster_visibility, np.zeros(w * h, np.uint64), [C.c_uint32(0)])):
        for flags, known in ((32, True), (33, True), (34, True), (40, True), (4, False), (16, False), (36, False), (48, False)):
            args = [p(words), C.c_uint32(mc), p(data), C.c_uint64(len(data)), p(vb), C.c_uint64(vcount), C.c_uint32(12),
                    C.c_uint32(0), p(ent), C.c_uint32(1), vpc, p(out), C.c_uint32(w), C.c_uint32(h), C.c_uint32(flags)]
            assert call(*args, *extra, None, None) == (0 if known else passes.HOST_PANIC), flags
    assert _lib.RASTER_WIDE_GUARD == 32 and raster.WIDE_GUARD == 32
    assert _lib.load().orbit_abi_version() == 6  # additive
    with open(os.path.join(ROOT, "include", "orbit_abi_ext.h")) as fh:
        assert "#define ORBIT_RASTER_WIDE_GUARD 32u" in fh.read()
