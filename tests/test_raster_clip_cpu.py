"""CPU checks of ORBIT_RASTER_CLIP_NEAR (include/orbit_abi_ext.h R3c): the host mirror that is the GPU
tests' reference equals the independent restatement tests/raster_clip_ref.py byte for byte and counter for counter on
every case of tests/raster_clip_cases.py, for both raster calls; the cases reach what they claim; a call whose input
holds nothing R3 rejects is unchanged by the flag, and the flag only ever adds depth; a camera inside the glTF scene
clips, and its two-pass frame loses nothing; the flag word still rejects what it does not know."""
import importlib.util
import os

import numpy as np
import pytest

import raster_cases as rc
import raster_clip_cases as cc
import raster_clip_ref as cref
import raster_scene as rs
import raster_vis_cases as vc
from orbit_amd import _lib, passes, raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cc.all_cases()
OLD = vc.all_cases()  # the census of raster_cases as VisCases, and raster_vis_cases' own


def assert_same(name, got, want, view=np.uint64):
    buf, stats, err = got
    wbuf, wstats, werr, _ = want
    for k in cref.STAT_NAMES:
        assert int(stats[k]) == wstats[k], f"{name}: {k} = {int(stats[k])}, restated {wstats[k]}"
    assert list(err) == werr, name
    diff = np.argwhere(buf.view(view) != wbuf.view(view))
    assert len(diff) == 0, f"{name}: {len(diff)} pixels differ, first at (y, x) = {diff[0]}"


def test_the_case_set_reaches_what_it_claims(capsys):
    missed = {k: v for k, v in cc.census(CASES).items() if v}
    assert not missed, missed
    assert len(capsys.readouterr().out.splitlines()) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_mirror_equals_the_restatement(case):
    pk = rc.Packed(case)
    vis, depth = cc.host_vis(pk), cc.host_depth(pk)
    want = cc.restated_vis(pk)
    assert_same(case.name, vis, want)
    assert_same(case.name, depth, cc.restated_depth(pk), np.uint32)
    assert not cc.check_claims(case, vis[0], vis[1], vis[2], want[3])  # the claims hold on the mirror's own output
    # V4 with the flag on both calls
    assert cref.depth_of(vis[0]).tobytes() == depth[0].tobytes() and vis[1].tobytes() == depth[1].tobytes()
    # without the flag the case is what it was before the flag existed: every crossing triangle is clip_skipped
    off = cc.host_vis(pk, clip_near=False)
    assert_same(case.name, off, cc.restated_vis(pk, clip_near=False))
    assert (vis[0] >> np.uint64(32) >= off[0] >> np.uint64(32)).all()
    assert int(off[1]["clip_skipped"]) == int(vis[1]["clip_skipped"]) + want[3]["one_in"] + want[3]["one_out"]


@pytest.mark.parametrize("stride,offset", [(32, 20)])
def test_host_mirror_reads_strided_vertices(stride, offset):
    for case in CASES:
        want = cc.host_vis(rc.Packed(case))
        got = cc.host_vis(rc.Packed(case, stride, offset, vertex_base=1, data_base=0))
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], case.name


def test_the_flag_changes_nothing_where_r3_rejects_nothing_and_only_adds_depth_elsewhere():
    unchanged, rejecting = 0, set()
    for case in OLD:
        pk = rc.Packed(case)
        for host in (cc.host_vis, cc.host_depth):
            off, on = host(pk, clip_near=False), host(pk)
            if int(off[1]["clip_skipped"]) == 0:
                assert on[0].tobytes() == off[0].tobytes() and on[1].tobytes() == off[1].tobytes(), case.name
                assert list(on[2]) == list(off[2])
                unchanged += 1
            else:
                rejecting.add(case.name)
            shift = 32 if host is cc.host_vis else 0
            bits = lambda r: r[0].view(np.uint64 if shift else np.uint32) >> (np.uint64(32) if shift else np.uint32(0))  # noqa: E731
            assert (bits(on) >= bits(off)).all(), case.name
            for k in ("commands", "triangles", "range_errors"):
                assert int(on[1][k]) == int(off[1][k])
    # the four cases of the census in which R3 rejects a triangle; every other one went through the comparison
    assert rejecting == {"behind_w0", "between_eye_and_near", "z_above_w_by_one_ulp", "nan_and_inf_positions"}
    assert unchanged == 2 * (len(OLD) - 4)


def test_the_census_neighbours_of_the_near_plane_are_now_drawn():
    """raster_cases' between_eye_and_near and behind_w0: the triangle R3 rejects is cut and drawn with the flag."""
    for name in ("between_eye_and_near", "behind_w0", "z_above_w_by_one_ulp"):
        pk = rc.Packed(next(c for c in rc.all_cases() if c.name == name))
        off, on = cc.host_depth(pk, clip_near=False), cc.host_depth(pk)
        assert_same(name, on, cc.restated_depth(pk), np.uint32)
        assert (int(off[1]["clip_skipped"]), int(on[1]["clip_skipped"])) == (1, 0), name


def test_load_without_clear_into_what_an_unflagged_call_left():
    pk = rc.Packed(next(c for c in CASES if c.name == "fan_around_a_vertex_behind_the_eye"))
    other = rc.Packed(next(c for c in CASES if c.name == "lone_out_vertex_0"))
    left_d, left_v = cc.host_depth(other, clip_near=False)[0], cc.host_vis(other, clip_near=False)[0]
    assert not left_d.any()  # unflagged, the crossing triangle left nothing ...
    left_d, left_v = cc.host_depth(rc.Packed(rc.all_cases()[0]))[0], vc.host(rc.Packed(vc.all_cases()[0]))[0]
    assert left_d.any() and left_v.any()  # ... so load what an unflagged call of the census left
    got_d = cc.host_depth(pk, depth=left_d, clear=False)
    assert_same("load depth", got_d, cc.restated_depth(pk, depth=left_d, clear=False), np.uint32)
    got_v = cc.host_vis(pk, visibility=left_v, clear=False)
    assert_same("load visibility", got_v, cc.restated_vis(pk, visibility=left_v, clear=False))
    assert got_d[0].tobytes() == np.maximum(left_d, cc.host_depth(pk)[0]).tobytes() != left_d.tobytes()
    assert cref.depth_of(got_v[0]).tobytes() == got_d[0].tobytes()


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("count_near_clip", os.path.join(ROOT, "tools", "count_near_clip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_inside_camera_scene_equals_the_restatement_and_clips(oracle, tool):
    scene = rs.glb_scene(tool.INSTANCES)
    w, h = 256, 144
    cam = rs.camera(w, h, tool.CAMERAS[1])
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    n = int(draw[:4].view(np.uint32)[0])
    args = (draw, n, scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, rs.view_proj(cam), w, h)
    got = raster.host_raster_visibility(*args, clip_near=True)
    want = cref.raster(*args, flags=cref.CLEAR | cref.CLIP_NEAR)
    assert_same("inside camera", got, want)
    off = raster.host_raster_visibility(*args)
    print(f"{n} commands; unflagged {off[1]}; flagged {got[1]}; {want[3]}")
    clipped = want[3]["one_in"] + want[3]["one_out"]
    assert clipped >= 100 and want[3]["one_in"] > 0 and want[3]["one_out"] > 0
    assert int(off[1]["clip_skipped"]) - int(got[1]["clip_skipped"]) == clipped
    assert (got[0] >> np.uint64(32) >= off[0] >> np.uint64(32)).all()
    assert int((got[0] != 0).sum()) > int((off[0] != 0).sum())  # the floor under the camera is in the buffer now
    depth = raster.host_raster_depth(*args, clip_near=True)
    assert cref.depth_of(got[0]).tobytes() == depth[0].tobytes() and got[1].tobytes() == depth[1].tobytes()


@pytest.mark.parametrize("clip_near", [True, False])
def test_inside_camera_two_pass_frame_loses_nothing_to_occlusion(oracle, tool, clip_near):
    """With the flag the frame loses nothing at all.  Without it the frame may lack a visible command that the
    reference's frustum / cone tests reject (coneCull transforms the cone axis by the model matrix and does not
    normalise it, so an entity scaled up is over-culled: meshlet_cull.comp:105,121) — such a command is absent from the
    pass-0 list too; what the frame's own occlusion culling loses against its raster depth is nothing either way."""
    scene = rs.glb_scene(tool.INSTANCES)
    w, h = 256, 144
    cams = [rs.camera(w, h, p) for p in tool.CAMERAS]
    counts, _, _ = tool.frame_counts(scene, oracle, cams, w, h, clip_near)
    print(counts)
    assert counts["missing_by_occlusion"] == 0 and counts["false_occlusion_pixels_vs_pass0"] == 0
    assert counts["missing_visible_commands"] == counts["missing_by_frustum_or_cone"]
    if clip_near:
        assert counts["false_occlusion_pixels"] == 0 and counts["missing_visible_commands"] == 0
    assert counts["early_commands"] > 1000 and counts["covered_pixels"] > 0


def test_unknown_flags_still_panic_and_the_version_stays():
    import ctypes as C

    pk = rc.Packed(CASES[0])
    _, (words, mc, data, vb, vcount, ent, vp, w, h) = pk.args()
    lib = passes.lib()
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    vpc = (C.c_float * 16)(*vp)
    for call, out, extra in ((lib.orbit_host_raster_depth, np.zeros(w * h, np.float32), []),
                             (lib.orbit_host_raster_visibility, np.zeros(w * h, np.uint64), [C.c_uint32(0)])):
        for flags, known in ((8, True), (9, True), (11, True), (4, False), (16, False), (12, False), (24, False)):
            args = [p(words), C.c_uint32(mc), p(data), C.c_uint64(len(data)), p(vb), C.c_uint64(vcount), C.c_uint32(12),
                    C.c_uint32(0), p(ent), C.c_uint32(1), vpc, p(out), C.c_uint32(w), C.c_uint32(h), C.c_uint32(flags)]
            assert call(*args, *extra, None, None) == (0 if known else passes.HOST_PANIC), flags
    assert _lib.RASTER_CLIP_NEAR == 8 and raster.CLIP_NEAR == 8
    assert _lib.load().orbit_abi_version() == 6  # additive
    with open(os.path.join(ROOT, "include", "orbit_abi_ext.h")) as fh:
        assert "#define ORBIT_RASTER_CLIP_NEAR 8u" in fh.read()
