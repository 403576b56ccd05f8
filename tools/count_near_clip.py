"""What ORBIT_RASTER_CLIP_NEAR changes for a camera INSIDE the glTF test scene, counted exactly on the CPU (DESIGN.md
§4.14): the oracle's culls, the host mirror's raster (orbit_amd.raster) and the oracle's depth_reduce.  No GPU.  The
scene is tests/raster_scene.glb_scene(100) at 320 x 180; frame 0 starts from empty visibility bits at CAMERAS[0], the
counted frame is the two-pass frame at CAMERAS[1] (early cull -> raster CLEAR -> pyramid -> late cull -> raster LOAD).
With and without the flag:
  clip_skipped, covered_pixels, pixels_at_depth_one   of the UNCULLED list (GlbScene.all_commands) at CAMERAS[1]
  early_commands, late_commands                       the two draw lists of the frame
  hiz_rejected                                        meshlets the late pass's HiZ test rejected
  false_occlusion_pixels                              pixels where the frame's final depth lies below the unculled
                                                      list's depth, both rasterised with the same flag
  missing_visible_commands                            commands that own a pixel of the unculled list's visibility buffer
                                                      and are in neither draw list, split by the stage that lost them:
  missing_by_frustum_or_cone                          ... absent from the pass-0 list as well (occlusion_pass 0: frustum
                                                      and cone only) — the reference's culls, nothing of the raster's
  missing_by_occlusion                                ... in the pass-0 list: lost to the frame's visibility bits or HiZ
  false_occlusion_pixels_vs_pass0                     pixels where the frame's final depth lies below the PASS-0 list's
                                                      depth: what occlusion culling against this raster's depth loses
--wide counts ORBIT_RASTER_WIDE_GUARD as well: the same frame a third time with both flags, with the
guard_skipped of every list beside the counts above, into profiles/wide_guard_cpu.json.
Usage: python tools/count_near_clip.py [--wide] [--out profiles/near_clip_cpu.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

INSTANCES, WIDTH, HEIGHT = 100, 320, 180
CAMERAS = ((0.0, -2.9, -27.0), (0.0, -2.9, -30.0))  # both inside the terrain mesh (entity 2, radius 28 around (0, -3, -30))


def command_rows(draw_bytes):
    b = np.ascontiguousarray(draw_bytes).view(np.uint8).reshape(-1)
    n = int(b[:4].view(np.uint32)[0])
    return b[4:4 + 28 * n].view(np.uint32).reshape(n, 7)


def host_raster(scene, draw, cam, width, height, clip_near, depth=None, clear=True, wide_guard=False):
    import raster_scene as rs
    from orbit_amd import raster

    words = np.ascontiguousarray(draw).view(np.uint8).reshape(-1)
    out = raster.host_raster_depth(words, (words.nbytes - 4) // 28, scene.meshlet_data, scene.vertices, len(scene.vertices),
                                   scene.entities, rs.view_proj(cam), width, height, depth=depth, clear=clear,
                                   clip_near=clip_near, wide_guard=wide_guard)
    assert not out[2].any()
    return out


def two_pass_frame(scene, oracle, cams, width, height, clip_near, wide_guard=False):
    """raster_scene.two_pass_frame with the flags on both raster calls -> the last camera's stages"""
    evis, mvis = np.zeros((scene.n + 31) // 32, np.uint32), np.zeros(scene.vis_words, np.uint32)
    for cam in cams:
        _, _, draw1, _, _ = scene.cull(oracle, cam, 1, evis=evis, mvis=mvis)
        depth1, st1, _ = host_raster(scene, draw1, cam, width, height, clip_near, wide_guard=wide_guard)
        pyr, pd = oracle.depth_reduce(depth1, width, height)
        _, _, draw2, evis2, mvis2 = scene.cull(oracle, cam, 2, evis=evis, mvis=mvis, pyramid=pyr,
                                               pyramid_size=(pd.width, pd.height))
        depth2, st2, _ = host_raster(scene, draw2, cam, width, height, clip_near, depth=depth1, clear=False,
                                     wide_guard=wide_guard)
        frame = dict(evis_in=evis, mvis_in=mvis, draw1=draw1, depth1=depth1, stats1=st1, pyramid=pyr, pyramid_desc=pd,
                     draw2=draw2, depth2=depth2, stats2=st2, evis=evis2, mvis=mvis2)
        evis, mvis = evis2, mvis2
    return frame


def frame_counts(scene, oracle, cams, width, height, clip_near, wide_guard=False, with_guard=False):
    import raster_scene as rs
    from orbit_amd import raster

    cam = cams[-1]
    fr = two_pass_frame(scene, oracle, cams, width, height, clip_near, wide_guard)
    words = scene.all_commands(oracle, cam)
    n = int(words[0])
    vis, st, err = raster.host_raster_visibility(words, n, scene.meshlet_data, scene.vertices, len(scene.vertices),
                                                 scene.entities, rs.view_proj(cam), width, height, clip_near=clip_near,
                                                 wide_guard=wide_guard)
    assert not err.any()
    depth_all, pixels_all, _ = raster.host_visibility_resolve(vis, 0, n)
    rows_all = command_rows(words)
    drawn = {r.tobytes() for r in command_rows(fr["draw1"])} | {r.tobytes() for r in command_rows(fr["draw2"])}
    missing = [int(k) for k in np.flatnonzero(pixels_all) if rows_all[k].tobytes() not in drawn]
    _, _, draw0, _, _ = scene.cull(oracle, cam, 0)  # frustum and cone only
    pass0 = {r.tobytes() for r in command_rows(draw0)}
    depth0, _, _ = host_raster(scene, draw0, cam, width, height, clip_near, wide_guard=wide_guard)
    by_occlusion = [k for k in missing if rows_all[k].tobytes() in pass0]
    # (only when asked for: without it the result has the keys it had before the flag existed)
    guard = dict(wide_guard=bool(wide_guard), guard_skipped=int(st["guard_skipped"]),
                 guard_skipped_early=int(fr["stats1"]["guard_skipped"]),
                 guard_skipped_late=int(fr["stats2"]["guard_skipped"])) if with_guard or wide_guard else {}
    return dict(clip_near=bool(clip_near), **guard, unculled_commands=n, unculled_triangles=int(st["triangles"]),
                clip_skipped=int(st["clip_skipped"]), covered_pixels=int((depth_all > 0).sum()),
                pixels_at_depth_one=int((depth_all == 1.0).sum()),
                early_commands=len(command_rows(fr["draw1"])), late_commands=len(command_rows(fr["draw2"])),
                hiz_rejected=rs.hiz_rejected(scene, oracle, cam, fr),
                false_occlusion_pixels=int((fr["depth2"].reshape(-1) < depth_all.reshape(-1)).sum()),
                missing_visible_commands=len(missing), missing_by_frustum_or_cone=len(missing) - len(by_occlusion),
                missing_by_occlusion=len(by_occlusion),
                false_occlusion_pixels_vs_pass0=int((fr["depth2"].reshape(-1) < depth0.reshape(-1)).sum()),
                missing_visible_pixels=int(pixels_all[missing].sum()) if missing else 0), fr, depth_all


def count(oracle, width=WIDTH, height=HEIGHT, wide=False):
    import raster_scene as rs

    scene = rs.glb_scene(INSTANCES)
    cams = [rs.camera(width, height, p) for p in CAMERAS]
    off, _, depth_off = frame_counts(scene, oracle, cams, width, height, False, with_guard=wide)
    on, _, depth_on = frame_counts(scene, oracle, cams, width, height, True, with_guard=wide)
    assert (depth_on.view(np.uint32) >= depth_off.view(np.uint32)).all()  # R3c: the flag only adds depth
    out = dict(scene=f"tools/make_test_glb.py, {INSTANCES} instances, seed 7", width=width, height=height,
               cameras=[list(c) for c in CAMERAS], unflagged=off, flagged=on)
    if wide:
        both, _, depth_both = frame_counts(scene, oracle, cams, width, height, True, True)
        assert (depth_both.view(np.uint32) >= depth_on.view(np.uint32)).all()  # R4w: and so does this one
        out["flagged_wide"] = both
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--wide", action="store_true", help="ORBIT_RASTER_WIDE_GUARD too; the default --out becomes wide_guard_cpu.json")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "wide_guard_cpu.json" if args.wide else "near_clip_cpu.json")
    from oracle import oracle

    oracle.build()
    oracle.lib()
    result = count(oracle, wide=args.wide)
    line = json.dumps(result)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
