"""What the two-pass frame loses and what it over-draws on the glTF test scene, counted exactly on the CPU (DESIGN.md
§4.12 / §4.13): the oracle's culls, the host mirror's visibility buffer (orbit_amd.raster.host_raster_visibility) and
its resolve.  No GPU.  The scene is tests/raster_scene.glb_scene(100) at 320 x 180 with the two cameras of
tests/test_raster_depth_gpu.py::test_two_pass_frame_equals_the_cpu_chain (frame 0 starts from empty visibility bits,
frame 1 from frame 0's).  Per frame:
  false_occlusion_pixels     (a) pixels where the frame's final depth lies below the depth of the UNCULLED draw list
                             (GlbScene.all_commands: the LOD pick applied, nothing culled)
  missing_visible_commands   (b) commands that own >= 1 pixel of the unculled list's visibility buffer and are in neither
                             the early nor the late draw list (matched on the command's seven words, not its position)
  overdraw_commands          (c) commands of the early and late lists that own no pixel of the frame's own visibility
                             buffer (early list at command_base 0, late list merged at command_base = the capacity)
and what they are counted against: the lists' lengths, the unculled list's visible set, the covered pixels.
Usage: python tools/count_false_occlusion.py [--out profiles/false_occlusion_cpu.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

INSTANCES, WIDTH, HEIGHT = 100, 320, 180
CAMERAS = ((0.0, 1.0, 6.0), (0.0, 1.0, 3.0))


def command_rows(draw_bytes):
    """the listed commands of a {count; 28-B commands} buffer as an (n, 7) uint32 array"""
    b = np.ascontiguousarray(draw_bytes).view(np.uint8).reshape(-1)
    n = int(b[:4].view(np.uint32)[0])
    return b[4:4 + 28 * n].view(np.uint32).reshape(n, 7)


def frame_counts(final_depth, unculled_depth, unculled_rows, unculled_pixels, rows1, rows2, pixels1, pixels2):
    """(a), (b), (c) from the frame's final depth, the unculled list's depth / commands / pixels per command, and the
    early and late lists' commands / pixels per command -> dict."""
    drawn = {r.tobytes() for r in rows1} | {r.tobytes() for r in rows2}
    visible = np.flatnonzero(np.asarray(unculled_pixels)[:len(unculled_rows)])
    missing = [int(k) for k in visible if unculled_rows[k].tobytes() not in drawn]
    seen1 = int(np.count_nonzero(np.asarray(pixels1)[:len(rows1)]))
    seen2 = int(np.count_nonzero(np.asarray(pixels2)[:len(rows2)]))
    return dict(false_occlusion_pixels=int((np.asarray(final_depth).reshape(-1) < np.asarray(unculled_depth).reshape(-1)).sum()),
                missing_visible_commands=len(missing),
                missing_visible_pixels=int(np.asarray(unculled_pixels)[missing].sum()) if missing else 0,
                overdraw_commands=len(rows1) + len(rows2) - seen1 - seen2,
                early_commands=len(rows1), late_commands=len(rows2), early_visible=seen1, late_visible=seen2,
                unculled_commands=len(unculled_rows), unculled_visible=len(visible),
                covered_pixels=int((np.asarray(unculled_depth) > 0).sum()))


def unculled(scene, oracle, cam):
    """-> (rows, visibility buffer, depth, pixels per command) of the unculled list on the host mirror"""
    import raster_scene as rs
    from orbit_amd import raster

    words = scene.all_commands(oracle, cam)
    n = int(words[0])
    vis, _, err = raster.host_raster_visibility(words, n, scene.meshlet_data, scene.vertices, len(scene.vertices),
                                                scene.entities, rs.view_proj(cam), WIDTH, HEIGHT)
    assert not err.any()
    depth, pixels, _ = raster.host_visibility_resolve(vis, 0, n)
    return command_rows(words), vis, depth, pixels


def count(oracle):
    import raster_scene as rs
    from orbit_amd import raster

    scene = rs.glb_scene(INSTANCES)
    cams = [rs.camera(WIDTH, HEIGHT, p) for p in CAMERAS]
    frames = rs.two_pass_frame(scene, oracle, cams[0], cams[1], WIDTH, HEIGHT)
    out = dict(scene=f"tools/make_test_glb.py, {INSTANCES} instances, seed 7", width=WIDTH, height=HEIGHT, frames=[])
    for f, cam in enumerate(cams):
        fr = frames[f]
        rows_all, _, depth_all, pixels_all = unculled(scene, oracle, cam)
        args = (scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, rs.view_proj(cam), WIDTH, HEIGHT)
        vis1, _, e1 = raster.host_raster_visibility(fr["draw1"], scene.cap_c, *args)
        vis2, _, e2 = raster.host_raster_visibility(fr["draw2"], scene.cap_c, *args, visibility=vis1, clear=False,
                                                    command_base=scene.cap_c)
        assert not e1.any() and not e2.any()
        depth2, pixels1, _ = raster.host_visibility_resolve(vis2, 0, scene.cap_c)
        _, pixels2, _ = raster.host_visibility_resolve(vis2, scene.cap_c, scene.cap_c)
        assert depth2.tobytes() == fr["depth2"].tobytes()  # V4: the visibility frame IS the depth frame
        c = frame_counts(depth2, depth_all, rows_all, pixels_all, command_rows(fr["draw1"]), command_rows(fr["draw2"]),
                         pixels1, pixels2)
        out["frames"].append(dict(camera=list(CAMERAS[f]), **c))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "false_occlusion_cpu.json"))
    args = ap.parse_args()
    from oracle import oracle

    oracle.build()
    oracle.lib()
    result = count(oracle)
    line = json.dumps(result)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
