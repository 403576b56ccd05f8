"""What orbit_visibility_compact makes of the two-pass frame's draw lists on the glTF test scene, counted exactly on the
CPU: the oracle's culls, the host mirror's visibility buffer and the host mirror's compaction
(orbit_amd.raster.host_visibility_compact).  No GPU.  The scene, the size and the two cameras are those of
tools/count_false_occlusion.py.  Per frame, the early list (command_base 0) and the late list (command_base = the
capacity) are each compacted from the frame's final buffer, with ORBIT_COMPACT_TRIANGLES:
  commands_in / triangles_in     the two lists' commands and their triangles
  commands_out / triangles_out   the visible commands and the triangles that own a pixel
  data_words_needed              the words of the two cut lists' visible_data, beside
  input_meshlet_words            the index words and corner words the input commands address in meshlet_data
  raster_out                     the raster counters of the two output lists drawn again (early CLEAR, late merged)
  c6_missed                      what of C6 did not hold on the way (the lists, both modes): must be empty
Usage: python tools/count_visible_list.py [--out profiles/visible_list_cpu.json]
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
RASTER_COUNTERS = ("commands", "triangles", "clip_skipped", "guard_skipped", "back_facing", "no_coverage", "fragments", "range_errors")


def frame_lists(scene, frame, cam):
    """-> (the frame's final buffer, [(name, CompactCase)] of its early and late list)"""
    import raster_scene as rs
    import visibility_compact_cases as cc
    from orbit_amd import raster

    args = (scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, rs.view_proj(cam), WIDTH, HEIGHT)
    vis1, _, e1 = raster.host_raster_visibility(frame["draw1"], scene.cap_c, *args)
    vis2, _, e2 = raster.host_raster_visibility(frame["draw2"], scene.cap_c, *args, visibility=vis1, clear=False,
                                                command_base=scene.cap_c)
    assert not e1.any() and not e2.any()
    lists = [(name, cc.CompactCase(name, vis2, np.ascontiguousarray(frame[key]).view(np.uint8).reshape(-1).view(np.uint32),
                                   scene.cap_c, scene.meshlet_data, base, one_clear_call=False))
             for name, key, base in (("early", "draw1", 0), ("late", "draw2", scene.cap_c))]
    return vis2, args, lists


def redraw(outs, args, triangles):
    """The two output lists drawn again: early CLEAR at base 0, late merged behind it -> (buffer, [stats], late's base)"""
    from orbit_amd import raster

    vis, stats, base = None, [], 0
    for got in outs:
        n = int(got["commands"][0])
        data = (got["data"], *args[1:]) if triangles else args
        vis, st, err = raster.host_raster_visibility(got["commands"], n, *data, visibility=vis, clear=vis is None, command_base=base)
        assert not err.any()
        stats.append(st)
        base += n
    return vis, stats, base - int(outs[-1]["commands"][0])


def count(oracle, check=None):
    """check(name, case, triangles, got), if given, is called with every compaction's case and outputs."""
    import raster_scene as rs
    import visibility_compact_cases as cc
    from orbit_amd import raster

    scene = rs.glb_scene(INSTANCES)
    cams = [rs.camera(WIDTH, HEIGHT, p) for p in CAMERAS]
    frames = rs.two_pass_frame(scene, oracle, cams[0], cams[1], WIDTH, HEIGHT)
    out = dict(scene=f"tools/make_test_glb.py, {INSTANCES} instances, seed 7", width=WIDTH, height=HEIGHT, frames=[])
    for f, cam in enumerate(cams):
        vis2, args, lists = frame_lists(scene, frames[f], cam)
        missed, row = [], None
        for triangles in (False, True):
            outs = []
            for name, case in lists:
                a, kw = case.args(triangles)
                outs.append(raster.host_visibility_compact(*a, **kw))
                if check:
                    check(f"frame {f} {name}", case, triangles, outs[-1])
            again, stats, late_base = redraw(outs, args, triangles)
            if (again >> np.uint64(32) != vis2 >> np.uint64(32)).any():
                missed.append(f"triangles={triangles}: the two output lists do not give the frame's depth")
            for (name, case), got, st, base in zip(lists, outs, stats, (0, late_base)):
                n = int(got["commands"][0])
                _, pixels, rst = raster.host_visibility_resolve(again, base, n)
                missed += cc.c6_misses(f"{name}, triangles={triangles}", vis2, case.command_base, got, triangles, again, st,
                                       pixels, rst, out_base=base, whole=False)
            if triangles:
                rows = [c.words[1:1 + 7 * int(c.words[0])].reshape(-1, 7).astype(np.int64) for _, c in lists]
                row = dict(camera=list(CAMERAS[f]),
                           commands_in=sum(len(r) for r in rows), triangles_in=int(sum((r[:, 0] // 3).sum() for r in rows)),
                           commands_out=sum(int(g["stats"]["visible_commands"]) for g in outs),
                           triangles_out=sum(int(g["stats"]["visible_triangles"]) for g in outs),
                           data_words_needed=sum(int(g["stats"]["data_words_needed"]) for g in outs),
                           input_meshlet_words=int(sum((r[:, 2] // 4 - r[:, 3] + (r[:, 0] + 3) // 4).sum() for r in rows)),
                           covered_pixels=int(outs[0]["stats"]["covered_pixels"]),
                           raster_out={k: sum(int(st[k]) for st in stats) for k in RASTER_COUNTERS})
        out["frames"].append(dict(row, c6_missed=missed))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visible_list_cpu.json"))
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
