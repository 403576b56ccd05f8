"""What orbit_visibility_surface_drawn makes of the glTF test scene, counted exactly on the CPU: the
oracle's culls, the host mirror's visibility buffer drawn with ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD and the host
mirror's surface (orbit_amd.raster.host_visibility_surface_drawn), one call per list into shared outputs, beside
orbit_visibility_surface on the same buffer.  No GPU.
  inside    both frames of tools/count_near_clip.py's two-pass frame (its two cameras inside the terrain mesh), 320 x 180
  outside   both frames of tools/count_visible_surface.py's cameras, drawn with the same flags
Per frame: covered, and written / unsupported / stale / degenerate of the old call and of the new one with both flags,
cut_pixels and wide_pixels of the new one.  Two accuracy figures over the frames above AND the census of
tests/surface_drawn_cases.py, taken with the restatement tests/surface_drawn_ref.py, which the mirror equals byte for byte:
  max_relative_error      the largest |l - exact| / exact over both l of every written pixel, in units of 2^-24; exact: the
                          rational value from the snapped integers and the floats w_i and t (evaluated in float64, which is
                          good to 2^-47 there, and in fractions.Fraction where float64 cannot decide the tests' bound)
  max_reprojection_error  the largest distance, in pixels, between the centre of a written CUT pixel and the projection of
                          sum_c l_c * clip_c over the ORIGINAL corners in float64 (S3c's formula is not used)
  max_reprojection_error_narrow_pieces   the same over the pixels of narrow pieces only.  (An fp32 l moves the projection by
                          its rounding times the distance to the corner: a wide piece's corners lie up to 2^31 sub-pixels
                          away, where one rounding of l is a quarter of a pixel.)
Usage: python tools/count_surface_drawn.py [--out profiles/surface_drawn_cpu.json]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

INSTANCES, WIDTH, HEIGHT = 100, 320, 180
CLIP, WIDE = 8, 32
COUNTERS = ("written_pixels", "unsupported_pixels", "stale_pixels", "degenerate_pixels", "cut_pixels", "wide_pixels")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def flagged_frames(scene, oracle, cams, width, height):
    """the two-pass frame of each camera in turn, every raster call with both flags -> [dict(cam, view_proj, draw1, draw2,
    visibility)]: the visibility buffer of both lists, the late one at base = the capacity"""
    import raster_scene as rs
    from orbit_amd import raster

    near = _tool("count_near_clip")
    out = []
    evis, mvis = np.zeros((scene.n + 31) // 32, np.uint32), np.zeros(scene.vis_words, np.uint32)
    for cam in cams:
        _, _, draw1, _, _ = scene.cull(oracle, cam, 1, evis=evis, mvis=mvis)
        depth1, _, _ = near.host_raster(scene, draw1, cam, width, height, True, wide_guard=True)
        pyr, pd = oracle.depth_reduce(depth1, width, height)
        _, _, draw2, evis, mvis = scene.cull(oracle, cam, 2, evis=evis, mvis=mvis, pyramid=pyr, pyramid_size=(pd.width, pd.height))
        vp, vis = rs.view_proj(cam), None
        for k, draw in enumerate((draw1, draw2)):
            vis, _, err = raster.host_raster_visibility(draw, scene.cap_c, scene.meshlet_data, scene.vertices, len(scene.vertices),
                                                        scene.entities, vp, width, height, visibility=vis, clear=k == 0,
                                                        command_base=k * scene.cap_c, clip_near=True, wide_guard=True)
            assert not err.any()
        out.append(dict(cam=cam, view_proj=vp, draw1=draw1, draw2=draw2, visibility=vis))
    return out


def surface_of(scene, frame, raster_flags, restated=False):
    """one call per list into shared outputs -> (outputs, counters summed over the calls, the calls' own results)"""
    import surface_drawn_ref as ref
    from orbit_amd import raster

    out, total, calls = None, dict.fromkeys(COUNTERS, 0), []
    for k, name in enumerate(("draw1", "draw2")):
        args = (frame["visibility"], frame[name], scene.cap_c, scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities,
                frame["view_proj"])
        if restated:
            out = ref.surface(*args, command_base=k * scene.cap_c, clear=k == 0, into=out, raster_flags=raster_flags, keep_detail=True)
        else:
            out = raster.host_visibility_surface_drawn(*args, command_base=k * scene.cap_c, clear=k == 0, into=out, raster_flags=raster_flags)
        calls.append(out)
        for name_ in COUNTERS:
            total[name_] += int(out["stats"][name_])
    return out, total, calls


def accuracy(bary, detail, width, height):
    """(largest relative error in 2^-24, largest reprojection distance of a cut pixel in pixels, the same over the pixels
    of NARROW pieces only) of one restated call's written pixels (`detail` of surface_drawn_ref.surface) in `bary`"""
    import surface_drawn_ref as ref

    written = detail["owner"] >= 0
    worst, far, far_narrow = 0.0, 0.0, 0.0
    if not written.any():
        return worst, far, far_narrow
    approx, got = detail["approx"][written], bary[written].astype(np.float64)
    sure = approx > 2.0 ** -90
    if sure.any():
        worst = float((np.abs(got - approx)[sure] / approx[sure]).max()) * 2.0 ** 24
    for q, (s, cut, clips) in enumerate(detail["setups"]):
        if not cut:
            continue
        ys, xs = np.nonzero(detail["owner"] == q)
        l1, l2 = bary[ys, xs, 0].astype(np.float64), bary[ys, xs, 1].astype(np.float64)
        l0 = 1.0 - l1 - l2
        c = [l0 * float(clips[0][r]) + l1 * float(clips[1][r]) + l2 * float(clips[2][r]) for r in (0, 1, 3)]
        sx, sy = (c[0] / c[2] * 0.5 + 0.5) * width, (c[1] / c[2] * -0.5 + 0.5) * height
        dist = float(np.hypot(sx - (xs + 0.5), sy - (ys + 0.5)).max(initial=0.0))
        far, far_narrow = max(far, dist), far_narrow if s["wide"] else max(far_narrow, dist)
    assert ref.F is np.float32
    return worst, far, far_narrow


def census_accuracy():
    import surface_drawn_cases as dc
    import surface_drawn_ref as ref

    worst, far, narrow, pixels = 0.0, 0.0, 0.0, 0
    for c in dc.all_cases():
        a, kw = c.args()
        want = ref.surface(*a, **kw, keep_detail=True)
        if want["stats"]["degenerate_pixels"] == want["stats"]["written_pixels"]:
            continue  # (S5 wrote zeros)
        h, w = c.visibility.shape
        e, d, dn = accuracy(want["bary"], want["detail"], w, h)
        worst, far, narrow, pixels = max(worst, e), max(far, d), max(narrow, dn), pixels + want["stats"]["written_pixels"]
    return worst, far, narrow, pixels


def count(oracle):
    import raster_scene as rs

    scene = rs.glb_scene(INSTANCES)
    near, outside = _tool("count_near_clip"), _tool("count_visible_surface")
    result = dict(scene=f"tools/make_test_glb.py, {INSTANCES} instances, seed 7", width=WIDTH, height=HEIGHT,
                  raster_flags="ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD")
    worst, far, narrow = 0.0, 0.0, 0.0
    for where, positions in (("inside", near.CAMERAS), ("outside", outside.CAMERAS)):
        rows = []
        for frame, pos in zip(flagged_frames(scene, oracle, [rs.camera(WIDTH, HEIGHT, p) for p in positions], WIDTH, HEIGHT), positions):
            _, old, _ = surface_of(scene, frame, 0)
            new_out, new, _ = surface_of(scene, frame, CLIP | WIDE)
            ref_out, restated, calls = surface_of(scene, frame, CLIP | WIDE, restated=True)
            assert restated == new and all(new_out[k].tobytes() == ref_out[k].tobytes() for k in ("bary", "grad", "triangle"))
            for call in calls:  # (the second call's outputs hold the first's pixels too: each call's own `detail` selects)
                e, d, dn = accuracy(ref_out["bary"], call["detail"], WIDTH, HEIGHT)
                worst, far, narrow = max(worst, e), max(far, d), max(narrow, dn)
            rows.append(dict(camera=list(pos), covered_pixels=int((frame["visibility"] != 0).sum()),
                             old={k: old[k] for k in COUNTERS[:4]}, new=new))
        result[where] = rows
    e, d, dn, pixels = census_accuracy()
    result["census_written_pixels"] = pixels
    result["max_relative_error"] = round(max(worst, e), 3)
    result["max_reprojection_error"] = float(f"{max(far, d):.3g}")
    result["max_reprojection_error_narrow_pieces"] = float(f"{max(narrow, dn):.3g}")
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_drawn_cpu.json"))
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
