"""What orbit_visibility_surface makes of the two-pass frame on the glTF test scene, counted exactly on the CPU (DESIGN.md
§4.21): the oracle's culls, the host mirror's visibility buffer and the host mirror's surface
(orbit_amd.raster.host_visibility_surface), one call per list into shared outputs.  No GPU.  The scene, the size and the
two cameras are those of tools/count_visible_list.py.  Per frame:
  covered_pixels, written_pixels, degenerate_pixels, unsupported_pixels, stale_pixels   summed over the two calls
  min_sum, max_sum          the smallest and largest l1 + l2 of a written pixel (in double)
  max_relative_error        the largest |l - exact| / exact over both l of every written pixel, exact = E_j / w_j over the
                            sum of the three in rational arithmetic from the snapped integers and the float w (values
                            below 2^-100 are left out: compared absolutely in the tests); in units of 2^-24
`inside` is the frame of tools/count_near_clip.py's inside-terrain camera drawn with ORBIT_RASTER_CLIP_NEAR |
ORBIT_RASTER_WIDE_GUARD: unsupported_share = unsupported / covered is what decides whether the pieces of R3c and the wide
triangles of R4w deserve a surface of their own.
Usage: python tools/count_visible_surface.py [--out profiles/visible_surface_cpu.json]
"""
import argparse
import importlib.util
import json
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

INSTANCES, WIDTH, HEIGHT = 100, 320, 180
CAMERAS = ((0.0, 1.0, 6.0), (0.0, 1.0, 3.0))
F = np.float32
COUNTERS = ("covered_pixels", "written_pixels", "degenerate_pixels", "unsupported_pixels", "stale_pixels", "foreign_pixels")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def max_relative_error(vis, out, scene, view_proj, width, height):
    """Every written pixel's two l against the exact rational value -> the largest relative error, in units of 2^-24."""
    import visibility_surface_ref as ref

    tri = out["triangle"]
    ys, xs = np.nonzero(tri[..., 0] != 0xFFFFFFFF)
    keys = tri[ys, xs]
    worst = Fraction(0)
    order = np.lexsort(keys.T[::-1])
    ys, xs, keys = ys[order], xs[order], keys[order]
    starts = np.flatnonzero(np.r_[True, (keys[1:] != keys[:-1]).any(axis=1)])
    vp = np.asarray(view_proj, F)
    for a, b in zip(starts, np.r_[starts[1:], len(keys)]):
        entity, g = int(keys[a][0]), [int(v) for v in keys[a][1:]]
        mvp = ref._mvp(vp, np.asarray(scene.entities[entity]["model_matrix"], F).reshape(16))
        X, Y, W = [], [], []
        for v in g:
            p = scene.vertices.reshape(-1, 3)[v]
            cx, cy, _, w = (F(F(F(mvp[r] * p[0]) + F(mvp[4 + r] * p[1])) + F(mvp[8 + r] * p[2])) + F(mvp[12 + r] * F(1)) for r in range(4))
            w = F(w)
            X.append(int(np.rint(F(F(F(F(F(cx) / w) * F(0.5)) + F(0.5)) * F(width)) * F(256))))
            Y.append(int(np.rint(F(F(F(F(F(cy) / w) * F(-0.5)) + F(0.5)) * F(height)) * F(256))))
            W.append(Fraction(float(w)))
        for y, x in zip(ys[a:b], xs[a:b]):
            px, py = 256 * int(x) + 128, 256 * int(y) + 128
            edge = lambda u, v: (X[v] - X[u]) * (py - Y[u]) - (Y[v] - Y[u]) * (px - X[u])  # noqa: E731
            q = [Fraction(e) / wj for e, wj in zip((edge(1, 2), edge(2, 0), edge(0, 1)), W)]
            s = sum(q)
            for value, exact in zip(out["bary"][y, x], (q[1] / s, q[2] / s)):
                if exact >= Fraction(1, 2 ** 100):
                    worst = max(worst, abs(Fraction(float(value)) - exact) / exact)
    return float(worst * 2 ** 24)


def surface_of(scene, vis, lists, view_proj):
    """lists: [(draw bytes, command_base)] -> (the shared outputs, the counters summed over the calls)"""
    from orbit_amd import raster

    out, total = None, dict.fromkeys(COUNTERS, 0)
    for k, (draw, base) in enumerate(lists):
        out = raster.host_visibility_surface(vis, draw, scene.cap_c, scene.meshlet_data, scene.vertices, len(scene.vertices),
                                             scene.entities, view_proj, command_base=base, clear=k == 0, into=out)
        for name in COUNTERS:
            total[name] += int(out["stats"][name])
    total["covered_pixels"] = int((vis != 0).sum())  # (each call counts every covered pixel: the other list's as foreign)
    del total["foreign_pixels"]
    return out, total


def frame_row(scene, frame, cam, width, height, **flags):
    import raster_scene as rs
    from orbit_amd import raster

    vp = rs.view_proj(cam)
    vis = None
    for k, name in enumerate(("draw1", "draw2")):
        vis, _, err = raster.host_raster_visibility(frame[name], scene.cap_c, scene.meshlet_data, scene.vertices, len(scene.vertices),
                                                    scene.entities, vp, width, height, visibility=vis, clear=k == 0,
                                                    command_base=k * scene.cap_c, **flags)
        assert not err.any()
    out, total = surface_of(scene, vis, [(frame["draw1"], 0), (frame["draw2"], scene.cap_c)], vp)
    written = out["triangle"][..., 0] != 0xFFFFFFFF
    sums = out["bary"][written].astype(np.float64).sum(axis=1)
    return dict(**total, min_sum=float(sums.min()), max_sum=float(sums.max()),
                max_relative_error=round(max_relative_error(vis, out, scene, vp, width, height), 3))


def count(oracle):
    import raster_scene as rs

    scene = rs.glb_scene(INSTANCES)
    cams = [rs.camera(WIDTH, HEIGHT, p) for p in CAMERAS]
    frames = rs.two_pass_frame(scene, oracle, cams[0], cams[1], WIDTH, HEIGHT)
    out = dict(scene=f"tools/make_test_glb.py, {INSTANCES} instances, seed 7", width=WIDTH, height=HEIGHT, frames=[])
    for f, cam in enumerate(cams):
        out["frames"].append(dict(camera=list(CAMERAS[f]), **frame_row(scene, frames[f], cam, WIDTH, HEIGHT)))
    near = _tool("count_near_clip")
    inside = [rs.camera(WIDTH, HEIGHT, p) for p in near.CAMERAS]
    frame = near.two_pass_frame(scene, oracle, inside, WIDTH, HEIGHT, True, True)
    row = frame_row(scene, frame, inside[-1], WIDTH, HEIGHT, clip_near=True, wide_guard=True)
    out["inside"] = dict(camera=list(near.CAMERAS[-1]), flags="ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD", **row,
                         unsupported_share=round(row["unsupported_pixels"] / max(row["covered_pixels"], 1), 4))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visible_surface_cpu.json"))
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
