"""What orbit_surface_fragments makes of the glTF test scene, counted exactly on the CPU: the oracle's
culls, the host mirror's visibility buffer drawn with ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD, the host mirror's
surface (host_visibility_surface_drawn with both flags) and the host mirror's fragments, one call per list into shared
outputs.  The scene's positions become the reference's 32-B MeshVertex rows with seeded normals, uvs and tangents (the glTF
loader reads positions only).  No GPU.
  inside    both frames of tools/count_near_clip.py's two-pass frame (its two cameras inside the terrain mesh), 320 x 180
  outside   both frames of tools/count_visible_surface.py's cameras, drawn with the same flags
Per frame: the six counters summed over the two calls.  Five accuracy figures over the frames above AND the census of
tests/surface_fragments_cases.py, taken with the restatement tests/surface_fragments_ref.py (which the mirror equals byte
for byte) against its own float64 evaluation of the same definition from the same bary, grad and triangle:
  max_relative_error            the largest |v - exact|_inf / scale over the vectors world_pos, normal, tangent.xyz and uv of
                                every written, non-degenerate pixel, in units of 2^-24; scale = max(|exact|_inf, max_c l_c
                                |a_c|_inf), the largest term of F4's sum (a wide triangle's corners lie 2^60 sub-pixels
                                away and cancel: an error relative to the result alone would measure that, not the call);
                                over the NARROW pixels, as defined next
  max_relative_error_wide       the same over the other pixels.  (F4's l0 = 1 - l1 - l2 carries an absolute error of 2^-24,
                                which a corner 2^50 pixels away multiplies: the consumer of a wide triangle's world_pos
                                meets what §4.23 met in the reprojection of a wide piece.)
  max_reprojection_error_narrow the largest distance, in pixels, between a written pixel's centre and the float64 projection
                                view_proj x world_pos of its fp32 world_pos, over the pixels whose triangle's three
                                ORIGINAL corners all project within 2^15 pixels of it
  max_reprojection_error_wide   the same over the other pixels: wide triangles, and cut ones, whose corner lies behind the
                                eye.  (An fp32 l moves the interpolated point by its rounding times the distance to the
                                corner, as in §4.23.)
  max_uv_grad_difference        the largest |(uv[neighbour] - uv[p]) - uv_grad[p]'s half| / max |uv_c| over the pixels whose
                                right (lower) neighbour is written from the same (entity, g0, g1, g2), in units of 2^-24.
                                (The largest values sit at the diagonal of a cut triangle: grad[p] is the difference within
                                p's piece, S3c, and the neighbour's l come from the other piece.)
A case whose surface call wrote S5's zeros everywhere (all its written pixels degenerate there) is left out.
Usage: python tools/count_surface_fragments.py [--out profiles/surface_fragments_cpu.json]
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
BOTH = 8 | 32
COUNTERS = ("covered_pixels", "written_pixels", "foreign_pixels", "unshaded_pixels", "stale_pixels", "degenerate_pixels")
FIGURES = ("max_relative_error", "max_relative_error_wide", "max_reprojection_error_narrow", "max_reprojection_error_wide", "max_uv_grad_difference")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def accuracy(case, view_proj, got=None):
    """the five figures of one surface_fragments_cases.FragCase (or anything with its args()) under `view_proj`; `got`: the
    restatement's fp32 result where the caller has it already"""
    import surface_fragments_ref as ref

    a, kw = case.args()
    got, exact = ref.fragments(*a, **kw) if got is None else got, ref.fragments(*a, **kw, dtype=np.float64)
    out = dict.fromkeys(FIGURES, 0.0)
    ys, xs = got["written"]
    if len(ys) == 0:
        return out
    fine = ~got["detail"]["degenerate"]
    stats = a[4].get("stats")
    if stats is not None and int(stats["degenerate_pixels"]) == int(stats["written_pixels"]):
        return out  # (S5 wrote zeros: the surface call's l say nothing)
    bary = np.asarray(a[4]["bary"], np.float64).reshape(case.visibility.shape + (2,))[ys, xs]
    weights = [np.maximum(1.0 - bary[:, 0] - bary[:, 1], 0.0), bary[:, 0], bary[:, 1]]
    with np.errstate(all="ignore"):
        # reprojection
        h, w = case.visibility.shape
        vp = np.asarray(view_proj, np.float64).reshape(4, 4).T  # column-major
        project = lambda p: (p @ vp.T)  # noqa: E731
        clip = project(got["detail"]["vals"]["world_pos"].astype(np.float64))
        sx, sy = (clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * w, (clip[:, 1] / clip[:, 3] * -0.5 + 0.5) * h
        dist = np.hypot(sx - (xs + 0.5), sy - (ys + 0.5))
        near = np.ones(len(ys), bool)
        for c in exact["detail"]["corners"]:
            cc = project(c["world_pos"])
            cx, cy = (cc[:, 0] / cc[:, 3] * 0.5 + 0.5) * w, (cc[:, 1] / cc[:, 3] * -0.5 + 0.5) * h
            near &= (cc[:, 3] > 0) & (np.hypot(cx - (xs + 0.5), cy - (ys + 0.5)) <= 2.0 ** 15)
        for name, comps in (("world_pos", 4), ("normal", 3), ("tangent", 3), ("uv", 2)):
            v, e = got["detail"]["vals"][name][:, :comps].astype(np.float64), exact["detail"]["vals"][name][:, :comps]
            terms = [np.abs(c[name][:, :comps]).max(axis=1) * l for c, l in zip(exact["detail"]["corners"], weights)]
            scale = np.maximum(np.abs(e).max(axis=1), np.max(terms, axis=0))
            ok = fine & np.isfinite(e).all(axis=1) & np.isfinite(scale) & (scale > 0)
            for key, mask in (("max_relative_error", ok & near), ("max_relative_error_wide", ok & ~near)):
                if mask.any():
                    out[key] = max(out[key], float((np.abs(v - e).max(axis=1)[mask] / scale[mask]).max()) * 2.0 ** 24)
        ok = fine & np.isfinite(dist)
        if (ok & near).any():
            out["max_reprojection_error_narrow"] = float(dist[ok & near].max())
        if (ok & ~near).any():
            out["max_reprojection_error_wide"] = float(dist[ok & ~near].max())
        # uv_grad against the finite difference
        if a[4].get("grad") is not None:
            index = -np.ones((h, w), np.int64)
            index[ys, xs] = np.arange(len(ys))
            tri = np.asarray(a[4]["triangle"]).reshape(h, w, 4)
            grad = np.asarray(a[4]["grad"], np.float32).reshape(h, w, 4)
            uv, uv_grad = got["detail"]["vals"]["uv"].astype(np.float64), got["detail"]["vals"]["uv_grad"].astype(np.float64)
            uv_scale = np.max([np.abs(c["uv"]).max(axis=1) for c in exact["detail"]["corners"]], axis=0)
            for axis, (dy, dx) in enumerate(((0, 1), (1, 0))):
                inside = (ys + dy < h) & (xs + dx < w)
                p = np.nonzero(inside)[0]
                q = index[ys[p] + dy, xs[p] + dx]
                same = (q >= 0) & (tri[ys[p], xs[p]] == tri[ys[p] + dy, xs[p] + dx]).all(axis=1)
                same &= (grad[ys[p], xs[p], 2 * axis:2 * axis + 2] != 0).any(axis=1)
                p, q = p[same], q[same]
                keep = fine[p] & fine[q] & (uv_scale[p] > 0)
                p, q = p[keep], q[keep]
                if len(p):
                    diff = np.abs((uv[q] - uv[p]) - uv_grad[p, 2 * axis:2 * axis + 2]).max(axis=1) / uv_scale[p]
                    out["max_uv_grad_difference"] = max(out["max_uv_grad_difference"], float(diff.max()) * 2.0 ** 24)
    return out


def census_accuracy():
    import surface_fragments_cases as fc

    worst, pixels = dict.fromkeys(FIGURES, 0.0), 0
    for c in fc.all_cases():
        for k, v in accuracy(c, c.source.packed.case.view_proj).items():
            worst[k] = max(worst[k], v)
        pixels += int((c.surface["triangle"][..., 0] != 0xFFFFFFFF).sum())
    return worst, pixels


def scene_rows(scene):
    """the scene's positions as 32-B MeshVertex rows with seeded attributes -> uint8 bytes"""
    import surface_fragments_cases as fc

    return fc.vertex_rows(scene.vertices, seed=7)


def frame_cases(scene, rows, frame):
    """the two calls of one frame as FragCases over the frame's shared surface (both lists surfaced with both flags)"""
    import surface_fragments_cases as fc
    from orbit_amd import raster

    surf = None
    for k, name in enumerate(("draw1", "draw2")):
        surf = raster.host_visibility_surface_drawn(frame["visibility"], frame[name], scene.cap_c, scene.meshlet_data, scene.vertices,
                                                    len(scene.vertices), scene.entities, frame["view_proj"], command_base=k * scene.cap_c,
                                                    clear=k == 0, into=surf, raster_flags=BOTH)
        assert surf["status"] == 0
    meshlets = np.ascontiguousarray(scene.meshlets).view(np.uint8).reshape(-1)
    surface = {k: surf[k] for k in ("bary", "grad", "triangle")}
    return [fc.FragCase(f"list {k}", frame["visibility"], np.ascontiguousarray(frame[name]).view(np.uint8).reshape(-1), scene.cap_c, meshlets,
                        surface, rows, len(scene.vertices), scene.entities,
                        dict(command_base=k * scene.cap_c, entity_count=scene.entity_count, meshlet_count=len(meshlets) // 32))
            for k, name in enumerate(("draw1", "draw2"))]


def fragments_of(cases):
    """one mirror call per list into shared outputs -> (outputs, counters summed over the calls)"""
    from orbit_amd import raster

    out, total = None, dict.fromkeys(COUNTERS, 0)
    for k, c in enumerate(cases):
        a, kw = c.args()
        out = raster.host_surface_fragments(*a, **kw, clear=k == 0, into=out)
        assert out["status"] == 0
        for name in COUNTERS:
            total[name] += int(out["stats"][name])
    return out, total


def count(oracle):
    import raster_scene as rs
    import surface_fragments_ref as ref

    scene = rs.glb_scene(INSTANCES)
    rows = scene_rows(scene)
    drawn, near, outside = _tool("count_surface_drawn"), _tool("count_near_clip"), _tool("count_visible_surface")
    result = dict(scene=f"tools/make_test_glb.py, {INSTANCES} instances, seed 7; attributes seeded", width=WIDTH, height=HEIGHT,
                  raster_flags="ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD")
    worst = dict.fromkeys(FIGURES, 0.0)
    for where, positions in (("inside", near.CAMERAS), ("outside", outside.CAMERAS)):
        table = []
        for frame, pos in zip(drawn.flagged_frames(scene, oracle, [rs.camera(WIDTH, HEIGHT, p) for p in positions], WIDTH, HEIGHT), positions):
            cases = frame_cases(scene, rows, frame)
            out, total = fragments_of(cases)
            restated = None
            for k, c in enumerate(cases):
                a, kw = c.args()
                restated = ref.fragments(*a, **kw, clear=k == 0, into=restated)
                for key, v in accuracy(c, frame["view_proj"]).items():
                    worst[key] = max(worst[key], v)
            assert all(out[k].tobytes() == restated[k].tobytes() for k in ("world_pos", "normal", "tangent", "uv", "uv_grad", "material"))
            assert total["written_pixels"] == int((frame["visibility"] != 0).sum()) and total["stale_pixels"] == total["unshaded_pixels"] == 0
            table.append(dict(camera=list(pos), **total))
        result[where] = table
    census, pixels = census_accuracy()
    result["census_written_pixels"] = pixels
    for k in FIGURES:
        result[k] = float(f"{max(worst[k], census[k]):.4g}")
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_fragments_cpu.json"))
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
