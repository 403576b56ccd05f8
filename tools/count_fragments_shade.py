"""What orbit_fragments_shade makes of the glTF test scene, counted exactly on the CPU: the host chain
raster -> resolve -> the oracle's cluster stages -> surface_drawn -> fragments -> shade of tools/count_surface_fragments.py's
outside frame (100 instances, 320 x 180), lit by 200 point lights placed on the visible surface with outer_radius = 1.05 x
sqrt(intensity / cutoff).  No GPU.
  frame             the eight counters, the mean and the largest lights_walked, and whether shading from the real lists
                    equals, byte for byte, shading every pixel from all 200 lights
  max_relative_error  the largest |rgb - exact|_inf / max(|exact|_inf, 2^-20) over the frame's and the hand-built census's
                    written, non-degenerate pixels whose float64 slice is the canonical one, in units of 2^-24; exact is the
                    GLSL in float64 with a true pow(x, 5.0) (tests/fragments_shade_ref.py shade64).  Pixels whose normal
                    faces away from V or from a light sit on max(., EPS): a clamp the float32 value may take and the
                    float64 one not, so pixels with a dot product within 2^-20 of a clamp are counted apart
                    (near_clamp_pixels) and not compared
  slice_differs     pixels whose float64 slice differs from the canonical one: counted, not compared
Usage: python tools/count_fragments_shade.py [--out profiles/fragments_shade_cpu.json]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

N_LIGHTS, TILE, CZ, Z_FAR, CUTOFF = 200, 16, 32, 200.0, 0.01
COUNTERS = ("covered_pixels", "written_pixels", "unshaded_pixels", "stale_pixels", "outside_pixels", "degenerate_pixels", "textured_pixels",
            "unserved_pixels")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cluster_setup(oracle, cam, width, height, n_lights, tile=TILE):
    """-> (push, info, (cx, cy, cz), z_scale, z_bias) of the cluster chain for this camera"""
    import scenes as sc
    from orbit_amd import layouts as L

    cx, cy = -(-width // tile), -(-height // tile)
    zs, zb = oracle.cluster_grid_info(cam.z_near, Z_FAR, CZ)
    push = np.zeros((), dtype=L.MARK_ACTIVE_PUSH)
    push["cluster_count"], push["tile_size_px"], push["screen_size"] = (cx, cy, CZ), tile, (width, height)
    push["z_near"], push["z_far"], push["z_scale"], push["z_bias"] = cam.z_near, Z_FAR, zs, zb
    push["depth_buffer_sample_count"] = 1
    info = np.zeros((), dtype=L.CLUSTER_CULL_INFO)
    info["world_to_view_matrix"] = sc.mat4_cols(cam.view)
    info["screen_to_view_matrix"] = sc.mat4_cols(np.linalg.inv(cam.proj.astype(np.float64)).astype(np.float32))
    info["cluster_count"], info["tile_size_px"], info["screen_size"] = (cx, cy, CZ), tile, (width, height)
    info["z_near"], info["z_far"], info["global_light_count"] = cam.z_near, Z_FAR, n_lights
    return push, info, (cx, cy, CZ), zs, zb


def surface_lights(world_pos, visibility, n=N_LIGHTS, seed=3, spread=1.0, intensity=(0.05, 0.6)):
    """n point lights a little off the visible surface: positions = world_pos of seeded covered pixels + a seeded offset;
    outer_radius = 1.05 x sqrt(intensity / cutoff), beyond which L5's attenuation is exactly +0"""
    from orbit_amd import layouts as L

    rng = np.random.default_rng(seed)
    ys, xs = np.nonzero(visibility)
    pick = rng.integers(0, len(ys), n)
    l = np.zeros(n, L.LIGHT)
    l["light_type"], l["shadow_data_index"] = L.LIGHT_TYPE_POINT, 0xFFFFFFFF
    l["irradiance_map_index"] = l["prefiltered_map_index"] = 0xFFFFFFFF
    l["color"], l["intensity"] = rng.uniform(0.2, 1.0, (n, 3)), rng.uniform(*intensity, n)
    l["position"] = world_pos[ys[pick], xs[pick], :3] + rng.uniform(-spread, spread, (n, 3)).astype(np.float32)
    l["inner_radius"] = 0.05
    l["outer_radius"] = np.float32(1.05) * np.sqrt(l["intensity"] / np.float32(CUTOFF))
    l["direction"] = (0.0, -1.0, 0.0)
    return l


def host_frame(oracle, width=None, height=None):
    """The whole frame on the host (width x height: tools/count_surface_fragments.py's 320 x 180 by default) -> dict: scene, rows, frame (visibility, draw1, draw2, view_proj, cam), planes (the
    fragments call's outputs), depth, lights, push, info, cluster_count, z_scale, z_bias, index_buffer, image, view_pos,
    index_capacity, and `args`: the positional arguments of raster.host_fragments_shade"""
    import raster_scene as rs
    from orbit_amd import raster

    frag = _tool("count_surface_fragments")
    outside = frag._tool("count_visible_surface")
    scene = rs.glb_scene(frag.INSTANCES)
    rows = frag.scene_rows(scene)
    w, h = width or frag.WIDTH, height or frag.HEIGHT
    frame = frag._tool("count_surface_drawn").flagged_frames(scene, oracle, [rs.camera(w, h, p) for p in outside.CAMERAS], w, h)[1]
    planes, total = frag.fragments_of(frag.frame_cases(scene, rows, frame))
    assert total["stale_pixels"] == total["unshaded_pixels"] == 0
    depth, _, _ = raster.host_visibility_resolve(frame["visibility"], want_command_pixels=False)
    cam = frame["cam"]
    lights = surface_lights(planes["world_pos"], frame["visibility"])
    push, info, cc, zs, zb = cluster_setup(oracle, cam, w, h, len(lights))
    masks, bounds = oracle.cluster_mark(push, depth)
    clusters = cc[0] * cc[1] * cc[2]
    unique, _ = oracle.cluster_compact(cc, masks, clusters)
    n_active = int(unique[12:16].view(np.uint32)[0])
    capacity = n_active * 256 + 8
    index_buffer, image, dropped = oracle.cluster_assign(info, unique, bounds, lights, capacity, clusters)
    view_pos = tuple(float(v) for v in np.linalg.inv(cam.view.astype(np.float64))[:3, 3])
    args = (frame["visibility"], planes["world_pos"], planes["normal"], planes["material"], scene.materials, lights, image, index_buffer, cc,
            TILE, zs, zb, CUTOFF, cam.z_near, view_pos)
    return dict(scene=scene, rows=rows, frame=frame, planes=planes, depth=depth, lights=lights, push=push, info=info, cluster_count=cc,
                z_scale=zs, z_bias=zb, index_buffer=index_buffer, image=image, view_pos=view_pos, index_capacity=capacity, dropped=dropped,
                n_active=n_active, args=args, width=w, height=h)


def all_lights_args(args, n_lights):
    """the same call with an image whose every cluster is (0, n_lights) over the list 0 .. n_lights - 1"""
    cc = args[8]
    image = np.tile(np.array([0, n_lights], np.uint32), (cc[0] * cc[1] * cc[2], 1))
    index_buffer = np.concatenate([np.array([n_lights], np.uint32), np.arange(n_lights, dtype=np.uint32)]).view(np.uint8)
    return args[:6] + (image, index_buffer) + args[8:]


def accuracy(oracle, args, kw=None):
    """-> (max relative error in units of 2^-24, compared pixels, slice_differs, near_clamp_pixels) of one call's inputs"""
    import fragments_shade_ref as ref

    kw = {k: v for k, v in (kw or {}).items() if k in ("material_count", "light_count", "index_capacity")}
    got = ref.shade(oracle, *args, **kw)
    pix = np.flatnonzero(got["live"].reshape(-1))
    if not len(pix):
        return 0.0, 0, 0, 0
    exact, sl64 = ref.shade64(*args, pixels=pix)
    canon = ref.slices(oracle, args[0], args[13], args[10], args[11]).reshape(-1)[pix].astype(np.int64)
    same = sl64 == canon
    rgb = got["color"].reshape(-1, 4)[pix, :3].astype(np.float64)
    fine = np.isfinite(exact).all(axis=1) & np.isfinite(got["color"].reshape(-1, 4)[pix, :3]).all(axis=1)
    near = near_clamp(args, pix, got)
    ok = same & fine & ~near
    if not ok.any():
        return 0.0, 0, int((~same).sum()), int(near.sum())
    scale = np.maximum(np.abs(exact).max(axis=1), 2.0 ** -20)
    err = np.abs(rgb - exact).max(axis=1) / scale
    return float(err[ok].max()) * 2.0 ** 24, int(ok.sum()), int((~same).sum()), int((near & same & fine).sum())


def near_clamp(args, pix, got, band=2.0 ** -20):
    """pixels of `pix` with a dot product of L6 within `band` of the value its max() clamps at (EPS or 0), for some walked
    light, or whose distance to a point light lies within a relative `band` of inner_radius or of the attenuation's zero"""
    import fragments_shade_ref as ref
    from orbit_amd import layouts as L

    vis, world_pos, normal, _, _, lights, image, index_buffer, cc, tile, zs, zb, cutoff, z_near, view_pos = args
    c = got["classified"]
    n, offset, indices = c["n"][pix], c["offset"][pix], c["indices"]
    lts = np.ascontiguousarray(lights).view(np.uint8).reshape(-1)
    lts = lts[:len(lts) // 64 * 64].view(L.LIGHT)
    wp = np.asarray(world_pos, np.float64).reshape(-1, 4)[pix, :3]
    N = np.asarray(normal, np.float64).reshape(-1, 3)[pix]
    near = np.zeros(len(pix), bool)
    with np.errstate(all="ignore"):
        V = np.asarray(view_pos, np.float64)[None, :] - wp
        V /= np.linalg.norm(V, axis=1)[:, None]
        near |= np.abs((N * V).sum(1) - 1e-4) < band
        for i in range(int(n.max()) if len(pix) else 0):
            at = np.flatnonzero(n > i)
            l = lts[indices[offset[at] + i]]
            point = l["light_type"] == L.LIGHT_TYPE_POINT
            Ld = l["position"].astype(np.float64) - wp[at]
            dist = np.linalg.norm(Ld, axis=1)
            Ld = np.where(point[:, None], Ld / dist[:, None], l["direction"].astype(np.float64))
            H = V[at] + Ld
            H /= np.linalg.norm(H, axis=1)[:, None]
            hit = np.abs((N[at] * Ld).sum(1) - 1e-4) < band
            hit |= (np.abs((N[at] * H).sum(1)) < band) | (np.abs((H * V[at]).sum(1)) < band)
            r0 = (l["intensity"].astype(np.float64) / cutoff * l["outer_radius"].astype(np.float64) ** 2) ** 0.25  # the attenuation's zero
            hit |= point & ((np.abs(dist / l["inner_radius"] - 1.0) < band) | (np.abs(dist / r0 - 1.0) < 2.0 ** -12))
            near[at] |= hit
    return near


def count(oracle):
    import fragments_shade_cases as cases
    from orbit_amd import raster

    f = host_frame(oracle)
    real = raster.host_fragments_shade(*f["args"])
    every = raster.host_fragments_shade(*all_lights_args(f["args"], len(f["lights"])))
    written = real["lights_walked"][f["frame"]["visibility"] != 0]
    result = dict(scene=f"tools/make_test_glb.py, {_tool('count_surface_fragments').INSTANCES} instances, seed 7; {N_LIGHTS} point lights on the surface",
                  width=f["width"], height=f["height"], tile_size_px=TILE, cluster_count=list(f["cluster_count"]), active_clusters=f["n_active"],
                  dropped=f["dropped"], **{k: int(real["stats"][k]) for k in COUNTERS}, mean_lights_walked=float(f"{written.mean():.4g}"),
                  max_lights_walked=int(written.max()), clustered_equals_all_lights=bool(real["color"].tobytes() == every["color"].tobytes()))
    worst, compared, differs, clamped = accuracy(oracle, f["args"])
    for c in cases.all_cases(oracle):
        a, kw = c.args()
        e, n, d, q = accuracy(oracle, a, kw)
        worst, compared, differs, clamped = max(worst, e), compared + n, differs + d, clamped + q
    result.update(max_relative_error=float(f"{worst:.4g}"), compared_pixels=compared, slice_differs=differs, near_clamp_pixels=clamped)
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fragments_shade_cpu.json"))
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
