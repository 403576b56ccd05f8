"""orbit_fragments_shade_shadowed on the glTF test scene, §4.25's protocol.  GPU box; prints one JSON line
and writes it to --out.  One process; per call the median of --iters event-timed launches after a warm-up, the first round
dropped; the outputs byte-equal to the host mirror in the same process (device_equals_host), or the exit code is 1.
The whole chain is made on the device as in tools/bench_fragments_shade.py (the 200-instance scene at 1920 x 1080, config
4's 10 000 point lights and 240 x 135 x 32 clusters) with one sun appended to the lights, whose four cascades come from
orbit_host_shadow_cascade and whose --resolution^2 maps orbit_raster_depth draws from every opaque meshlet into one atlas.
  shadowed_us     the new call, the sun shadowed (library's choice of the form; colour, lights_walked, both stats, shadow_factor, cascade)
  shadowed_staged_us / shadowed_per_lane_us  the same, the form forced
  unshadowed_us   the new call on the same frame with the sun's shadow_data_index = 0xFFFFFFFF
  old_us          orbit_fragments_shade on that unshadowed frame: the yardstick (the new call may be at most 5 % slower)
  cascades_us     the four orbit_raster_depth calls that draw the atlas
floor_us: §4.25's 40 B read + 16 B written per pixel plus the 8 B per pixel the two new planes take, at 8 TB/s; tap
traffic is cache traffic and is not in the floor.
Usage: python tools/bench_fragments_shade_shadowed.py [--instances 200] [--resolution 2048] [--iters 30]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--resolution", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fragments_shade_shadowed_mi355x.json"))
    args = ap.parse_args()
    import torch

    import config_scenes as cs
    import raster_scene as rs
    from oracle import oracle
    from orbit_amd import raster
    from orbit_amd import layouts as L
    from orbit_amd.engine import Engine

    timed = _tool("bench_visibility_surface")._timed
    count = _tool("count_surface_fragments")
    tool = _tool("count_fragments_shade_shadowed")
    oracle.build()
    oracle.lib()
    scene, (w, h), res = rs.glb_scene(args.instances), (args.width, args.height), args.resolution
    assert (w, h) == tuple(cs.SCREEN), "config 4's clusters are laid out for its screen"
    words, rows = len(scene.meshlet_data), count.scene_rows(scene)
    meshlets = np.ascontiguousarray(scene.meshlets).view(np.uint8).reshape(-1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    z = lambda n, dt=torch.int32: torch.zeros(max(int(n), 1), dtype=dt, device="cuda")  # noqa: E731
    cam = rs.camera(w, h)
    push, info, lights = cs.config4_inputs(oracle, cam)
    base = 2048
    q = np.asarray(tool.SUN_Q, np.float64)
    q = tuple(float(v) for v in q / np.linalg.norm(q))
    lights = np.concatenate([lights, tool.sun_light(base, q)])
    plain = lights.copy()
    plain["shadow_data_index"][-1] = 0xFFFFFFFF
    info = info.copy()
    info["global_light_count"] = len(lights)
    cc, tile = cs.CLUSTERS, 8
    clusters = cc[0] * cc[1] * cc[2]
    cap, lcap = cc[0] * cc[1] * max(4, cc[2]), clusters * 33
    cutoff = 0.25  # make_lights' default: outer_radius = sqrt(intensity / cutoff)
    d_data, d_vb, d_ent, d_rows, d_mlt = up(scene.meshlet_data), up(scene.vertices), up(scene.entities), up(rows), up(meshlets)
    d_lights, d_plain, d_materials = up(lights), up(plain), up(scene.materials)
    vis, depth, stats, fstats, sstats = z(w * h, torch.int64), z(w * h, torch.float32), z(8), z(8), z(4)
    surf = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))
    planes = dict(world_pos=z(4 * w * h, torch.float32), normal=z(3 * w * h, torch.float32), material=z(w * h))
    gm, gb, gimg = z(cc[0] * cc[1]), torch.zeros((clusters, 2), dtype=torch.int32, device="cuda"), torch.zeros((clusters, 2), dtype=torch.int32, device="cuda")
    gu, gl = z(16 + 4 * cap, torch.uint8), z(4 + 4 * lcap, torch.uint8)
    color, walked, factor, cascade = z(4 * w * h, torch.float32), z(w * h), z(w * h, torch.float32), z(w * h)
    atlas = torch.zeros((4, res, res), dtype=torch.float32, device="cuda")
    eng = Engine(0, max_entities=4096, max_dispatches=1024, max_draws=1024, max_lights=12_000, max_clusters=clusters)
    floor_us = round(w * h * 64 / 8e12 * 1e6, 1)
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    n = int(draw[:4].view(np.uint32)[0])
    d_draw, vp = up(draw[:4 + 28 * n]), rs.view_proj(cam)
    casters = scene.all_commands(oracle, cam)
    n_casters = (casters.nbytes - 4) // 28
    d_casters = up(casters)
    geometry = (d_vb, len(scene.vertices), d_ent, scene.entity_count, vp)
    view_pos = tuple(float(v) for v in np.linalg.inv(cam.view.astype(np.float64))[:3, 3])
    zs, zb = float(push["z_scale"]), float(push["z_bias"])
    cascades = tool.cascades_of(cam, q, res, view_pos, w / h)
    matrices = [m for m, _ in cascades]
    shadow_rows = raster.shadow_rows(matrices, [s for _, s in cascades])
    d_shadow = up(shadow_rows)
    s = tool.SETTINGS
    cascades_call = lambda: raster.shadow_atlas(eng, atlas, d_casters, n_casters, d_data, d_vb, len(scene.vertices), d_ent, scene.entity_count,  # noqa: E731
                                                matrices, res, cull_none=True, meshlet_data_words=words, clip_near=True, wide_guard=True)
    cascades_call()
    eng.raster_visibility(d_draw, n, d_data, *geometry, vis, w, h, clear=True, meshlet_data_words=words, clip_near=True, wide_guard=True)
    eng.visibility_resolve(vis, w, h, depth=depth)
    eng.compute_clusters(push, info, depth, d_lights, gm, gb, gu, cap, gl, lcap, gimg)
    eng.visibility_surface_drawn(vis, w, h, d_draw, n, d_data, *geometry, **surf, clear=True, meshlet_data_words=words, clip_near=True,
                                 wide_guard=True)
    eng.surface_fragments(vis, w, h, d_draw, n, d_mlt, len(meshlets) // 32, surf["bary"], surf["triangle"], d_rows, len(scene.vertices), d_ent,
                          scene.entity_count, **planes, stats=fstats, clear=True)
    common = lambda lts: (vis, w, h, planes["world_pos"], planes["normal"], planes["material"], d_materials, len(scene.materials), lts, len(lights),  # noqa: E731
                          gimg, gl, lcap, cc, tile, zs, zb, cutoff, cam.z_near, view_pos, color)
    new = lambda lts, form=None: eng.fragments_shade_shadowed(  # noqa: E731
        *common(lts), d_shadow, 1, atlas, 4, res, s["blocker_search_radius"], s["normal_bias_scale"], s["oriented_bias"], shadow_index_base=base,
        shadow_factor=factor, cascade=cascade, shadow_stats=sstats, lights_walked=walked, stats=stats, clear=True, form=form)
    old = lambda: eng.fragments_shade(*common(d_plain), lights_walked=walked, stats=stats, clear=True)  # noqa: E731
    calls = dict(shadowed=lambda: new(d_lights), shadowed_staged=lambda: new(d_lights, "staged"), shadowed_per_lane=lambda: new(d_lights, "per_lane"),
                 unshadowed=lambda: new(d_plain), old=old, cascades=cascades_call)
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    eng.status()
    us = {}
    for _ in range(2):  # the first round also settles the clocks: its figures are dropped
        for name, fn in calls.items():
            us[name] = float(np.median(timed(torch, fn, args.iters)))
    h_vis = vis.cpu().numpy().view(np.uint64).reshape(h, w)
    h_planes = {k: v.cpu().numpy() for k, v in planes.items()}
    h_img, h_idx, h_atlas = gimg.cpu().numpy().view(np.uint32), gl.cpu().numpy(), atlas.cpu().numpy()
    host_args = (h_vis, h_planes["world_pos"], h_planes["normal"], h_planes["material"].view(np.uint32), scene.materials)
    rest = (h_img, h_idx, cc, tile, zs, zb, cutoff, cam.z_near, view_pos, shadow_rows, h_atlas, res, s["blocker_search_radius"],
            s["normal_bias_scale"], s["oriented_bias"])
    equal, want = {}, {}
    for name, lts, d_lts in (("shadowed", lights, d_lights), ("unshadowed", plain, d_plain)):
        want[name] = raster.host_fragments_shade_shadowed(*host_args, lts, *rest, shadow_index_base=base, index_capacity=lcap)
        for form in ("staged", "per_lane"):
            color.fill_(7.0)
            new(d_lts, form)
            torch.cuda.synchronize()
            eng.status()
            got = dict(color=color, lights_walked=walked, stats=stats, shadow_factor=factor, cascade=cascade, shadow_stats=sstats)
            equal[f"{name}_{form}"] = all(got[k].cpu().numpy().tobytes() == want[name][k].tobytes() for k in got)
    color.fill_(7.0)
    old()
    torch.cuda.synchronize()
    equal["old_equals_unshadowed"] = bool(color.cpu().numpy().tobytes() == want["unshadowed"]["color"].tobytes())
    sh, st = want["shadowed"]["shadow_stats"], want["shadowed"]["stats"]
    cas = want["shadowed"]["cascade"]
    ratio = us["unshadowed"] / us["old"]
    line = {"instances": args.instances, "width": w, "height": h, "iters": args.iters, "device": torch.cuda.get_device_name(0), "commands": n,
            "caster_commands": n_casters, "lights": len(lights), "cluster_count": list(cc), "tile_size_px": tile, "shadow_resolution": res,
            **{k: int(st[k]) for k in L.SHADE_STATS.names}, **{k: int(sh[k]) for k in L.SHADOW_STATS.names},
            "pixels_per_cascade": {str(k): int((cas == k).sum()) for k in range(5)},
            **{f"{k}_us": round(v, 1) for k, v in us.items()}, "floor_us": floor_us,
            "floor": "40 B read + 16 B written per pixel (§4.25) + 8 B written per pixel for shadow_factor and cascade, at 8 TB/s; taps are cache traffic",
            "shadowed_over_floor": round(us["shadowed"] / floor_us, 1), "shadowed_over_old": round(us["shadowed"] / us["old"], 3),
            "unshadowed_over_old": round(ratio, 3), "within_5_percent_of_old": bool(ratio <= 1.05), "device_equals_host": equal,
            "not_measured": "where the time goes (no counters were collected); other scenes, sun directions, map resolutions and settings; "
                            "more than one shadowed light; regrouping of early-out and filtering lanes"}
    eng.close()
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if all(equal.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
