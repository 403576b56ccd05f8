"""orbit_fragments_shade on the glTF test scene, §4.24's protocol.  GPU box; prints one JSON line and
writes it to --out.  One process; per call the median of --iters event-timed launches after a warm-up, the first round
dropped; the outputs byte-equal to the host mirror in the same process (device_equals_host), or the exit code is 1.
The whole chain is made on the device: the buffer drawn with ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD from the
frustum-and-cone list of tests/raster_scene.camera's default position, resolved, the clusters of config 4 (8-px tiles, 240 x
135 x 32, tests/config_scenes.config4_inputs: make_lights' 10 000 point lights) computed from the resolved depth, surfaced,
turned into fragments with ORBIT_FRAGMENTS_CLEAR and shaded.
  staged_us / per_lane_us  orbit_fragments_shade, render_mode 0, colour, lights_walked and stats, the form forced
  default_us               the same, the library's choice
  heat_us                  render_mode 8, the library's choice
  fragments_us             orbit_surface_fragments (world_pos, normal, material) on the same frame
  clusters_us              orbit_compute_clusters on the same frame
floor_us: 40 B read + 16 B written per pixel at 8 TB/s.  decision: the rule of §4.25 (the lower median is the default).
Usage: python tools/bench_fragments_shade.py [--instances 200] [--width 1920] [--height 1080] [--iters 30]
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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fragments_shade_mi355x.json"))
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
    oracle.build()
    oracle.lib()
    scene, (w, h) = rs.glb_scene(args.instances), (args.width, args.height)
    assert (w, h) == tuple(cs.SCREEN), "config 4's clusters are laid out for its screen"
    words, rows = len(scene.meshlet_data), count.scene_rows(scene)
    meshlets = np.ascontiguousarray(scene.meshlets).view(np.uint8).reshape(-1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    z = lambda n, dt=torch.int32: torch.zeros(max(int(n), 1), dtype=dt, device="cuda")  # noqa: E731
    cam = rs.camera(w, h)
    push, info, lights = cs.config4_inputs(oracle, cam)
    cc, tile = cs.CLUSTERS, 8
    clusters = cc[0] * cc[1] * cc[2]
    cap, lcap = cc[0] * cc[1] * max(4, cc[2]), clusters * 32
    cutoff = 0.25  # make_lights' default: outer_radius = sqrt(intensity / cutoff)
    d_data, d_vb, d_ent, d_rows, d_mlt = up(scene.meshlet_data), up(scene.vertices), up(scene.entities), up(rows), up(meshlets)
    d_lights, d_materials = up(lights), up(scene.materials)
    vis, depth, stats, fstats = z(w * h, torch.int64), z(w * h, torch.float32), z(8), z(8)
    surf = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))
    planes = dict(world_pos=z(4 * w * h, torch.float32), normal=z(3 * w * h, torch.float32), material=z(w * h))
    gm, gb, gimg = z(cc[0] * cc[1]), torch.zeros((clusters, 2), dtype=torch.int32, device="cuda"), torch.zeros((clusters, 2), dtype=torch.int32, device="cuda")
    gu, gl = z(16 + 4 * cap, torch.uint8), z(4 + 4 * lcap, torch.uint8)
    color, walked = z(4 * w * h, torch.float32), z(w * h)
    eng = Engine(0, max_entities=4096, max_dispatches=1024, max_draws=1024, max_lights=12_000, max_clusters=clusters)
    floor_us = round(w * h * 56 / 8e12 * 1e6, 1)
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    n = int(draw[:4].view(np.uint32)[0])
    d_draw, vp = up(draw[:4 + 28 * n]), rs.view_proj(cam)
    geometry = (d_vb, len(scene.vertices), d_ent, scene.entity_count, vp)
    view_pos = tuple(float(v) for v in np.linalg.inv(cam.view.astype(np.float64))[:3, 3])
    zs, zb = float(push["z_scale"]), float(push["z_bias"])
    eng.raster_visibility(d_draw, n, d_data, *geometry, vis, w, h, clear=True, meshlet_data_words=words, clip_near=True, wide_guard=True)
    eng.visibility_resolve(vis, w, h, depth=depth)
    clusters_call = lambda: eng.compute_clusters(push, info, depth, d_lights, gm, gb, gu, cap, gl, lcap, gimg)  # noqa: E731
    clusters_call()
    eng.visibility_surface_drawn(vis, w, h, d_draw, n, d_data, *geometry, **surf, clear=True, meshlet_data_words=words, clip_near=True,
                                 wide_guard=True)
    fragments_call = lambda: eng.surface_fragments(vis, w, h, d_draw, n, d_mlt, len(meshlets) // 32, surf["bary"], surf["triangle"], d_rows,  # noqa: E731
                                                   len(scene.vertices), d_ent, scene.entity_count, **planes, stats=fstats, clear=True)
    fragments_call()
    shade = lambda form=None, mode=0: eng.fragments_shade(  # noqa: E731
        vis, w, h, planes["world_pos"], planes["normal"], planes["material"], d_materials, len(scene.materials), d_lights, len(lights), gimg, gl,
        lcap, cc, tile, zs, zb, cutoff, cam.z_near, view_pos, color, lights_walked=walked, stats=stats, render_mode=mode, clear=True, form=form)
    calls = dict(staged=lambda: shade("staged"), per_lane=lambda: shade("per_lane"), default=shade, heat=lambda: shade(None, 8),
                 fragments=fragments_call, clusters=clusters_call)
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
    h_img, h_idx = gimg.cpu().numpy().view(np.uint32), gl.cpu().numpy()
    want = raster.host_fragments_shade(h_vis, h_planes["world_pos"], h_planes["normal"], h_planes["material"].view(np.uint32), scene.materials, lights,
                                       h_img, h_idx, cc, tile, zs, zb, cutoff, cam.z_near, view_pos, index_capacity=lcap)
    same, equal = True, {}
    for form in ("staged", "per_lane"):
        color.fill_(7.0)
        shade(form)
        torch.cuda.synchronize()
        eng.status()
        equal[form] = bool(color.cpu().numpy().tobytes() == want["color"].tobytes() and walked.cpu().numpy().tobytes() == want["lights_walked"].tobytes()
                           and stats.cpu().numpy().tobytes() == want["stats"].tobytes())
        same = same and equal[form]
    lit = want["lights_walked"][h_vis != 0]
    line = {"instances": args.instances, "width": w, "height": h, "iters": args.iters, "device": torch.cuda.get_device_name(0), "commands": n,
            "lights": len(lights), "cluster_count": list(cc), "tile_size_px": tile, **{k: int(want["stats"][k]) for k in L.SHADE_STATS.names},
            "mean_lights_walked": round(float(lit.mean()), 2), "max_lights_walked": int(lit.max()),
            **{f"{k}_us": round(v, 1) for k, v in us.items()}, "floor_us": floor_us, "floor": "40 B read + 16 B written per pixel at 8 TB/s",
            "staged_over_floor": round(us["staged"] / floor_us, 1), "per_lane_over_floor": round(us["per_lane"] / floor_us, 1),
            "device_equals_host": equal,
            "decision": ("staged" if us["staged"] <= us["per_lane"] else "per_lane") + " has the lower median on this frame: the default of eligible grids",
            "not_measured": "where the time goes (no counters were collected); other scenes, tile sizes and light densities; lists longer "
                            "than this frame's; whether the IEEE divides (13 per light) or the gathers bound the walk"}
    eng.close()
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
