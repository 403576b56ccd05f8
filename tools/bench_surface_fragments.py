"""orbit_surface_fragments on the glTF test scene, §4.21's protocol.  GPU box; prints one JSON line and
writes it to --out.  One process; per call the median of --iters event-timed launches after a warm-up, the first round
dropped; the outputs byte-equal to the host mirror in the same process (device_equals_host), or the exit code is 1.
Two buffers, both drawn on the device with ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD from the frustum-and-cone list
and surfaced on the device with both flags; the scene's positions as 32-B MeshVertex rows with seeded attributes:
  outside   tests/raster_scene.camera's default position
  inside    tools/count_near_clip.py's second camera, inside the terrain mesh: a third of the pixels are a piece's
Per buffer:
  all_us        orbit_surface_fragments, all six outputs and stats, no CLEAR
  all_clear_us  the same with ORBIT_FRAGMENTS_CLEAR
  pos_normal_us world_pos and normal only (no grad read)
  surface_us    orbit_visibility_surface on the same buffer (the decision rule's yardstick)
  drawn_us      orbit_visibility_surface_drawn with both flags on the same buffer
floor_us: 48 B read + 72 B written per pixel at 8 TB/s.  decision: the rule of §4.24 applied to the outside buffer.
Usage: python tools/bench_surface_fragments.py [--instances 200] [--width 1920] [--height 1080] [--iters 30]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_fragments_mi355x.json"))
    args = ap.parse_args()
    import torch

    import raster_scene as rs
    from oracle import oracle
    from orbit_amd import raster
    from orbit_amd import layouts as L
    from orbit_amd.engine import Engine

    timed = _tool("bench_visibility_surface")._timed
    count = _tool("count_surface_fragments")
    inside_position = _tool("count_near_clip").CAMERAS[1]
    oracle.build()
    oracle.lib()
    scene, (w, h) = rs.glb_scene(args.instances), (args.width, args.height)
    words, rows = len(scene.meshlet_data), count.scene_rows(scene)
    meshlets = np.ascontiguousarray(scene.meshlets).view(np.uint8).reshape(-1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    z = lambda n, dt=torch.int32: torch.zeros(max(int(n), 1), dtype=dt, device="cuda")  # noqa: E731
    d_data, d_vb, d_ent, d_rows, d_mlt = up(scene.meshlet_data), up(scene.vertices), up(scene.entities), up(rows), up(meshlets)
    vis, sstats, fstats = z(w * h, torch.int64), z(8), z(8)
    surf = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))
    scratch = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))  # the yardsticks' outputs
    outs = {k: z(per * w * h, torch.int32 if k == "material" else torch.float32) for k, per, _ in raster.FRAGMENT_OUTPUTS}
    eng = Engine(0, max_entities=4096, max_dispatches=1024, max_draws=1024)
    floor_us = round(w * h * 120 / 8e12 * 1e6, 1)
    line = {"instances": args.instances, "width": w, "height": h, "iters": args.iters, "device": torch.cuda.get_device_name(0),
            "floor_us": floor_us, "floor": "48 B read + 72 B written per pixel at 8 TB/s"}
    same = True
    for where, cam in (("outside", rs.camera(w, h)), ("inside", rs.camera(w, h, inside_position))):
        _, _, draw, _, _ = scene.cull(oracle, cam, 0)
        n = int(draw[:4].view(np.uint32)[0])
        d_draw, vp = up(draw[:4 + 28 * n]), rs.view_proj(cam)
        geometry = (d_vb, len(scene.vertices), d_ent, scene.entity_count, vp)
        eng.raster_visibility(d_draw, n, d_data, *geometry, vis, w, h, clear=True, meshlet_data_words=words, clip_near=True, wide_guard=True)
        eng.visibility_surface_drawn(vis, w, h, d_draw, n, d_data, *geometry, **surf, stats=sstats, clear=True, meshlet_data_words=words,
                                     clip_near=True, wide_guard=True)
        frag = lambda clear=False, **o: eng.surface_fragments(vis, w, h, d_draw, n, d_mlt, len(meshlets) // 32, surf["bary"], surf["triangle"],  # noqa: E731
                                                               d_rows, len(scene.vertices), d_ent, scene.entity_count, stats=fstats, clear=clear, **o)
        calls = dict(
            all=lambda: frag(grad=surf["grad"], **outs),
            all_clear=lambda: frag(clear=True, grad=surf["grad"], **outs),
            pos_normal=lambda: frag(world_pos=outs["world_pos"], normal=outs["normal"]),
            surface=lambda: eng.visibility_surface(vis, w, h, d_draw, n, d_data, *geometry, **scratch, stats=sstats, meshlet_data_words=words),
            drawn=lambda: eng.visibility_surface_drawn(vis, w, h, d_draw, n, d_data, *geometry, **scratch, stats=sstats,
                                                       meshlet_data_words=words, clip_near=True, wide_guard=True))
        for _ in range(3):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        eng.status()
        us = {}
        for _ in range(2):  # the first round also settles the clocks: its figures are dropped
            for name, fn in calls.items():
                us[name] = float(np.median(timed(torch, fn, args.iters)))
        for o in outs.values():
            o.zero_()
        calls["all_clear"]()
        torch.cuda.synchronize()
        eng.status()
        h_vis = vis.cpu().numpy().view(np.uint64).reshape(h, w)
        h_surf = {k: v.cpu().numpy() for k, v in surf.items()}
        want = raster.host_surface_fragments(h_vis, draw, n, meshlets, h_surf, rows, len(scene.vertices), scene.entities,
                                             entity_count=scene.entity_count)
        equal = all(outs[k].cpu().numpy().tobytes() == want[k].tobytes() for k in outs)
        equal = equal and fstats.cpu().numpy().tobytes() == want["stats"].tobytes()
        same = same and equal
        line[where] = dict(commands=n, **{k: int(want["stats"][k]) for k in L.SURFACE_FRAGMENT_STATS.names[:6]},
                           **{f"{k}_us": round(v, 1) for k, v in us.items()}, all_over_surface=round(us["all"] / us["surface"], 3),
                           all_over_floor=round(us["all"] / floor_us, 2), device_equals_host=bool(equal))
    slower = line["outside"]["all_us"] > line["outside"]["surface_us"]
    line["decision"] = ("slower than orbit_visibility_surface: the dedupe variant is due" if slower
                        else "not slower than orbit_visibility_surface: a lane keeps its own vertex stage, the dedupe variant is out of scope")
    eng.close()
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
