"""orbit_visibility_surface_drawn on the glTF test scene, §4.21's protocol.  GPU box; prints one JSON line
and writes it to --out.  One process; per call the median of --iters event-timed launches after a warm-up, the first round
dropped; the outputs byte-equal to the host mirror in the same process (device_equals_host), or the exit code is 1.
Two buffers, both drawn on the device with ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD from the frustum-and-cone list:
  outside   tests/raster_scene.camera's default position: no cut and no wide triangle, every tile takes the fast path
  inside    tools/count_near_clip.py's second camera, inside the terrain mesh: a third of the pixels are a piece's
Per buffer (all three outputs and stats, no CLEAR):
  old_us     orbit_visibility_surface (the parent's kernels, unchanged): leaves the cut and wide pixels unsupported
  drawn_us   orbit_visibility_surface_drawn with both flags
  raster_us  orbit_raster_visibility of the same list with both flags and CLEAR
Usage: python tools/bench_surface_drawn.py [--instances 200] [--width 1920] [--height 1080] [--iters 30]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_drawn_mi355x.json"))
    args = ap.parse_args()
    import torch

    import raster_scene as rs
    from oracle import oracle
    from orbit_amd import raster
    from orbit_amd import layouts as L
    from orbit_amd.engine import Engine

    timed = _tool("bench_visibility_surface")._timed
    inside_position = _tool("count_near_clip").CAMERAS[1]
    oracle.build()
    oracle.lib()
    scene, (w, h) = rs.glb_scene(args.instances), (args.width, args.height)
    words = len(scene.meshlet_data)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    z = lambda count, dt=torch.int32: torch.zeros(max(int(count), 1), dtype=dt, device="cuda")  # noqa: E731
    d_data, d_vb, d_ent = up(scene.meshlet_data), up(scene.vertices), up(scene.entities)
    vis, rstats, sstats = z(w * h, torch.int64), z(8), z(8)
    outs = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))
    eng = Engine(0, max_entities=4096, max_dispatches=1024, max_draws=1024)
    line = {"instances": args.instances, "width": w, "height": h, "iters": args.iters, "device": torch.cuda.get_device_name(0)}
    same = True
    for where, cam in (("outside", rs.camera(w, h)), ("inside", rs.camera(w, h, inside_position))):
        _, _, draw, _, _ = scene.cull(oracle, cam, 0)
        n = int(draw[:4].view(np.uint32)[0])
        d_draw, vp = up(draw[:4 + 28 * n]), rs.view_proj(cam)
        geometry = (d_vb, len(scene.vertices), d_ent, scene.entity_count, vp)
        calls = dict(
            old=lambda: eng.visibility_surface(vis, w, h, d_draw, n, d_data, *geometry, **outs, stats=sstats, meshlet_data_words=words),
            drawn=lambda: eng.visibility_surface_drawn(vis, w, h, d_draw, n, d_data, *geometry, **outs, stats=sstats,
                                                       meshlet_data_words=words, clip_near=True, wide_guard=True),
            # last: it rewrites `vis` (with the same words)
            raster=lambda: eng.raster_visibility(d_draw, n, d_data, *geometry, vis, w, h, clear=True, stats=rstats,
                                                 meshlet_data_words=words, clip_near=True, wide_guard=True))
        calls["raster"]()
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
        for o in outs.values():
            o.zero_()
        eng.visibility_surface_drawn(vis, w, h, d_draw, n, d_data, *geometry, **outs, stats=sstats, clear=True, meshlet_data_words=words,
                                     clip_near=True, wide_guard=True)
        torch.cuda.synchronize()
        eng.status()
        want = raster.host_visibility_surface_drawn(h_vis, draw, n, scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities,
                                                    vp, clip_near=True, wide_guard=True)
        equal = all(outs[k].cpu().numpy().tobytes() == want[k].tobytes() for k in ("bary", "grad", "triangle"))
        equal = equal and sstats.cpu().numpy().tobytes() == want["stats"].tobytes()
        same = same and equal
        line[where] = dict(commands=n, **{k: int(want["stats"][k]) for k in L.SURFACE_DRAWN_STATS.names},
                           **{f"{k}_us": round(v, 1) for k, v in us.items()}, drawn_over_old=round(us["drawn"] / us["old"], 3),
                           drawn_over_raster=round(us["drawn"] / us["raster"], 3), device_equals_host=bool(equal))
    eng.close()
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
