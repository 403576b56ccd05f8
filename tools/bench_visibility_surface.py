"""orbit_visibility_surface on the glTF test scene.  GPU box; prints one JSON line and writes it to --out.

Scene and protocol are tools/bench_visibility_compact.py's: tests/raster_scene.glb_scene(instances) at width x height from
its default camera, the pass-0 list of the oracle's culls rasterised once into the visibility buffer that every timed
call then reads; every figure is the median of `iters` event-timed calls after warm-up; one GPU process.
  surface_us          orbit_visibility_surface with all three outputs and stats, no CLEAR
  surface_clear_us    the same with ORBIT_SURFACE_CLEAR (the fill launch in front)
  surface_bary_us     bary alone
  resolve_us          orbit_visibility_resolve of the same buffer (command_pixels and stats): the same tile walk without the
                      work per triangle
  raster_us           orbit_raster_visibility of the same list (CLEAR, stats): what a consumer would pay to redraw with an
                      attribute sink of its own
  surface_over_resolve, surface_over_raster
  floor_us, surface_over_floor   streaming 48 B per pixel (8 read, 40 written) at 8 TB/s, and the distance to it
device_equals_host: every output and the counters against the host mirror on the device's own buffer, byte for byte.
The per-kernel split comes from the same program under a kernel trace (--iters 5 keeps the trace small).
Usage: python tools/bench_visibility_surface.py [--instances 200] [--width 1920] [--height 1080] [--iters 30]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _timed(torch, fn, iters):
    """Device times of `fn`'s work between two events, in µs (a sleep kernel keeps the stream busy while the host
    enqueues every (event, work, event) triple, so the pairs bracket the work and not the host's enqueue)."""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda._sleep(50_000_000)
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in evs]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_surface_mi355x.json"))
    args = ap.parse_args()
    import torch

    import raster_scene as rs
    from oracle import oracle
    from orbit_amd import raster
    from orbit_amd import layouts as L
    from orbit_amd.engine import Engine

    oracle.build()
    oracle.lib()
    scene, (w, h) = rs.glb_scene(args.instances), (args.width, args.height)
    cam = rs.camera(w, h)
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    n, words = int(draw[:4].view(np.uint32)[0]), len(scene.meshlet_data)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    z = lambda count, dt=torch.int32: torch.zeros(max(int(count), 1), dtype=dt, device="cuda")  # noqa: E731
    d_draw, d_data, d_vb, d_ent = up(draw[:4 + 28 * n]), up(scene.meshlet_data), up(scene.vertices), up(scene.entities)
    vis, pixels, rstats, vstats, sstats = z(w * h, torch.int64), z(n), z(8), z(4), z(8)
    outs = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))
    eng = Engine(0, max_entities=4096, max_dispatches=1024, max_draws=1024)
    vp = rs.view_proj(cam)
    geometry = (d_vb, len(scene.vertices), d_ent, scene.entity_count, vp)

    def surface(clear=False, **o):
        eng.visibility_surface(vis, w, h, d_draw, n, d_data, *geometry, **o, stats=sstats, clear=clear, meshlet_data_words=words)

    calls = dict(
        resolve=lambda: eng.visibility_resolve(vis, w, h, 0, n, command_pixels=pixels, stats=vstats),
        surface=lambda: surface(**outs), surface_clear=lambda: surface(True, **outs), surface_bary=lambda: surface(bary=outs["bary"]),
        # last: it rewrites `vis` (with the same words)
        raster=lambda: eng.raster_visibility(d_draw, n, d_data, *geometry, vis, w, h, clear=True, stats=rstats,
                                             meshlet_data_words=words))
    calls["raster"]()
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    eng.status()
    us = {}
    for r in range(2):  # the first round also settles the clocks: its figures are dropped
        for name, fn in calls.items():
            us[name] = float(np.median(_timed(torch, fn, args.iters)))
    # the results, against the host mirror on the device's own buffer
    h_vis = vis.cpu().numpy().view(np.uint64).reshape(h, w)
    surface(True, **outs)
    torch.cuda.synchronize()
    eng.status()
    want = raster.host_visibility_surface(h_vis, draw, n, scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, vp)
    same = all(outs[k].cpu().numpy().tobytes() == want[k].tobytes() for k in ("bary", "grad", "triangle"))
    same = same and sstats.cpu().numpy().tobytes() == want["stats"].tobytes()
    counts = {k: int(want["stats"][k]) for k in L.SURFACE_STATS.names if not k.startswith("_")}
    eng.close()
    floor_us = 48.0 * w * h / 8e12 * 1e6
    line = {"instances": args.instances, "width": w, "height": h, "iters": args.iters, "device": torch.cuda.get_device_name(0),
            "commands": n, **counts, **{f"{k}_us": round(v, 1) for k, v in us.items()},
            "surface_over_resolve": round(us["surface"] / us["resolve"], 2),
            "surface_over_raster": round(us["surface"] / us["raster"], 3),
            "floor_us": round(floor_us, 1), "surface_over_floor": round(us["surface"] / floor_us, 1),
            "device_equals_host": bool(same)}
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
