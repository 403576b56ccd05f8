"""orbit_raster_depth, orbit_raster_visibility and orbit_visibility_resolve on the glTF test scene.
GPU box; prints one JSON line and writes it to --out.

Scene: tests/raster_scene.glb_scene(instances) at width x height from its default camera; the draw list is the pass-0
list of the oracle's culls (200 instances at 1920 x 1080: 18 025 commands), uploaded once.  Each call clears its
target (ORBIT_RASTER_CLEAR) and counts into its stats, as the early pass of a frame does.
  depth_us, visibility_us, resolve_us   device time of one call, median of `iters` event-timed calls after warm-up
  visibility_over_depth                 the visibility call against its yardstick, the depth call on the same job
  resolve_stream_us, resolve_over_stream   8 B per pixel at the HBM peak of the project's roofline, and the resolve against it
  *_mfragments_s, *_mtriangles_s        the raster calls' rates by the stats they wrote
  device_equals_host                    the three results against the host mirror on the same buffers, byte for byte
Usage: python tools/bench_raster_visibility.py [--instances 200] [--width 1920] [--height 1080] [--iters 30]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK = 8.0e12


def _timed(torch, fn, iters):
    """Median device time of `fn`'s work between two events, in µs (a sleep kernel keeps the stream busy while the host
    enqueues every (event, work, event) triple, so the pairs bracket the work and not the host's enqueue)."""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda._sleep(50_000_000)
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) * 1e3 for a, b in evs]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_visibility_mi355x.json"))
    args = ap.parse_args()
    import torch

    import raster_scene as rs
    from oracle import oracle
    from orbit_amd import layouts as L
    from orbit_amd import raster
    from orbit_amd.engine import Engine

    oracle.build()
    oracle.lib()
    scene, (w, h) = rs.glb_scene(args.instances), (args.width, args.height)
    cam = rs.camera(w, h)
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    n = int(draw[:4].view(np.uint32)[0])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_draw, d_data, d_vb, d_ent = up(draw[:4 + 28 * n]), up(scene.meshlet_data), up(scene.vertices), up(scene.entities)
    depth = torch.zeros(w * h, dtype=torch.float32, device="cuda")
    vis = torch.zeros(w * h, dtype=torch.int64, device="cuda")
    rdepth = torch.zeros(w * h, dtype=torch.float32, device="cuda")
    pixels = torch.zeros(n, dtype=torch.int32, device="cuda")
    stats = [torch.zeros(32, dtype=torch.uint8, device="cuda") for _ in range(2)]
    rstats = torch.zeros(16, dtype=torch.uint8, device="cuda")
    eng = Engine(0, max_entities=4096, max_dispatches=1024, max_draws=1024)
    job = (d_draw, n, d_data, d_vb, len(scene.vertices), d_ent, scene.entity_count, rs.view_proj(cam))

    def run_depth():
        eng.raster_depth(*job, depth, w, h, clear=True, stats=stats[0])

    def run_visibility():
        eng.raster_visibility(*job, vis, w, h, clear=True, stats=stats[1])

    def run_resolve():
        eng.visibility_resolve(vis, w, h, 0, n, depth=rdepth, command_pixels=pixels, stats=rstats)

    for _ in range(3):
        run_depth()
        run_visibility()
        run_resolve()
    torch.cuda.synchronize()
    eng.status()
    us = {}
    for _ in range(2):  # twice round, the later figure of each: the first round also settles the clocks
        for name, fn in (("depth", run_depth), ("visibility", run_visibility), ("resolve", run_resolve)):
            us[name] = _timed(torch, fn, args.iters)
    eng.status()
    want_vis, want_stats, err = raster.host_raster_visibility(draw, n, scene.meshlet_data, scene.vertices, len(scene.vertices),
                                                              scene.entities, rs.view_proj(cam), w, h)
    want_depth, want_pixels, want_rstats = raster.host_visibility_resolve(want_vis, 0, n)
    st = stats[1].cpu().numpy().view(L.RASTER_STATS)[0]
    same = (not err.any() and vis.cpu().numpy().view(np.uint64).tobytes() == want_vis.tobytes()
            and st.tobytes() == want_stats.tobytes() == stats[0].cpu().numpy().tobytes()
            and depth.cpu().numpy().tobytes() == want_depth.tobytes() == rdepth.cpu().numpy().tobytes()
            and pixels.cpu().numpy().view(np.uint32).tobytes() == want_pixels.tobytes()
            and rstats.cpu().numpy().tobytes() == want_rstats.tobytes())
    stream_us = 8.0 * w * h / HBM_PEAK * 1e6
    line = {
        "instances": args.instances, "width": w, "height": h, "iters": args.iters, "device": torch.cuda.get_device_name(0),
        "commands": n, "triangles": int(st["triangles"]), "fragments": int(st["fragments"]),
        "covered_pixels": int(want_rstats["covered_pixels"]), "visible_commands": int(want_rstats["visible_commands"]),
        "depth_us": round(us["depth"], 1), "visibility_us": round(us["visibility"], 1), "resolve_us": round(us["resolve"], 1),
        "visibility_over_depth": round(us["visibility"] / us["depth"], 3),
        "resolve_stream_us": round(stream_us, 2), "resolve_over_stream": round(us["resolve"] / stream_us, 2),
        "depth_mfragments_s": round(int(st["fragments"]) / us["depth"], 1),
        "visibility_mfragments_s": round(int(st["fragments"]) / us["visibility"], 1),
        "depth_mtriangles_s": round(int(st["triangles"]) / us["depth"], 1),
        "visibility_mtriangles_s": round(int(st["triangles"]) / us["visibility"], 1),
        "device_equals_host": bool(same)}
    eng.close()
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
