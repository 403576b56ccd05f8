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

--libs PATH [PATH ...] is the A/B of builds of the library (as tools/ab_libs.py; its docstring has the recipe for
tools/variants/): one engine per path, in the order given, on the same buffers; each call is timed through every engine
in turn, --rounds times, and every engine's results are checked against the host mirror.  The line's figures are then
the first library's, and "libs" holds {lib, depth_us, visibility_us, resolve_us, device_equals_host} of each.  Run it
with a byte copy of one library as a control and in both orders: the first engine of a process can be slower whatever
its code (profiles/r02_notes.md).
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
    ap.add_argument("--libs", nargs="+", default=None, metavar="PATH", help="builds of the library to time in alternation")
    ap.add_argument("--rounds", type=int, default=1, help="timed rounds over the calls and engines, after one that is dropped")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_visibility_mi355x.json"))
    args = ap.parse_args()
    import torch

    import raster_scene as rs
    from oracle import oracle
    from orbit_amd import _lib, raster
    from orbit_amd import layouts as L
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
    libs = [None] if args.libs is None else [os.path.abspath(p) for p in args.libs]
    engs = [Engine(0, _library=None if p is None else _lib.load_variant(p), max_entities=4096, max_dispatches=1024,
                   max_draws=1024) for p in libs]
    job = (d_draw, n, d_data, d_vb, len(scene.vertices), d_ent, scene.entity_count, rs.view_proj(cam))
    calls = dict(
        depth=lambda eng: eng.raster_depth(*job, depth, w, h, clear=True, stats=stats[0]),
        visibility=lambda eng: eng.raster_visibility(*job, vis, w, h, clear=True, stats=stats[1]),
        resolve=lambda eng: eng.visibility_resolve(vis, w, h, 0, n, depth=rdepth, command_pixels=pixels, stats=rstats))

    for eng in engs:
        for _ in range(3):
            for fn in calls.values():
                fn(eng)
        torch.cuda.synchronize()
        eng.status()
    samples = [{name: [] for name in calls} for _ in engs]
    for r in range(1 + args.rounds):  # the first round also settles the clocks: its figures are dropped
        for name, fn in calls.items():
            for k, eng in enumerate(engs):
                t = _timed(torch, lambda: fn(eng), args.iters)
                if r:
                    samples[k][name] += t
    per_lib = [{name: float(np.median(t)) for name, t in s.items()} for s in samples]
    want_vis, want_stats, err = raster.host_raster_visibility(draw, n, scene.meshlet_data, scene.vertices, len(scene.vertices),
                                                              scene.entities, rs.view_proj(cam), w, h)
    want_depth, want_pixels, want_rstats = raster.host_visibility_resolve(want_vis, 0, n)
    for k, eng in enumerate(engs):  # every engine's own results: the outputs are spoilt first, each call clears its own
        for t in (depth, vis, rdepth, pixels, rstats, *stats):
            t.fill_(1)
        for fn in calls.values():
            fn(eng)
        torch.cuda.synchronize()
        eng.status()
        st = stats[1].cpu().numpy().view(L.RASTER_STATS)[0]
        per_lib[k]["same"] = bool(
            not err.any() and vis.cpu().numpy().view(np.uint64).tobytes() == want_vis.tobytes()
            and st.tobytes() == want_stats.tobytes() == stats[0].cpu().numpy().tobytes()
            and depth.cpu().numpy().tobytes() == want_depth.tobytes() == rdepth.cpu().numpy().tobytes()
            and pixels.cpu().numpy().view(np.uint32).tobytes() == want_pixels.tobytes()
            and rstats.cpu().numpy().tobytes() == want_rstats.tobytes())
        eng.close()
    us, same = per_lib[0], all(p["same"] for p in per_lib)
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
    if args.libs is not None:
        line["rounds"] = args.rounds
        line["libs"] = [{"lib": os.path.basename(p), "depth_us": round(u["depth"], 1), "visibility_us": round(u["visibility"], 1),
                         "resolve_us": round(u["resolve"], 1), "device_equals_host": u["same"]} for p, u in zip(libs, per_lib)]
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
