"""orbit_visibility_compact on the glTF test scene.  GPU box; prints one JSON line and writes it to --out.

Scene: tests/raster_scene.glb_scene(instances) at width x height from its default camera; the draw list is the pass-0
list of the oracle's culls, as in tools/bench_raster_visibility.py, rasterised once into the visibility buffer that
every timed call then reads.
  resolve_us                        orbit_visibility_resolve of that buffer (command_pixels and stats): the yardstick —
                                    both read 8 B per pixel and aggregate per 8 x 8 tile
  compact_us, compact_triangles_us  orbit_visibility_compact without and with ORBIT_COMPACT_TRIANGLES
  compact_over_resolve, compact_triangles_over_resolve
  raster_in_us                      orbit_raster_visibility of the input list (CLEAR, stats)
  raster_out_us, raster_cut_us      the same call on the output list (original meshlet_data) and on the cut list
                                    (visible_data): what the feature buys
  raster_out_over_in, raster_cut_over_in
Every figure is the median of `iters` event-timed calls after warm-up.  device_equals_host: every output of both modes
against the host mirror on the same buffer, byte for byte, and C6 (a) of the two redrawn buffers.
The per-kernel split comes from the same program under a kernel trace (--iters 5 keeps the trace small).
Usage: python tools/bench_visibility_compact.py [--instances 200] [--width 1920] [--height 1080] [--iters 30]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_compact_mi355x.json"))
    args = ap.parse_args()
    import torch

    import raster_scene as rs
    from oracle import oracle
    from orbit_amd import raster
    from orbit_amd import layouts as L
    from orbit_amd.engine import Engine, visibility_compact_workspace

    oracle.build()
    oracle.lib()
    scene, (w, h) = rs.glb_scene(args.instances), (args.width, args.height)
    cam = rs.camera(w, h)
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    n, words = int(draw[:4].view(np.uint32)[0]), len(scene.meshlet_data)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    z = lambda count, dt=torch.int32: torch.zeros(max(int(count), 1), dtype=dt, device="cuda")  # noqa: E731
    d_draw, d_data, d_vb, d_ent = up(draw[:4 + 28 * n]), up(scene.meshlet_data), up(scene.vertices), up(scene.entities)
    vis, again, pixels, rstats, vstats = z(w * h, torch.int64), z(w * h, torch.int64), z(n), z(8), z(4)
    work = z(visibility_compact_workspace(n) // 8, torch.int64)
    outs = {t: dict(masks=z(8 * n), commands=z(1 + 7 * n), ids=z(n), data=z(words), stats=z(8)) for t in (False, True)}
    eng = Engine(0, max_entities=4096, max_dispatches=1024, max_draws=1024)
    geometry = (d_vb, len(scene.vertices), d_ent, scene.entity_count, rs.view_proj(cam))

    def compact(t):
        o = outs[t]
        eng.visibility_compact(vis, w, h, d_draw, n, o["masks"], o["commands"], n, work, meshlet_data=d_data, visible_ids=o["ids"],
                               visible_data=o["data"] if t else None, visible_data_words=words if t else 0, stats=o["stats"],
                               triangles=t)

    def redraw(t, target=again):
        eng.raster_visibility(outs[t]["commands"], n, outs[t]["data"] if t else d_data, *geometry, target, w, h, clear=True,
                              stats=rstats, meshlet_data_words=words)

    calls = dict(
        resolve=lambda: eng.visibility_resolve(vis, w, h, 0, n, command_pixels=pixels, stats=vstats),
        compact=lambda: compact(False), compact_triangles=lambda: compact(True),
        raster_out=lambda: redraw(False), raster_cut=lambda: redraw(True),
        # last: it rewrites `vis` (with the same words)
        raster_in=lambda: eng.raster_visibility(d_draw, n, d_data, *geometry, vis, w, h, clear=True, stats=rstats,
                                                meshlet_data_words=words))
    calls["raster_in"]()
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
    same, counts = True, {}
    for t in (False, True):
        for o in outs[t].values():
            o.fill_(0)
        compact(t)
        redraw(t)
        torch.cuda.synchronize()
        eng.status()
        want = raster.host_visibility_compact(h_vis, draw, n, 0, scene.meshlet_data, t)
        got = {k: v.cpu().numpy().view(np.uint32) for k, v in outs[t].items()}
        same = same and all(got[k].tobytes() == want[k].tobytes() for k in ("masks", "commands", "ids"))
        same = same and got["stats"].tobytes() == want["stats"].tobytes() and (not t or got["data"].tobytes() == want["data"].tobytes())
        same = same and (again.cpu().numpy().view(np.uint64).reshape(h, w) >> np.uint64(32) == h_vis >> np.uint64(32)).all()
        counts = {k: int(want["stats"][k]) for k in L.VIS_COMPACT_STATS.names}
    eng.close()
    line = {"instances": args.instances, "width": w, "height": h, "iters": args.iters, "device": torch.cuda.get_device_name(0),
            "commands": n, "triangles_in": int((draw[4:4 + 28 * n].view(np.uint32).reshape(n, 7)[:, 0] // 3).sum()),
            "input_meshlet_words": words, **counts,
            **{f"{k}_us": round(v, 1) for k, v in us.items()},
            "compact_over_resolve": round(us["compact"] / us["resolve"], 2),
            "compact_triangles_over_resolve": round(us["compact_triangles"] / us["resolve"], 2),
            "raster_out_over_in": round(us["raster_out"] / us["raster_in"], 3),
            "raster_cut_over_in": round(us["raster_cut"] / us["raster_in"], 3),
            "device_equals_host": bool(same)}
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
