"""What ORBIT_RASTER_CLIP_NEAR costs on the device.  GPU box; prints one JSON line and writes it to --out.

Scene: tests/raster_scene.glb_scene(instances) at width x height, the pass-0 draw list of the oracle's culls, uploaded
once.  Two cameras: the OUTSIDE camera of tools/bench_raster_visibility.py, where no triangle crosses the near plane
that the flag could draw — there the flagged call against the unflagged one is the cost of the flag itself (the other
kernel, its registers, its occupancy) —, and the INSIDE camera of tools/count_near_clip.py, flagged and unflagged.
Each call clears its target and counts into its stats.  The four (call, flag) pairs of a camera are timed in the same
process, alternating, `rounds` times after a round that is dropped; a figure is the median of the event-timed calls.
  outside / inside: {depth_us, depth_clip_us, visibility_us, visibility_clip_us, depth_clip_over_plain,
                     visibility_clip_over_plain, clip_skipped, clip_skipped_flagged, guard_skipped_flagged}
  device_equals_host    the flagged results of both cameras against the host mirror, byte for byte
--wide adds the pair with ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD to the alternation
(depth_wide_us, visibility_wide_us, *_wide_over_clip, guard_skipped_wide, fragments_wide), holds it to the host mirror
as well, counts on the host the wide triangles and pieces of the list and the 64 x 64 blocks and 8 x 8 tiles the device's
wide walk tests for them (wide_walk), and writes profiles/wide_guard_mi355x.json.
No target is fixed.  Usage: python tools/bench_near_clip.py [--wide] [--instances 200] [--width 1920] [--height 1080] [--iters 20]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _timed(torch, fn, iters):
    """Device times of `fn`'s work between two events, in µs (a sleep kernel keeps the stream busy while the host
    enqueues every (event, work, event) triple)."""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda._sleep(50_000_000)
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in evs]


def wide_walk_counts(host_args):
    """What the device's wide walk (raster_walk.h walk_wide) does for the list, counted on the host with the restatement
    tests/raster_wide_ref.py: the wide pieces that reach the walk, the 64 x 64 blocks and 8 x 8 tiles it tests with the
    rectangle test, the tiles it walks sample by sample, and the samples inside."""
    import raster_wide_ref as wref

    counts = dict(wide_pieces=0, walked_pieces=0, box_pixels=0, blocks_tested=0, tiles_tested=0, tiles_walked=0, inside_samples=0)
    width, height = host_args[7], host_args[8]

    def rect_out(tx, ty, x0, y0, x1, y1):
        for u, v in ((0, 1), (1, 2), (2, 0)):
            dx, dy = tx[v] - tx[u], ty[v] - ty[u]
            nb = 0 if (dy < 0 or (dy == 0 and dx > 0)) else 1
            x, y = (x0 if dy > 0 else x1), (y1 if dx > 0 else y0)
            if dx * (256 * y + 128 - ty[u]) - dy * (256 * x + 128 - tx[u]) - nb < 0:
                return True
        return False

    def draw_piece(piece, w_, h_, cull_none, vis, ident, extras, opts):
        kinds = [v[3] for v in piece]
        if wref.OUT in kinds or wref.WIDE not in kinds:
            return "no_coverage", 0
        counts["wide_pieces"] += 1
        verdict, tri = wref.oriented(piece, cull_none)
        if tri is None:
            return verdict, 0
        tx, ty, _, _ = tri
        x_lo, x_hi, y_lo, y_hi = wref.box_of(tx, ty, width, height)
        if x_lo > x_hi or y_lo > y_hi:
            return "no_coverage", 0
        counts["walked_pieces"] += 1
        counts["box_pixels"] += (x_hi - x_lo + 1) * (y_hi - y_lo + 1)
        for by in range(y_lo >> 6, (y_hi >> 6) + 1):
            for bx in range(x_lo >> 6, (x_hi >> 6) + 1):
                counts["blocks_tested"] += 1
                if rect_out(tx, ty, max(64 * bx, x_lo), max(64 * by, y_lo), min(64 * bx + 63, x_hi), min(64 * by + 63, y_hi)):
                    continue
                for t in range(64):
                    x0, y0 = 64 * bx + 8 * (t & 7), 64 * by + 8 * (t >> 3)
                    cx0, cy0, cx1, cy1 = max(x0, x_lo), max(y0, y_lo), min(x0 + 7, x_hi), min(y0 + 7, y_hi)
                    if cx0 > cx1 or cy0 > cy1:
                        continue
                    counts["tiles_tested"] += 1
                    counts["tiles_walked"] += not rect_out(tx, ty, cx0, cy0, cx1, cy1)
        counts["inside_samples"] += len(wref.covered_samples(tx, ty, (x_lo, x_hi, y_lo, y_hi))[0])
        return "no_coverage", 0

    wref.raster(*host_args, flags=wref.CLEAR | wref.CLIP_NEAR | wref.WIDE_GUARD, max_triangles=None, draw_piece=draw_piece)
    return counts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--wide", action="store_true", help="ORBIT_RASTER_WIDE_GUARD too; the default --out becomes wide_guard_mi355x.json")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "wide_guard_mi355x.json" if args.wide else "near_clip_mi355x.json")
    import torch

    import raster_scene as rs
    from oracle import oracle
    from orbit_amd import layouts as L
    from orbit_amd import raster
    from orbit_amd.engine import Engine

    spec = importlib.util.spec_from_file_location("count_near_clip", os.path.join(ROOT, "tools", "count_near_clip.py"))
    count_tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(count_tool)
    oracle.build()
    oracle.lib()
    scene, (w, h) = rs.glb_scene(args.instances), (args.width, args.height)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_data, d_vb, d_ent = up(scene.meshlet_data), up(scene.vertices), up(scene.entities)
    depth = torch.zeros(w * h, dtype=torch.float32, device="cuda")
    vis = torch.zeros(w * h, dtype=torch.int64, device="cuda")
    stats = torch.zeros(32, dtype=torch.uint8, device="cuda")
    eng = Engine(0, max_entities=4096, max_dispatches=1024, max_draws=1024)
    line = {"instances": args.instances, "width": w, "height": h, "iters": args.iters, "rounds": args.rounds,
            "device": torch.cuda.get_device_name(0)}
    same = True
    for name, cam in (("outside", rs.camera(w, h)), ("inside", rs.camera(w, h, count_tool.CAMERAS[1]))):
        _, _, draw, _, _ = scene.cull(oracle, cam, 0)
        n = int(draw[:4].view(np.uint32)[0])
        d_draw = up(draw[:4 + 28 * n])
        job = (d_draw, n, d_data, d_vb, len(scene.vertices), d_ent, scene.entity_count, rs.view_proj(cam))
        calls = {
            "depth": lambda: eng.raster_depth(*job, depth, w, h, clear=True, stats=stats),
            "depth_clip": lambda: eng.raster_depth(*job, depth, w, h, clear=True, stats=stats, clip_near=True),
            "visibility": lambda: eng.raster_visibility(*job, vis, w, h, clear=True, stats=stats),
            "visibility_clip": lambda: eng.raster_visibility(*job, vis, w, h, clear=True, stats=stats, clip_near=True)}
        if args.wide:
            calls["depth_wide"] = lambda: eng.raster_depth(*job, depth, w, h, clear=True, stats=stats, clip_near=True, wide_guard=True)
            calls["visibility_wide"] = lambda: eng.raster_visibility(*job, vis, w, h, clear=True, stats=stats, clip_near=True,
                                                                     wide_guard=True)
        for _ in range(3):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        eng.status()
        samples = {k: [] for k in calls}
        for r in range(1 + args.rounds):  # the first round also settles the clocks: its figures are dropped
            for k, fn in calls.items():
                t = _timed(torch, fn, args.iters)
                if r:
                    samples[k] += t
        us = {k: float(np.median(t)) for k, t in samples.items()}
        host_args = (draw, n, scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, rs.view_proj(cam), w, h)
        want_vis, want_stats, err = raster.host_raster_visibility(*host_args, clip_near=True)
        _, off_stats, _ = raster.host_raster_visibility(*host_args)
        depth.fill_(1), vis.fill_(1)
        calls["depth_clip"]()
        d_stats = stats.cpu().numpy().copy()
        calls["visibility_clip"]()
        torch.cuda.synchronize()
        eng.status()
        ok = bool(not err.any() and vis.cpu().numpy().view(np.uint64).tobytes() == want_vis.tobytes()
                  and stats.cpu().numpy().tobytes() == want_stats.tobytes() == d_stats.tobytes()
                  and depth.cpu().numpy().view(np.uint32).tobytes() == (want_vis >> np.uint64(32)).astype(np.uint32).tobytes())
        same = same and ok
        wide = {}
        if args.wide:
            wide_vis, wide_stats, werr = raster.host_raster_visibility(*host_args, clip_near=True, wide_guard=True)
            depth.fill_(1), vis.fill_(1)
            calls["depth_wide"]()
            d_stats = stats.cpu().numpy().copy()
            calls["visibility_wide"]()
            torch.cuda.synchronize()
            eng.status()
            wide_ok = bool(not werr.any() and vis.cpu().numpy().view(np.uint64).tobytes() == wide_vis.tobytes()
                           and stats.cpu().numpy().tobytes() == wide_stats.tobytes() == d_stats.tobytes()
                           and depth.cpu().numpy().view(np.uint32).tobytes() == (wide_vis >> np.uint64(32)).astype(np.uint32).tobytes())
            same = same and wide_ok
            wide = {"depth_wide_us": round(us["depth_wide"], 1), "visibility_wide_us": round(us["visibility_wide"], 1),
                    "depth_wide_over_clip": round(us["depth_wide"] / us["depth_clip"], 3),
                    "visibility_wide_over_clip": round(us["visibility_wide"] / us["visibility_clip"], 3),
                    "guard_skipped_wide": int(wide_stats["guard_skipped"]), "fragments_wide": int(wide_stats["fragments"]),
                    "wide_device_equals_host": wide_ok, "wide_walk": wide_walk_counts(host_args)}
        line[name] = {"commands": n, "triangles": int(want_stats["triangles"]),
                      **{f"{k}_us": round(v, 1) for k, v in us.items()},
                      "depth_clip_over_plain": round(us["depth_clip"] / us["depth"], 3),
                      "visibility_clip_over_plain": round(us["visibility_clip"] / us["visibility"], 3),
                      "clip_skipped": int(off_stats["clip_skipped"]), "clip_skipped_flagged": int(want_stats["clip_skipped"]),
                      "guard_skipped": int(off_stats["guard_skipped"]), "guard_skipped_flagged": int(want_stats["guard_skipped"]),
                      "fragments": int(off_stats["fragments"]), "fragments_flagged": int(want_stats["fragments"]),
                      "device_equals_host": ok, **wide}
    eng.close()
    line["device_equals_host"] = same
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
