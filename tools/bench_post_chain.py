"""orbit_bloom and orbit_post_process on the glTF test scene's shaded frame, §4.25's protocol.  GPU box;
prints one JSON line and writes it to --out.  One process; per call the median, the smallest and the largest of --iters
event-timed calls after a warm-up, the first round dropped; the outputs byte-equal to the host mirrors in the same process
(device_equals_host), or the exit code is 1.
The frame is made on the device as in tools/bench_fragments_shade_shadowed.py: the 200-instance scene at 1920 x 1080,
config 4's 10 000 point lights and one sun with four cascades, shaded by orbit_fragments_shade_shadowed.
  bloom_us / bloom_direct_us   orbit_bloom, its one launch form (LDS staging as the launch decides; every tap from global
                       memory), alternating, twice each; BloomSettings::default
  post_us / post_ldr_us        orbit_post_process with bloom into rgba8 alone; into rgba8 and ldr
  shade_us             orbit_fragments_shade_shadowed on the same frame, for scale
floors: the bytes the rules force, at 8 TB/s.  Bloom: level 0 reads 16 B and writes 4 B per pixel; a lower level reads 4 B
per source texel and writes 4 B per texel; an upsample reads 4 B per source texel and reads and writes 4 B per destination
texel.  Post process: 16 + 4 B in, 4 (+ 16) B out per pixel.  Tap traffic is cache and LDS traffic and is not in the floor.
Usage: python tools/bench_post_chain.py [--instances 200] [--resolution 2048] [--iters 30]
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


def floors_us(layout, bandwidth=8e12):
    """-> (bloom floor, post floor into rgba8, post floor into rgba8 and ldr) in µs, from the bytes the rules force"""
    sizes = [w * h for w, h in layout["sizes"]]
    down = sizes[0] * 20 + sum(4 * sizes[k - 1] + 4 * sizes[k] for k in range(1, len(sizes)))
    up = sum(4 * sizes[k] + 8 * sizes[k - 1] for k in range(1, len(sizes)))
    return (down + up) / bandwidth * 1e6, sizes[0] * 24 / bandwidth * 1e6, sizes[0] * 40 / bandwidth * 1e6


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--resolution", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_chain_mi355x.json"))
    args = ap.parse_args()
    import torch

    import config_scenes as cs
    import raster_scene as rs
    from oracle import oracle
    from orbit_amd import post, raster
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
    info = info.copy()
    info["global_light_count"] = len(lights)
    cc, tile = cs.CLUSTERS, 8
    clusters = cc[0] * cc[1] * cc[2]
    cap, lcap = cc[0] * cc[1] * max(4, cc[2]), clusters * 33
    cutoff = 0.25
    d_data, d_vb, d_ent, d_rows, d_mlt = up(scene.meshlet_data), up(scene.vertices), up(scene.entities), up(rows), up(meshlets)
    d_lights, d_materials = up(lights), up(scene.materials)
    vis, depth = z(w * h, torch.int64), z(w * h, torch.float32)
    surf = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))
    planes = dict(world_pos=z(4 * w * h, torch.float32), normal=z(3 * w * h, torch.float32), material=z(w * h))
    gm, gb, gimg = z(cc[0] * cc[1]), torch.zeros((clusters, 2), dtype=torch.int32, device="cuda"), torch.zeros((clusters, 2), dtype=torch.int32, device="cuda")
    gu, gl = z(16 + 4 * cap, torch.uint8), z(4 + 4 * lcap, torch.uint8)
    color = z(4 * w * h, torch.float32)
    atlas = torch.zeros((4, res, res), dtype=torch.float32, device="cuda")
    eng = Engine(0, max_entities=4096, max_dispatches=1024, max_draws=1024, max_lights=12_000, max_clusters=clusters)
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
    d_shadow = up(raster.shadow_rows(matrices, [s for _, s in cascades]))
    s = tool.SETTINGS
    raster.shadow_atlas(eng, atlas, d_casters, n_casters, d_data, d_vb, len(scene.vertices), d_ent, scene.entity_count, matrices, res, cull_none=True,
                        meshlet_data_words=words, clip_near=True, wide_guard=True)
    eng.raster_visibility(d_draw, n, d_data, *geometry, vis, w, h, clear=True, meshlet_data_words=words, clip_near=True, wide_guard=True)
    eng.visibility_resolve(vis, w, h, depth=depth)
    eng.compute_clusters(push, info, depth, d_lights, gm, gb, gu, cap, gl, lcap, gimg)
    eng.visibility_surface_drawn(vis, w, h, d_draw, n, d_data, *geometry, **surf, clear=True, meshlet_data_words=words, clip_near=True, wide_guard=True)
    eng.surface_fragments(vis, w, h, d_draw, n, d_mlt, len(meshlets) // 32, surf["bary"], surf["triangle"], d_rows, len(scene.vertices), d_ent,
                          scene.entity_count, **planes, clear=True)
    shade = lambda: eng.fragments_shade_shadowed(  # noqa: E731
        vis, w, h, planes["world_pos"], planes["normal"], planes["material"], d_materials, len(scene.materials), d_lights, len(lights), gimg, gl, lcap,
        cc, tile, zs, zb, cutoff, cam.z_near, view_pos, color, d_shadow, 1, atlas, 4, res, s["blocker_search_radius"], s["normal_bias_scale"],
        s["oriented_bias"], shadow_index_base=base, clear=True)
    shade()
    torch.cuda.synchronize()
    eng.status()
    lay = post.bloom_layout(w, h)
    mips, ldr, rgba8 = z(lay["total_texels"]), z(4 * w * h, torch.float32), z(4 * w * h, torch.uint8)
    bstats, pstats = z(4), z(4)
    calls = dict(bloom=lambda: eng.bloom(color, w, h, mips, stats=bstats), bloom_direct=lambda: eng.bloom(color, w, h, mips, stats=bstats, form="direct"),
                 post=lambda: eng.post_process(color, w, h, bloom=mips, rgba8=rgba8, stats=pstats),
                 post_ldr=lambda: eng.post_process(color, w, h, bloom=mips, ldr=ldr, rgba8=rgba8, stats=pstats), shade=shade)
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    eng.status()
    rounds = []
    for _ in range(3):  # the first round also settles the clocks: its figures are dropped; the forms alternate in the other two
        rounds.append({name: timed(torch, fn, args.iters) for name, fn in calls.items()})
    kept = rounds[1:]
    us = {name: float(np.median(np.concatenate([r[name] for r in kept]))) for name in calls}
    spread = {name: [round(float(min(min(r[name]) for r in kept)), 1), round(float(max(max(r[name]) for r in kept)), 1)] for name in calls}
    per_round = {name: [round(float(np.median(r[name])), 1) for r in kept] for name in calls}
    h_color = color.cpu().numpy().reshape(h, w, 4)
    want_b = post.host_bloom(h_color)
    want_p = post.host_post_process(h_color, want_b["mips"])
    equal = {}
    for form in (None, "direct"):
        mips.fill_(7)
        eng.bloom(color, w, h, mips, stats=bstats, form=form)
        torch.cuda.synchronize()
        equal[f"bloom_{form or 'default'}"] = bool(mips.cpu().numpy().tobytes() == want_b["mips"].tobytes() and bstats.cpu().numpy().tobytes() == want_b["stats"].tobytes())
    calls["post_ldr"]()
    torch.cuda.synchronize()
    eng.status()
    equal["post_process"] = bool(ldr.cpu().numpy().tobytes() == want_p["ldr"].tobytes() and rgba8.cpu().numpy().tobytes() == want_p["rgba8"].tobytes()
                                 and pstats.cpu().numpy().tobytes() == want_p["stats"].tobytes())
    f_bloom, f_post, f_post_ldr = floors_us(lay)
    line = {"instances": args.instances, "width": w, "height": h, "iters": args.iters, "device": torch.cuda.get_device_name(0), "lights": len(lights),
            "levels": lay["levels"], "total_texels": lay["total_texels"], **{k: int(want_b["stats"][k]) for k in L.BLOOM_STATS.names},
            **{k: int(want_p["stats"][k]) for k in ("pixels", "nonfinite_pixels", "bloom_pixels")},
            **{f"{k}_us": round(v, 1) for k, v in us.items()}, "min_max_us": spread, "median_us_per_round": per_round,
            "bloom_floor_us": round(f_bloom, 2), "post_floor_us": round(f_post, 2), "post_ldr_floor_us": round(f_post_ldr, 2),
            "floor": "the bytes the rules force at 8 TB/s; taps are cache and LDS traffic",
            "bloom_over_floor": round(us["bloom"] / f_bloom, 1), "post_over_floor": round(us["post"] / f_post, 1),
            "post_ldr_over_floor": round(us["post_ldr"] / f_post_ldr, 1), "bloom_over_shade": round(us["bloom"] / us["shade"], 3),
            "post_over_shade": round(us["post"] / us["shade"], 3), "launch_form": "per level: 1 + 2 * levels - 1 launches; no fused form is built",
            "device_equals_host": equal,
            "not_measured": "where the time goes per level (no kernel trace or counters were collected); other sizes, settings and radii; a fused launch form"}
    eng.close()
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if all(equal.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
