"""orbit_ssao on the glTF test scene's depth plane, §4.25's protocol.  GPU box; prints one JSON line and
writes it to --out.  One process; per call the median, the smallest and the largest of --iters event-timed calls after a
warm-up, the first round dropped; the outputs byte-equal to the host mirror in the same process (device_equals_host), or the
exit code is 1.
The frame is §4.26's, made on the device as in tools/bench_post_chain.py: the 200-instance scene at 1920 x 1080, its depth
from orbit_raster_visibility and orbit_visibility_resolve; SsaoSettings::default (32 samples, radii 0.1 / 0.5), the tables of
orbit_amd.post.ssao_tables(1); at half resolution (the reference's default) and at full resolution.
  ssao_*_us            the whole call: the clearing launch, the SSAO launch, the blur and the fragment read
  raw_*_us             the call with raw alone (the clearing and the SSAO launch); raw_blurred_*_us: with the blur
  blur_*_us, read_*_us the blur and the fragment read BY DIFFERENCE of those medians, to the microsecond: the call gives no way
                       to run them alone, and the differences lie inside the calls' own spread
  shade_us             orbit_fragments_shade_shadowed on the same frame, for scale
floor: the bytes the rules force, at 8 TB/s: 4 B of depth per screen pixel once, 1 B written per SSAO pixel, 16 B read and 1 B
written per SSAO pixel for the blur, 4 B written per screen pixel for ao_pixel.  Depth taps are cache traffic and are not in
the floor.
Usage: python tools/bench_ssao.py [--instances 200] [--iters 30]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
TABLE_SEED = 1


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def floor_us(screen_pixels, ssao_pixels, bandwidth=8e12):
    """the streaming floor of the whole call in µs, from the bytes the rules force"""
    return (4 * screen_pixels + ssao_pixels + 17 * ssao_pixels + 4 * screen_pixels) / bandwidth * 1e6


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--resolution", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssao_mi355x.json"))
    args = ap.parse_args()
    import torch

    import config_scenes as cs
    import raster_scene as rs
    from oracle import oracle
    import scenes as sc
    from orbit_amd import passes, post, raster
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
    proj = sc.mat4_cols(cam.proj)
    inv = passes.mat4_inverse(proj)
    noise, samples = post.ssao_tables(TABLE_SEED)
    d_noise, d_samples = up(noise), up(samples)
    d = post.SSAO_DEFAULTS
    settings = dict(sample_count=d["sample_count"], min_radius=d["min_radius"], max_radius=d["max_radius"])
    sizes = dict(half=post.ssao_resolution(w, h, False), full=post.ssao_resolution(w, h, True))
    bufs = {k: dict(raw=z(sw * sh, torch.uint8), blurred=z(sw * sh, torch.uint8)) for k, (sw, sh) in sizes.items()}
    ao, stats = z(w * h, torch.float32), z(3, torch.int64)

    def call(k, *outputs):
        sw, sh = sizes[k]
        outs = dict(raw=bufs[k]["raw"], blurred=bufs[k]["blurred"] if "blurred" in outputs else None, ao_pixel=ao if "ao_pixel" in outputs else None)
        return lambda: eng.ssao(depth, w, h, sw, sh, proj, inv, d_noise, noise.shape[0], d_samples, samples.shape[0], stats=stats, **outs, **settings)

    calls = {}
    for k in sizes:
        calls[f"ssao_{k}"] = call(k, "blurred", "ao_pixel")
        calls[f"raw_{k}"] = call(k)
        calls[f"raw_blurred_{k}"] = call(k, "blurred")
    calls["shade"] = shade
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    eng.status()
    rounds = []
    for _ in range(3):  # the first round also settles the clocks: its figures are dropped
        rounds.append({name: timed(torch, fn, args.iters) for name, fn in calls.items()})
    kept = rounds[1:]
    us = {name: float(np.median(np.concatenate([r[name] for r in kept]))) for name in calls}
    spread = {name: [round(float(min(min(r[name]) for r in kept)), 1), round(float(max(max(r[name]) for r in kept)), 1)] for name in calls}
    per_round = {name: [round(float(np.median(r[name])), 1) for r in kept] for name in calls}
    h_depth = depth.cpu().numpy().reshape(h, w)
    equal, counters, floors = {}, {}, {}
    for k, (sw, sh) in sizes.items():
        want = post.host_ssao(h_depth, proj, inv, noise, samples, sw, sh, **settings)
        for t in (bufs[k]["raw"], bufs[k]["blurred"], ao, stats):
            t.fill_(7)
        calls[f"ssao_{k}"]()
        torch.cuda.synchronize()
        eng.status()
        equal[k] = bool(bufs[k]["raw"].cpu().numpy().tobytes() == want["raw"].tobytes() and bufs[k]["blurred"].cpu().numpy().tobytes() == want["blurred"].tobytes()
                        and ao.cpu().numpy().tobytes() == want["ao_pixel"].tobytes() and stats.cpu().numpy().tobytes() == want["stats"].tobytes())
        counters[k] = {n: int(want["stats"][n]) for n in L.SSAO_STATS.names if n != "_pad"}
        counters[k]["mean_ao"] = round(float(want["ao_pixel"].mean()), 4)
        floors[k] = floor_us(w * h, sw * sh)
    line = {"instances": args.instances, "width": w, "height": h, "iters": args.iters, "device": torch.cuda.get_device_name(0), **settings,
            "covered_pixels": int((h_depth != 0).sum()), "ssao_sizes": {k: list(v) for k, v in sizes.items()}, "counters": counters,
            **{f"{k}_us": round(v, 1) for k, v in us.items()},
            **{f"blur_{k}_us": round(us[f"raw_blurred_{k}"] - us[f"raw_{k}"]) for k in sizes},
            **{f"read_{k}_us": round(us[f"ssao_{k}"] - us[f"raw_blurred_{k}"]) for k in sizes},
            "blur_and_read": "differences of the medians of the calls with and without them, to the microsecond: they are smaller than the "
                             "calls' own min-max spread, so they say that the two launches are small, not how long they take", "min_max_us": spread, "median_us_per_round": per_round,
            **{f"floor_{k}_us": round(v, 2) for k, v in floors.items()}, "floor": "the bytes the rules force at 8 TB/s; depth taps are cache traffic",
            **{f"ssao_{k}_over_floor": round(us[f"ssao_{k}"] / floors[k], 1) for k in sizes},
            **{f"ssao_{k}_over_shade": round(us[f"ssao_{k}"] / us["shade"], 3) for k in sizes}, "launches": "1 clearing + SSAO + blur + read",
            "device_equals_host": equal,
            "not_measured": "per-launch counters and a kernel trace (the blur and the read are timed by difference only); a form that stages a depth "
                            "window in LDS (a tap's reach depends on the pixel's depth: no tile bound without a pre-pass); other sample counts, radii and sizes"}
    eng.close()
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if all(equal.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
