"""orbit_fragments_shade_sky on the glTF test scene, §4.25's protocol.  GPU box; prints one JSON line and
writes it to --out.  One process; per call the median of --iters (20) event-timed launches after 3 warm-up calls, the first
round dropped; the new call's outputs byte-equal to the host mirror in the same process (device_equals_host), or the exit
code is 1.  The frame is tools/bench_fragments_shade_shadowed.py's (the 200-instance scene at 1920 x 1080, config 4's 10 000
point lights and 240 x 135 x 32 clusters, one sun with four --resolution^2 cascades), made on the device.
  shadowed_us        orbit_fragments_shade_shadowed on that frame: the yardstick
  nothing_us         the new call on the same frame with the environment and sky NULL (it may be at most 5 % slower)
  old_us, unshadowed_us  orbit_fragments_shade and the shadowed call without a shadowed light, as §4.26 timed them: their
                     kernels are unchanged, the ratios to the recorded figures are written beside them
  with the light table's last row a sky light (the cluster pass puts it into every active cluster):
  shadowed_sky_skipped_us  the shadowed call, which skips it
  sky_env_us         the new call with the environment at the reference's sizes (irradiance 32, prefiltered 512 x 5, table
                     512; made by orbit_env_map from a seeded panorama with reduced sample counts: the sizes decide the
                     gathers, not the contents)
  from --far-position, which leaves about a third of the screen uncovered:
  far_sky_env_us     the same call on that frame
  far_sky_env_box_us the same plus the skybox from a 1024 sky cube with its full chain
floor_us: §4.26's 64 B per pixel at 8 TB/s (40 B read, 16 B + 8 B written); cube and table taps are cache traffic and are not
in the floor.
Usage: python tools/bench_fragments_shade_sky.py [--instances 200] [--resolution 2048] [--iters 20]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
REFERENCE_ENV = dict(sky_size=1024, irradiance_size=32, prefiltered_size=512, prefiltered_levels=5, brdf_size=512)
REDUCED_COUNTS = dict(sample_count=64, sample_delta=0.25, brdf_sample_count=64)


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
    ap.add_argument("--resolution", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--far-position", type=float, nargs=3, default=(0.0, 1.0, 15.0))
    ap.add_argument("--no-host-check", action="store_true", help="skip the mirror (minutes at this size); device_equals_host stays empty")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fragments_shade_sky_mi355x.json"))
    args = ap.parse_args()
    import torch

    import config_scenes as cs
    import raster_scene as rs
    from oracle import oracle
    from orbit_amd import camera, raster
    from orbit_amd import env_map as em
    from orbit_amd import layouts as L
    from orbit_amd.engine import Engine

    timed = _tool("bench_visibility_surface")._timed
    count = _tool("count_surface_fragments")
    tool = _tool("count_fragments_shade_shadowed")
    sky_tool = _tool("count_fragments_shade_sky")
    oracle.build()
    oracle.lib()
    scene, (w, h), res = rs.glb_scene(args.instances), (args.width, args.height), args.resolution
    assert (w, h) == tuple(cs.SCREEN), "config 4's clusters are laid out for its screen"
    words, rows = len(scene.meshlet_data), count.scene_rows(scene)
    meshlets = np.ascontiguousarray(scene.meshlets).view(np.uint8).reshape(-1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    z = lambda n, dt=torch.int32: torch.zeros(max(int(n), 1), dtype=dt, device="cuda")  # noqa: E731
    base = 2048
    q = np.asarray(tool.SUN_Q, np.float64)
    q = tuple(float(v) for v in q / np.linalg.norm(q))
    cc, tile = cs.CLUSTERS, 8
    clusters = cc[0] * cc[1] * cc[2]
    cap, lcap = cc[0] * cc[1] * max(4, cc[2]), clusters * 34
    cutoff = 0.25  # make_lights' default: outer_radius = sqrt(intensity / cutoff)
    d_data, d_vb, d_ent, d_rows, d_mlt = up(scene.meshlet_data), up(scene.vertices), up(scene.entities), up(rows), up(meshlets)
    d_materials = up(scene.materials)
    vis, depth, stats, fstats, sstats, kstats = z(w * h, torch.int64), z(w * h, torch.float32), z(8), z(8), z(4), z(8)
    surf = dict(bary=z(2 * w * h, torch.float32), grad=z(4 * w * h, torch.float32), triangle=z(4 * w * h))
    planes = dict(world_pos=z(4 * w * h, torch.float32), normal=z(3 * w * h, torch.float32), material=z(w * h))
    gm, gb, gimg = z(cc[0] * cc[1]), torch.zeros((clusters, 2), dtype=torch.int32, device="cuda"), torch.zeros((clusters, 2), dtype=torch.int32, device="cuda")
    gu, gl = z(16 + 4 * cap, torch.uint8), z(4 + 4 * lcap, torch.uint8)
    color, walked, factor, cascade = z(4 * w * h, torch.float32), z(w * h), z(w * h, torch.float32), z(w * h)
    atlas = torch.zeros((4, res, res), dtype=torch.float32, device="cuda")
    eng = Engine(0, max_entities=4096, max_dispatches=1024, max_draws=1024, max_lights=12_000, max_clusters=clusters)
    floor_us = round(w * h * 64 / 8e12 * 1e6, 1)
    # the environment at the reference's sizes and the 1024 sky cube, made on the device
    lay = em.layout(**REFERENCE_ENV)
    pano = sky_tool.panorama(shape=(128, 256))
    cubes = {k: z(int(lay[k + "_texels"]) * 4, torch.int16) for k in ("sky", "irradiance", "prefiltered")}
    table = z(int(lay["brdf_texels"]) * 2, torch.int16)
    em.device_env_map(eng, equirect=up(pano), sky=cubes["sky"], irradiance=cubes["irradiance"], prefiltered=cubes["prefiltered"], brdf=table,
                      equirect_w=pano.shape[1], equirect_h=pano.shape[0], **REFERENCE_ENV, **REDUCED_COUNTS)
    torch.cuda.synchronize()
    env_kw = dict(irradiance=cubes["irradiance"], irradiance_size=REFERENCE_ENV["irradiance_size"], prefiltered=cubes["prefiltered"],
                  prefiltered_size=REFERENCE_ENV["prefiltered_size"], prefiltered_levels=REFERENCE_ENV["prefiltered_levels"], brdf=table,
                  brdf_size=REFERENCE_ENV["brdf_size"])
    s = tool.SETTINGS
    state = {}

    def frame(position, with_sky_light):
        """the chain for a camera at `position` into the buffers above; -> the camera, the light table and its device copy"""
        cam = rs.camera(w, h, position=tuple(float(v) for v in position))
        push, info, lights = cs.config4_inputs(oracle, cam)
        lights = np.concatenate([lights, tool.sun_light(base, q)] + ([sky_tool.sky_light()] if with_sky_light else []))
        info = info.copy()
        info["global_light_count"] = len(lights)
        d_lights = up(lights)
        _, _, draw, _, _ = scene.cull(oracle, cam, 0)
        n = int(draw[:4].view(np.uint32)[0])
        d_draw, vp = up(draw[:4 + 28 * n]), rs.view_proj(cam)
        geometry = (d_vb, len(scene.vertices), d_ent, scene.entity_count, vp)
        view_pos = tuple(float(v) for v in np.linalg.inv(cam.view.astype(np.float64))[:3, 3])
        if state.get("position") != tuple(position):  # the maps follow the camera's cascades
            casters = scene.all_commands(oracle, cam)
            cascades = tool.cascades_of(cam, q, res, view_pos, w / h)
            matrices = [m for m, _ in cascades]
            state.update(position=tuple(position), shadow_rows=raster.shadow_rows(matrices, [x for _, x in cascades]))
            state["d_shadow"] = up(state["shadow_rows"])
            raster.shadow_atlas(eng, atlas, up(casters), (casters.nbytes - 4) // 28, d_data, d_vb, len(scene.vertices), d_ent, scene.entity_count,
                                matrices, res, cull_none=True, meshlet_data_words=words, clip_near=True, wide_guard=True)
        eng.raster_visibility(d_draw, n, d_data, *geometry, vis, w, h, clear=True, meshlet_data_words=words, clip_near=True, wide_guard=True)
        eng.visibility_resolve(vis, w, h, depth=depth)
        eng.compute_clusters(push, info, depth, d_lights, gm, gb, gu, cap, gl, lcap, gimg)
        eng.visibility_surface_drawn(vis, w, h, d_draw, n, d_data, *geometry, **surf, clear=True, meshlet_data_words=words, clip_near=True,
                                     wide_guard=True)
        eng.surface_fragments(vis, w, h, d_draw, n, d_mlt, len(meshlets) // 32, surf["bary"], surf["triangle"], d_rows, len(scene.vertices), d_ent,
                              scene.entity_count, **planes, stats=fstats, clear=True)
        torch.cuda.synchronize()
        eng.status()
        zs, zb = float(push["z_scale"]), float(push["z_bias"])
        common = (vis, w, h, planes["world_pos"], planes["normal"], planes["material"], d_materials, len(scene.materials), d_lights, len(lights), gimg, gl,
                  lcap, cc, tile, zs, zb, cutoff, cam.z_near, view_pos, color)
        tail = (state["d_shadow"], 1, atlas, 4, res, s["blocker_search_radius"], s["normal_bias_scale"], s["oriented_bias"])
        outs = dict(shadow_index_base=base, shadow_factor=factor, cascade=cascade, shadow_stats=sstats, lights_walked=walked, stats=stats, clear=True)
        return dict(cam=cam, lights=lights, d_lights=d_lights, common=common, tail=tail, outs=outs, zs=zs, zb=zb, view_pos=view_pos)

    def measure(calls):
        for _ in range(3):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        eng.status()
        us = {}
        for _ in range(2):  # the first round also settles the clocks: its figures are dropped
            for name, fn in calls.items():
                us[name] = float(np.median(timed(torch, fn, args.iters)))
        return us

    us = {}
    # 1. the bench frame as §4.26 timed it: the yardstick and the new call with nothing to add
    f = frame((0.0, 1.0, 6.0), False)
    plain = f["lights"].copy()
    plain["shadow_data_index"][-1] = 0xFFFFFFFF
    d_plain = up(plain)
    unshadowed_common = f["common"][:8] + (d_plain,) + f["common"][9:]
    us.update(measure(dict(
        shadowed=lambda: eng.fragments_shade_shadowed(*f["common"], *f["tail"], **f["outs"]),
        nothing=lambda: eng.fragments_shade_sky(*f["common"], *f["tail"], sky_stats=kstats, **f["outs"]),
        unshadowed=lambda: eng.fragments_shade_shadowed(*unshadowed_common, *f["tail"], **f["outs"]),
        old=lambda: eng.fragments_shade(*unshadowed_common, lights_walked=walked, stats=stats, clear=True))))
    # 2. the same camera, a sky light behind the sun
    f = frame((0.0, 1.0, 6.0), True)
    us.update(measure(dict(
        shadowed_sky_skipped=lambda: eng.fragments_shade_shadowed(*f["common"], *f["tail"], **f["outs"]),
        sky_env=lambda: eng.fragments_shade_sky(*f["common"], *f["tail"], **env_kw, sky_stats=kstats, **f["outs"]))))
    near_stats = {k: int(v) for k, v in zip(L.SKY_STATS.names, kstats.cpu().numpy().view(L.SKY_STATS)[0].tolist())}
    # 3. the far camera: about a third of the screen uncovered
    f = frame(args.far_position, True)
    basis = camera.skybox_basis((0.0, 0.0, 0.0, 1.0), float(np.rad2deg(f["cam"].fov)), w / h)
    box_kw = dict(env_kw, sky=cubes["sky"], sky_size=REFERENCE_ENV["sky_size"], sky_levels=lay["sky_levels"], skybox_lod=0.0, basis=basis)
    us.update(measure(dict(
        far_sky_env=lambda: eng.fragments_shade_sky(*f["common"], *f["tail"], **env_kw, sky_stats=kstats, **f["outs"]),
        far_sky_env_box=lambda: eng.fragments_shade_sky(*f["common"], *f["tail"], **box_kw, sky_stats=kstats, **f["outs"]))))
    far_stats = {k: int(v) for k, v in zip(L.SKY_STATS.names, kstats.cpu().numpy().view(L.SKY_STATS)[0].tolist())}
    far_base = {k: int(v) for k, v in zip(L.SHADE_STATS.names, stats.cpu().numpy().view(L.SHADE_STATS)[0].tolist())}
    equal = {}
    print(json.dumps({f"{k}_us": round(v, 1) for k, v in us.items()}), file=sys.stderr, flush=True)  # (the mirror below takes minutes)
    if not args.no_host_check:  # the far frame with everything given, both forms, against the mirror on the device's own planes
        h_vis = vis.cpu().numpy().view(np.uint64).reshape(h, w)
        h_planes = {k: v.cpu().numpy() for k, v in planes.items()}
        host_cubes = {k: v.cpu().numpy().view(np.uint16) for k, v in cubes.items()}
        env = dict(irradiance=host_cubes["irradiance"], irradiance_size=REFERENCE_ENV["irradiance_size"], prefiltered=host_cubes["prefiltered"],
                   prefiltered_size=REFERENCE_ENV["prefiltered_size"], prefiltered_levels=REFERENCE_ENV["prefiltered_levels"],
                   brdf=table.cpu().numpy().view(np.uint16), brdf_size=REFERENCE_ENV["brdf_size"])
        want = raster.host_fragments_shade_sky(h_vis, h_planes["world_pos"], h_planes["normal"], h_planes["material"].view(np.uint32), scene.materials,
                                               f["lights"], gimg.cpu().numpy().view(np.uint32), gl.cpu().numpy(), cc, tile, f["zs"], f["zb"], cutoff,
                                               f["cam"].z_near, f["view_pos"], state["shadow_rows"], atlas.cpu().numpy(), res, s["blocker_search_radius"],
                                               s["normal_bias_scale"], s["oriented_bias"], env=env,
                                               sky=dict(cube=host_cubes["sky"], size=REFERENCE_ENV["sky_size"], levels=lay["sky_levels"]), skybox_lod=0.0,
                                               basis=basis, shadow_index_base=base, index_capacity=lcap)
        for form in ("staged", "per_lane"):
            color.fill_(7.0)
            eng.fragments_shade_sky(*f["common"], *f["tail"], **box_kw, sky_stats=kstats, form=form, **f["outs"])
            torch.cuda.synchronize()
            eng.status()
            got = dict(color=color, lights_walked=walked, stats=stats, shadow_factor=factor, cascade=cascade, shadow_stats=sstats, sky_stats=kstats)
            equal[f"far_sky_env_box_{form}"] = all(got[k].cpu().numpy().tobytes() == want[k].tobytes() for k in got)
    recorded = json.load(open(os.path.join(ROOT, "profiles", "fragments_shade_shadowed_mi355x.json")))
    ratio = us["nothing"] / us["shadowed"]
    line = {"instances": args.instances, "width": w, "height": h, "iters": args.iters, "warm_up_calls": 3, "device": torch.cuda.get_device_name(0),
            "lights": len(f["lights"]), "cluster_count": list(cc), "tile_size_px": tile, "shadow_resolution": res, "environment": REFERENCE_ENV,
            "environment_made_with": REDUCED_COUNTS, "far_position": list(args.far_position),
            **{f"{k}_us": round(v, 1) for k, v in us.items()}, "floor_us": floor_us,
            "floor": "40 B read + 16 B + 8 B written per pixel (§4.26) at 8 TB/s; cube and table taps are cache traffic",
            "nothing_over_shadowed": round(ratio, 3), "within_5_percent_of_shadowed": bool(ratio <= 1.05),
            "shadowed_over_recorded": round(us["shadowed"] / recorded["shadowed_us"], 3), "unshadowed_over_recorded": round(us["unshadowed"] / recorded["unshadowed_us"], 3),
            "old_over_recorded": round(us["old"] / recorded["old_us"], 3), "sky_env_over_shadowed_sky_skipped": round(us["sky_env"] / us["shadowed_sky_skipped"], 3),
            "sky_env_over_floor": round(us["sky_env"] / floor_us, 1), "far_sky_env_box_over_floor": round(us["far_sky_env_box"] / floor_us, 1),
            "skybox_us": round(us["far_sky_env_box"] - us["far_sky_env"], 1), "near_sky_stats": near_stats, "far_sky_stats": far_stats,
            "far_uncovered_share": round(1.0 - far_base["covered_pixels"] / (w * h), 3), "device_equals_host": equal,
            "not_measured": "where the time goes (no counters were collected); the ao plane; other environments' sizes, scenes and cameras; a skybox lod "
                            "above 0; the skybox inside the shade launch (not built: DESIGN.md §4.31 says why)"}
    eng.close()
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if all(equal.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
