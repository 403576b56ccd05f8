"""A frame of the glTF test scene as a picture: tools/count_fragments_shade_shadowed.py's frame (100
instances, 320 x 180, 200 point lights and a sun with four 256^2 cascades) shaded, bloomed and tone-mapped — shade -> bloom
-> post process -> a binary PPM.
  on the CPU (default)  through the host mirrors (orbit_host_fragments_shade_shadowed, orbit_host_bloom,
                        orbit_host_post_process); prints the counters and writes --out, which also keeps the accuracy figures
                        tests/test_post_chain_cpu.py holds (powc against float64, the share of packed texels and rgba8
                        bytes that differ from the GLSL in float64)
  --device              the three calls on the GPU from the same planes, compared byte for byte with the mirrors' picture;
                        exit code 1 if a byte differs.  Writes the device's picture; --out is not touched.
  --ao FILE             also writes the frame's blurred ambient occlusion (orbit_ssao at half resolution, SsaoSettings'
                        defaults) as a binary PGM: the mirror's bytes, or with --device the GPU's, compared
                        byte for byte with the mirror's (raw, blurred, ao_pixel and the counters).  Nothing else changes.
  --sky                 the frame of tools/count_fragments_shade_sky.py instead: one sky light added, the four
                        images of orbit_env_map from a seeded panorama at reduced sizes, orbit_fragments_shade_sky with the
                        skybox behind the scene (with --ao its ao_pixel plane feeds the sky term), bloom and post process; with
                        --device the whole chain on the GPU, env_map included, compared byte for byte with the mirrors'.  Prints
                        the counters and writes the picture; --out is not touched.
Without --sky, uncovered pixels show what the colour plane holds there (0: black).
Usage: python tools/render_frame.py [--device] [--sky] [--picture frame.ppm] [--ao ao.pgm] [--exposure 4.0] [--out profiles/post_chain_cpu.json]
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


def host_picture(f, exposure):
    """the frame through the three mirrors -> (shaded, bloom, post process) dicts"""
    from orbit_amd import post, raster

    shaded = raster.host_fragments_shade_shadowed(*f["args"], **f["kw"])
    bloom = post.host_bloom(shaded["color"], **{k: post.DEFAULTS[k] for k in ("threshold", "soft_threshold", "filter_radius")})
    out = post.host_post_process(shaded["color"], bloom["mips"], exposure=exposure, bloom_intensity=post.DEFAULTS["bloom_intensity"])
    return shaded, bloom, out


def device_picture(f, tool, exposure):
    """the same three calls on the GPU -> (color, mips, ldr, rgba8, bloom stats, post stats) as host arrays"""
    import torch

    from orbit_amd import post
    from orbit_amd.engine import Engine

    base = tool._tool("count_fragments_shade")
    w, h, cc, s = f["width"], f["height"], f["cluster_count"], f["settings"]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    vis, wp, nrm, mat, mats, lights, image, index_buffer = f["args"][:8]
    d = [up(x) for x in (vis, wp, nrm, mat, mats, lights, image, index_buffer, f["shadow_rows"], f["atlas"])]
    lay = post.bloom_layout(w, h)
    color, ldr = (torch.zeros(4 * w * h, dtype=torch.float32, device="cuda") for _ in range(2))
    mips = torch.zeros(lay["total_texels"], dtype=torch.int32, device="cuda")
    rgba8 = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
    bstats, pstats = (torch.zeros(4, dtype=torch.int32, device="cuda") for _ in range(2))
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)
    eng.fragments_shade_shadowed(d[0], w, h, d[1], d[2], d[3], d[4], len(mats), d[5], len(lights), d[6], d[7], f["index_capacity"], cc, base.TILE,
                                 f["z_scale"], f["z_bias"], base.CUTOFF, f["frame"]["cam"].z_near, f["view_pos"], color, d[8], 1, d[9], 4,
                                 f["atlas"].shape[-1], s["blocker_search_radius"], s["normal_bias_scale"], s["oriented_bias"],
                                 shadow_index_base=f["shadow_index_base"], clear=True)
    eng.bloom(color, w, h, mips, stats=bstats, **{k: post.DEFAULTS[k] for k in ("threshold", "soft_threshold", "filter_radius")})
    eng.post_process(color, w, h, bloom=mips, ldr=ldr, rgba8=rgba8, stats=pstats, exposure=exposure, bloom_intensity=post.DEFAULTS["bloom_intensity"])
    torch.cuda.synchronize()
    eng.status()
    out = [t.cpu().numpy() for t in (color, mips, ldr, rgba8, bstats, pstats)]
    eng.close()
    return out


SSAO_TABLE_SEED = 1


def ssao_inputs(f):
    """the frame's depth plane, the camera's two matrices, the two tables and the half-resolution size"""
    import scenes as sc
    from orbit_amd import passes, post, raster

    depth, _, _ = raster.host_visibility_resolve(f["frame"]["visibility"], want_command_pixels=False)
    proj = sc.mat4_cols(f["frame"]["cam"].proj)
    noise, samples = post.ssao_tables(SSAO_TABLE_SEED)
    depth = np.ascontiguousarray(depth, np.float32).reshape(f["height"], f["width"])
    return depth, proj, passes.mat4_inverse(proj), noise, samples, post.ssao_resolution(f["width"], f["height"])


def host_ao(f):
    from orbit_amd import post

    depth, proj, inv, noise, samples, (sw, sh) = ssao_inputs(f)
    return post.host_ssao(depth, proj, inv, noise, samples, sw, sh)


def device_ao(f):
    """orbit_ssao on the GPU from the same depth -> (raw, blurred, ao_pixel, stats) as host arrays"""
    import torch

    from orbit_amd.engine import Engine

    depth, proj, inv, noise, samples, (sw, sh) = ssao_inputs(f)
    w, h = f["width"], f["height"]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_depth, d_noise, d_samples = up(depth), up(noise), up(samples)
    raw, blurred = (torch.zeros(sw * sh, dtype=torch.uint8, device="cuda") for _ in range(2))
    ao = torch.zeros(w * h, dtype=torch.float32, device="cuda")
    stats = torch.zeros(3, dtype=torch.int64, device="cuda")
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)
    eng.ssao(d_depth, w, h, sw, sh, proj, inv, d_noise, noise.shape[0], d_samples, samples.shape[0], raw=raw, blurred=blurred, ao_pixel=ao, stats=stats)
    torch.cuda.synchronize()
    eng.status()
    out = [t.cpu().numpy() for t in (raw, blurred, ao, stats)]
    eng.close()
    return out


def host_sky_picture(f, sky_tool, exposure, with_ao):
    """--sky on the CPU: env_map (inside the frame), ssao, shade_sky, bloom, post process through the mirrors -> (ao or None,
    shaded, bloom, post process) dicts"""
    from orbit_amd import post, raster

    ao = host_ao(f) if with_ao else None
    kw = dict(f["kw"], ao=None if ao is None else ao["ao_pixel"])
    shaded = raster.host_fragments_shade_sky(*f["args"], **kw)
    bloom = post.host_bloom(shaded["color"], **{k: post.DEFAULTS[k] for k in ("threshold", "soft_threshold", "filter_radius")})
    out = post.host_post_process(shaded["color"], bloom["mips"], exposure=exposure, bloom_intensity=post.DEFAULTS["bloom_intensity"])
    return ao, shaded, bloom, out


def device_sky_picture(f, sky_tool, exposure, with_ao, eng):
    """--sky on the GPU: orbit_env_map from the panorama, orbit_ssao, orbit_fragments_shade_sky, orbit_bloom and
    orbit_post_process on one stream, nothing copied to the host in between -> dict of host arrays: the env's four images,
    ao_pixel (or None), color, sky_stats, stats, mips, ldr, rgba8"""
    import torch

    from orbit_amd import env_map as em
    from orbit_amd import post

    base = _tool("count_fragments_shade")
    w, h, cc, s = f["width"], f["height"], f["cluster_count"], f["settings"]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    vis, wp, nrm, mat, mats, lights, image, index_buffer = f["args"][:8]
    d = [up(x) for x in (vis, wp, nrm, mat, mats, lights, image, index_buffer, f["shadow_rows"], f["atlas"])]
    sizes = sky_tool.SCENE_ENV
    lay = em.layout(**{k: sizes[k] for k in ("sky_size", "irradiance_size", "prefiltered_size", "prefiltered_levels", "brdf_size")})
    pano = sky_tool.panorama()
    cubes = {k: torch.zeros(int(lay[k + "_texels"]) * 4, dtype=torch.int16, device="cuda") for k in ("sky", "irradiance", "prefiltered")}
    table = torch.zeros(int(lay["brdf_texels"]) * 2, dtype=torch.int16, device="cuda")
    em.device_env_map(eng, equirect=up(pano), sky=cubes["sky"], irradiance=cubes["irradiance"], prefiltered=cubes["prefiltered"], brdf=table,
                      equirect_w=pano.shape[1], equirect_h=pano.shape[0], **sizes)
    ao = None
    if with_ao:
        depth, proj, inv, noise, samples, (sw, sh) = ssao_inputs(f)
        d_depth, d_noise, d_samples = up(depth), up(noise), up(samples)
        raw, blurred = (torch.zeros(sw * sh, dtype=torch.uint8, device="cuda") for _ in range(2))
        ao = torch.zeros(w * h, dtype=torch.float32, device="cuda")
        eng.ssao(d_depth, w, h, sw, sh, proj, inv, d_noise, noise.shape[0], d_samples, samples.shape[0], raw=raw, blurred=blurred, ao_pixel=ao)
    blay = post.bloom_layout(w, h)
    color, ldr = (torch.zeros(4 * w * h, dtype=torch.float32, device="cuda") for _ in range(2))
    mips = torch.zeros(blay["total_texels"], dtype=torch.int32, device="cuda")
    rgba8 = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
    stats, sky_stats = (torch.zeros(8, dtype=torch.int32, device="cuda") for _ in range(2))
    eng.fragments_shade_sky(d[0], w, h, d[1], d[2], d[3], d[4], len(mats), d[5], len(lights), d[6], d[7], f["index_capacity"], cc, base.TILE,
                            f["z_scale"], f["z_bias"], base.CUTOFF, f["frame"]["cam"].z_near, f["view_pos"], color, d[8], 1, d[9], 4,
                            f["atlas"].shape[-1], s["blocker_search_radius"], s["normal_bias_scale"], s["oriented_bias"],
                            irradiance=cubes["irradiance"], irradiance_size=sizes["irradiance_size"], prefiltered=cubes["prefiltered"],
                            prefiltered_size=sizes["prefiltered_size"], prefiltered_levels=sizes["prefiltered_levels"], brdf=table,
                            brdf_size=sizes["brdf_size"], sky=cubes["sky"], sky_size=sizes["sky_size"], sky_levels=lay["sky_levels"],
                            skybox_lod=f["kw"]["skybox_lod"], basis=f["basis"], ao=ao, sky_stats=sky_stats, stats=stats,
                            shadow_index_base=f["shadow_index_base"], clear=True)
    eng.bloom(color, w, h, mips, **{k: post.DEFAULTS[k] for k in ("threshold", "soft_threshold", "filter_radius")})
    eng.post_process(color, w, h, bloom=mips, ldr=ldr, rgba8=rgba8, exposure=exposure, bloom_intensity=post.DEFAULTS["bloom_intensity"])
    torch.cuda.synchronize()
    eng.status()
    out = dict(cubes, brdf=table, ao_pixel=ao, color=color, stats=stats, sky_stats=sky_stats, mips=mips, ldr=ldr, rgba8=rgba8)
    return {k: None if t is None else t.cpu().numpy() for k, t in out.items()}


def sky_equal(f, host, got):
    """device_sky_picture's arrays against host_sky_picture's (and the frame's environment), name by name -> {name: equal}"""
    ao, shaded, bloom, out = host
    want = dict(sky=f["sky"]["cube"], irradiance=f["env"]["irradiance"], prefiltered=f["env"]["prefiltered"], brdf=f["env"]["brdf"],
                ao_pixel=None if ao is None else ao["ao_pixel"], color=shaded["color"], stats=shaded["stats"], sky_stats=shaded["sky_stats"],
                mips=bloom["mips"], ldr=out["ldr"], rgba8=out["rgba8"])
    return {k: np.ascontiguousarray(v).tobytes() == np.ascontiguousarray(got[k]).tobytes() for k, v in want.items() if v is not None}


def sky_main(args, oracle):
    from orbit_amd import post

    sky_tool = _tool("count_fragments_shade_sky")
    f = sky_tool.host_frame(oracle)
    w, h = f["width"], f["height"]
    host = host_sky_picture(f, sky_tool, args.exposure, args.ao is not None)
    ao, shaded, bloom, out = host
    line = dict(width=w, height=h, picture=os.path.basename(args.picture), **sky_tool.SCENE_ENV,
                **{k: int(shaded["stats"][k]) for k in ("covered_pixels", "written_pixels", "unserved_pixels")},
                **{k: int(shaded["sky_stats"][k]) for k in ("sky_evaluations", "sky_lit_pixels", "skybox_pixels", "bad_directions")})
    if args.device:
        from orbit_amd.engine import Engine

        eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)
        try:
            got = device_sky_picture(f, sky_tool, args.exposure, args.ao is not None, eng)
        finally:
            eng.close()
        equal = sky_equal(f, host, got)
        post.write_ppm(args.picture, got["rgba8"].reshape(h, w, 4))
        print(json.dumps(dict(line, device_equals_host=equal)))
        return 0 if all(equal.values()) else 1
    post.write_ppm(args.picture, out["rgba8"])
    if ao is not None:
        post.write_pgm(args.ao, ao["blurred"])
    print(json.dumps(dict(line, mean_byte=round(float(out["rgba8"][..., :3].mean()), 2))))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--picture", default="frame.ppm")
    ap.add_argument("--ao", default=None, metavar="FILE")
    ap.add_argument("--sky", action="store_true")
    ap.add_argument("--exposure", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_chain_cpu.json"))
    args = ap.parse_args()
    from oracle import oracle
    from orbit_amd import post
    from orbit_amd import layouts as L

    oracle.build()
    if args.sky:
        return sky_main(args, oracle)
    tool = _tool("count_fragments_shade_shadowed")
    f = tool.host_frame(oracle)
    w, h = f["width"], f["height"]
    shaded, bloom, out = host_picture(f, args.exposure)
    if args.device:
        color, mips, ldr, rgba8, bstats, pstats = device_picture(f, tool, args.exposure)
        equal = dict(color=color.tobytes() == shaded["color"].tobytes(), mips=mips.tobytes() == bloom["mips"].tobytes(),
                     ldr=ldr.tobytes() == out["ldr"].tobytes(), rgba8=rgba8.tobytes() == out["rgba8"].tobytes(),
                     bloom_stats=bstats.tobytes() == bloom["stats"].tobytes(), post_stats=pstats.tobytes() == out["stats"].tobytes())
        post.write_ppm(args.picture, rgba8.reshape(h, w, 4))
        print(json.dumps(dict(width=w, height=h, picture=os.path.basename(args.picture), device_equals_host=equal)))
        if args.ao:
            want = host_ao(f)
            raw, blurred, ao, stats = device_ao(f)
            ao_equal = dict(raw=raw.tobytes() == want["raw"].tobytes(), blurred=blurred.tobytes() == want["blurred"].tobytes(),
                            ao_pixel=ao.tobytes() == want["ao_pixel"].tobytes(), ssao_stats=stats.tobytes() == want["stats"].tobytes())
            post.write_pgm(args.ao, blurred.reshape(want["blurred"].shape))
            print(json.dumps(dict(ao=os.path.basename(args.ao), ssao=list(want["blurred"].shape[::-1]), device_equals_host=ao_equal)))
            assert all(ao_equal.values()), ao_equal
            equal.update(ao_equal)
        return 0 if all(equal.values()) else 1
    import test_post_chain_cpu as held  # the figures the CPU tests hold, measured the same way

    post.write_ppm(args.picture, out["rgba8"])
    rgb = out["rgba8"][..., :3]
    line = {"scene": "tools/make_test_glb.py, 100 instances, seed 7; 200 point lights and a sun with four 256^2 cascades", "width": w, "height": h,
            "exposure": args.exposure, **post.DEFAULTS, "picture": os.path.basename(args.picture),
            **{k: int(shaded["stats"][k]) for k in ("covered_pixels", "written_pixels")}, **{k: int(bloom["stats"][k]) for k in L.BLOOM_STATS.names},
            **{k: int(out["stats"][k]) for k in ("pixels", "nonfinite_pixels", "bloom_pixels")},
            "distinct_rgb_values": int(len(np.unique(rgb.reshape(-1, 3), axis=0))), "mean_byte": round(float(rgb.mean()), 2),
            **held.measure_powc(), **held.measure_shares(),
            "against": "the GLSL in float64 with a true pow, levels stored through B7 (tests/post_chain_ref.py), over tests/post_chain_cases.py"}
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    if args.ao:
        got = host_ao(f)
        post.write_pgm(args.ao, got["blurred"])
        print(json.dumps(dict(ao=os.path.basename(args.ao), ssao=list(got["blurred"].shape[::-1]), mean_byte=round(float(got["blurred"].mean()), 2),
                              **{k: int(got["stats"][k]) for k in L.SSAO_STATS.names if k != "_pad"})))
    return 0


if __name__ == "__main__":
    sys.exit(main())
