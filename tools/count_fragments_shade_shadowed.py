"""What orbit_fragments_shade_shadowed makes of the glTF test scene, counted exactly on the CPU: the frame
of tools/count_fragments_shade.py (100 instances, 320 x 180, 200 point lights) with one sun added, whose four cascades
come from orbit_host_shadow_cascade and whose 256^2 maps the host raster draws from every opaque meshlet.  No GPU.
  frame              the eight base counters and the four shadow counters; pixels per cascade; the early_out share; the
                     histogram of lit-tap counts of the filtered pixels; the share of 8 x 8 tiles with shadowed pixels
                     whose lanes mix early-out and filtered pixels (the lanes that idle while their neighbours filter)
  lit_differs        pixels whose lit count differs from the GLSL in float64 with the true sin / cos and double
                     coordinates (tests/fragments_shade_shadowed_ref.py shadow64), and the largest difference among them;
                     knife-edge pixels — a tap coordinate within 2^-18 of a texel boundary or a z within one ulp of a
                     compared texel — are counted apart and not compared.  Accuracy: reported only.
  sincos_max_abs_error  the largest |sinc - sin|, |cosc - cos| against float64 over every angle the pixel centres of a
                     4096 x 4096 target produce; tests/test_fragments_shade_shadowed_cpu.py bounds it by twice this value
                     rounded up to a power of two
Usage: python tools/count_fragments_shade_shadowed.py [--out profiles/fragments_shade_shadowed_cpu.json]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

RESOLUTION = 256
SUN_Q = (-0.45, 0.2, 0.1, 0.86)  # normalised below; the light travels along q . (0, 0, -1)
SETTINGS = dict(blocker_search_radius=0.3, normal_bias_scale=2.0, oriented_bias=-0.02)  # the reference's, with a normal bias
SHADOW_COUNTERS = ("shadowed_pixels", "no_cascade_pixels", "early_out_pixels", "shadow_evaluations")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def quat_rotate(q, v):
    x, y, z, w = q
    u = np.array([x, y, z])
    return 2.0 * np.dot(u, v) * u + (w * w - np.dot(u, u)) * np.asarray(v, np.float64) + 2.0 * w * np.cross(u, v)


def sun_light(shadow_index, q, intensity=3.0, size=0.5):
    """a directional LightData row as scene.rs:84-118 writes it: direction = -(q . (0, 0, -1))"""
    from orbit_amd import layouts as L

    l = np.zeros(1, L.LIGHT)
    l["light_type"], l["shadow_data_index"] = L.LIGHT_TYPE_DIRECTIONAL, shadow_index
    l["irradiance_map_index"] = l["prefiltered_map_index"] = 0xFFFFFFFF
    l["color"], l["intensity"], l["inner_radius"] = (1.0, 0.95, 0.85), intensity, size
    l["direction"] = quat_rotate(q, (0.0, 0.0, 1.0)).astype(np.float32)
    return l


def cascades_of(cam, q, resolution, position, aspect):
    """the four (light_projection_matrix, shadow_map_world_size) of orbit_host_shadow_cascade for an unrotated camera"""
    from orbit_amd import passes

    return [passes.shadow_cascade(q, position, (0.0, 0.0, 0.0, 1.0), cam.fov, cam.z_near, aspect, k, shadow_resolution=resolution)[1:]
            for k in range(4)]


def host_frame(oracle, resolution=RESOLUTION, shadow_index_base=2048, width=None, height=None):
    """tools/count_fragments_shade.py's frame with one sun, its cascades and their maps -> that dict with lights, image,
    index_buffer, index_capacity and info replaced, and casters (every opaque meshlet's command), cascades, shadow_rows, atlas,
    settings, shadow_index_base, `args` / `kw`: the arguments of raster.host_fragments_shade_shadowed"""
    from orbit_amd import raster

    base = _tool("count_fragments_shade")
    f = base.host_frame(oracle, width, height)
    scene, cam, cc = f["scene"], f["frame"]["cam"], f["cluster_count"]
    q = np.asarray(SUN_Q, np.float64)
    q = tuple(float(v) for v in q / np.linalg.norm(q))
    lights = np.concatenate([f["lights"], sun_light(shadow_index_base, q)])
    info = f["info"].copy()
    info["global_light_count"] = len(lights)
    clusters = cc[0] * cc[1] * cc[2]
    masks, bounds = oracle.cluster_mark(f["push"], f["depth"])
    unique, _ = oracle.cluster_compact(cc, masks, clusters)
    capacity = f["n_active"] * 257 + 8
    index_buffer, image, dropped = oracle.cluster_assign(info, unique, bounds, lights, capacity, clusters)
    casters = scene.all_commands(oracle, cam)
    max_casters = (casters.nbytes - 4) // 28
    cascades = cascades_of(cam, q, resolution, f["view_pos"], f["width"] / f["height"])
    matrices = [m for m, _ in cascades]
    atlas = raster.host_shadow_atlas(casters, max_casters, scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, matrices,
                                     resolution, cull_none=True, clip_near=True, wide_guard=True)
    rows = raster.shadow_rows(matrices, [s for _, s in cascades])
    a = f["args"]
    args = a[:5] + (lights, image, index_buffer) + a[8:] + (rows, atlas, resolution, SETTINGS["blocker_search_radius"],
                                                           SETTINGS["normal_bias_scale"], SETTINGS["oriented_bias"])
    return dict(f, lights=lights, info=info, image=image, index_buffer=index_buffer, index_capacity=capacity, dropped=dropped, casters=casters,
                max_casters=max_casters, cascades=cascades, shadow_rows=rows, atlas=atlas, settings=SETTINGS, shadow_index_base=shadow_index_base,
                args=args, kw=dict(shadow_index_base=shadow_index_base))


def mixed_tiles(early, shadowed):
    """(tiles with shadowed pixels, those among them whose shadowed pixels mix early-out and filtered ones), 8 x 8 tiles"""
    h, w = shadowed.shape
    with_shadow = mixed = 0
    for y in range(0, h, 8):
        for x in range(0, w, 8):
            s, e = shadowed[y:y + 8, x:x + 8], early[y:y + 8, x:x + 8]
            if s.any():
                with_shadow += 1
                mixed += bool((s & e).any() and (s & ~e).any())
    return with_shadow, mixed


def sincos_error():
    from orbit_amd import raster

    worst = 0.0
    for y0 in range(0, 4096, 256):
        theta, s, c = raster.host_shadow_rotation(0, y0, 4096, 256)
        t = theta.astype(np.float64)
        worst = max(worst, float(np.abs(s - np.sin(t)).max()), float(np.abs(c - np.cos(t)).max()))
    return worst


def count(oracle):
    import fragments_shade_shadowed_ref as ref
    from orbit_amd import raster

    f = host_frame(oracle)
    got = raster.host_fragments_shade_shadowed(*f["args"], **f["kw"])
    want = ref.shade(oracle, *f["args"], **f["kw"])
    same = all(got[k].tobytes() == want[k].tobytes() for k in ("color", "lights_walked", "stats", "shadow_factor", "cascade", "shadow_stats"))
    cascade, factor = got["cascade"], got["shadow_factor"]
    shadowed = cascade != 0xFFFFFFFF
    filtered = want["lit"] >= 0
    early = shadowed & ~filtered & (cascade < 4)
    with_shadow, mixed = mixed_tiles(early | (cascade == 4), shadowed)
    # accuracy: the sun is the one shadowed light, so `lit` is its filter's count
    pix = np.flatnonzero(shadowed.reshape(-1) & (cascade.reshape(-1) < 4))
    h, w = cascade.shape
    ys, xs = np.divmod(pix, w)
    sun = f["lights"][-1:]
    n = len(pix)
    lit64, knife = ref.shadow64(np.repeat(f["shadow_rows"], n), f["args"][1].reshape(-1, 4)[pix], f["args"][2].reshape(-1, 3)[pix],
                                np.repeat(sun["direction"], n, axis=0), np.repeat(sun["inner_radius"], n), xs, ys, f["atlas"].reshape(-1),
                                f["atlas"].shape[-1], cascade=cascade.reshape(-1)[pix].astype(np.int64), **f["settings"])
    lit32 = want["lit"].reshape(-1)[pix]
    compared = ~knife
    differs = compared & (lit32 != lit64)
    assert knife.sum() <= 0.05 * n, (int(knife.sum()), n)  # the scene stays within the cap on knife-edge pixels
    histogram = np.bincount(lit32[lit32 >= 0], minlength=129)
    st, sh = got["stats"], got["shadow_stats"]
    return dict(
        scene="100 instances, 320 x 180, 200 point lights and one sun, four 256^2 cascades", mirror_equals_restatement=bool(same),
        frame=dict({k: int(st[k]) for k in st.dtype.names}, **{k: int(sh[k]) for k in SHADOW_COUNTERS}),
        pixels_per_cascade={str(k): int((cascade == k).sum()) for k in range(5)},
        early_out_share=float(sh["early_out_pixels"]) / max(int(sh["shadowed_pixels"]), 1),
        lit_histogram={str(k): int(v) for k, v in enumerate(histogram) if v}, fully_lit_share=float((factor[shadowed] == 1).mean()),
        tiles_with_shadowed_pixels=with_shadow, mixed_tiles=mixed, mixed_tile_share=mixed / max(with_shadow, 1),
        lit_differs=dict(compared=int(compared.sum()), knife_edge=int(knife.sum()), differing=int(differs.sum()),
                         largest_difference=int(np.abs(lit32 - lit64)[differs].max()) if differs.any() else 0),
        sincos_max_abs_error=sincos_error())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from oracle import oracle

    oracle.build()
    oracle.lib()
    out = count(oracle)
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
