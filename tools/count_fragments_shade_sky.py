#!/usr/bin/env python
"""What orbit_fragments_shade_sky computes, measured on the CPU through the host mirror
(orbit_amd.raster.host_fragments_shade_sky): the distance of the mirror's colour from forward.frag:378-405
and skybox.frag evaluated in float64 on the stored fp16 texels (tests/fragments_shade_sky_ref.py with T = float64: the sky
term, the skybox and the light sum in double precision; the point and directional terms enter as their float32 values, whose
own distance is §4.25's and §4.26's figure) — per channel the largest absolute and the largest relative error and the share
of pixels above 2^-10 relative, the pixels lit by a sky light and the skybox pixels apart — over the case matrix of
tests/fragments_shade_sky_cases.py and over the frame of tools/count_fragments_shade_shadowed.py (100 instances, 320 x 180,
200 point lights, one sun) with one sky light added to the light table, an environment made by orbit_host_env_map from a
seeded 64 x 32 panorama at reduced sizes (SCENE_ENV below) and the skybox behind it.  Pixels whose float64 colour is 0 in a
channel are left out of that channel's relative figures.  No GPU.
Usage: python tools/count_fragments_shade_sky.py [--out profiles/fragments_shade_sky_cpu.json]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SCENE_ENV = dict(sky_size=32, irradiance_size=8, prefiltered_size=16, prefiltered_levels=5, brdf_size=32, sample_count=64, sample_delta=0.25,
                 brdf_sample_count=64)
PANORAMA = (32, 64)
CAMERA_Q = (0.0, 0.0, 0.0, 1.0)  # the frame's camera is unrotated
THRESHOLD = 2.0 ** -10


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def panorama(seed=11, shape=PANORAMA):
    """a seeded sky: a vertical gradient with a bright patch, noise on top; RGBA float32"""
    h, w = shape
    rng = np.random.default_rng(seed)
    v = np.linspace(1.0, 0.0, h)[:, None, None]
    p = np.concatenate([0.2 + 0.8 * v * np.array([0.5, 0.7, 1.0]) + rng.uniform(0, 0.1, (h, w, 3)), np.ones((h, w, 1))], axis=2)
    p[h // 4:h // 4 + 2, w // 3:w // 3 + 3, :3] = 30.0
    return p.astype(np.float32)


def sky_light(intensity=0.6):
    from orbit_amd import layouts as L

    l = np.zeros(1, L.LIGHT)
    l["light_type"], l["shadow_data_index"] = L.LIGHT_TYPE_SKY, 0xFFFFFFFF
    l["irradiance_map_index"], l["prefiltered_map_index"] = 0, 1
    l["color"], l["intensity"] = (1.0, 1.0, 1.0), intensity
    return l


def environment(sizes=None, seed=11):
    """orbit_host_env_map of the seeded panorama -> (env, sky): host_fragments_shade_sky's two dicts"""
    from orbit_amd import env_map as em

    sizes = dict(SCENE_ENV, **(sizes or {}))
    made = em.host_env_map(equirect=panorama(seed), **sizes)
    env = dict(irradiance=made["irradiance"], irradiance_size=sizes["irradiance_size"], prefiltered=made["prefiltered"],
               prefiltered_size=sizes["prefiltered_size"], prefiltered_levels=sizes["prefiltered_levels"], brdf=made["brdf"],
               brdf_size=sizes["brdf_size"])
    return env, dict(cube=made["sky"], size=sizes["sky_size"], levels=made["layout"]["sky_levels"])


def host_frame(oracle, width=None, height=None, sizes=None, ao=None, fov_deg=90.0):
    """tools/count_fragments_shade_shadowed.py's frame with one sky light behind its lights (the cluster pass puts it into every
    active cluster, light_culling.comp:115-117), the environment and the sky cube -> that dict with lights, image, index_buffer
    and info replaced, and env, sky, basis, `args` / `kw`: the arguments of raster.host_fragments_shade_sky"""
    from orbit_amd import camera

    shadowed = _tool("count_fragments_shade_shadowed")
    f = shadowed.host_frame(oracle, width=width, height=height)
    cc = f["cluster_count"]
    lights = np.concatenate([f["lights"], sky_light()])
    info = f["info"].copy()
    info["global_light_count"] = len(lights)
    clusters = cc[0] * cc[1] * cc[2]
    masks, bounds = oracle.cluster_mark(f["push"], f["depth"])
    unique, _ = oracle.cluster_compact(cc, masks, clusters)
    capacity = f["n_active"] * 257 + 8
    index_buffer, image, dropped = oracle.cluster_assign(info, unique, bounds, lights, capacity, clusters)
    env, sky = environment(sizes)
    basis = camera.skybox_basis(CAMERA_Q, fov_deg, f["width"] / f["height"])
    a = f["args"]
    args = a[:5] + (lights, image, index_buffer) + a[8:]
    kw = dict(f["kw"], env=env, sky=sky, skybox_lod=0.0, basis=basis, ao=ao)
    return dict(f, lights=lights, info=info, image=image, index_buffer=index_buffer, index_capacity=capacity, dropped=dropped, env=env, sky=sky,
                basis=basis, args=args, kw=kw)


class Tally:
    """per channel: the largest absolute and relative error and the share of pixels above 2^-10 relative"""

    def __init__(self):
        self.n = 0
        self.max_abs, self.max_rel, self.above = np.zeros(3), np.zeros(3), np.zeros(3, np.int64)

    def add(self, got, want):
        got, want = got.reshape(-1, 4)[:, :3].astype(np.float64), want.reshape(-1, 4)[:, :3].astype(np.float64)
        if not len(got):
            return
        err = np.abs(got - want)
        self.n += len(got)
        self.max_abs = np.maximum(self.max_abs, err.max(axis=0))
        with np.errstate(all="ignore"):
            rel = np.where(want != 0, err / np.abs(want), 0.0)
        self.max_rel = np.maximum(self.max_rel, rel.max(axis=0))
        self.above += (rel > THRESHOLD).sum(axis=0)

    def row(self):
        return dict(pixels=self.n, max_abs=[float(v) for v in self.max_abs], max_rel=[float(v) for v in self.max_rel],
                    share_above_2_pow_minus_10=[float(v) / max(self.n, 1) for v in self.above])


def compare(oracle, args, kw, lit, box):
    import fragments_shade_sky_cases as kc
    import fragments_shade_sky_ref as ref
    from orbit_amd import raster

    got = raster.host_fragments_shade_sky(*args, **kw)
    rest = {k: v for k, v in kw.items() if k not in kc.DROP}
    want = ref.shade(oracle, *args, T=np.float64, **rest)
    lit.add(got["color"][want["sky_lit"]], want["color"][want["sky_lit"]])
    box.add(got["color"][want["skybox"]], want["color"][want["skybox"]])
    return got


def matrix_figures(oracle):
    import fragments_shade_sky_cases as kc

    lit, box = Tally(), Tally()
    for case in kc.all_cases(oracle):
        compare(oracle, *case.args(), lit, box)
    return dict(lit=lit.row(), skybox=box.row())


def scene_figures(oracle):
    f = host_frame(oracle)
    lit, box = Tally(), Tally()
    got = compare(oracle, f["args"], f["kw"], lit, box)
    st, sk = got["stats"], got["sky_stats"]
    counters = dict({k: int(st[k]) for k in st.dtype.names}, **{k: int(sk[k]) for k in ("sky_evaluations", "sky_lit_pixels", "skybox_pixels", "bad_directions")})
    return dict(lit=lit.row(), skybox=box.row()), counters


def count(oracle):
    scene, counters = scene_figures(oracle)
    return dict(scene_over=dict(SCENE_ENV, frame="100 instances, 320 x 180, 200 point lights, one sun and one sky light", panorama="64 x 32, seeded"),
                scene_counters=counters, scene=scene, matrix=matrix_figures(oracle))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from oracle import oracle

    oracle.build()
    oracle.lib()
    text = json.dumps(count(oracle))
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
