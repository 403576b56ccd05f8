#!/usr/bin/env python
"""What orbit_env_map computes, measured on the CPU through the host mirror (orbit_amd.env_map.host_env_map): the mirror
against the GLSL of the env_map shaders and brdf_integration.frag evaluated in float64 with the true sin, cos, atan and asin
and exact fp16 storage (tests/env_map_ref.py with T = float64; each product from the mirror's own sky cube, so a product's
figure is its own error and not the sky cube's handed on) — per product the largest and the mean absolute and relative error
of the stored fp16 and the share of halves that differ by more than one fp16 step — over the case matrix of
tests/env_map_cases.py and over one chain at sky 64, irradiance 16, prefiltered 32 x 5 and table 32 from a seeded 256 x 128
panorama (CHAIN below: the restatement is a Python loop over the samples, so the chain runs 256 samples and a delta of
0.1); the largest error of the routines E2 and E5-E7 use (atan2c, asinc, sine and cosine on [-1e-6, 2 pi + 0.1]) against
float64 over dense sweeps; and, for one small irradiance case, the distance between E5's constant lod and a float64
evaluation that takes each tap's lod from the differences across its 2 x 2 quad of texels, as a fragment shader would.  No GPU.

Usage: python tools/count_env_map.py [--out profiles/env_map_cpu.json] [--no-chain]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import env_map_cases as ec  # noqa: E402
import env_map_ref as ref  # noqa: E402
from orbit_amd import env_map as em  # noqa: E402

F, D = np.float32, np.float64
PRODUCTS = ("sky", "irradiance", "prefiltered", "brdf")
CHAIN = dict(sky_size=64, irradiance_size=16, prefiltered_size=32, prefiltered_levels=5, brdf_size=32, sample_count=256, sample_delta=0.1,
             brdf_sample_count=256)
QUAD_CASE = dict(sky_size=16, irradiance_size=8, sample_delta=0.25)


def up(x):
    """a figure as it is recorded: three significant digits, rounded up"""
    if x == 0:
        return 0.0
    e = int(np.floor(np.log10(abs(x)))) - 2
    return float(f"{np.ceil(x / 10.0 ** e) * 10.0 ** e:.3g}")


def routine_errors():
    """the largest absolute error of each routine against float64 of the same float32 arguments"""
    theta = np.linspace(-np.pi, np.pi, 2000001)
    out = {}
    worst = 0.0
    for radius in (1.0, 1e-3, 37.5):
        y, x = (radius * np.sin(theta)).astype(F), (radius * np.cos(theta)).astype(F)
        worst = max(worst, float(np.abs(em.host_atan2c(y, x).astype(D) - np.arctan2(y.astype(D), x.astype(D))).max()))
    out["atan2c_max_abs"] = worst
    x = np.linspace(-1.0, 1.0, 2000001).astype(F)
    out["asinc_max_abs"] = float(np.abs(em.host_asinc(x).astype(D) - np.arcsin(x.astype(D))).max())
    t = np.linspace(-1e-6, 2.0 * np.pi + 0.1, 4000001).astype(F)
    s, c = em.host_sincos(t)
    out["sin_max_abs"] = float(np.abs(s.astype(D) - np.sin(t.astype(D))).max())
    out["cos_max_abs"] = float(np.abs(c.astype(D) - np.cos(t.astype(D))).max())
    return out


def _ordered(h):
    """fp16 bit patterns as integers that step by one per representable value"""
    h = h.astype(np.int32)
    return np.where(h & 0x8000, -(h & 0x7FFF), h)


class Tally:
    def __init__(self):
        self.n = self.beyond = 0
        self.max_abs = self.max_rel = self.sum_abs = self.sum_rel = 0.0
        self.n_rel = 0

    def add(self, got, want):
        a, b = got.view(np.float16).astype(D), want.view(np.float16).astype(D)
        err = np.abs(a - b)
        self.n += err.size
        self.beyond += int((np.abs(_ordered(got) - _ordered(want)) > 1).sum())
        self.max_abs, self.sum_abs = max(self.max_abs, float(err.max())), self.sum_abs + float(err.sum())
        nz = b != 0
        if nz.any():
            rel = err[nz] / np.abs(b[nz])
            self.max_rel, self.sum_rel, self.n_rel = max(self.max_rel, float(rel.max())), self.sum_rel + float(rel.sum()), self.n_rel + int(nz.sum())

    def row(self):
        return dict(max_abs=self.max_abs, mean_abs=self.sum_abs / max(self.n, 1), max_rel=self.max_rel, mean_rel=self.sum_rel / max(self.n_rel, 1),
                    share_beyond_one_step=self.beyond / max(self.n, 1))


def _compare(kw, tally):
    got = em.host_env_map(**kw)
    rest = {k: v for k, v in kw.items() if k != "equirect"}
    if got["sky"] is not None:
        tally["sky"].add(got["sky"], ref.sky_cube(kw["equirect"], kw["sky_size"], D)[0])
    # the later products from the mirror's own sky cube: their own error alone
    want = ref.env_map(sky_words=got["sky"], T=D, **rest)
    for k in PRODUCTS[1:]:
        if got[k] is not None:
            tally[k].add(got[k], want[k])


def matrix_figures():
    tally = {k: Tally() for k in PRODUCTS}
    for _, kw in ec.chain_cases():
        _compare(kw, tally)
    return {k: t.row() for k, t in tally.items()}


def chain_figures():
    rng = np.random.default_rng(64)
    pano = (rng.random((128, 256, 4)) ** 4 * 16.0).astype(F)  # a few bright texels among dim ones
    tally = {k: Tally() for k in PRODUCTS}
    _compare(dict(CHAIN, equirect=pano), tally)
    return {k: t.row() for k, t in tally.items()}


def quad_lod_distance():
    """E5's constant lod against lods from 2 x 2 quad differences, both in float64 from the mirror's sky cube: the largest
    and the mean absolute difference of the irradiance texels and the largest relative one"""
    kw = QUAD_CASE
    n, size = kw["irradiance_size"], kw["sky_size"]
    sky_words = em.host_env_map(equirect=ec.panorama("noise"), sky_size=size)["sky"]
    sky = ref.Cube(sky_words, size, size.bit_length(), D)
    constant, _ = ref.irradiance(sky, n, kw["sample_delta"], D)
    quad = np.empty_like(constant)
    delta = D(kw["sample_delta"])
    for face in range(6):
        p = [c.reshape(-1) for c in ref.local_pos(face, n, D)]
        normal = ref.normalize(p)
        up_v = [np.zeros_like(p[0]), np.ones_like(p[0]), np.zeros_like(p[0])]
        right = ref.normalize(ref.cross(up_v, normal))
        up_v = ref.normalize(ref.cross(normal, right))
        total, count, phi = np.zeros((n * n, 3)), 0.0, 0.0
        idx = np.arange(n * n).reshape(n, n)
        base = (idx // n // 2 * 2 * n + idx % n // 2 * 2).reshape(-1)  # the quad's first texel
        while phi < 2.0 * ref.PI:
            theta = 0.0
            while theta < 0.5 * ref.PI:
                st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
                vec = [(st * cp * right[k] + st * sp * up_v[k]) + ct * p[k] for k in range(3)]
                # the quad's footprint in texels of level 0, on the layer the quad's first texel falls on
                f0, _, _, _ = ref.face_select([v[base] for v in vec])
                st_of = []
                for f in range(6):
                    fx, sc, tc, ma = _on_face(f, vec)
                    st_of.append((0.5 * sc / ma + 0.5, 0.5 * tc / ma + 0.5))
                s = np.choose(f0, [a[0] for a in st_of])
                t = np.choose(f0, [a[1] for a in st_of])
                dx = np.hypot(s[np.minimum(base + 1, n * n - 1)] - s[base], t[np.minimum(base + 1, n * n - 1)] - t[base]) * size
                dy = np.hypot(s[np.minimum(base + n, n * n - 1)] - s[base], t[np.minimum(base + n, n * n - 1)] - t[base]) * size
                with np.errstate(all="ignore"):
                    lod = np.where(np.maximum(dx, dy) > 0, np.log2(np.maximum(dx, dy)), 0.0)
                lod = np.where(np.isfinite(lod), np.maximum(lod, 0.0), 0.0)
                c, _ = sky.sample(vec, lod)
                total, count = total + c * ct * st, count + 1.0
                theta += delta
            phi += delta
        quad[face] = (ref.PI * total / count).reshape(n, n, 3)
    ok = np.isfinite(constant) & np.isfinite(quad)
    err = np.abs(constant - quad)[ok]
    rel = err[np.abs(quad[ok]) > 0] / np.abs(quad[ok])[np.abs(quad[ok]) > 0]
    return dict(max_abs=float(err.max()), mean_abs=float(err.mean()), max_rel=float(rel.max()), mean_value=float(np.abs(quad[ok]).mean()), over=dict(kw))


def _on_face(f, vec):
    """(sc, tc, ma) of directions on layer f's plane whatever their major axis (a quad shares one layer)"""
    x, y, z = vec
    return [(f, -z, -y, np.abs(x)), (f, z, -y, np.abs(x)), (f, x, z, np.abs(y)), (f, x, -z, np.abs(y)), (f, x, -y, np.abs(z)), (f, -x, -y, np.abs(z))][f]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_map_cpu.json"))
    ap.add_argument("--no-chain", action="store_true")
    args = ap.parse_args()
    record = lambda rows: {p: {k: up(v) for k, v in row.items()} for p, row in rows.items()}  # noqa: E731
    out = {"against": "the GLSL in float64 with the true sin / cos / atan / asin and exact fp16 storage (tests/env_map_ref.py, T = float64)",
           "recorded_as": "three significant digits, rounded up",
           "routines": {k: up(v) for k, v in routine_errors().items()},
           "matrix": dict(record(matrix_figures())), "matrix_over": "tests/env_map_cases.py: chain_cases()"}
    if not args.no_chain:
        out["chain"] = record(chain_figures())
        out["chain_over"] = dict(CHAIN, panorama="256 x 128, seeded")
    q = quad_lod_distance()
    out["constant_lod_against_quad_lod"] = {k: (up(v) if isinstance(v, float) else v) for k, v in q.items()}
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
