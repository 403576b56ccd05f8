#!/usr/bin/env python
"""What orbit_ssao computes, counted on the CPU through the host mirror (orbit_amd.post.host_ssao): the mirror against the
GLSL of ssao.comp / ssao_blur.comp evaluated in float64 with the true sine and cosine (tests/ssao_ref.py with F = float64)
over the case matrix of tests/ssao_cases.py and over the 100-instance glTF scene at 320 x 180 and 160 x 90, at full and at
half resolution — the share of raw and of blurred bytes that differ at all and by more than 1, the SSAO pixels that are NaN in
one precision only, and the largest and the mean error of ao_pixel away from those —, and the scene's census: mean AO, pixels
with byte 255, samples in range, A2's branches, and column 0 against column 1 (A1's wrapped neighbour).  The pass has hard comparisons (>=, the range test, A2's branch): a last-bit difference
can flip a sample, and the "more than 1" figure says how often.  No GPU.

Usage: python tools/count_ssao.py [--out profiles/ssao_cpu.json]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INSTANCES = 100
SCENE_SIZES = ((320, 180), (160, 90))
TABLE_SEED = 1
FIGURES = ("raw_share_differing", "raw_share_beyond_1", "blurred_share_differing", "blurred_share_beyond_1", "ao_pixel_max_error",
           "ao_pixel_mean_error")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def host_frame(oracle, width, height, instances=INSTANCES):
    """The depth prepass of the glTF scene on the host -> dict(scene, frame (visibility, draw1, draw2, view_proj, cam),
    depth (height, width) float32, projection, inverse_projection: the camera's, column-major)"""
    import raster_scene as rs
    import scenes as sc
    from orbit_amd import passes, raster

    outside = _tool("count_visible_surface")
    scene = rs.glb_scene(instances)
    frame = _tool("count_surface_drawn").flagged_frames(scene, oracle, [rs.camera(width, height, p) for p in outside.CAMERAS], width, height)[1]
    depth, _, _ = raster.host_visibility_resolve(frame["visibility"], want_command_pixels=False)
    proj = sc.mat4_cols(frame["cam"].proj)
    return dict(scene=scene, frame=frame, depth=np.ascontiguousarray(depth, np.float32).reshape(height, width), projection=proj,
                inverse_projection=passes.mat4_inverse(proj))


class Tally:
    """the figures over a set of runs"""

    def __init__(self):
        self.n = dict(raw=0, blurred=0)
        self.differing = dict(raw=0, blurred=0)
        self.beyond = dict(raw=0, blurred=0)
        self.ao, self.ao_sum, self.ao_n, self.nan_one_way = 0.0, 0.0, 0, 0

    def add(self, got, want, nan32):
        """got: the mirror's outputs; want: the float64 reading; nan32: the SSAO pixels that are NaN in float32 (the
        restatement's mask, whose bytes and count the tests hold equal to the mirror's)"""
        for k in ("raw", "blurred"):
            d = np.abs(got[k].astype(np.int64) - want[k].astype(np.int64))
            self.n[k] += d.size
            self.differing[k] += int((d != 0).sum())
            self.beyond[k] += int((d > 1).sum())
        # a pixel that is NaN in one precision only stores 0 one way and its value the other: counted on its own, and the screen
        # pixels its byte can reach (the blur's 4 x 4 texels, then the read's 2 x 2: five texels each way) are left out of the
        # ao_pixel figure, which would otherwise be 1.0 whatever the code did
        one_way = nan32 != want["nonfinite"]
        self.nan_one_way += int(one_way.sum())
        h, w = one_way.shape
        reach = np.zeros((h, w), bool)
        for y, x in zip(*np.nonzero(one_way)):
            reach[max(y - 5, 0):y + 6, max(x - 5, 0):x + 6] = True
        sh, sw = got["ao_pixel"].shape
        ty = np.minimum((np.arange(sh) + 0.5) * h / sh, h - 1).astype(int)
        tx = np.minimum((np.arange(sw) + 0.5) * w / sw, w - 1).astype(int)
        keep = ~reach[ty[:, None], tx[None, :]]
        err = np.abs(got["ao_pixel"].astype(np.float64) - want["ao_pixel"])[keep]
        self.ao_n += int(keep.sum())
        if err.size:
            self.ao, self.ao_sum = max(self.ao, float(err.max())), self.ao_sum + float(err.sum())

    def figures(self):
        out = dict(bytes=self.n["raw"])
        for k in ("raw", "blurred"):
            out[f"{k}_share_differing"] = self.differing[k] / self.n[k]
            out[f"{k}_share_beyond_1"] = self.beyond[k] / self.n[k]
        out["ao_pixel_max_error"] = self.ao
        out["ao_pixel_mean_error"] = self.ao_sum / max(self.ao_n, 1)
        out["ao_pixels_compared"] = self.ao_n
        out["nan_one_way_pixels"] = self.nan_one_way
        return out


def measure_cases():
    """the mirror against float64 over the whole case matrix -> the figures"""
    import ssao_cases as sc
    import ssao_ref as ref
    from orbit_amd import post

    t = Tally()
    for _, kw in sc.all_cases() + sc.settings_cases():
        t.add(post.host_ssao(**kw), ref.ssao(F=np.float64, **kw), ref.ssao(**kw)["nonfinite"])
    return t.figures()


def measure_scene(oracle):
    """the mirror against float64 over the scene, and its census -> (figures, [census per size and resolution])"""
    import ssao_ref as ref
    from orbit_amd import post

    noise, samples = post.ssao_tables(TABLE_SEED)
    t, census = Tally(), []
    for w, h in SCENE_SIZES:
        f = host_frame(oracle, w, h)
        for full_res in (True, False):
            sw, sh = post.ssao_resolution(w, h, full_res)
            args = (f["depth"], f["projection"], f["inverse_projection"], noise, samples, sw, sh)
            got = post.host_ssao(*args, want_census=True)
            t.add(got, ref.ssao(*args, F=np.float64), ref.ssao(*args)["nonfinite"])
            raw, c, st = got["raw"], got["census"], got["stats"]
            samples_total = c["in_range"] + c["out_of_range"]
            census.append(dict(screen=[w, h], ssao=[sw, sh], covered_pixels=int((f["depth"] != 0).sum()), mean_ao=round(float(got["ao_pixel"].mean()), 4),
                               mean_raw_byte=round(float(raw.mean()), 2), unoccluded_pixels=int(st["unoccluded_pixels"]),
                               nonfinite_pixels=int(st["nonfinite_pixels"]), samples_in_range=int(st["samples_in_range"]),
                               share_in_range=round(c["in_range"] / samples_total, 4), branches=[c[k] for k in post.SSAO_CENSUS[:4]],
                               occluded=c["occluded"], range_inside=c["range_inside"], column_0_mean_byte=round(float(raw[:, 0].mean()), 2),
                               column_1_mean_byte=round(float(raw[:, 1].mean()), 2), row_0_mean_byte=round(float(raw[0].mean()), 2),
                               row_1_mean_byte=round(float(raw[1].mean()), 2)))
    return t.figures(), census


def printed(x):
    """a figure as it is recorded: three significant digits, rounded up; the test holds the mirror at this plus one unit of
    its last digit"""
    if x == 0:
        return "0"
    from decimal import ROUND_CEILING, Decimal

    d = Decimal(repr(float(x)))
    return str(d.quantize(Decimal(1).scaleb(d.adjusted() - 2), rounding=ROUND_CEILING))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from oracle import oracle

    oracle.build()
    cases = measure_cases()
    scene, census = measure_scene(oracle)
    out = dict(against="the GLSL in float64 with the true sin / cos (tests/ssao_ref.py, F = float64)",
               case_matrix=dict(cases, over="tests/ssao_cases.py: all_cases() and settings_cases()"),
               scene=dict(scene, over=f"tools/make_test_glb.py, {INSTANCES} instances, seed 7; tables of seed {TABLE_SEED}; 32 samples, radii 0.1 / 0.5"),
               printed=dict(case_matrix={k: printed(cases[k]) for k in FIGURES}, scene={k: printed(scene[k]) for k in FIGURES}),
               census=census)
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
