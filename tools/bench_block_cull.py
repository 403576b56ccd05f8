"""In-process alternating on / off of the per-block pass-0 evaluation (orbit_ctx_set_block_cull): the same config-5 frame
through ONE engine and ONE stream with the path on and off in turn, HIP-event medians of the whole frame and of the
evaluation launch.  Process-to-process and box-to-box spread never enters the comparison.  Both draw lists must agree.
usage: python tools/bench_block_cull.py [--entities N] [--scene-shape scattered|coherent] [--camera x,y,z] [--reps R]
Prints one JSON line.  The camera at 0,0,0 sits inside the scene: most rows there are dense, and the path must not be
slower than off beyond the spread (ORBIT_BLK_RATIO in block_pretest.h is what decides it)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from orbit_amd import camera, layouts as L, synth
from orbit_amd.engine import Engine

ap = argparse.ArgumentParser()
ap.add_argument("--entities", type=int, default=195_313)
ap.add_argument("--scene-shape", choices=("scattered", "coherent"), default="scattered")
ap.add_argument("--camera", default="0,0,1300")
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()

dev = torch.device("cuda", 0)
spec = synth.C5Spec(entities=args.entities)
E, M = spec.entities, spec.meshlets_per_entity
draws, mesh, ent, half = synth.gen_entity_tables(spec, dev)
meshlets = synth.gen_meshlets(spec, 0, E, dev, half, shape=args.scene_shape)
materials = synth.gen_materials(spec, dev)
ci = camera.frame_cull_info(tuple(float(v) for v in args.camera.split(",")))
disp_cap, draw_cap = E * spec.records_per_entity + 8, E * M // 2 + 1024
disp = torch.zeros(L.DISPATCH_HEADER + 16 * disp_cap, dtype=torch.uint8, device=dev)
draw = torch.zeros(L.DRAW_HEADER + 28 * draw_cap, dtype=torch.uint8, device=dev)
eng = Engine(0, max_entities=E + 256, max_dispatches=disp_cap, max_draws=draw_cap)
ms = eng.meshlet_stream(meshlets, 0, E * M)
ms.set_materials(materials, spec.materials)
eng.bind_meshlet_stream(ms)
torch.cuda.synchronize()


def frame():
    eng.entity_cull(ci, draws, mesh, disp, ent, E, disp_cap)
    eng.meshlet_cull(ci, disp, meshlets, draw, ent, materials, disp_cap, draw_cap, material_count=spec.materials)


lists = []
for on in (True, False):
    eng.set_block_cull(on)
    before = eng.block_culls()
    for _ in range(3):
        frame()
    torch.cuda.synchronize()
    eng.status()
    assert eng.block_culls() - before == (3 if on else 0)
    n = int(draw[:4].view(torch.int32).item())
    lists.append(draw[:4 + 28 * n].clone())
assert torch.equal(lists[0], lists[1]), "on and off disagree on the draw list"
records = int(disp[:4].view(torch.int32).item())

tf, te = {True: [], False: []}, {True: [], False: []}
eng.profile(True)
for r in range(args.reps):
    for on in (True, False) if r % 2 == 0 else (False, True):
        eng.set_block_cull(on)
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        frame()
        z.record()
        torch.cuda.synchronize()
        tf[on].append(a.elapsed_time(z))
        t, _ = eng.profile_read()
        te[on].append(t)
        eng.profile(True)


def stats(v):
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}


print(json.dumps({"entities": E, "scene_shape": args.scene_shape, "camera": args.camera, "records": records,
                  "survivors": int(lists[0].numel() - 4) // 28, "reps": args.reps,
                  "frame_ms": {"on": stats(tf[True]), "off": stats(tf[False])},
                  "eval_ms": {"on": stats(te[True]), "off": stats(te[False])}}))
