"""orbit_cull_stats on BASELINE config 5 (195 313 entities x 256 meshlets, 32-B Meshlet buffer: 1.6 GB) and config 2
(DESIGN.md §4.9).  GPU box; prints one JSON line:

  c5_stats_us, c2_stats_us   device time of one orbit_cull_stats call (the counter clear + the one launch): median of
                             `iters` event-timed calls after warm-up
  c5_cull_us, c2_cull_us     entity_cull + meshlet_cull of the same arguments, timed the same way (the scale it sits next to)
  c5_meshlet_bytes           bytes of 32-B meshlet rows the call streams, and c5_hbm_fraction: those over 8 TB/s / time
  c5_stats, c2_stats         the counters (engine.cull_stats_dict), checked against the cull: records = the dispatch count,
                             meshlet_drawn = the command count, the class sums = the totals
Run it under `rocprofv3 --kernel-trace --stats` for the kernel table (profiles/cull_stats_kernel_stats.csv).
Usage: python tools/bench_cull_stats.py [--iters 30] [--entities 195313]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from orbit_amd import layouts as L  # noqa: E402

HBM_PEAK = 8.0e12


def _timed(torch, fn, iters):
    """Median device time of `fn`'s work between two events, in µs (a sleep kernel keeps the stream busy while the host
    enqueues every (event, work, event) triple, so the pairs bracket the work and not the host's enqueue)."""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda._sleep(50_000_000)
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) * 1e3 for a, b in evs]))


def _measure(torch, eng, ci, draws, mesh, ent, n, meshlets, materials, n_materials, disp_cap, draw_cap, iters):
    from orbit_amd.engine import cull_stats_dict

    stats = torch.zeros(256, dtype=torch.uint8, device="cuda")
    disp = torch.zeros(L.DISPATCH_HEADER + 16 * disp_cap, dtype=torch.uint8, device="cuda")
    draw = torch.zeros(L.DRAW_HEADER + 28 * draw_cap, dtype=torch.uint8, device="cuda")

    def call():
        eng.cull_stats(stats, ci, draws, mesh, disp, ent, n, disp_cap, meshlets, draw, materials, draw_cap,
                       material_count=n_materials)

    def cull():
        eng.entity_cull(ci, draws, mesh, disp, ent, n, disp_cap)
        eng.meshlet_cull(ci, disp, meshlets, draw, ent, materials, disp_cap, draw_cap, material_count=n_materials)

    for _ in range(5):
        call()
        cull()
    torch.cuda.synchronize()
    eng.status()
    s = cull_stats_dict(stats)
    nrec, ncmd = int(disp[:4].view(torch.int32).item()), int(draw[:4].view(torch.int32).item())
    ok = (s["records"] == nrec and s["meshlet_drawn"] == ncmd
          and s["entities"] == sum(s[k] for k in L.CULL_STATS_ENTITY[1:])
          and s["meshlets"] == sum(s[k] for k in L.CULL_STATS_MESHLET[1:]))
    stats_us = _timed(torch, call, iters)
    cull_us = _timed(torch, cull, iters)
    torch.cuda.synchronize()
    eng.status()
    return stats_us, cull_us, s, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--entities", type=int, default=195_313)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_cull_stats.py needs an MI355X")
    import config_scenes as cs
    import scenes as sc
    from orbit_amd import synth
    from orbit_amd.engine import Engine

    dev = torch.device("cuda", 0)
    line = {}
    # config 5: the headline scene, every entity in the frustum, ~10 % of the meshlets survive the cone
    spec = synth.C5Spec(entities=args.entities)
    E, M = spec.entities, spec.meshlets_per_entity
    draws, mesh, ent, half = synth.gen_entity_tables(spec, dev)
    meshlets = synth.gen_meshlets(spec, 0, E, dev, half, survive_target=0.095)
    materials = synth.gen_materials(spec, dev)
    disp_cap, draw_cap = E * spec.records_per_entity + 8, E * M // 2 + 1024
    eng = Engine(0, max_entities=E + 256, max_dispatches=disp_cap, max_draws=draw_cap)
    cam = sc.default_camera(position=(0.0, 0.0, 1300.0))
    ci = sc.make_cull_info(cam.view, cam.planes[:5], alpha_mode_flag=L.ALPHA_ALL)
    us, cull_us, s, ok5 = _measure(torch, eng, ci, draws, mesh, ent, E, meshlets, materials, spec.materials, disp_cap,
                                   draw_cap, args.iters)
    eng.close()
    del meshlets
    torch.cuda.empty_cache()
    nbytes = 32 * s["meshlets"]
    line.update(c5_entities=E, c5_meshlets=s["meshlets"], c5_stats_us=round(us, 1), c5_cull_us=round(cull_us, 1),
                c5_meshlet_bytes=nbytes, c5_hbm_fraction=round(nbytes / HBM_PEAK / (us * 1e-6), 3),
                c5_target_us=450.0, c5_stats=s)
    # config 2 (Sponza-class stand-in, tools/bench_configs.py): one launch at launch latency
    s2 = cs.config2_scene()
    cam2 = sc.default_camera()
    ci2 = cs.pass0_cull_info(cam2)
    g = {k: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
         for k, a in (("draws", s2.entity_draw_buffer()), ("mesh", s2.mesh_infos), ("ent", s2.entities),
                      ("meshlets", s2.meshlets), ("materials", s2.materials))}
    cap_d, cap_c = s2.max_dispatches() + 8, s2.lod0_meshlets + 8
    eng = Engine(0, max_entities=4096, max_dispatches=cap_d, max_draws=cap_c)
    us2, cull2, st2, ok2 = _measure(torch, eng, ci2, g["draws"], g["mesh"], g["ent"], s2.entity_draw_count, g["meshlets"],
                                    g["materials"], len(s2.materials), cap_d, cap_c, args.iters)
    eng.close()
    line.update(c2_entities=s2.entity_draw_count, c2_meshlets=st2["meshlets"], c2_stats_us=round(us2, 1),
                c2_cull_us=round(cull2, 1), c2_stats=st2, counters_match_the_cull=bool(ok5 and ok2),
                device=torch.cuda.get_device_name(0))
    print(json.dumps(line))
    if not (ok5 and ok2):
        raise SystemExit("the counters disagree with the cull")


if __name__ == "__main__":
    main()
