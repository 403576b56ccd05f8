#!/usr/bin/env python
"""Times orbit_expand_visible_records on the record lists of two culled scenes (tests/record_lists.py): the dense one
(about 1.8 survivors per record) and the sparse one with keep = 0.05 (77 % of the records empty), each with the command
buffer at the scene's LOD-0 meshlets + 8 and at exactly the list's survivors.  HIP events around every call, `--iters`
calls after `--warmup`; prints ONE JSON line.  `--lib PATH` times another build of the library (the parent commit's, for
profiles/expand_records.md); every process times one build.

    python tools/bench_expand_records.py [--lib PATH] [--iters 30] [--warmup 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()

    import numpy as np
    import torch

    import record_lists as rl
    from oracle import oracle
    from orbit_amd import _lib
    from orbit_amd import layouts as L

    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from orbit_amd.engine import Engine
    from test_gpu_parity import _expected_visible_records, run_oracle

    oracle.build()
    oracle.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    eng = Engine(0)
    out = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "iters": args.iters, "lists": {}}
    for name, scene in (("dense", rl.dense_scene()), ("sparse_keep_0.05", rl.sparse_scene(0.05))):
        ref = run_oracle(oracle, scene, rl.scene_cull_info())
        _, orecs = L.dispatch_buffer_records(ref[0])
        on, ocmds = L.draw_buffer_commands(ref[1])
        case = rl.scene_case(name, _expected_visible_records(orecs, ocmds), len(scene.meshlets))
        rec_d, meshlets_d = dev(case.buffer), dev(scene.meshlets)
        for label, cap in (("capacity_lod0_meshlets", scene.lod0_meshlets + 8), ("capacity_survivors", on)):
            draw = torch.zeros(L.DRAW_HEADER + 28 * cap + 64, dtype=torch.uint8, device="cuda")
            for _ in range(args.warmup):
                eng.expand_visible_records(rec_d, meshlets_d, draw, cap)
            torch.cuda.synchronize()
            us = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.expand_visible_records(rec_d, meshlets_d, draw, cap)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1000.0)
            try:
                eng.status()
                status = "ok"
            except _lib.OrbitError as e:
                status = _lib.ERROR_NAMES.get(e.code, str(e.code))
            n, cmds = L.draw_buffer_commands(draw.cpu().numpy())
            us.sort()
            out["lists"][f"{name}/{label}"] = {
                "records": case.n, "survivors": on, "capacity": cap, "header": n, "status": status,
                "equals_oracle": bool(n == min(on, cap) and np.array_equal(cmds.view(np.uint32), ocmds[:cap].view(np.uint32))),
                "us_median": round(us[len(us) // 2], 2), "us_min": round(us[0], 2), "us_p90": round(us[len(us) * 9 // 10], 2),
            }
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
