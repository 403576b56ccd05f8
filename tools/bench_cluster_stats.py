"""orbit_cluster_stats on BASELINE config 4 (1920x1080 depth, 240 x 135 x 32 clusters, 10 000 point lights) and on the
regime scene of tests/test_cluster_regimes_gpu.py.  GPU box; prints one JSON line:

  c4_stats_us, regime_stats_us   device time of one orbit_cluster_stats call (the counter clear + the one launch):
                                 median of `iters` event-timed calls after warm-up
  c4_chain_us, regime_chain_us   orbit_compute_clusters on the same arguments, timed the same way
  c4_stats, regime_stats         the counters (engine.cluster_stats_dict), checked against the chain's headers
                                 (compaction = active_clusters, light_count = light_indices) and the invariants
Run it under `rocprofv3 --kernel-trace --stats` for the kernel table (profiles/cluster_stats_kernel_stats.csv).
Usage: python tools/bench_cluster_stats.py [--iters 30]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from orbit_amd import layouts as L  # noqa: E402


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


def _measure(torch, push, info, depth, lights, iters):
    from orbit_amd.engine import Engine, cluster_stats_dict

    cc = [int(v) for v in push["cluster_count"]]
    total = cc[0] * cc[1] * cc[2]
    eng = Engine(0, max_clusters=total, max_lights=max(len(lights), 1))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d, lt = up(depth), up(lights)
    stats = torch.zeros(256, dtype=torch.uint8, device="cuda")
    masks = torch.zeros(cc[0] * cc[1], dtype=torch.int32, device="cuda")
    bounds = torch.zeros(total * 2, dtype=torch.int32, device="cuda")
    unique = torch.zeros(L.COMPACT_HEADER + 4 * total, dtype=torch.uint8, device="cuda")
    lcap = 32 * total  # generous: the chain must not latch here
    lists = torch.zeros(L.LIGHT_INDEX_HEADER + 4 * lcap, dtype=torch.uint8, device="cuda")
    image = torch.zeros(total * 2, dtype=torch.int32, device="cuda")

    def call():
        eng.cluster_stats(stats, push, info, d, lt)

    def chain():
        eng.compute_clusters(push, info, d, lt, masks, bounds, unique, total, lists, lcap, image)

    for _ in range(5):
        call()
        chain()
    torch.cuda.synchronize()
    eng.status()
    s = cluster_stats_dict(stats)
    n_active, n_indices = int(unique[12:16].view(torch.int32).item()), int(lists[:4].view(torch.int32).item())
    ok = (s["active_clusters"] == n_active and s["light_indices"] == n_indices
          and s["samples"] == s["samples_outside_grid"] + sum(s["samples_by_lights"])
          and s["active_clusters"] == sum(s["clusters_by_lights"])
          and (s["light_refs"] == s["light_indices"]) == (s["clusters_by_lights"][4] == 0))
    stats_us = _timed(torch, call, iters)
    chain_us = _timed(torch, chain, iters)
    torch.cuda.synchronize()
    eng.status()
    eng.close()
    return stats_us, chain_us, s, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster_stats.py needs an MI355X")
    import config_scenes as cs
    from oracle import oracle
    from test_cluster_regimes_gpu import regime_scene

    oracle.build()
    cam = cs.camera()
    push, info, lights = cs.config4_inputs(oracle, cam)
    us4, chain4, s4, ok4 = _measure(torch, push, info, cs.config3_depth(cam), lights, args.iters)
    rpush, rdepth, rinfo, rlights, _, _, n_lights, _ = regime_scene(oracle, 3)
    usr, chainr, sr, okr = _measure(torch, rpush, rinfo, rdepth, rlights[:n_lights], args.iters)
    line = dict(c4_stats_us=round(us4, 1), c4_chain_us=round(chain4, 1), c4_target_us=150.0, c4_stats=s4,
                regime_stats_us=round(usr, 1), regime_chain_us=round(chainr, 1), regime_stats=sr,
                counters_match_the_chain=bool(ok4 and okr), device=torch.cuda.get_device_name(0))
    print(json.dumps(line))
    if not (ok4 and okr):
        raise SystemExit("the counters disagree with the chain")


if __name__ == "__main__":
    main()
