"""orbit_scene_update_entities on the headline scene's entity count.  GPU box; prints one JSON line:

  n                        entities (default 195 313: the headline scene's)
  dense_us, sparse_us      device time of the dense update and of a 1 % sparse scatter: median of 30 event-timed launches
                           after warm-up
  dense_bytes, sparse_bytes  bytes the launch must move (40 B in + 128 B out per row; the sparse form also reads a 4-B
                           index) and dense/sparse_hbm_fraction: those bytes over 8 TB/s, divided by the measured time
  host_update_scene_ms     the host mirror's SceneData::update_scene over the same entities on this box (median of 5,
                           steady state: visibility ranges allocated)
  h2d_128B_us, h2d_40B_us  pinned-memory upload of 128 B x n (what update_scene's caller uploads) and of 40 B x n (what
                           the device update needs): median of 30 event-timed copies
Usage: python tools/bench_scene_update.py [--n N] [--iters 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orbit_amd import layouts as L  # noqa: E402
from orbit_amd import scene as S  # noqa: E402

HBM_PEAK = 8.0e12


def _timed(torch, fn, iters):
    """Median device time of `fn`'s work between two events, in µs.  A sleep kernel keeps the stream busy while the
    host enqueues every (event, work, event) triple, so the pairs bracket the work and not the host's enqueue."""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda._sleep(50_000_000)
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) * 1e3 for a, b in evs]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=195_313)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_update.py needs an MI355X")
    from orbit_amd.engine import Engine

    n, iters = args.n, args.iters
    rng = np.random.default_rng(1)
    t = np.zeros(n, dtype=L.ENTITY_TRANSFORM)
    t["position"] = rng.uniform(-500, 500, (n, 3))
    q = rng.normal(size=(n, 4))
    t["orientation"] = q / np.linalg.norm(q, axis=1, keepdims=True)
    t["scale"] = rng.uniform(0.5, 2.0, (n, 3))
    m = max(1, n // 100)
    idx = np.sort(rng.choice(n, m, replace=False)).astype(np.uint32)

    # host mirror: update_scene over the same entities
    sd = S.SceneData()
    for r in t:
        sd.add_entity(position=r["position"], orientation=r["orientation"], scale=r["scale"], mesh=0)
    mesh_infos = np.zeros(1, dtype=L.MESH_INFO)
    mesh_infos["lod_count"] = 1
    mesh_infos["mesh_lods"][0, 0] = (0, 1)
    sd.update_scene(mesh_infos)  # allocates the visibility ranges
    host_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        sd.update_scene(mesh_infos)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    want = sd.entity_data_cache()

    dev = torch.device("cuda", 0)
    eng = Engine(0)
    src = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
    sparse_src = torch.from_numpy(t[idx].view(np.uint8).copy()).to(dev)
    sparse_idx = torch.from_numpy(idx.view(np.int32).copy()).to(dev)
    out = torch.zeros(128 * n, dtype=torch.uint8, device=dev)

    def dense():
        eng.scene_update_entities(src, out, count=n, entity_capacity=n)

    def sparse():
        eng.scene_update_entities(sparse_src, out, count=m, instance_indices=sparse_idx, entity_capacity=n)

    for _ in range(10):
        dense()
        sparse()
    torch.cuda.synchronize()
    eng.status()
    dense_us = _timed(torch, dense, iters)
    sparse_us = _timed(torch, sparse, iters)
    torch.cuda.synchronize()
    eng.status()
    exact = out.cpu().numpy().tobytes() == want.tobytes()

    pin128 = torch.empty(128 * n, dtype=torch.uint8).pin_memory()
    pin40 = torch.empty(40 * n, dtype=torch.uint8).pin_memory()
    dst = torch.empty(128 * n, dtype=torch.uint8, device=dev)
    for _ in range(5):
        dst.copy_(pin128, non_blocking=True)
    h2d128 = _timed(torch, lambda: dst.copy_(pin128, non_blocking=True), iters)
    h2d40 = _timed(torch, lambda: dst[:40 * n].copy_(pin40, non_blocking=True), iters)
    eng.close()

    dense_bytes, sparse_bytes = 168 * n, 172 * m
    line = dict(n=n, sparse_rows=m, dense_us=round(dense_us, 2), sparse_us=round(sparse_us, 2),
                dense_bytes=dense_bytes, sparse_bytes=sparse_bytes,
                dense_hbm_fraction=round(dense_bytes / HBM_PEAK / (dense_us * 1e-6), 3),
                sparse_hbm_fraction=round(sparse_bytes / HBM_PEAK / (sparse_us * 1e-6), 3),
                host_update_scene_ms=round(float(np.median(host_ms)), 2),
                h2d_128B_us=round(h2d128, 1), h2d_40B_us=round(h2d40, 1), bit_exact_vs_host=exact,
                device=torch.cuda.get_device_name(0))
    print(json.dumps(line))
    if not exact:
        raise SystemExit("device rows differ from the host mirror's update_scene")


if __name__ == "__main__":
    main()
