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

--full measures orbit_scene_update instead (the whole of update_scene on the device) on the same entity count: 90 % of
the entities with a mesh, 2 000 lights, 8 shadow casters.  One JSON line, also written to --out if given:

  full_us                  (a) device time between events around the call's two launches (median of --iters)
  dense_us, dense_tbps     (b) the dense orbit_scene_update_entities over the drawn entities in the same process, and the
                           bandwidth its 168 B per row reach: the yardstick
  full_bytes               88 B read per entity + 140 B written per drawn entity + 64 B per light
  full_us_at_dense_bw, full_over_dense_bw   those bytes at (b)'s bandwidth, and (a) over that; target_met: <= 1.5
  host_deferred_ms, h2d_us, parent_path_us  (c) what the same buffers cost without the call: the host mirror's
                           update_scene_deferred, the pinned upload of transforms, draws and lights, the dense kernel
  bit_exact_vs_host        every output equals the host mirror's update_scene
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


def full(torch, n, iters, out_path):
    from orbit_amd.engine import Engine

    rng = np.random.default_rng(1)
    t = np.zeros(n, dtype=L.ENTITY_TRANSFORM)
    t["position"] = rng.uniform(-500, 500, (n, 3))
    q = rng.normal(size=(n, 4))
    t["orientation"] = q / np.linalg.norm(q, axis=1, keepdims=True)
    t["scale"] = rng.uniform(0.5, 2.0, (n, 3))
    tab = np.zeros(n, dtype=L.SCENE_ENTITY)
    tab["mesh_index"] = np.where(rng.random(n) < 0.9, 0, L.NONE)
    tab["light_kind"] = L.NONE
    lit = np.sort(rng.choice(n, min(2000, n), replace=False))
    tab["light_kind"][lit] = S.POINT
    tab["light_kind"][lit[:: max(1, len(lit) // 8)][:8]] = S.DIRECTIONAL
    tab["light_flags"][tab["light_kind"] == S.DIRECTIONAL] = 1
    tab["light_color"][lit] = rng.uniform(0, 1, (len(lit), 3))
    tab["light_intensity"][lit] = rng.uniform(1, 50, len(lit))
    tab["light_param"][lit] = 0.5
    mesh_infos = np.zeros(1, dtype=L.MESH_INFO)
    mesh_infos["lod_count"] = 1
    mesh_infos["mesh_lods"][0, 0] = (0, 1)
    sd = S.SceneData()
    sd.add_entities(tab, t)
    sd.update_scene_device(mesh_infos)  # allocates the visibility ranges
    tab = sd.entity_table()
    host_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        sd.update_scene_deferred(mesh_infos)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    ordered = sd.transform_cache()
    sd.update_scene(mesh_infos)
    rows, draws, lights = sd.entity_data_cache(), sd.entity_draw_buffer_bytes(), sd.light_data_cache()
    nd, nl, ns = len(rows), len(lights), sd.shadow_command_count()

    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    eng = Engine(0, max_entities=n)
    d_tab, d_t, d_ordered = up(tab), up(t), up(ordered)
    o_rows = torch.zeros(128 * n, dtype=torch.uint8, device=dev)
    o_draws = torch.zeros(4 + 12 * n, dtype=torch.uint8, device=dev)
    o_lights = torch.zeros(64 * 2048, dtype=torch.uint8, device=dev)
    o_shadows = torch.zeros(16 * 256, dtype=torch.uint8, device=dev)
    o_counts = torch.zeros(16, dtype=torch.uint8, device=dev)
    o_dense = torch.zeros(128 * n, dtype=torch.uint8, device=dev)

    def update():
        eng.scene_update(d_tab, d_t, o_rows, o_draws, o_lights, entity_count=n, shadow_orientations=o_shadows,
                         counts=o_counts)

    def dense():
        eng.scene_update_entities(d_ordered, o_dense, count=nd, entity_capacity=n)

    for _ in range(10):
        update()
        dense()
    torch.cuda.synchronize()
    eng.status()
    full_us = _timed(torch, update, iters)
    dense_us = _timed(torch, dense, iters)
    torch.cuda.synchronize()
    eng.status()
    counts = o_counts.cpu().numpy().view(np.uint32)
    exact = (counts.tolist() == [nd, nl, ns, n] and o_rows.cpu().numpy()[:128 * nd].tobytes() == rows.tobytes()
             and o_draws.cpu().numpy()[:4 + 12 * nd].tobytes() == draws.tobytes()
             and o_lights.cpu().numpy()[:64 * nl].tobytes() == lights.tobytes()
             and o_shadows.cpu().numpy()[:16 * ns].tobytes() == sd.shadow_orientations().tobytes()
             and o_dense.cpu().numpy()[:128 * nd].tobytes() == rows.tobytes())

    # (c) the uploads the parent's path needs: instance-ordered transforms, the draw buffer, the light rows
    pins = [torch.empty(k, dtype=torch.uint8).pin_memory() for k in (40 * nd, 4 + 12 * nd, 64 * nl)]
    dsts = [torch.empty(k, dtype=torch.uint8, device=dev) for k in (40 * nd, 4 + 12 * nd, 64 * nl)]

    def uploads():
        for d, p in zip(dsts, pins):
            d.copy_(p, non_blocking=True)

    for _ in range(5):
        uploads()
    h2d_us = _timed(torch, uploads, iters)
    eng.close()

    full_bytes, dense_bytes = 88 * n + 140 * nd + 64 * nl, 168 * nd
    dense_bw = dense_bytes / (dense_us * 1e-6)
    at_bw = full_bytes / dense_bw * 1e6
    host_ms = float(np.median(host_ms))
    line = dict(mode="full", n=n, draws=nd, lights=nl, shadows=ns, launches=2, full_us=round(full_us, 2),
                dense_us=round(dense_us, 2), dense_bytes=dense_bytes, dense_tbps=round(dense_bw / 1e12, 3),
                full_bytes=full_bytes, full_tbps=round(full_bytes / (full_us * 1e-6) / 1e12, 3),
                full_us_at_dense_bw=round(at_bw, 2), full_over_dense_bw=round(full_us / at_bw, 3),
                target_met=bool(full_us <= 1.5 * at_bw), host_deferred_ms=round(host_ms, 2), h2d_us=round(h2d_us, 1),
                parent_path_us=round(host_ms * 1e3 + h2d_us + dense_us, 1), bit_exact_vs_host=bool(exact),
                device=torch.cuda.get_device_name(0))
    print(json.dumps(line))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(json.dumps(line) + "\n")
    if not exact:
        raise SystemExit("device buffers differ from the host mirror's update_scene")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=195_313)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--full", action="store_true", help="measure orbit_scene_update (see the module docstring)")
    ap.add_argument("--out", default=None, help="--full: also write the JSON line to this file")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_update.py needs an MI355X")
    if args.full:
        return full(torch, args.n, args.iters, args.out)
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
