"""orbit_meshlet_bounds on a synthetic mesh of about a million meshlets.  GPU box; prints one JSON line.

Two meshes, each with 32-B vertices (position at byte 8) and 64 vertex slots per meshlet:
  full     every meshlet a closed band of 64 vertices and 64 triangles (the reference's limits, mesh.rs:8-9)
  ragged   every meshlet an open strip of 8..64 vertices and vertex_count - 2 triangles
and for each the range form over all meshlets and an index list of a random 10 % of them:
  *_us             device time of one call, median of `iters` event-timed calls after warm-up
  *_mmeshlets_s    millions of meshlets per second
  *_bytes          algorithmic bytes: per meshlet 32 (record) + 4 per data word + 12 per gathered position
  *_hbm_fraction   their rate as a share of the HBM peak
  host_1t_ms, host_16t_ms   the host export (orbit_host_meshlet_bounds) on the same job, on one thread and cut over 16
  chunked_meshlets          meshlets of more than 64 triangles (they loop over chunks of 64); wide_cone_exits: mindp <= 0.1
  mean / max_sphere_updates rounds of the growth loop per meshlet (both Ritter spheres), counted by the host export
  checked          rows of the device's result compared with the host's, bit for bit (all of them)
Usage: python tools/bench_meshlet_bounds.py [--meshlets 1048576] [--iters 20]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from orbit_amd import assets  # noqa: E402
from orbit_amd import layouts as L  # noqa: E402

HBM_PEAK = 8.0e12
SLOT, STRIDE, OFFSET = 64, 32, 8
SLOT_WORDS = SLOT + 48  # vertex indices + the corners of up to 64 triangles


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


def make_mesh(torch, m, ragged, seed):
    """-> (records np[MESHLET], meshlet_data np.uint32, vertices: device float32 [m * 64, 8])."""
    rng = np.random.default_rng(seed)
    nv = rng.integers(8, SLOT + 1, m).astype(np.uint32) if ragged else np.full(m, SLOT, np.uint32)
    nt = nv - 2 if ragged else nv
    rec = np.zeros(m, L.MESHLET)
    rec["vertex_offset"] = np.arange(m, dtype=np.uint32) * SLOT
    rec["data_offset"] = np.arange(m, dtype=np.uint32) * SLOT_WORDS
    rec["vertex_count"], rec["triangle_count"] = nv, nt
    t = np.arange(SLOT)
    tri = np.stack([np.where(t % 2 == 0, t, t + 1), np.where(t % 2 == 0, t + 1, t), t + 2], axis=1)
    data = np.zeros((m, SLOT_WORDS), np.uint32)
    for v in np.unique(nv):  # the corners start right behind the meshlet's own vertex indices
        rows = np.nonzero(nv == v)[0]
        n_tri = int(v) - 2 if ragged else int(v)
        corners = np.zeros(((3 * n_tri + 3) // 4) * 4, np.uint8)
        corners[:3 * n_tri] = (tri[:n_tri] % v).reshape(-1)
        data[rows[:, None], np.arange(v)[None, :]] = np.arange(v, dtype=np.uint32)
        data[rows[:, None], (v + np.arange(len(corners) // 4))[None, :]] = corners.view(np.uint32)
    # a band around a slightly conical tube, in strip order; every meshlet has its own place, size and bend
    g = torch.Generator(device="cuda").manual_seed(seed)
    i = torch.arange(SLOT, device="cuda")
    a = (i // 2).float() * (2 * np.pi / 32) * (0.2 if ragged else 1.0)
    z = (i % 2).float()
    scale = torch.rand((m, 1), device="cuda", generator=g) * 2 + 0.5
    bend = torch.rand((m, 1), device="cuda", generator=g) * 0.3 + 1.0
    centre = (torch.rand((m, 1, 3), device="cuda", generator=g) - 0.5) * 2000
    p = torch.stack([torch.cos(a)[None, :] * scale * (1 + (bend - 1) * z[None, :]), torch.sin(a)[None, :] * scale,
                     z[None, :] * scale * bend], dim=2) + centre
    vertices = torch.zeros((m * SLOT, STRIDE // 4), dtype=torch.float32, device="cuda")
    vertices[:, OFFSET // 4:OFFSET // 4 + 3] = p.reshape(-1, 3)
    return rec, data.reshape(-1), vertices, nv, nt


def host_ms(rec, data, vb, vertex_count, threads):
    m = len(rec)
    cuts = np.linspace(0, m, threads + 1).astype(int)

    def part(k):
        full, _, updates = assets.meshlet_bounds(rec, data, vb, vertex_count, STRIDE, OFFSET, first=int(cuts[k]),
                                                 count=int(cuts[k + 1] - cuts[k]))
        return full, updates

    t0 = time.perf_counter()
    if threads == 1:
        parts = [part(0)]
    else:
        with ThreadPoolExecutor(threads) as ex:  # ctypes releases the GIL for the length of the call
            parts = list(ex.map(part, range(threads)))
    return (time.perf_counter() - t0) * 1e3, np.concatenate([f for f, _ in parts]), np.concatenate([u for _, u in parts])


def measure(torch, eng, m, ragged, iters):
    rec, data, vertices, nv, nt = make_mesh(torch, m, ragged, 7 + ragged)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_rec, d_data = up(rec), up(data)
    d_full = torch.zeros(48 * m, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(1)
    sel = rng.permutation(m)[:m // 10].astype(np.uint32)
    d_sel = up(sel)
    vcount = m * SLOT

    def whole():
        eng.meshlet_bounds(d_rec, d_data, vertices, vcount, STRIDE, OFFSET, meshlet_count=m)

    def listed():
        eng.meshlet_bounds(d_rec, d_data, vertices, vcount, STRIDE, OFFSET, meshlet_indices=d_sel)

    for _ in range(3):
        whole()
        listed()
    eng.meshlet_bounds(d_rec, d_data, vertices, vcount, STRIDE, OFFSET, meshlet_count=m, full=d_full)
    torch.cuda.synchronize()
    eng.status()
    whole_us, list_us = _timed(torch, whole, iters), _timed(torch, listed, iters)
    per = 32 + 4 * (nv + (3 * nt + 3) // 4).astype(np.int64) + 12 * nv.astype(np.int64)
    vb = vertices.cpu().numpy()
    h1, want, updates = host_ms(rec, data, vb, vcount, 1)
    h16, want16, _ = host_ms(rec, data, vb, vcount, 16)
    got = d_full.cpu().numpy().view(L.MESHLET_BOUNDS_FULL)
    same = got.tobytes() == want.tobytes() == want16.tobytes()
    name = "ragged" if ragged else "full"
    wide = int(((want["cone_cutoff_s8"] == 127) & (want["cone_cutoff"] == 1)).sum())
    return same, {
        f"{name}_range_us": round(whole_us, 1), f"{name}_range_mmeshlets_s": round(m / whole_us, 1),
        f"{name}_range_bytes": int(per.sum()), f"{name}_range_hbm_fraction": round(per.sum() / (whole_us * 1e-6) / HBM_PEAK, 4),
        f"{name}_list_us": round(list_us, 1), f"{name}_list_mmeshlets_s": round(len(sel) / list_us, 1),
        f"{name}_list_bytes": int(per[sel].sum()), f"{name}_list_hbm_fraction": round(per[sel].sum() / (list_us * 1e-6) / HBM_PEAK, 4),
        f"{name}_host_1t_ms": round(h1, 1), f"{name}_host_16t_ms": round(h16, 1),
        f"{name}_chunked_meshlets": int((nt > 64).sum()), f"{name}_wide_cone_exits": wide,
        f"{name}_mean_sphere_updates": round(float(updates.mean()), 2), f"{name}_max_sphere_updates": int(updates.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshlets", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_meshlet_bounds.py needs an MI355X")
    from orbit_amd.engine import Engine

    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)
    line = dict(meshlets=args.meshlets, vertex_stride=STRIDE, device=torch.cuda.get_device_name(0))
    ok = True
    for ragged in (0, 1):
        same, part = measure(torch, eng, args.meshlets, ragged, args.iters)
        ok = ok and same
        line.update(part)
    line["checked"] = args.meshlets * 2
    line["device_equals_host"] = bool(ok)
    eng.close()
    print(json.dumps(line))
    if not ok:
        raise SystemExit("the device's bounds differ from the host export's")


if __name__ == "__main__":
    main()
