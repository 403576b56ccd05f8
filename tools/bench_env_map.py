"""orbit_env_map at the reference's sizes: sky 1024 from a seeded 2048 x 1024 panorama, irradiance 32 at
delta 0.025, prefiltered 512 x 5 at 4 096 samples, the BRDF table 512 (forward.rs:135) at 1 024 samples.  GPU box; prints
one JSON line and writes it to --out.  One process; per call the median, the smallest and the largest of --iters
event-timed calls after --warmup calls: the whole call, then each product alone (irradiance and prefiltered from the sky
cube the whole call left, the table with no cube at all), and orbit_env_sample over 2^22 seeded directions.
  samples_per_s      prefilter samples (texels x sample_count, each at most one trilinear cube fetch of up to 8 texels) per
                     second of the prefiltered product alone; irradiance_taps_per_s alike (texels x trips, one fetch each)
  prefilter_share    the prefiltered product's median over the whole call's
Verification in the same process, or the exit code is 1: at the reduced size of tests/env_map_cases.py CHAINED (sky 16,
irradiance 8, prefiltered 16 x 5 at 64 samples, table 16 at 64) every byte and counter against the host mirror; at full
size the whole sky cube, the whole irradiance cube and the whole table against the mirror run on the device's sky cube
(--no-full-verify skips these three, minutes of host time), and of the prefiltered cube the first, the last and 30 seeded
texels of every level (orbit_host_env_prefilter_texels): the mirror at 8.5e9 fetches is not a test.
Usage: python tools/bench_env_map.py [--iters 20] [--warmup 3] [--out profiles/env_map_mi355x.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed(torch, fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0)
    return dict(median_us=round(float(np.median(out)), 1), min_us=round(min(out), 1), max_us=round(max(out), 1), iters=iters)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-full-verify", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_map_mi355x.json"))
    args = ap.parse_args()
    import torch

    import env_map_cases as ec
    from orbit_amd import env_map as em
    from orbit_amd.engine import Engine

    assert torch.cuda.is_available(), "needs an MI355X"
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    ok = True

    # -- the reduced size: every byte
    _, small = ec.CHAINED
    want = em.host_env_map(**small)
    lay = want["layout"]
    bufs = {k: torch.zeros(int(lay[k + "_texels"]) * (4 if k == "brdf" else 8), dtype=torch.uint8, device="cuda") for k in ("sky", "irradiance", "prefiltered", "brdf")}
    stats = torch.zeros(48, dtype=torch.uint8, device="cuda")
    eh, ew = small["equirect"].shape[:2]
    em.device_env_map(eng, dev(small["equirect"]), bufs["sky"], bufs["irradiance"], bufs["prefiltered"], bufs["brdf"], stats, ew, eh,
                      **{k: v for k, v in small.items() if k != "equirect"})
    torch.cuda.synchronize()
    reduced = {k: bufs[k].cpu().numpy().tobytes() == want[k].tobytes() for k in bufs}
    reduced["stats"] = stats.cpu().numpy().tobytes() == want["stats"].tobytes()
    ok = ok and all(reduced.values())

    # -- the reference's sizes
    R = dict(em.REFERENCE)
    rng = np.random.default_rng(1024)
    pano = (rng.random((1024, 2048, 4)) ** 4 * 16.0).astype(np.float32)
    lay = em.layout(R["sky_size"], R["irradiance_size"], R["prefiltered_size"], R["prefiltered_levels"], R["brdf_size"])
    d_pano = dev(pano)
    bufs = {k: torch.zeros(int(lay[k + "_texels"]) * (4 if k == "brdf" else 8), dtype=torch.uint8, device="cuda") for k in ("sky", "irradiance", "prefiltered", "brdf")}
    stats = torch.zeros(48, dtype=torch.uint8, device="cuda")
    sizes = {k: R[k] for k in ("sky_size", "irradiance_size", "prefiltered_size", "prefiltered_levels", "brdf_size", "sample_count", "sample_delta", "brdf_sample_count")}

    def call(equirect=None, sky=None, irradiance=None, prefiltered=None, brdf=None, with_stats=True):
        keep = dict(sizes)
        if sky is None:
            keep["sky_size"] = 0
        em.device_env_map(eng, equirect, sky, irradiance, prefiltered, brdf, stats if with_stats else None,
                          2048 if equirect is not None else 0, 1024 if equirect is not None else 0, **keep)

    calls = dict(
        whole=lambda: call(d_pano, bufs["sky"], bufs["irradiance"], bufs["prefiltered"], bufs["brdf"]),
        sky=lambda: call(d_pano, bufs["sky"]),
        irradiance=lambda: call(None, bufs["sky"], irradiance=bufs["irradiance"]),
        prefiltered=lambda: call(None, bufs["sky"], prefiltered=bufs["prefiltered"]),
        brdf=lambda: call(brdf=bufs["brdf"]))
    times = {name: timed(torch, fn, args.iters, args.warmup) for name, fn in calls.items()}
    calls["whole"]()
    torch.cuda.synchronize()
    eng.status()
    got = {k: bufs[k].cpu().numpy().view(np.uint16) for k in bufs}
    got_stats = stats.cpu().numpy().copy()

    # -- full size: a stated subset of the prefiltered texels, and the other three products whole
    full = {}
    checked = 0
    pre_ok = True
    for m, (n, first) in enumerate(zip(lay["prefiltered_sizes"], lay["prefiltered_offsets"])):
        texels = np.unique(np.concatenate([[0, 6 * n * n - 1], np.random.default_rng(m).integers(0, 6 * n * n, 30)])).astype(np.uint32)
        mirror = em.host_prefilter_texels(got["sky"], R["sky_size"], R["prefiltered_size"], R["prefiltered_levels"], R["sample_count"], m, texels)
        device = got["prefiltered"].reshape(-1, 4)[first + texels.astype(np.int64)]
        pre_ok = pre_ok and bool(np.array_equal(mirror, device))
        checked += len(texels)
    full["prefiltered_texels_checked"], full["prefiltered_subset_equal"] = checked, pre_ok
    ok = ok and pre_ok
    if not args.no_full_verify:
        host = em.host_env_map(equirect=pano, sky_size=R["sky_size"])
        full["sky_equal"] = host["sky"].tobytes() == got["sky"].tobytes()
        host = em.host_env_map(sky=got["sky"], sky_size=R["sky_size"], irradiance_size=R["irradiance_size"], sample_delta=R["sample_delta"],
                               brdf_size=R["brdf_size"], brdf_sample_count=R["brdf_sample_count"])
        full["irradiance_equal"] = host["irradiance"].tobytes() == got["irradiance"].tobytes()
        full["brdf_equal"] = host["brdf"].tobytes() == got["brdf"].tobytes()
        ok = ok and full["sky_equal"] and full["irradiance_equal"] and full["brdf_equal"]

    # -- the sampler
    n_dirs = 1 << 22
    d = rng.standard_normal((n_dirs, 3)).astype(np.float32)
    lods = (rng.random(n_dirs) * 10.0).astype(np.float32)
    d_d, d_l, d_rgb = dev(d), dev(lods), torch.zeros(n_dirs * 12, dtype=torch.uint8, device="cuda")
    times["sample"] = timed(torch, lambda: em.device_env_sample(eng, bufs["sky"], R["sky_size"], lay["sky_levels"], d_d, d_l, d_rgb, n_dirs),
                            max(args.iters, 10), args.warmup)
    head = 4096
    mirror = em.host_env_sample(got["sky"], R["sky_size"], lay["sky_levels"], d[:head], lods[:head])
    full["sample_head_equal"] = d_rgb.cpu().numpy()[:head * 12].tobytes() == mirror["rgb"].tobytes()
    ok = ok and full["sample_head_equal"]
    eng.close()

    pre_samples = lay["prefiltered_texels"] * R["sample_count"]
    trips = lambda limit: int(np.ceil(limit / R["sample_delta"]))  # noqa: E731  (252 x 63 at 0.025)
    irr_taps = lay["irradiance_texels"] * trips(2 * np.pi) * trips(0.5 * np.pi)
    out = {"device": torch.cuda.get_device_name(0), "sizes": sizes, "panorama": "2048 x 1024, seeded", "times": times,
           "prefilter_share": round(times["prefiltered"]["median_us"] / times["whole"]["median_us"], 4),
           "prefilter_samples": int(pre_samples), "samples_per_s": round(pre_samples / (times["prefiltered"]["median_us"] * 1e-6), 0),
           "irradiance_taps": int(irr_taps), "irradiance_taps_per_s": round(irr_taps / (times["irradiance"]["median_us"] * 1e-6), 0),
           "sample_directions": n_dirs, "sample_directions_per_s": round(n_dirs / (times["sample"]["median_us"] * 1e-6), 0),
           "stats_full": {k: int(v) for k, v in zip(("sky_nonfinite", "irradiance_nonfinite", "prefiltered_nonfinite", "brdf_nonfinite", "bad_directions"),
                                                     got_stats.view(np.uint64))},
           "reduced_size_equal": reduced, "reduced_size": "tests/env_map_cases.py CHAINED: sky 16, irradiance 8 at 0.25, prefiltered 16 x 5 at 64 samples, table 16 at 64",
           "full_size": full, "forms_built": "one: fold-over-the-edge taps, LDS-staged sample table in chunks of 256; no bordered copy, no second form to compare",
           "device_equals_host": bool(ok)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
