"""The per-block pre-test's candidate share at bench.py's OWN geometry, on the host (no GPU): C5Spec(entities=195_313),
camera (0, 0, 1300), 600 entities each from the start, the middle and the end of the scene through
orbit_host_block_pretest.  The cells of the full-size lattice are 4.6 times smaller than those of the 2 000-entity scene of
test_block_pretest_cpu.py, and so is the share of lanes the pre-test leaves open: what the end-of-tile flush of
meshlet_eval_blocks.hip works on is measured here, per tile of 16 records."""
import numpy as np
import pytest

from orbit_amd import layouts as L
from test_block_pretest_cpu import F, PER, pretest

SAMPLE = 600
TILE = 16  # records


def test_candidate_share_at_the_benchmarks_geometry():
    torch = pytest.importorskip("torch")
    from orbit_amd import camera, synth

    dev = torch.device("cpu")
    spec = synth.C5Spec(entities=195_313)
    _, _, ent, half = synth.gen_entity_tables(spec, dev)
    e = ent.numpy().view(np.uint8).reshape(-1).view(L.ENTITY_DATA)
    ci = np.frombuffer(bytes(camera.frame_cull_info((0.0, 0.0, 1300.0))), dtype=L.GPU_CULL_INFO)[0]
    view = ci["view_matrix"].reshape(4, 4).T.astype(F)
    planes = ci["cull_planes"][:int(ci["cull_plane_count"])]
    per_entity = spec.meshlets_per_entity // PER
    assert spec.meshlets_per_entity % PER == 0 and (SAMPLE * per_entity) % TILE == 0
    shares = []
    for name, first in (("start", 0), ("middle", (spec.entities - SAMPLE) // 2), ("end", spec.entities - SAMPLE)):
        ml = synth.gen_meshlets(spec, first, first + SAMPLE, dev, half).numpy().view(np.uint8).reshape(-1).view(L.MESHLET)
        # the slab's (view x model) in binary32, term by term as mat4_mul_col sums it
        model = e["model_matrix"][first:first + SAMPLE].reshape(-1, 4, 4).transpose(0, 2, 1).astype(F)
        vm = np.zeros_like(model)
        for k in range(4):
            vm = (vm + view[None, :, k, None] * model[:, None, k, :]).astype(F)
        models = np.repeat(np.ascontiguousarray(vm.transpose(0, 2, 1)).reshape(-1, 16), per_entity, axis=0)
        cones = (ml["cone_axis"].view(np.uint8).astype(np.uint32) * np.array([1, 1 << 8, 1 << 16], dtype=np.uint32)).sum(1).astype(np.uint32) \
            | ml["cone_cutoff"].view(np.uint8).astype(np.uint32) << 24
        v, flags, _ = pretest(models, ml["bounding_sphere"], cones, planes, -1.0)
        sparse, inside = (flags & 1) != 0, (flags & 2) != 0
        # a candidate: cone verdict open, or kept for certain by the cone but not certainly inside every plane
        open_lanes = (((v & 3) == 0) | (((v & 3) == 2) & ((v & 4) == 0))) & sparse[:, None]
        tiles = open_lanes.reshape(-1, TILE, PER)
        cand = tiles.sum((1, 2))
        index = (first * spec.meshlets_per_entity + np.arange(open_lanes.size)).reshape(-1, TILE * PER)
        flat = tiles.reshape(-1, TILE * PER)
        sphere_lines = [len(set((index[t][flat[t]] // 8).tolist())) for t in range(len(flat))]   # 16 B each
        cone_lines = [len(set((index[t][flat[t]] // 32).tolist())) for t in range(len(flat))]    # 4 B each
        share = float(open_lanes.mean())
        shares.append(share)
        print(f"{name:6s} entities {first}..{first + SAMPLE}: sparse {sparse.mean():.4f}, inside every plane {inside.mean():.4f}, "
              f"lanes left open {100 * share:.2f} %; per tile: candidates {cand.mean():.1f} (max {cand.max()}), "
              f"128-B sphere lines {np.mean(sphere_lines):.1f}, 128-B cone lines {np.mean(cone_lines):.1f}")
        assert sparse.all(), f"{name}: every record is sparse from this camera"
        assert inside.all(), f"{name}: every block is inside every plane from this camera"
    assert max(shares) < 0.05
