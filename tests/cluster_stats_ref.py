"""numpy statement of orbit_cluster_stats: the uncapped light counts of the cluster chain for one set of inputs.

Built from tests/np_restatement.py's primitives (log2c, f2u_sat, fma32, cluster_aabb, lights_in_clusters), which are
pinned to the oracle and through it to the reference's binaries.  A depth sample's slice is mark_active's
(cluster_common.glsl:18-20 as compiled: uint(fma(log2(z_near / d), z_scale, z_bias))); `mark` rebuilds the tile masks
and depth bounds from those slices so the tests can hold them against oracle.cluster_mark.  `stats` returns the
counters under OrbitClusterStats' names (include/orbit_abi_ext.h), and the active clusters with their sample and light
counts for the checks against np_restatement.cluster_assign and the chain's outputs.
"""
import os

import numpy as np

import np_restatement as npr
from orbit_amd import layouts as L

F = np.float32
CAP = 256
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def light_class(count):
    """The classes of a cluster's uncapped count: 0, 1-16, 17-64, 65-256, > 256."""
    count = np.asarray(count, np.int64)
    return np.select([count == 0, count <= 16, count <= 64, count <= CAP], [0, 1, 2, 3], 4)


def _pc(push):
    return np.asarray(push).reshape(-1).view(np.uint8).view(L.MARK_ACTIVE_PUSH)[0]


def sample_slices(push, depth):
    """The slice of every depth sample -> uint64[H, W, samples] (mark_active.comp:28-30)."""
    pc = _pc(push)
    W, H = (int(v) for v in pc["screen_size"])
    sc = int(pc["depth_buffer_sample_count"])
    d = np.ascontiguousarray(depth, F).reshape(H, W, sc)
    with np.errstate(all="ignore"):
        lz = (F(pc["z_near"]) / d).astype(F)
        return npr.f2u_sat(npr.fma32(npr.log2c(lz), F(pc["z_scale"]), F(pc["z_bias"])))


def _samples(push, depth):
    """(slice, linear cluster index or -1, covered by a tile) of every sample, flattened."""
    pc = _pc(push)
    cx, cy, cz = (int(v) for v in pc["cluster_count"])
    ts = int(pc["tile_size_px"])
    W, H = (int(v) for v in pc["screen_size"])
    sc = int(pc["depth_buffer_sample_count"])
    sl = sample_slices(push, depth)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tx, ty = np.repeat((px // ts)[..., None], sc, 2), np.repeat((py // ts)[..., None], sc, 2)
    covered = (tx < cx) & (ty < cy)
    in_grid = covered & (sl < cz)
    cluster = np.where(in_grid, tx + ty * cx + sl.astype(np.int64) * (cx * cy), -1)
    return sl.reshape(-1), cluster.reshape(-1), covered.reshape(-1), ty.reshape(-1) * cx + tx.reshape(-1)


def mark(push, depth):
    """(tile masks, depth bounds[tiles * cz, 2]) from the restated slices: what cluster_mark writes."""
    pc = _pc(push)
    cx, cy, cz = (int(v) for v in pc["cluster_count"])
    d = np.ascontiguousarray(depth, F).reshape(-1)
    sl, cluster, covered, tile = _samples(push, depth)
    masks = np.zeros(cx * cy, np.uint32)
    bit = np.where(sl < 32, np.left_shift(np.uint64(1), np.minimum(sl, 31).astype(np.uint64)), 0).astype(np.uint32)
    np.bitwise_or.at(masks, tile[covered], bit[covered])
    with np.errstate(all="ignore"):
        inv = (F(1.0) - d).astype(F)
    bmin = np.where(np.isnan(inv), np.uint32(0x7FC00000), inv.view(np.uint32))
    bounds = np.zeros((cx * cy * cz, 2), np.uint32)
    g = cluster >= 0
    np.maximum.at(bounds[:, 0], cluster[g], bmin[g])
    np.maximum.at(bounds[:, 1], cluster[g], d.view(np.uint32)[g])
    return masks, bounds


def cluster_counts(info, bounds, active, lights):
    """count(c) of every cluster in `active` (linear indices): the lights < global_light_count in it, uncapped."""
    nl = int(np.asarray(info).reshape(-1)[0]["global_light_count"])
    lights = np.asarray(lights).reshape(-1).view(np.uint8).view(L.LIGHT)[:nl]
    out = np.zeros(len(active), np.int64)
    if nl == 0 or len(active) == 0:
        return out
    centres = npr.light_view_centres(info, lights)
    point = lights["light_type"] == L.LIGHT_TYPE_POINT
    step = max(1, (1 << 21) // nl)
    for c0 in range(0, len(active), step):
        mn, mx = npr.cluster_aabb(info, bounds, active[c0:c0 + step])
        out[c0:c0 + step] = npr.lights_in_clusters(mn, mx, centres, lights["outer_radius"], point).sum(axis=1)
    return out


def stats(push, info, depth, lights):
    """The OrbitClusterStats counters as {name: int | list}, and (active clusters ascending, their in-grid samples,
    their uncapped counts)."""
    pc = _pc(push)
    W, H = (int(v) for v in pc["screen_size"])
    sc = int(pc["depth_buffer_sample_count"])
    _, cluster, _, _ = _samples(push, depth)
    _, bounds = mark(push, depth)
    active, n_samples = np.unique(cluster[cluster >= 0], return_counts=True)
    count = cluster_counts(info, bounds, active, lights)
    capped = np.minimum(count, CAP)
    cls = light_class(count)
    out = dict(samples=W * H * sc, samples_outside_grid=W * H * sc - int(n_samples.sum()), active_clusters=len(active),
               light_refs=int(count.sum()), light_indices=int(capped.sum()),
               max_cluster_lights=int(count.max()) if len(count) else 0,
               sample_light_refs=int((n_samples * capped).sum()),
               clusters_by_lights=[int((cls == k).sum()) for k in range(5)],
               samples_by_lights=[int(n_samples[cls == k].sum()) for k in range(5)])
    return out, (active, n_samples, count)


def check_invariants(s):
    """The invariants include/orbit_abi_ext.h documents (all but the one against the chain)."""
    assert s["samples"] == s["samples_outside_grid"] + sum(s["samples_by_lights"]), s
    assert s["active_clusters"] == sum(s["clusters_by_lights"]), s
    assert s["light_refs"] >= s["light_indices"], s
    assert (s["light_refs"] == s["light_indices"]) == (s["clusters_by_lights"][4] == 0), s
    assert s["max_cluster_lights"] <= s["light_refs"], s


# ------------------------------------------------------------------------------------------------ the golden cases
SPIRV_CASES = ["s1", "s2", "s4", "s5", "s6"]
SHAPE_CASES = ["edge12_sat", "t5_z7_ms2", "t3_z16_ms4", "t16_none", "t16_poison"]
CASES = [f"spirv_cluster/{n}" for n in SPIRV_CASES] + [f"spirv_cluster_shapes/{n}" for n in SHAPE_CASES] + ["cluster_small"]


def load_case(case):
    """{push, info, depth, lights} of one golden case ("file/name", or "cluster_small")."""
    if case == "cluster_small":
        g = np.load(os.path.join(GOLDEN, "cluster_small.npz"))
        return dict(push=g["push"].view(L.MARK_ACTIVE_PUSH).reshape(()), info=g["info"].view(L.CLUSTER_CULL_INFO).reshape(()),
                    depth=g["depth"], lights=g["lights"].view(L.LIGHT))
    f, name = case.split("/")
    g = np.load(os.path.join(GOLDEN, f + ".npz"))
    return dict(push=g[f"{name}/push"].view(L.MARK_ACTIVE_PUSH).reshape(()),
                info=g[f"{name}/info"].view(L.CLUSTER_CULL_INFO).reshape(()), depth=g[f"{name}/depth"],
                lights=g[f"{name}/lights"].view(L.LIGHT))
