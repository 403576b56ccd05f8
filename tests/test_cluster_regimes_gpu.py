"""The light assignment's data-dependent paths (orbit_amd/csrc/light_cluster.hip), each reached on purpose and checked
against the oracle bit for bit.

The kernel picks its path from the data:
  per cluster, by its hit count (kernels.h kHitCache = 64, kPlaceDirect = 16): up to 16 hits are placed by the write
    launch in one round, 17-64 are copied from the hit cache over several rounds, 65-256 are tested again by the write
    launch through the heavy-block list, more than 256 are capped at 256 (light_culling.comp:135);
  per group of 256 active clusters, by its coarse segment counts (cluster_assign_kernel's s_fast): every segment within
    8 candidates is one wave's item, within 16 one speculative fetch, within 64 one fetched step, longer segments the
    stepped path — several steps once the group has more than kLightTile = 1024 candidates.  The segments split the
    light array in round64(ceil(max_lights / 16)) lights each (abi_ctx.hip).
The scene puts zero-radius point lights at the centres of chosen active clusters' boxes (oracle.cluster_aabb), the
lights of different clusters interleaved, a few directional lights at chosen indices, and asserts on the host — from
tests/np_restatement.py's uncapped counts and a restatement of the group union boxes and the segment split — that every
path above holds work before anything runs on the GPU."""
import numpy as np
import pytest

import np_restatement as npr
from orbit_amd import layouts as L
from test_gpu_parity import cluster_inputs, dev, host, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

W, H, TILE, SLICES = 320, 180, 8, 32
GROUP, SEGMENTS, CAP = 256, 16, 256
# target hit counts per group role; "slow" holds more than 1024 lights, 64 and 65 share a block of eight clusters
TARGETS = {"spec": (0, 1, 16), "mid": (17, 40), "slow": (64, 65, 255, 256, 257, 300)}
DIRECTIONAL_AT = (2, 700, -3)  # light indices of the directional lights (negative: from the end)


def _inside(mn, mx, p):
    return bool((mn <= p).all() and (p <= mx).all())


def regime_scene(oracle, n_directional):
    """(push, depth, info, lights, unique, bounds, max_lights, {cluster list position: its expected hit count})."""
    push, depth, info, _ = cluster_inputs(oracle, 4, W, H, 0, TILE, SLICES)
    cc = [int(v) for v in push["cluster_count"]]
    total = cc[0] * cc[1] * cc[2]
    masks, bounds = oracle.cluster_mark(push, depth)
    unique, _ = oracle.cluster_compact(cc, masks, total)
    na = int(unique[12:16].view(np.uint32)[0])
    act = unique[16:16 + 4 * na].view(np.uint32)
    assert na >= 4 * GROUP, na
    mn, mx = npr.cluster_aabb(info, bounds, act)
    finite = np.isfinite(mn).all(axis=1) & np.isfinite(mx).all(axis=1) & ((mx - mn) > 1e-3).all(axis=1)
    centre = ((mn + mx) * np.float32(0.5)).astype(np.float32)
    groups = {"spec": 0, "mid": (na // GROUP) // 2, "slow": na // GROUP - 1}
    chosen, role_of = {}, {}  # list position -> target, role

    def usable(u):  # its centre lies in no other active box, and no chosen centre lies in its box
        if not finite[u]:
            return False
        c = centre[u]
        inside = (mn <= c).all(axis=1) & (c <= mx).all(axis=1)
        if inside.sum() != 1:
            return False
        return not any(_inside(mn[u], mx[u], centre[v]) or _inside(mn[v], mx[v], centre[u]) for v in chosen)
    for role, g in groups.items():
        want = list(TARGETS[role])
        lo = g * GROUP
        for b in range(lo, lo + GROUP, 8):  # 64 and 65 in one block of eight: the block is heavy, the 64 copied
            if role == "slow" and len(want) == 6:
                pair = [u for u in range(b, b + 8) if usable(u)]
                if len(pair) >= 2:
                    chosen[pair[0]], chosen[pair[1]] = 64, 65
                    role_of[pair[0]] = role_of[pair[1]] = role
                    want = want[2:]
                continue
            for u in range(b, b + 8):
                if want and usable(u):
                    chosen[u], role_of[u] = want.pop(0), role
        assert not want, (role, want)
    # the light array: per role its clusters' lights interleaved (round robin); "mid" split over segments 1 and 2,
    # "spec" in segment 3 (its one-light cluster in segment 4), the directional lights at DIRECTIONAL_AT.  A cluster's
    # count is its placed lights + the directional ones (a target below that count keeps its placed lights).
    placed = {u: t - n_directional if t >= n_directional else t for u, t in chosen.items()}

    def interleave(role):
        lists = [[u] * placed[u] for u in placed if role_of[u] == role]
        out = []
        while any(lists):
            for lst in lists:
                if lst:
                    out.append(lst.pop())
        return out
    n_lights = sum(placed.values()) + n_directional
    seg = -(-(-(-n_lights // SEGMENTS)) // 64) * 64
    slots = [None] * n_lights
    dir_at = [d % n_lights for d in DIRECTIONAL_AT[:n_directional]]
    for d in dir_at:
        slots[d] = "dir"
    spec = interleave("spec")
    one = [u for u in spec if chosen[u] == 1]
    rest = [u for u in spec if chosen[u] != 1]
    mid = interleave("mid")

    def put(items, start):
        k = start
        for it in items:
            while slots[k] is not None:
                k += 1
            slots[k] = it
    put(mid[:len(mid) // 2], seg + 5)
    put(mid[len(mid) // 2:], 2 * seg + 5)
    put(rest, 3 * seg + 5)
    put(one, 4 * seg + 5)
    slow = iter(interleave("slow"))
    for k in range(n_lights):
        if slots[k] is None:
            slots[k] = next(slow)
    lights = np.zeros(n_lights, dtype=L.LIGHT)
    view_inv = np.linalg.inv(np.asarray(info["world_to_view_matrix"], np.float64).reshape(4, 4).T)
    for k, s in enumerate(slots):
        if s == "dir":
            lights["light_type"][k] = L.LIGHT_TYPE_DIRECTIONAL
            lights["position"][k] = (1.0, 2.0, 3.0)
            lights["outer_radius"][k] = 1.0
        else:
            lights["light_type"][k] = L.LIGHT_TYPE_POINT
            c = np.append(centre[s].astype(np.float64), 1.0)
            lights["position"][k] = (view_inv @ c)[:3].astype(np.float32)
            lights["outer_radius"][k] = 0.0
    lights["intensity"], lights["direction"][:, 1] = 1.0, -1.0
    info = np.array(info).copy()
    info["global_light_count"] = n_lights
    return push, depth, info, lights, unique, bounds, n_lights, {u: placed[u] + n_directional for u in chosen}


def group_paths(info, unique, bounds, lights, max_lights):
    """Per group of 256 active clusters: the count launch's path, from a restatement of cluster_aabb_kernel's union box
    and cluster_coarse_kernel's segments -> (list of 'wave' | 'spec' | 'one_step' | 'slow', candidates per group)."""
    na = int(unique[12:16].view(np.uint32)[0])
    act = unique[16:16 + 4 * na].view(np.uint32)
    mn, mx = npr.cluster_aabb(info, bounds, act)
    centres = npr.light_view_centres(info, lights)
    point = lights["light_type"] == L.LIGHT_TYPE_POINT
    seg = -(-(-(-max_lights // SEGMENTS)) // 64) * 64
    nl = len(lights)
    paths, totals = [], []
    for g in range(-(-na // GROUP)):
        lo, hi = mn[g * GROUP:(g + 1) * GROUP], mx[g * GROUP:(g + 1) * GROUP]
        if np.isnan(lo).any() or np.isnan(hi).any():
            passes = np.ones(nl, bool)
        else:
            passes = npr.lights_in_clusters(lo.min(axis=0)[None], hi.max(axis=0)[None], centres,
                                            lights["outer_radius"], point)[0]
        counts = np.array([passes[s * seg:min((s + 1) * seg, nl)].sum() for s in range(SEGMENTS)])
        paths.append("wave" if counts.max() <= 8 else "spec" if counts.max() <= 16 else
                     "one_step" if counts.max() <= 64 else "slow")
        totals.append(int(counts.sum()))
    return paths, totals


def _engine_run(torch, eng, info, unique, bounds, lights, total, lcap, pad=64):
    gl = torch.full((L.LIGHT_INDEX_HEADER + 4 * lcap + pad,), 0xEE, dtype=torch.uint8, device="cuda")
    gimg = torch.zeros((total, 2), dtype=torch.int32, device="cuda")
    eng.cluster_assign(info, dev(torch, unique), dev(torch, bounds), dev(torch, lights), gl, lcap, gimg)
    torch.cuda.synchronize()
    return host(gl), host(gimg, np.uint32).reshape(-1, 2)


@pytest.fixture(scope="module", params=[0, 3], ids=["point_only", "directional"])
def scene(request):
    from oracle import oracle

    oracle.build()
    n_dir = request.param
    push, depth, info, lights, unique, bounds, n_lights, chosen = regime_scene(oracle, n_dir)
    cc = [int(v) for v in push["cluster_count"]]
    total = cc[0] * cc[1] * cc[2]
    na = int(unique[12:16].view(np.uint32)[0])
    ol, oimg, dropped = oracle.cluster_assign(info, unique, bounds, lights, 256 * na + 16, total)
    assert dropped == 0
    nl_, nimg, count, _ = npr.cluster_assign(info, unique, bounds, lights, 256 * na + 16, total)
    assert np.array_equal(nl_, ol) and np.array_equal(nimg, oimg)
    return dict(info=info, unique=unique, bounds=bounds, lights=lights, max_lights=n_lights, total=total, na=na,
                ol=ol, oimg=oimg, count=count, chosen=chosen, n_dir=n_dir)


def test_the_scene_reaches_every_path(scene):
    """Host only: the hit-count classes and the group paths hold work, and the chosen clusters have their counts."""
    count, chosen, n_dir = scene["count"], scene["chosen"], scene["n_dir"]
    for u, t in chosen.items():
        assert count[u] == t, (u, t, count[u])
    assert ((count >= 1) & (count <= 16)).any() and (count == 16).any()
    assert ((count >= 17) & (count <= 64)).any() and (count == 17).any() and (count == 64).any()
    assert ((count >= 65) & (count <= 256)).any() and (count == 65).any() and (count == 255).any() and (count == 256).any()
    assert (count == 257).any() and (count >= 300).any()
    if n_dir == 0:
        assert (count == 0).any()
    paths, totals = group_paths(scene["info"], scene["unique"], scene["bounds"], scene["lights"], scene["max_lights"])
    assert {"wave", "spec", "one_step", "slow"} <= set(paths), paths
    assert any(p == "slow" and t > 1024 for p, t in zip(paths, totals)), (paths, totals)
    # a heavy block (a cluster past kHitCache) that also holds a cluster of exactly kHitCache hits
    u64, u65 = (next(u for u, t in chosen.items() if t == k) for k in (64, 65))
    assert u64 // 8 == u65 // 8


def test_product_equals_the_oracle_on_every_path(torch_mod, scene):
    from orbit_amd.engine import Engine

    torch = torch_mod
    eng = Engine(0, max_lights=scene["max_lights"], max_clusters=scene["total"])
    lcap = 256 * scene["na"] + 16
    gl, gimg = _engine_run(torch, eng, scene["info"], scene["unique"], scene["bounds"], scene["lights"], scene["total"], lcap)
    eng.status()
    n_idx = int(scene["ol"][:4].view(np.uint32)[0])
    assert int(gl[:4].view(np.uint32)[0]) == n_idx
    assert np.array_equal(gl[:4 + 4 * n_idx], scene["ol"][:4 + 4 * n_idx]), "cluster light index lists differ"
    assert bool((gl[4 + 4 * n_idx:] == 0xEE).all()), "written past the light list"
    assert np.array_equal(gimg, scene["oimg"]), "(offset, count) image differs"
    eng.close()


@pytest.mark.parametrize("where", ["end_of_saturated", "inside_saturated", "inside_hit_cache_list"])
def test_capacity_cut_on_every_path(torch_mod, scene, where):
    """light_index_capacity cut at the end of a saturated cluster's range, inside it, and inside the range of a
    cluster whose list the write launch copies from the hit cache: the same bytes as the oracle at that capacity,
    nothing written past it, E_CAPACITY latched."""
    from orbit_amd._lib import E_CAPACITY, OrbitError
    from orbit_amd.engine import Engine

    torch = torch_mod
    act = scene["unique"][16:16 + 4 * scene["na"]].view(np.uint32)
    off, cnt = (scene["oimg"][act][:, k].astype(np.int64) for k in (0, 1))
    count = scene["count"]
    if where == "end_of_saturated":
        u = int(np.flatnonzero(count > 256)[0])
        cut = int(off[u] + cnt[u])
    elif where == "inside_saturated":
        u = int(np.flatnonzero(count > 256)[-1])
        cut = int(off[u] + 100)
    else:
        u = int(np.flatnonzero((count > 16) & (count <= 64))[0])
        cut = int(off[u] + cnt[u] // 2 + 1)
    n_idx = int(scene["ol"][:4].view(np.uint32)[0])
    assert cut < n_idx and off[u] < cut <= off[u] + cnt[u]
    from oracle import oracle

    ol, oimg, dropped = oracle.cluster_assign(scene["info"], scene["unique"], scene["bounds"], scene["lights"], cut,
                                              scene["total"])
    assert dropped == n_idx - cut
    eng = Engine(0, max_lights=scene["max_lights"], max_clusters=scene["total"])
    gl, gimg = _engine_run(torch, eng, scene["info"], scene["unique"], scene["bounds"], scene["lights"], scene["total"],
                           cut, pad=4 * 300)
    assert np.array_equal(gl[:4 + 4 * cut], ol[:4 + 4 * cut]), "cut light index list differs"
    assert bool((gl[4 + 4 * cut:] == 0xEE).all()), "written past the capacity"
    assert np.array_equal(gimg, oimg)
    with pytest.raises(OrbitError) as ei:
        eng.status()
    assert ei.value.code == E_CAPACITY
    eng.close()
