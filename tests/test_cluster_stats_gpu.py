"""orbit_cluster_stats on the MI355X: every counter equal to tests/cluster_stats_ref.py on the golden cluster cases, the
regime scene (every class boundary), a poisoned depth buffer and config 4 at full size; and against the chain: its
headers and image with ample capacities, unchanged counts under cut capacities, no side effect on the chain's buffers
or the latched status, the same argument errors, graph capture on the first call, and a call beside a running chain."""
import numpy as np
import pytest

import cluster_stats_ref as ref
from orbit_amd import _lib
from orbit_amd import layouts as L
from test_gpu_parity import dev, host, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu


def _engine(push, lights, **caps):
    from orbit_amd.engine import Engine

    cc = [int(v) for v in push["cluster_count"]]
    caps.setdefault("max_clusters", max(cc[0] * cc[1] * cc[2], 1))
    caps.setdefault("max_lights", max(len(lights), 1))
    return Engine(0, **caps)


class Case:
    """Device inputs of one case, the chain's outputs sized for its uncut result, a stats block."""

    def __init__(self, torch, c, index_capacity=None, light_index_capacity=None):
        self.c = c
        self.push, self.info = c["push"], c["info"]
        cc = [int(v) for v in self.push["cluster_count"]]
        self.total = cc[0] * cc[1] * cc[2]
        self.depth = dev(torch, c["depth"])
        self.lights = dev(torch, c["lights"]) if len(c["lights"]) else None
        self.icap = self.total if index_capacity is None else index_capacity
        self.lcap = 256 * self.total + 16 if light_index_capacity is None else light_index_capacity
        self.masks = torch.full((max(cc[0] * cc[1], 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.bounds = torch.full((max(self.total, 1), 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.unique = torch.full((L.COMPACT_HEADER + 4 * max(self.icap, 1),), 0xEE, dtype=torch.uint8, device="cuda")
        self.lists = torch.full((L.LIGHT_INDEX_HEADER + 4 * max(self.lcap, 1),), 0xEE, dtype=torch.uint8, device="cuda")
        self.image = torch.full((max(self.total, 1), 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.stats = torch.full((32,), 0x77, dtype=torch.int64, device="cuda")

    def stats_call(self, eng, stream=None):
        eng.cluster_stats(self.stats, self.push, self.info, self.depth, self.lights, stream=stream)

    def chain(self, eng, stream=None):
        eng.compute_clusters(self.push, self.info, self.depth, self.lights, self.masks, self.bounds, self.unique, self.icap,
                             self.lists, self.lcap, self.image, stream=stream)

    def got(self):
        from orbit_amd.engine import cluster_stats_dict

        return cluster_stats_dict(self.stats)

    def chain_outputs(self):
        return [host(t).copy() for t in (self.masks, self.bounds, self.unique, self.lists, self.image)]

    def headers(self):
        return int(host(self.unique, np.uint32)[3]), int(host(self.lists, np.uint32)[0])


def _run(torch, c, **caps):
    eng = _engine(c["push"], c["lights"], **caps)
    try:
        b = Case(torch, c)
        b.stats_call(eng)
        torch.cuda.synchronize()
        eng.status()
        return b.got()
    finally:
        eng.close()


@pytest.mark.parametrize("case", ref.CASES)
def test_counters_equal_the_reference_on_the_golden_cases(torch_mod, case):
    c = ref.load_case(case)
    want, _ = ref.stats(c["push"], c["info"], c["depth"], c["lights"])
    assert _run(torch_mod, c) == want


@pytest.fixture(scope="module", params=[0, 3], ids=["point_only", "directional"])
def regime(request):
    from oracle import oracle
    from test_cluster_regimes_gpu import regime_scene

    oracle.build()
    push, depth, info, lights, _, _, n_lights, _ = regime_scene(oracle, request.param)
    return dict(push=push, info=info, depth=depth, lights=lights[:n_lights])


def test_counters_equal_the_reference_on_the_regime_scene(torch_mod, regime):
    want, (_, _, count) = ref.stats(regime["push"], regime["info"], regime["depth"], regime["lights"])
    for k in (0, 16, 17, 64, 65, 255, 256, 257):  # every class boundary (the 0 only without directional lights)
        assert (count == k).any() or (k == 0 and want["clusters_by_lights"][0] == 0), k
    assert (count >= 300).any() and all(v > 0 for v in want["clusters_by_lights"][1:])
    assert _run(torch_mod, regime) == want


def test_counters_on_a_poisoned_depth(torch_mod):
    """0, -0, denormals, negatives, inf and NaN among the samples: the mark's slices and bounds decide them."""
    c = ref.load_case("spirv_cluster/s2")
    d = np.array(c["depth"], np.float32).reshape(-1)
    rng = np.random.default_rng(7)
    bad = np.array([0.0, -0.0, 1e-40, -1e-40, -0.5, np.inf, -np.inf, np.nan, 1e-45, 3.0], np.float32)
    at = rng.choice(len(d), 600, replace=False)
    d[at] = bad[np.arange(600) % len(bad)]
    d[:8] = bad[:8]  # a tile that holds all of them
    c = dict(c, depth=d.reshape(np.shape(c["depth"])))
    want, _ = ref.stats(c["push"], c["info"], c["depth"], c["lights"])
    assert _run(torch_mod, c) == want


def test_config4_at_full_size(torch_mod):
    torch = torch_mod
    import config_scenes as cs
    from oracle import oracle

    oracle.build()
    cam = cs.camera()
    push, info, lights = cs.config4_inputs(oracle, cam)
    c = dict(push=push, info=info, depth=cs.config3_depth(cam), lights=lights)
    want, _ = ref.stats(c["push"], c["info"], c["depth"], c["lights"])
    eng = _engine(push, lights)
    try:
        b = Case(torch, c)
        b.stats_call(eng)
        b.chain(eng)
        torch.cuda.synchronize()
        eng.status()
        got = b.got()
        assert got == want
        assert b.headers() == (got["active_clusters"], got["light_indices"])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ against the chain
CHAIN_CASES = ["spirv_cluster_shapes/edge12_sat", "spirv_cluster/s5", "spirv_cluster_shapes/t3_z16_ms4"]


@pytest.mark.parametrize("case", CHAIN_CASES)
def test_chain_headers_and_image_agree_with_ample_capacities(torch_mod, case):
    torch = torch_mod
    c = ref.load_case(case)
    want, (active, _, count) = ref.stats(c["push"], c["info"], c["depth"], c["lights"])
    eng = _engine(c["push"], c["lights"])
    try:
        b = Case(torch, c)
        b.chain(eng)
        b.stats_call(eng)
        torch.cuda.synchronize()
        eng.status()
        got = b.got()
        assert got == want
        assert b.headers() == (got["active_clusters"], got["light_indices"])
        img = host(b.image, np.uint32).reshape(-1, 2)
        assert np.array_equal(img[active, 1], np.minimum(count, 256))
        assert int(img[active, 1].max(initial=0)) == min(got["max_cluster_lights"], 256)
    finally:
        eng.close()


def test_cut_capacities_leave_the_counts_and_latch_the_chain(torch_mod):
    torch = torch_mod
    c = ref.load_case("spirv_cluster_shapes/edge12_sat")
    want, _ = ref.stats(c["push"], c["info"], c["depth"], c["lights"])
    eng = _engine(c["push"], c["lights"])
    try:
        b = Case(torch, c, index_capacity=want["active_clusters"] // 3, light_index_capacity=want["light_indices"] // 5)
        b.stats_call(eng)
        torch.cuda.synchronize()
        eng.status()
        assert b.got() == want
        b.chain(eng)
        b.stats_call(eng)
        torch.cuda.synchronize()
        with pytest.raises(_lib.OrbitError) as e:
            eng.status()
        assert e.value.code == _lib.E_CAPACITY
        assert b.got() == want
        assert b.headers()[0] == want["active_clusters"] // 3
    finally:
        eng.close()


def test_a_stats_call_writes_nothing_else_and_the_chain_stays_exact(torch_mod):
    torch = torch_mod
    from oracle import oracle

    oracle.build()
    c = ref.load_case("spirv_cluster_shapes/edge12_sat")
    want, _ = ref.stats(c["push"], c["info"], c["depth"], c["lights"])
    eng = _engine(c["push"], c["lights"])
    try:
        b = Case(torch, c)
        before = b.chain_outputs()
        depth0, lights0 = host(b.depth).copy(), host(b.lights).copy()
        b.stats_call(eng)
        torch.cuda.synchronize()
        eng.status()  # nothing latched
        assert b.got() == want
        for x, y in zip(before, b.chain_outputs()):
            assert np.array_equal(x, y), "a chain buffer changed"
        assert np.array_equal(host(b.depth), depth0) and np.array_equal(host(b.lights), lights0)
        # the chain behind it is still the oracle's, bit for bit
        b.chain(eng)
        torch.cuda.synchronize()
        eng.status()
        om, ob = oracle.cluster_mark(c["push"], c["depth"])
        ou, _ = oracle.cluster_compact([int(v) for v in c["push"]["cluster_count"]], om, b.total)
        na = int(ou[12:16].view(np.uint32)[0])
        ol, oimg, _ = oracle.cluster_assign(c["info"], ou, ob, c["lights"], b.lcap, b.total)
        nl = int(ol[:4].view(np.uint32)[0])
        assert np.array_equal(host(b.masks, np.uint32), om)
        assert np.array_equal(host(b.bounds, np.uint32).reshape(-1, 2), ob)
        assert np.array_equal(host(b.unique)[:16 + 4 * na], ou[:16 + 4 * na])
        assert np.array_equal(host(b.lists)[:4 + 4 * nl], ol[:4 + 4 * nl])
        act = ou[16:16 + 4 * na].view(np.uint32)
        assert np.array_equal(host(b.image, np.uint32).reshape(-1, 2)[act], oimg[act])
    finally:
        eng.close()


def _code(fn):
    try:
        fn()
    except _lib.OrbitError as e:
        return e.code
    return 0


def test_argument_errors_match_compute_clusters(torch_mod):
    torch = torch_mod
    c = ref.load_case("spirv_cluster/s2")
    n_lights = len(c["lights"])
    cc = [int(v) for v in c["push"]["cluster_count"]]
    total = cc[0] * cc[1] * cc[2]

    def variant(**kw):
        push, info = c["push"].copy(), c["info"].copy()
        for k, v in kw.items():
            (info if k.startswith("info_") else push)[k.replace("info_", "")] = v
        return push, info

    bad = {
        "grid differs": variant(info_cluster_count=(cc[0], cc[1], cc[2] - 1)),
        "33 slices": variant(cluster_count=(cc[0], cc[1], 33), info_cluster_count=(cc[0], cc[1], 33)),
        "tile 0": variant(tile_size_px=0),
        "samples 0": variant(depth_buffer_sample_count=0),
        "too many lights": variant(info_global_light_count=n_lights + 1),
    }
    eng = _engine(c["push"], c["lights"])
    small = _engine(c["push"], c["lights"], max_clusters=total - 1)
    try:
        b = Case(torch, c)
        for name, (push, info) in bad.items():
            b.push, b.info = push, info
            want = _code(lambda: b.chain(eng))
            assert want != 0, name
            assert _code(lambda: b.stats_call(eng)) == want, name
        b.push, b.info = c["push"], c["info"]
        for e, what in ((small, "grid > max_clusters"),):
            want = _code(lambda: b.chain(e))
            assert want == _lib.E_CAPACITY and _code(lambda: b.stats_call(e)) == want, what
        depth = b.depth
        b.depth = None
        want = _code(lambda: b.chain(eng))
        assert want == _lib.E_MISSING and _code(lambda: b.stats_call(eng)) == want, "depth NULL"
        b.depth, lights = depth, b.lights
        b.lights = None
        want = _code(lambda: b.chain(eng))
        assert want == _lib.E_MISSING and _code(lambda: b.stats_call(eng)) == want, "lights NULL"
        b.lights = lights
        # the stats block itself
        raw = torch.zeros(272, dtype=torch.uint8, device="cuda")
        assert _code(lambda: eng.cluster_stats(raw[4:260], b.push, b.info, b.depth, b.lights)) == _lib.E_INVALID
        rc = eng._lib.orbit_cluster_stats(eng._ctx, b.push.ctypes.data, b.info.ctypes.data, b.depth.data_ptr(),
                                          b.lights.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.E_INVALID
        torch.cuda.synchronize()
        eng.status()
    finally:
        eng.close()
        small.close()


def test_stats_then_chain_capture_into_a_graph_on_the_first_call(torch_mod):
    torch = torch_mod
    c = ref.load_case("spirv_cluster_shapes/edge12_sat")
    depths = [np.array(c["depth"], np.float32), np.array(c["depth"], np.float32)[::-1].copy()]
    depths[1][:10] = 0.0  # the second frame: other depths, more samples outside the grid
    eng = _engine(c["push"], c["lights"])  # a context that never ran either call
    try:
        b = Case(torch, c)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            b.stats_call(eng)
            b.chain(eng)
        for d in depths + depths[:1]:
            b.depth.copy_(torch.from_numpy(d.view(np.uint8).reshape(-1)))
            b.stats.fill_(0x77)
            g.replay()
            torch.cuda.synchronize()
            eng.status()
            want, _ = ref.stats(c["push"], c["info"], d, c["lights"])
            assert b.got() == want
            assert b.headers() == (want["active_clusters"], want["light_indices"])
    finally:
        eng.close()


def test_a_stats_call_beside_a_running_chain(torch_mod):
    torch = torch_mod
    import config_scenes as cs
    from oracle import oracle

    oracle.build()
    cam = cs.camera()
    push, info, lights = cs.config4_inputs(oracle, cam)
    c = dict(push=push, info=info, depth=cs.config3_depth(cam), lights=lights)
    eng = _engine(push, lights)
    try:
        b = Case(torch, c)
        b.stats_call(eng)
        torch.cuda.synchronize()
        serial = b.got()
        side = torch.cuda.Stream()
        for _ in range(3):
            b.stats.fill_(0x77)
            torch.cuda.synchronize()
            b.chain(eng)  # the current stream
            b.stats_call(eng, stream=side)
            b.chain(eng)
            torch.cuda.synchronize()
            eng.status()
            assert b.got() == serial
        assert b.headers() == (serial["active_clusters"], serial["light_indices"])
    finally:
        eng.close()
