"""orbit_env_map and orbit_env_sample on the device (include/orbit_abi_ext.h E0-E12) against the host mirror
(orbit_amd.env_map.host_env_map / host_env_sample, which tests/test_env_map_cpu.py holds to the numpy restatement): every byte
of the sky cube, the irradiance cube, the prefiltered cube, the BRDF table and the counters over tests/env_map_cases.py,
between guards, inputs unchanged, no latched error; each product alone and from a caller's sky cube; the argument errors;
the first call of a fresh context captured into a graph and replayed; orbit_env_sample on the hostile directions; one
chained run."""
import ctypes as C

import numpy as np
import pytest

import env_map_cases as ec
from orbit_amd import _lib
from orbit_amd import env_map as em
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import Guarded, latched

pytestmark = pytest.mark.gpu
PRODUCTS = ("sky", "irradiance", "prefiltered", "brdf")
CASES = ec.chain_cases()


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def engine(torch_mod):
    from orbit_amd.engine import Engine

    e = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)
    yield e
    e.close()


def run(torch, engine, kw, want=PRODUCTS, sky=None, with_stats=True):
    """One orbit_env_map call on guarded buffers -> dict(sky, irradiance, prefiltered, brdf: np.uint16 or None, stats).  sky:
    a caller's cube (then no panorama is handed over and the cube must stay as it is)."""
    lay = em.layout(kw["sky_size"], kw["irradiance_size"], kw["prefiltered_size"], kw["prefiltered_levels"], kw["brdf_size"])
    sizes = dict(sky=8 * lay["sky_texels"], irradiance=8 * lay["irradiance_texels"], prefiltered=8 * lay["prefiltered_texels"],
                 brdf=4 * lay["brdf_texels"], stats=48)
    wanted = [k for k in want if sizes[k]] + (["stats"] if with_stats else [])
    pano = None if sky is not None or not kw["sky_size"] else Guarded(torch, kw["equirect"])
    out = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=int(n)) for k, n in sizes.items()}
    if sky is not None:
        out["sky"] = Guarded(torch, sky)
    ptr = lambda k: out[k].ptr if k in wanted else None  # noqa: E731
    eh, ew = (0, 0) if pano is None else kw["equirect"].shape[:2]
    em.device_env_map(engine, None if pano is None else pano.ptr, ptr("sky") if sky is None else out["sky"].ptr, ptr("irradiance"),
                      ptr("prefiltered"), ptr("brdf"), ptr("stats"), ew, eh, kw["sky_size"], kw["irradiance_size"], kw["prefiltered_size"],
                      kw["prefiltered_levels"], kw["brdf_size"], kw["sample_count"], kw["sample_delta"], kw["brdf_sample_count"])
    torch.cuda.synchronize()
    assert latched(engine) == 0
    if pano is not None:
        pano.unchanged()
    got = {}
    for k in sizes:
        if k in wanted and not (k == "sky" and sky is not None):
            got[k] = out[k].read().view(np.uint16 if k != "stats" else np.uint8)
        else:
            out[k].unchanged()
            got[k] = None
    return got


def assert_equal(name, got, want):
    for k in PRODUCTS:
        if got[k] is not None:
            diff = np.flatnonzero(got[k] != want[k])
            assert len(diff) == 0, f"{name}: {len(diff)} halves of {k} differ, first {diff[0]}: device {got[k][diff[0]]:#x}, host {want[k][diff[0]]:#x}"
    if got["stats"] is not None:
        assert got["stats"].tobytes() == want["stats"].tobytes(), f"{name}: device stats {got['stats'].view(L.ENV_MAP_STATS)[0]} != host {want['stats']}"


# -- 1. the matrix: whole calls
@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_device_equals_mirror(torch_mod, engine, name, kw):
    assert_equal(name, run(torch_mod, engine, kw), em.host_env_map(**kw))


# -- 2. each product alone, from the call's own sky cube and from a caller's
@pytest.mark.parametrize("product", PRODUCTS)
def test_each_product_alone(torch_mod, engine, product):
    name, kw = CASES[3]  # sky 8, irradiance 5, prefiltered 16 x 1, table 17
    whole = em.host_env_map(**kw)
    alone = dict(kw)
    for k in ("irradiance", "prefiltered", "brdf"):
        if k != product:
            alone[k + "_size"] = 0
    if product == "brdf":
        alone["sky_size"] = 0
        got = run(torch_mod, engine, alone, want=("brdf",))
        assert got["sky"] is None and np.array_equal(got["brdf"], whole["brdf"])
        return
    got = run(torch_mod, engine, alone, want=("sky", product), with_stats=False)
    assert np.array_equal(got["sky"], whole["sky"]) and np.array_equal(got[product], whole[product])
    if product != "sky":  # and from a caller's sky cube: the panorama is not handed over, the cube is not written
        got = run(torch_mod, engine, alone, want=(product,), sky=whole["sky"])
        want = em.host_env_map(sky=whole["sky"], **{k: v for k, v in alone.items() if k != "equirect"})
        assert np.array_equal(want[product], whole[product])
        assert_equal(f"{name} from a caller's sky", got, want)


# -- 3. the argument errors: the same verdicts as the mirror's, nothing launched, nothing latched
def test_the_errors(torch_mod, engine):
    torch = torch_mod
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    good = dict(equirect=base, sky=base + 4096, irradiance=base + 16384, prefiltered=base + 20480, brdf=base + 40960, stats=base + 49152,
                equirect_w=4, equirect_h=2, sky_size=4, irradiance_size=2, prefiltered_size=4, prefiltered_levels=2, brdf_size=4, sample_count=4,
                sample_delta=0.5, brdf_sample_count=4)
    lib = _lib.load()

    def status(**change):
        j = em.env_map_job(**{**good, **change})
        return lib.orbit_env_map(engine._ctx, C.byref(j), None)

    assert status() == _lib.OK
    bad = [dict(sky_size=3), dict(sky_size=0), dict(sky_size=8192), dict(irradiance_size=0), dict(prefiltered_size=5000), dict(prefiltered_levels=0),
           dict(prefiltered_levels=14), dict(sample_count=0), dict(sample_count=65537), dict(brdf_sample_count=0), dict(sample_delta=0.0),
           dict(sample_delta=-0.5), dict(sample_delta=float("nan")), dict(sample_delta=float("inf")), dict(sample_delta=0.00005), dict(sample_delta=0.0049),
           dict(sky=base + 4100), dict(equirect=base + 8), dict(brdf=base + 40962), dict(stats=base + 49156), dict(flags=1),
           dict(equirect_w=0), dict(sky=None), dict(irradiance=good["prefiltered"]), dict(prefiltered=good["sky"] + 1000), dict(stats=good["brdf"] + 56),
           dict(sky=None, irradiance=None, prefiltered=None, brdf=None)]
    for change in bad:
        assert status(**change) == _lib.E_INVALID, change
    assert lib.orbit_env_map(engine._ctx, None, None) == _lib.E_INVALID
    sample = dict(cube=base, directions=base + 4096, lods=base + 8192, rgb=base + 12288, bad_directions=base + 16384, size=4, levels=2, n=4)

    def sample_status(**change):
        j = em.env_sample_job(**{**sample, **change})
        return lib.orbit_env_sample(engine._ctx, C.byref(j), None)

    assert sample_status() == _lib.OK and sample_status(n=0, directions=None, lods=None, rgb=None) == _lib.OK
    for change in (dict(size=0), dict(size=4097), dict(levels=0), dict(levels=14), dict(cube=None), dict(rgb=None), dict(cube=base + 4),
                   dict(rgb=base + 12290), dict(bad_directions=base + 16388), dict(flags=2), dict(rgb=sample["lods"]), dict(rgb=sample["cube"] + 952),
                   dict(bad_directions=sample["rgb"] + 40)):
        assert sample_status(**change) == _lib.E_INVALID, change
    torch.cuda.synchronize()
    assert latched(engine) == 0


# -- 4. the first call of a fresh context captured into a graph, replayed twice per panorama
def test_the_first_call_captures_into_a_graph(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine

    kw = dict(ec.CHAINED[1], sky_size=8, prefiltered_size=5, prefiltered_levels=3, sample_count=17, irradiance_size=3, brdf_size=5, brdf_sample_count=9)
    panos = [kw["equirect"], kw["equirect"][::-1, ::-1] * np.float32(0.5)]
    lay = em.layout(kw["sky_size"], kw["irradiance_size"], kw["prefiltered_size"], kw["prefiltered_levels"], kw["brdf_size"])
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        pano = dev(torch, panos[0])
        outs = {k: torch.full((int(lay[k + "_texels"]) * (4 if k == "brdf" else 8) + 16,), 0x5A, dtype=torch.uint8, device="cuda") for k in PRODUCTS}
        stats = torch.full((6,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        eh, ew = panos[0].shape[:2]
        with torch.cuda.graph(g):
            em.device_env_map(eng, pano, outs["sky"], outs["irradiance"], outs["prefiltered"], outs["brdf"], stats, ew, eh, kw["sky_size"],
                              kw["irradiance_size"], kw["prefiltered_size"], kw["prefiltered_levels"], kw["brdf_size"], kw["sample_count"],
                              kw["sample_delta"], kw["brdf_sample_count"])
        for p in panos:
            pano.copy_(dev(torch, p))
            want = em.host_env_map(**dict(kw, equirect=p))
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == 0
                for k in PRODUCTS:
                    b = host(outs[k])
                    assert (b[-16:] == 0x5A).all() and b[:-16].tobytes() == want[k].tobytes(), (k, replay)
                assert host(stats).tobytes() == want["stats"].tobytes()
    finally:
        eng.close()


# -- 5. the sampler on the hostile directions
@pytest.mark.parametrize("size,levels", ec.SAMPLE_CUBES)
def test_sampler_equals_mirror(torch_mod, engine, size, levels):
    torch = torch_mod
    cube = ec.noise_cube(size, levels)
    d, lods = ec.sample_directions(levels)
    want = em.host_env_sample(cube, size, levels, d, lods)
    g_in = [Guarded(torch, cube), Guarded(torch, d), Guarded(torch, lods)]
    rgb, bad = Guarded(torch, np.zeros(0, np.uint8), nbytes=12 * len(d)), Guarded(torch, np.zeros(0, np.uint8), nbytes=8)
    em.device_env_sample(engine, g_in[0].ptr, size, levels, g_in[1].ptr, g_in[2].ptr, rgb.ptr, len(d), bad.ptr)
    torch.cuda.synchronize()
    assert latched(engine) == 0
    for g in g_in:
        g.unchanged()
    got = rgb.read().view(np.uint32).reshape(-1, 3)
    diff = np.flatnonzero((got != want["rgb"].view(np.uint32)).any(-1))
    assert len(diff) == 0, f"{len(diff)} directions differ, first {d[diff[0]]} lod {lods[diff[0]]}: device {got[diff[0]].view(np.float32)}, host {want['rgb'][diff[0]]}"
    assert int(bad.read().view(np.uint64)[0]) == want["bad_directions"] > 0


# -- 6. one chained run
def test_chained_run(torch_mod, engine):
    name, kw = ec.CHAINED
    want = em.host_env_map(**kw)
    assert all(want[k] is not None for k in PRODUCTS)
    assert_equal(name, run(torch_mod, engine, kw), want)
