"""orbit_ssao on the device (include/orbit_abi_ext.h A1-A9) against the host mirror
(orbit_amd.post.host_ssao, which tests/test_ssao_cpu.py holds to the numpy restatement): every byte of raw, blurred, ao_pixel
and stats on the sizes, depth images and tables of tests/ssao_cases.py — SSAO sizes one texel either side of the shader's 8 x 8
group and the kernel's 16 x 16 tile, each with the screen at that size, at twice it and at twice it plus one —, every sample
count and radius pair of the matrix, each legal output subset; between guards, inputs unchanged, no latched error; the
argument errors; the first call of a fresh context captured into a graph and replayed; the whole frame on the device."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import raster_scene as rs
import ssao_cases as sc
from orbit_amd import _lib, post
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import Guarded, latched

pytestmark = pytest.mark.gpu
OUTPUTS = ("raw", "blurred", "ao_pixel")


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


def run(torch, engine, kw, want=OUTPUTS, with_stats=True):
    """One orbit_ssao call on guarded copies of a case's inputs -> dict(raw, blurred, ao_pixel, stats), None where not
    wanted; the outputs not wanted are handed NULL and their buffers must stay as they were"""
    depth = np.ascontiguousarray(kw["depth"], np.float32)
    sh, sw = depth.shape
    w, h = kw["ssao_w"], kw["ssao_h"]
    noise, samples = np.ascontiguousarray(kw["noise"]), np.ascontiguousarray(kw["samples"])
    g_in = [Guarded(torch, depth), Guarded(torch, noise), Guarded(torch, samples)]
    sizes = dict(raw=w * h, blurred=w * h, ao_pixel=4 * sw * sh, stats=24)
    out = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=n) for k, n in sizes.items()}
    wanted = tuple(want) + (("stats",) if with_stats else ())
    ptr = lambda k: out[k].ptr if k in wanted else None  # noqa: E731
    settings = {k: kw[k] for k in ("sample_count", "min_radius", "max_radius") if k in kw}
    engine.ssao(g_in[0].ptr, sw, sh, w, h, kw["projection"], kw["inverse_projection"], g_in[1].ptr, noise.shape[0], g_in[2].ptr, samples.shape[0],
                raw=ptr("raw"), blurred=ptr("blurred"), ao_pixel=ptr("ao_pixel"), stats=ptr("stats"), **settings)
    torch.cuda.synchronize()
    for g in g_in:
        g.unchanged()
    got = {}
    for k in sizes:
        if k in wanted:
            got[k] = out[k].read()
        else:
            out[k].unchanged()
            got[k] = None
    return got


def assert_equal(name, got, want):
    for k in OUTPUTS:
        if got[k] is not None:
            a, b = got[k], np.ascontiguousarray(want[k]).view(np.uint8).reshape(-1)
            diff = np.flatnonzero(a != b)
            assert len(diff) == 0, f"{name}: {len(diff)} bytes of {k} differ, first {diff[0]}: device {a[diff[0]]}, host {b[diff[0]]}"
    if got["stats"] is not None:
        assert got["stats"].tobytes() == want["stats"].tobytes(), f"{name}: device stats {got['stats'].view(L.SSAO_STATS)[0]} != host {want['stats']}"


# -- 1. every size, screen, image: bytes, counters, guards, inputs
@pytest.mark.parametrize("sizes", (sc.SSAO_SIZES[:7], sc.SSAO_SIZES[7:10], sc.SSAO_SIZES[10:]), ids=("small", "tile", "large"))
def test_every_case_equals_the_host_mirror(torch_mod, engine, sizes):
    assert latched(engine) == 0
    in_range = nonfinite = 0
    for name, kw in sc.all_cases(sizes):
        want = post.host_ssao(**kw)
        assert_equal(name, run(torch_mod, engine, kw), want)
        in_range, nonfinite = in_range + int(want["stats"]["samples_in_range"]), nonfinite + int(want["stats"]["nonfinite_pixels"])
    assert in_range > 0 and nonfinite > 0 and latched(engine) == 0


def test_sample_counts_radii_tables_and_the_searched_edges(torch_mod, engine):
    # the edge cases: samples with a proj component exactly 0 or 1, and one step outside (tests/ssao_cases.py edge_cases)
    for name, kw in sc.settings_cases() + sc.edge_cases():
        assert_equal(name, run(torch_mod, engine, kw), post.host_ssao(**kw))
    assert latched(engine) == 0


def test_each_legal_output_subset(torch_mod, engine):
    for size in ((1, 1), (9, 9), (33, 31)):
        for screen in sc.screens(*size)[1:]:
            name, kw = sc.case("floor_box", size, screen)
            want = post.host_ssao(**kw)
            for subset in sc.OUTPUT_SUBSETS:
                for with_stats in (True, False):
                    assert_equal(f"{name} {subset} stats={with_stats}", run(torch_mod, engine, kw, subset, with_stats), want)
    assert latched(engine) == 0


# -- 2. ORBIT_E_INVALID, decided before the context is looked at
def test_the_argument_errors(torch_mod, engine):
    t = torch_mod.zeros(8192, dtype=torch_mod.float32, device="cuda")
    a = t.data_ptr()
    proj, inv = sc.camera(8, 4)
    ok = dict(depth=a, screen_w=8, screen_h=4, ssao_w=4, ssao_h=2, projection=proj, inverse_projection=inv, noise=a + 1024, noise_size=4,
              samples=a + 2048, samples_size=64, raw=a + 4096, blurred=a + 8192, ao_pixel=a + 12288, stats=a + 16384)
    engine.ssao(**ok)
    bad = (dict(depth=None), dict(noise=None), dict(samples=None), dict(raw=None, blurred=None, ao_pixel=None), dict(raw=None), dict(blurred=None),
           dict(raw=None, blurred=None), dict(depth=a + 2), dict(ao_pixel=a + 12290), dict(samples=a + 2049), dict(noise=a + 1025), dict(stats=a + 16388),
           dict(screen_w=0), dict(screen_h=_lib.RASTER_MAX_DIM + 1), dict(ssao_w=0), dict(ssao_h=0), dict(ssao_w=9), dict(ssao_h=5),
           dict(noise_size=0), dict(noise_size=_lib.SSAO_MAX_NOISE_SIZE + 1), dict(samples_size=0), dict(samples_size=_lib.SSAO_MAX_SAMPLES_SIZE + 1),
           dict(sample_count=0), dict(sample_count=_lib.SSAO_MAX_SAMPLES + 1),
           dict(min_radius=-0.1), dict(max_radius=float("inf")), dict(min_radius=float("nan")), dict(flags=1), dict(flags=0x80000000),
           dict(raw=a), dict(blurred=a + 1024), dict(ao_pixel=a + 2048), dict(stats=a), dict(blurred=a + 4096), dict(ao_pixel=a + 8192),
           dict(stats=a + 12288))
    for kw in bad:
        with pytest.raises(_lib.OrbitError, match="ORBIT_E_INVALID: ssao:"):
            engine.ssao(**dict(ok, **kw))
    lib = _lib.load()
    j = _lib.Ssao()  # a bad job is rejected before the context is looked at: a NULL context is never reached
    assert lib.orbit_ssao(None, C.byref(j), None) == _lib.E_INVALID and lib.orbit_last_error(None).decode().startswith("ssao: screen")
    assert lib.orbit_ssao(None, None, None) == _lib.E_INVALID and lib.orbit_last_error(None).decode().startswith("ssao: job")
    torch_mod.cuda.synchronize()
    assert latched(engine) == 0


# -- 3. the first call of a fresh context captured into a graph, replayed twice per input
def test_the_first_call_captures_into_a_graph(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine

    size, screen = (33, 31), (67, 63)
    cases = [sc.case(k, size, screen)[1] for k in ("floor_box", "nonfinite", "noise")]
    (w, h), (sw, sh) = size, screen
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        depth = dev(torch, cases[0]["depth"])
        noise, samples = dev(torch, cases[0]["noise"]), dev(torch, cases[0]["samples"])
        raw, blurred = (torch.full((w * h + 8,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2))
        ao = torch.full((sw * sh + 4,), 7.0, dtype=torch.float32, device="cuda")
        stats = torch.full((3,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.ssao(depth, sw, sh, w, h, cases[0]["projection"], cases[0]["inverse_projection"], noise, 4, samples, 64, raw=raw, blurred=blurred,
                     ao_pixel=ao, stats=stats)
        for kw in cases:
            depth.copy_(dev(torch, kw["depth"]))
            want = post.host_ssao(**kw)
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == 0
                for t, k in ((raw, "raw"), (blurred, "blurred")):
                    got = host(t)
                    assert got[:-8].tobytes() == want[k].tobytes() and (got[-8:] == 0x5A).all(), (k, replay)
                got = host(ao, np.float32)
                assert got[:-4].tobytes() == want["ao_pixel"].tobytes() and (got[-4:] == 7.0).all(), replay
                assert host(stats).tobytes() == want["stats"].tobytes()
    finally:
        eng.close()


# -- 4. the whole frame on the device: orbit_raster_visibility -> orbit_visibility_resolve -> orbit_ssao on the glTF scene at 160 x
#       90, at full and at half resolution, against the mirror run on the downloaded depth
def test_the_frame_on_the_device(torch_mod, engine, oracle):
    torch = torch_mod
    spec = importlib.util.spec_from_file_location("count_ssao", os.path.join(rs.ROOT, "tools", "count_ssao.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    f = tool.host_frame(oracle, 160, 90)
    scene, frame, w, h, cap = f["scene"], f["frame"], 160, 90, f["scene"].cap_c
    d_data, d_pos, d_ent = (dev(torch, x) for x in (scene.meshlet_data, scene.vertices, scene.entities))
    vis = torch.zeros(w * h, dtype=torch.int64, device="cuda")
    depth = torch.zeros(w * h, dtype=torch.float32, device="cuda")
    for k, name in enumerate(("draw1", "draw2")):
        engine.raster_visibility(dev(torch, frame[name]), cap, d_data, d_pos, len(scene.vertices), d_ent, scene.entity_count, frame["view_proj"], vis,
                                 w, h, command_base=k * cap, clear=k == 0, meshlet_data_words=len(scene.meshlet_data), clip_near=True, wide_guard=True)
    engine.visibility_resolve(vis, w, h, depth=depth)
    noise, samples = post.ssao_tables(1)
    d_noise, d_samples = dev(torch, noise), dev(torch, samples)
    outs = {}
    for full_res in (True, False):
        sw_, sh_ = post.ssao_resolution(w, h, full_res)
        o = dict(raw=torch.zeros(sw_ * sh_, dtype=torch.uint8, device="cuda"), blurred=torch.zeros(sw_ * sh_, dtype=torch.uint8, device="cuda"),
                 ao_pixel=torch.zeros(w * h, dtype=torch.float32, device="cuda"), stats=torch.zeros(3, dtype=torch.int64, device="cuda"))
        engine.ssao(depth, w, h, sw_, sh_, f["projection"], f["inverse_projection"], d_noise, 4, d_samples, 64, **o)
        outs[full_res] = o
    torch.cuda.synchronize()
    assert latched(engine) == 0
    got_depth = host(depth, np.float32).reshape(h, w)
    assert got_depth.tobytes() == f["depth"].tobytes() and int((got_depth != 0).sum()) > 5000
    for full_res, o in outs.items():
        sw_, sh_ = post.ssao_resolution(w, h, full_res)
        want = post.host_ssao(got_depth, f["projection"], f["inverse_projection"], noise, samples, sw_, sh_)
        for k in OUTPUTS:
            assert host(o[k]).tobytes() == want[k].tobytes(), (k, full_res)
        assert host(o["stats"]).tobytes() == want["stats"].tobytes()
        assert int(want["stats"]["samples_in_range"]) > 10000 and len(np.unique(want["blurred"])) > 20  # occlusion, not a constant
