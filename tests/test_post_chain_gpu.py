"""orbit_bloom and orbit_post_process on the device (include/orbit_abi_ext.h B1-B9 and T1-T5) against the
host mirrors (orbit_amd.post.host_bloom / host_post_process, which tests/test_post_chain_cpu.py holds to the numpy
restatement and to the reference's binary): every byte of mips, ldr, rgba8 and both stats on the targets and images of
tests/post_chain_cases.py — targets one texel either side of the kernels' 16 x 16 tiles, the chain's edges —, with the
default launch, ORBIT_BLOOM_FORCE_PER_LEVEL and ORBIT_BLOOM_FORCE_DIRECT, max_levels 1, 2 and 6, filter_radius 0, 0.003,
0.025 and one large enough to leave the LDS staging on its own; both render modes, bloom NULL and given, ORBIT_POST_BGRA,
each output alone; between guards, inputs unchanged; the argument errors; the first call of a fresh context captured into
a graph and replayed; the whole frame on the device."""
import importlib.util
import os

import numpy as np
import pytest

import post_chain_cases as pc
import raster_scene as rs
from orbit_amd import _lib, post, raster
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import Guarded, latched

pytestmark = pytest.mark.gpu
FORMS = (None, "per_level", "direct")


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


def run_bloom(torch, engine, color, form=None, with_stats=True, **settings):
    """One orbit_bloom call on guarded copies -> (mips np.uint32, stats row or None); the guards are the canaries behind
    mips and stats"""
    h, w = color.shape[:2]
    lay = post.bloom_layout(w, h, settings.get("max_levels", 6))
    g_color = Guarded(torch, color)
    g_mips = Guarded(torch, np.zeros(0, np.uint8), nbytes=4 * lay["total_texels"])
    g_stats = Guarded(torch, np.zeros(0, np.uint8), nbytes=16) if with_stats else None
    engine.bloom(g_color.ptr, w, h, g_mips.ptr, stats=None if g_stats is None else g_stats.ptr, form=form, **settings)
    torch.cuda.synchronize()
    g_color.unchanged()
    return g_mips.read().view(np.uint32), None if g_stats is None else g_stats.read().view(L.BLOOM_STATS)[0]


def assert_bloom(name, got, want):
    mips, stats = got
    diff = np.flatnonzero(mips != want["mips"])
    assert len(diff) == 0, f"{name}: {len(diff)} texels differ, first {diff[0]}: device {mips[diff[0]]:#x}, host {want['mips'][diff[0]]:#x}"
    if stats is not None:
        assert stats.tobytes() == want["stats"].tobytes(), f"{name}: device stats {stats} != host {want['stats']}"


# -- 1. every target and image, each form: bytes, counters, guards, inputs
@pytest.mark.parametrize("form", FORMS)
def test_every_case_equals_the_host_mirror(torch_mod, engine, form):
    assert latched(engine) == 0
    clamped = nonfinite = 0
    for name, color, settings in pc.all_cases():
        want = post.host_bloom(color, **settings)
        assert_bloom(f"{name} ({form})", run_bloom(torch_mod, engine, color, form, **settings), want)
        clamped, nonfinite = clamped + int(want["stats"]["clamped_texels"]), nonfinite + int(want["stats"]["nonfinite_inputs"])
    assert clamped > 0 and nonfinite > 0 and latched(engine) == 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("max_levels", (1, 2, 6))
def test_short_chains_and_filter_radii(torch_mod, engine, form, max_levels):
    for w, h in pc.TARGETS:
        for kind in ("random", "checker"):
            color = pc.image(kind, w, h)
            for radius in (0.0, 0.003, 0.025):
                kw = dict(pc.SETTINGS[kind], filter_radius=radius, max_levels=max_levels)
                assert_bloom(f"{kind} {w}x{h} r={radius} levels<={max_levels} ({form})", run_bloom(torch_mod, engine, color, form, **kw),
                             post.host_bloom(color, **kw))


def test_a_large_filter_radius_leaves_the_staging(torch_mod, engine):
    # 0.5 x 65 source texels each way from a 16-texel tile is more than the LDS tile holds: the level runs with direct reads
    # under the default flags; 0.025 on 130 x 70 still fits
    for w, h in ((130, 70), (70, 33), (33, 31)):
        for kind in ("random", "checker", "blaze"):
            color = pc.image(kind, w, h)
            for radius in (0.025, 0.5, 3.0, 1e30):
                want = post.host_bloom(color, filter_radius=radius)
                for form in FORMS:
                    assert_bloom(f"{kind} {w}x{h} r={radius} ({form})", run_bloom(torch_mod, engine, color, form, filter_radius=radius), want)


def test_stats_may_be_null(torch_mod, engine):
    color = pc.image("nonfinite", 70, 33)
    assert_bloom("no stats", run_bloom(torch_mod, engine, color, with_stats=False), post.host_bloom(color))


# -- 2. orbit_post_process
def run_post(torch, engine, color, mips, without=(), **kw):
    h, w = color.shape[:2]
    g_color = Guarded(torch, color)
    g_bloom = None if mips is None else Guarded(torch, mips)
    sizes = dict(ldr=16 * w * h, rgba8=4 * w * h, stats=16)
    out = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=n) for k, n in sizes.items()}
    ptr = lambda k: None if k in without else out[k].ptr  # noqa: E731
    engine.post_process(g_color.ptr, w, h, bloom=None if g_bloom is None else g_bloom.ptr, ldr=ptr("ldr"), rgba8=ptr("rgba8"), stats=ptr("stats"), **kw)
    torch.cuda.synchronize()
    g_color.unchanged()
    if g_bloom is not None:
        g_bloom.unchanged()
    for k in without:
        out[k].unchanged()
    return dict(ldr=None if "ldr" in without else out["ldr"].read().view(np.float32).reshape(h, w, 4),
                rgba8=None if "rgba8" in without else out["rgba8"].read().reshape(h, w, 4),
                stats=None if "stats" in without else out["stats"].read().view(L.POST_STATS)[0])


def assert_post(name, got, want):
    for k in ("ldr", "rgba8", "stats"):
        if got[k] is not None:
            assert got[k].tobytes() == want[k].tobytes(), f"{name}: {k} differs"


@pytest.mark.parametrize("render_mode,with_bloom,bgra", [(0, False, False), (0, True, False), (8, True, False), (0, True, True), (8, False, True)])
def test_post_process_equals_the_host_mirror(torch_mod, engine, render_mode, with_bloom, bgra):
    bloomed = 0
    for name, color, settings in pc.all_cases():
        mips = post.host_bloom(color, **settings)["mips"] if with_bloom else None
        kw = dict(exposure=1.7, bloom_intensity=0.4, render_mode=render_mode, bgra=bgra)
        want = post.host_post_process(color, mips, **kw)
        assert_post(name, run_post(torch_mod, engine, color, mips, **kw), want)
        bloomed += int(want["stats"]["bloom_pixels"])
    assert (bloomed > 0) == (with_bloom and render_mode == 0) and latched(engine) == 0


def test_each_output_alone(torch_mod, engine):
    for w, h in ((1, 1), (17, 9), (130, 70)):
        color = pc.image("nonfinite", w, h)
        mips = post.host_bloom(color)["mips"]
        want = post.host_post_process(color, mips)
        for without in (("ldr",), ("rgba8",), ("stats",), ("ldr", "stats"), ("rgba8", "stats")):
            assert_post(f"{w}x{h} without {without}", run_post(torch_mod, engine, color, mips, without=without), want)


# -- 3. ORBIT_E_INVALID, decided before the context is looked at
def test_the_argument_errors(torch_mod, engine):
    t = torch_mod.zeros(4096, dtype=torch_mod.float32, device="cuda")
    a = t.data_ptr()
    ok = dict(color=a, width=8, height=4, mips=a + 2048)
    for kw in (dict(color=None), dict(mips=None), dict(color=a + 4), dict(mips=a + 2050), dict(stats=a + 1), dict(width=0), dict(height=_lib.RASTER_MAX_DIM + 1),
               dict(max_levels=0), dict(max_levels=7), dict(threshold=-1.0), dict(soft_threshold=float("nan")), dict(filter_radius=float("inf")),
               dict(form=2), dict(form=8), dict(mips=a)):
        with pytest.raises(_lib.OrbitError, match="ORBIT_E_INVALID: bloom:"):
            engine.bloom(**dict(ok, **kw))
    ok = dict(color=a, width=8, height=4, ldr=a + 2048, rgba8=a + 4096)
    for kw in (dict(color=None), dict(ldr=None, rgba8=None), dict(color=a + 8), dict(ldr=a + 2052), dict(rgba8=a + 4097), dict(bloom=a + 8194), dict(width=0),
               dict(render_mode=7), dict(exposure=float("nan")), dict(bloom_intensity=float("inf")), dict(bgra=2), dict(ldr=a), dict(bloom=a + 8192, rgba8=a + 8192),
               dict(rgba8=a + 2048)):
        with pytest.raises(_lib.OrbitError, match="ORBIT_E_INVALID: post_process:"):
            engine.post_process(**dict(ok, **kw))
    lib = _lib.load()
    import ctypes as C
    j = _lib.Bloom()  # a bad job is rejected before the context is looked at: a NULL context is never reached
    assert lib.orbit_bloom(None, C.byref(j), None) == _lib.E_INVALID and lib.orbit_last_error(None).decode().startswith("bloom: target")
    p = _lib.PostProcess()
    assert lib.orbit_post_process(None, C.byref(p), None) == _lib.E_INVALID and lib.orbit_last_error(None).decode().startswith("post_process: target")
    torch_mod.cuda.synchronize()
    assert latched(engine) == 0 and not t.any()


# -- 4. the first calls of a fresh context captured into a graph, replayed twice per input
def test_the_first_calls_capture_into_a_graph(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine

    w, h = 70, 33
    images = [pc.image(k, w, h) for k in ("random", "nonfinite", "random")]
    lay = post.bloom_layout(w, h)
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran either call
    try:
        color = dev(torch, images[0])
        mips = torch.full((lay["total_texels"] + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        ldr = torch.zeros(4 * w * h + 4, dtype=torch.float32, device="cuda")
        rgba8 = torch.zeros(4 * w * h + 4, dtype=torch.uint8, device="cuda")
        bloom_stats, post_stats = (torch.full((4,), 7, dtype=torch.int32, device="cuda") for _ in range(2))
        kw = dict(threshold=0.25, soft_threshold=1.0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.bloom(color, w, h, mips, stats=bloom_stats, **kw)
            eng.post_process(color, w, h, bloom=mips, ldr=ldr, rgba8=rgba8, stats=post_stats, exposure=1.5)
        for img in images:
            color.copy_(dev(torch, img))
            want_b = post.host_bloom(img, **kw)
            want_p = post.host_post_process(img, want_b["mips"], exposure=1.5)
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == 0
                got = host(mips, np.uint32)
                assert got[:-4].tobytes() == want_b["mips"].tobytes() and (got[-4:] == 0x5A5A5A5A).all(), replay
                assert host(bloom_stats, np.uint32).tobytes() == want_b["stats"].tobytes()
                assert host(ldr, np.float32)[:-4].tobytes() == want_p["ldr"].tobytes() and not host(ldr, np.float32)[-4:].any()
                assert host(rgba8, np.uint8)[:-4].tobytes() == want_p["rgba8"].tobytes() and not host(rgba8, np.uint8)[-4:].any()
                assert host(post_stats, np.uint32).tobytes() == want_p["stats"].tobytes()
    finally:
        eng.close()


# -- 5. the whole frame on the device: orbit_fragments_shade_shadowed -> orbit_bloom -> orbit_post_process on the glTF scene at
#       160 x 90, nothing copied to the host in between, against the mirrors' frame
def test_the_frame_on_the_device(torch_mod, engine, oracle):
    torch = torch_mod
    spec = importlib.util.spec_from_file_location("count_fragments_shade_shadowed", os.path.join(rs.ROOT, "tools", "count_fragments_shade_shadowed.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = tool._tool("count_fragments_shade")
    f = tool.host_frame(oracle, resolution=128, width=160, height=90)
    w, h, cc, s = f["width"], f["height"], f["cluster_count"], f["settings"]
    assert (w, h) == (160, 90)
    vis, wp, nrm, mat, mats, lights, image, index_buffer = f["args"][:8]
    d = [dev(torch, np.ascontiguousarray(x)) for x in (vis, wp, nrm, mat, mats, lights, image, index_buffer, f["shadow_rows"], f["atlas"])]
    color = torch.zeros(4 * w * h, dtype=torch.float32, device="cuda")
    lay = post.bloom_layout(w, h)
    mips = torch.zeros(lay["total_texels"], dtype=torch.int32, device="cuda")
    ldr = torch.zeros(4 * w * h, dtype=torch.float32, device="cuda")
    rgba8 = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
    bloom_stats, post_stats = (torch.zeros(4, dtype=torch.int32, device="cuda") for _ in range(2))
    engine.fragments_shade_shadowed(d[0], w, h, d[1], d[2], d[3], d[4], len(mats), d[5], len(lights), d[6], d[7], f["index_capacity"], cc, base.TILE,
                                    f["z_scale"], f["z_bias"], base.CUTOFF, f["frame"]["cam"].z_near, f["view_pos"], color, d[8], 1, d[9], 4,
                                    f["atlas"].shape[-1], s["blocker_search_radius"], s["normal_bias_scale"], s["oriented_bias"],
                                    shadow_index_base=f["shadow_index_base"], clear=True)
    engine.bloom(color, w, h, mips, stats=bloom_stats)
    engine.post_process(color, w, h, bloom=mips, ldr=ldr, rgba8=rgba8, stats=post_stats, exposure=4.0)
    torch.cuda.synchronize()
    assert latched(engine) == 0
    shaded = raster.host_fragments_shade_shadowed(*f["args"], **f["kw"])
    assert shaded["status"] == 0 and host(color, np.float32).tobytes() == shaded["color"].tobytes()
    want_b = post.host_bloom(shaded["color"])
    want_p = post.host_post_process(shaded["color"], want_b["mips"], exposure=4.0)
    assert host(mips, np.uint32).tobytes() == want_b["mips"].tobytes() and host(bloom_stats, np.uint32).tobytes() == want_b["stats"].tobytes()
    assert host(ldr, np.float32).tobytes() == want_p["ldr"].tobytes() and host(rgba8, np.uint8).tobytes() == want_p["rgba8"].tobytes()
    assert host(post_stats, np.uint32).tobytes() == want_p["stats"].tobytes()
    assert int(want_p["stats"]["bloom_pixels"]) > 10000 and len(np.unique(want_p["rgba8"][..., :3])) > 100  # a picture, not a constant
