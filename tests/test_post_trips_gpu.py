"""orbit_post_process on the MI355X with its pixel loop entered MORE THAN ONCE per wave: the planes of
tests/post_chain_cases.py's TRIP_TARGETS under caps of 1, 2 and 3 workgroups (orbit_ctx_set_visibility_grid) — 1, 2, 3 and 5
trips, a last trip with a partial wave and with wholly dead waves, a workgroup of one trip beside one of two —, non-finite and
bloom-marked pixels placed so that each counter gets shares from two trips of a wave, two waves of a workgroup and two
workgroups; both render modes, bloom given and NULL, ORBIT_POST_BGRA, each output alone, NULL stats, counters that stay 0;
one natural-grid run on a 1921 x 1081 target, where the resident grid itself takes three trips or more; a capped first call
of a fresh context captured into a graph.  Bytes and counters equal the host mirror's (tests/test_post_trips_cpu.py holds it
to the restatement), nonfinite_pixels and bloom_pixels also the placement's closed form; buffers sit between guards."""
import numpy as np
import pytest

import post_chain_cases as pc
import test_post_chain_gpu as tpg
from orbit_amd import post
from test_gpu_parity import dev, host
from test_raster_depth_gpu import latched

pytestmark = pytest.mark.gpu
MODES = [(0, False, False), (0, True, False), (8, True, False), (0, True, True), (8, False, True)]  # render_mode, bloom given, bgra
KW = dict(exposure=1.7, bloom_intensity=0.4)


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
    e.set_visibility_grid(0)
    e.close()


@pytest.fixture(scope="module")
def mirrors():
    """the mirror's results by (target, marked, mode): computed once — they do not depend on the grid —, left unchanged"""
    return {}


def mirror_of(mirrors, w, h, marked, mode):
    key = (w, h, marked, mode)
    if key not in mirrors:
        color, bloom, expect = pc.trip_image(w, h, marked)
        render_mode, with_bloom, bgra = mode
        mips = bloom if with_bloom else None
        mirrors[key] = (color, mips, expect, post.host_post_process(color, mips, render_mode=render_mode, bgra=bgra, **KW))
    return mirrors[key]


@pytest.mark.parametrize("cap", pc.TRIP_CAPS)
def test_the_trip_planes_under_a_cap(torch_mod, engine, mirrors, cap):
    shapes = [pc.trip_shape(w * h, cap) for w, h in pc.TRIP_TARGETS]  # what this cap is there for
    assert max(max(s["trips"]) for s in shapes) >= 2 and any(max(s["trips"]) > 1 and s["partial_wave"] for s in shapes)
    assert any(max(s["trips"]) > 1 and s["dead_waves"] == 3 for s in shapes)
    assert latched(engine) == 0
    try:
        engine.set_visibility_grid(cap)
        for w, h in pc.TRIP_TARGETS:
            for marked in (True, False):
                for mode in MODES:
                    render_mode, with_bloom, bgra = mode
                    color, mips, expect, want = mirror_of(mirrors, w, h, marked, mode)
                    name = f"{w}x{h} marked={marked} mode={mode} (cap {cap})"
                    got = tpg.run_post(torch_mod, engine, color, mips, render_mode=render_mode, bgra=bgra, **KW)
                    tpg.assert_post(name, got, want)
                    assert int(got["stats"]["pixels"]) == w * h and int(got["stats"]["nonfinite_pixels"]) == expect["nonfinite_pixels"], name
                    assert int(got["stats"]["bloom_pixels"]) == (expect["bloom_pixels"] if with_bloom and render_mode == 0 else 0), name
    finally:
        engine.set_visibility_grid(0)
    assert latched(engine) == 0


@pytest.mark.parametrize("cap", pc.TRIP_CAPS)
def test_each_output_alone_under_a_cap(torch_mod, engine, mirrors, cap):
    try:
        engine.set_visibility_grid(cap)
        for w, h in ((1025, 1), (769, 1), (300, 1), (257, 3)):
            color, mips, expect, want = mirror_of(mirrors, w, h, True, MODES[1])
            for without in (("ldr",), ("rgba8",), ("stats",), ("ldr", "stats"), ("rgba8", "stats")):
                got = tpg.run_post(torch_mod, engine, color, mips, without=without, **KW)
                tpg.assert_post(f"{w}x{h} without {without} (cap {cap})", got, want)
                assert all(got[k] is None for k in without)
    finally:
        engine.set_visibility_grid(0)


def test_the_resident_grid_takes_several_trips(torch_mod, engine):
    """No cap: visibility_tile_cases.natural_target's 1921 x 1081 (or taller) plane, marked pixels in the first block of 256, in
    the last, partial one and one resident grid's worth further on"""
    import visibility_tile_cases as tc

    num_cus = torch_mod.cuda.get_device_properties(0).multi_processor_count
    w, h, _ = tc.natural_target(num_cus)
    pixels, per_trip = w * h, 8 * num_cus * pc.POST_THREADS
    trips = -(-pixels // per_trip)
    shape = pc.trip_shape(pixels, 0, 8 * num_cus)
    assert trips >= 3 and max(shape["trips"]) == trips and pixels % per_trip != 0 and (shape["partial_wave"] or shape["dead_waves"] > 0)
    assert len(set(shape["trips"])) == 2  # a workgroup with one trip fewer beside the others
    rng = np.random.default_rng(5)
    color = np.ones((h, w, 4), np.float32)
    color[..., :3] = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32) ** 3 * 4.0
    bloom = np.zeros(pixels, np.uint32)
    flat = color.reshape(-1, 4)
    bad = sorted({0, 67, per_trip, per_trip + 67, 2 * per_trip + 5, pixels - 1})  # two trips of one wave, two waves, two workgroups
    lit = sorted({1, 130, 300, per_trip + 1, 2 * per_trip + 300, pixels - 2})
    for i, p in enumerate(bad):
        flat[p, p % 3] = (np.nan, np.inf, -np.inf)[i % 3]
    bloom[lit] = pc.TRIP_BLOOM_WORD
    assert {"trips", "waves", "workgroups"} <= pc.trip_shares(bad, pixels, 0, 8 * num_cus) & pc.trip_shares(lit, pixels, 0, 8 * num_cus)
    assert latched(engine) == 0
    engine.set_visibility_grid(0)
    want = post.host_post_process(color, bloom, **KW)
    got = tpg.run_post(torch_mod, engine, color, bloom, **KW)
    tpg.assert_post(f"natural grid {w} x {h}", got, want)
    assert int(got["stats"]["nonfinite_pixels"]) == len(bad) and int(got["stats"]["bloom_pixels"]) == len(lit)


def test_a_capped_first_call_captures_into_a_graph(torch_mod):
    torch = torch_mod
    from orbit_amd.engine import Engine

    w, h = 1025, 1
    images = [pc.trip_image(w, h, True), pc.trip_image(w, h, False), pc.trip_image(w, h, True)]
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        color, bloom = dev(torch, images[0][0]), dev(torch, images[0][1])
        ldr = torch.zeros(4 * w * h + 4, dtype=torch.float32, device="cuda")
        rgba8 = torch.zeros(4 * w * h + 4, dtype=torch.uint8, device="cuda")
        stats = torch.full((4,), 7, dtype=torch.int32, device="cuda")
        eng.set_visibility_grid(1)  # five trips of one workgroup
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.post_process(color, w, h, bloom=bloom, ldr=ldr, rgba8=rgba8, stats=stats, **KW)
        eng.set_visibility_grid(0)  # (the captured launch carries its grid)
        for img, words, expect in images:
            color.copy_(dev(torch, img))
            bloom.copy_(dev(torch, words))
            want = post.host_post_process(img, words, **KW)
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == 0
                assert host(ldr, np.float32)[:-4].tobytes() == want["ldr"].tobytes() and not host(ldr, np.float32)[-4:].any()
                assert host(rgba8, np.uint8)[:-4].tobytes() == want["rgba8"].tobytes() and not host(rgba8, np.uint8)[-4:].any()
                assert host(stats, np.uint32).tobytes() == want["stats"].tobytes()
                assert int(want["stats"]["nonfinite_pixels"]) == expect["nonfinite_pixels"] and int(want["stats"]["bloom_pixels"]) == expect["bloom_pixels"]
    finally:
        eng.set_visibility_grid(0)
        eng.close()
