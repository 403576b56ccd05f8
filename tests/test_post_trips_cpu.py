"""The planes that make orbit_post_process' pixel loop take more than one trip (tests/post_chain_cases.py: TRIP_TARGETS under
TRIP_CAPS), on the host: the mirror (orbit_amd.post.host_post_process, the reference of
tests/test_post_trips_gpu.py) against the numpy restatement (tests/post_chain_ref.py) byte for byte, the closed-form
counters against both, and the trip shapes that the planes and caps must hold together, computed from the pixel count and
the cap alone.  No GPU."""
import numpy as np
import pytest

import post_chain_cases as pc
import post_chain_ref as ref
from orbit_amd import post

MODES = [(0, False, False), (0, True, False), (8, True, False), (0, True, True), (8, False, True)]  # test_post_chain_cpu.py's


@pytest.mark.parametrize("render_mode,with_bloom,bgra", MODES)
def test_the_mirror_equals_the_restatement_on_the_trip_planes(render_mode, with_bloom, bgra):
    for w, h in pc.TRIP_TARGETS:
        for marked in (True, False):
            color, bloom, expect = pc.trip_image(w, h, marked)
            mips = bloom if with_bloom else None
            got = post.host_post_process(color, mips, 1.7, 0.4, render_mode, bgra, fill=0xA5A5A5A5)
            want = ref.post_process(color, mips, 1.7, 0.4, render_mode, bgra)
            name = f"{w}x{h} marked={marked}"
            assert np.array_equal(got["ldr"].view(np.uint32), want["ldr"].view(np.uint32)), name
            assert np.array_equal(got["rgba8"], want["rgba8"]), name
            assert all(int(got["stats"][k]) == int(v) for k, v in want["stats"].items()), f"{name}: {got['stats']} != {want['stats']}"
            # the closed form: the placement's pixels, nothing else
            assert int(got["stats"]["pixels"]) == expect["pixels"] == w * h
            assert int(got["stats"]["nonfinite_pixels"]) == expect["nonfinite_pixels"], name
            assert int(got["stats"]["bloom_pixels"]) == (expect["bloom_pixels"] if with_bloom and render_mode == 0 else 0), name
            assert np.isfinite(got["ldr"]).all()


def test_the_placement():
    for w, h in pc.TRIP_TARGETS:
        n = w * h
        bad, lit = pc.trip_placement(n)
        assert not set(bad) & set(lit) and all(0 <= p < n for p in bad + lit)
        assert bad and (lit or n == 1)  # pixel 0 is non-finite on every plane
        color, bloom, expect = pc.trip_image(w, h)
        flat = color.reshape(-1, 4)
        assert np.flatnonzero(~np.isfinite(flat[:, :3]).all(axis=1)).tolist() == bad and np.flatnonzero(bloom).tolist() == lit
        assert expect == dict(pixels=n, nonfinite_pixels=len(bad), bloom_pixels=len(lit))
        assert (post.host_unpack(bloom[lit]) > 0.5).all() and np.isfinite(post.host_unpack(bloom)).all()
        color, bloom, expect = pc.trip_image(w, h, marked=False)  # the counters that stay 0
        assert np.isfinite(color).all() and not bloom.any() and expect["nonfinite_pixels"] == expect["bloom_pixels"] == 0
    assert len(pc.trip_placement(1025)[0]) != len(pc.trip_placement(1025)[1])  # a swapped counter shows


def test_the_trip_shapes_the_planes_hold():
    shapes = {(w * h, cap): pc.trip_shape(w * h, cap) for w, h in pc.TRIP_TARGETS for cap in pc.TRIP_CAPS}
    assert {w * h for w, h in pc.TRIP_TARGETS} >= {1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769, 1025}
    most = {max(s["trips"]) for s in shapes.values()}
    assert {1, 2, 3, 5} <= most
    last = lambda s: max(s["trips"]) > 1  # noqa: E731 (the shape's last trip is not its first)
    assert any(last(s) and s["partial_wave"] for s in shapes.values())       # 1025 under 1: one pixel in the fifth trip
    assert any(last(s) and s["dead_waves"] == 3 for s in shapes.values())    # 257 under 1: waves 1 to 3 of the second trip
    assert any(last(s) and s["dead_waves"] > 0 and not s["partial_wave"] for s in shapes.values())  # 64 x 5 under 1: one whole wave
    assert any(len(set(s["trips"])) == 2 for s in shapes.values())           # 769 under 3: trips 2, 1, 1
    assert shapes[(769, 3)]["trips"] == [2, 1, 1] and shapes[(1025, 1)]["trips"] == [5] and shapes[(1025, 2)]["trips"] == [3, 2]
    assert shapes[(513, 1)] == dict(grid=1, trips=[3], partial_wave=True, dead_waves=3)
    assert shapes[(512, 2)] == dict(grid=2, trips=[1, 1], partial_wave=False, dead_waves=0)
    # the grid is min(need, cap): no launch holds a workgroup without a trip.  300 pixels under a cap of 3 are two
    # workgroups of one trip each, the second with 44 pixels: a partial wave and three dead ones
    assert shapes[(300, 3)] == dict(grid=2, trips=[1, 1], partial_wave=True, dead_waves=3)
    assert all(min(s["trips"]) >= 1 and s["grid"] <= cap for (_, cap), s in shapes.items())
    # uncapped on the resident grid of a 256-CU device, none of these planes takes a second trip: what the hook is for
    assert all(pc.trip_shape(w * h, 0)["trips"] == [1] * pc.trip_shape(w * h, 0)["grid"] for w, h in pc.TRIP_TARGETS)


def test_each_counter_is_shared_every_way():
    for marks_of in (lambda n: pc.trip_placement(n)[0], lambda n: pc.trip_placement(n)[1]):
        held = {}
        for w, h in pc.TRIP_TARGETS:
            for cap in pc.TRIP_CAPS:
                held[(w * h, cap)] = pc.trip_shares(marks_of(w * h), w * h, cap)
        assert all({"trips", "waves", "workgroups"} <= set().union(*(v for (_, c), v in held.items() if c == cap)) for cap in (2, 3))
        assert {"trips", "waves"} <= held[(1025, 1)] and "workgroups" not in held[(1025, 1)]
        assert {"trips", "waves", "workgroups"} <= held[(1025, 2)]  # all three in one launch
        assert held[(1, 1)] == set()
