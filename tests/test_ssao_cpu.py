"""The host mirror of orbit_ssao (include/orbit_abi_ext.h A1-A9; orbit_amd.post.host_ssao, the reference of
tests/test_ssao_gpu.py) against tests/ssao_ref.py, the independent numpy restatement of ssao.comp and ssao_blur.comp: every
byte of raw, blurred and ao_pixel and every counter over tests/ssao_cases.py, each legal output subset, between guard
bytes; A4's table against float64 for every (i, sample_count); the knife edges of A5's range test and range_check one ulp
either side; the census of what the cases exercise; the figures against the GLSL in float64 (profiles/ssao_cpu.json keeps
them; held at the recorded value plus one unit of its last printed digit); the argument errors.  No GPU."""
import ctypes as C
import importlib.util
import json
import math
import os
from decimal import Decimal

import numpy as np
import pytest

import ssao_cases as sc
import ssao_ref as ref
from orbit_amd import _lib, passes, post
from orbit_amd import layouts as L

F = np.float32
FILL = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tool():
    spec = importlib.util.spec_from_file_location("count_ssao", os.path.join(ROOT, "tools", "count_ssao.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assert_equal(name, got, want):
    for k in ("raw", "blurred"):
        diff = np.argwhere(got[k] != want[k])
        assert len(diff) == 0, f"{name}: {len(diff)} bytes of {k} differ, first at (y, x) = {diff[0]}: mirror {got[k][tuple(diff[0])]}, restated {want[k][tuple(diff[0])]}"
    assert got["ao_pixel"].tobytes() == want["ao_pixel"].astype(F).tobytes(), f"{name}: ao_pixel differs"
    assert {k: int(got["stats"][k]) for k in want["stats"]} == want["stats"], name


# -- 1. mirror = restatement, byte for byte and counter for counter
@pytest.mark.parametrize("sizes", (sc.SSAO_SIZES[:7], sc.SSAO_SIZES[7:10], sc.SSAO_SIZES[10:]), ids=("small", "tile", "large"))
def test_the_mirror_equals_the_restatement(sizes):
    for name, kw in sc.all_cases(sizes):
        assert_equal(name, post.host_ssao(**kw), ref.ssao(**kw))


def test_sample_counts_radii_and_tables():
    cases = sc.settings_cases()
    assert {kw["sample_count"] for _, kw in cases if "sample_count" in kw} == set(sc.SAMPLE_COUNTS)
    assert {(kw["min_radius"], kw["max_radius"]) for _, kw in cases if "min_radius" in kw} == set(sc.RADII)
    for name, kw in cases:
        assert_equal(name, post.host_ssao(**kw), ref.ssao(**kw))


def test_each_legal_output_subset_between_guard_bytes():
    for size in ((1, 1), (9, 9), (17, 15)):
        for screen in sc.screens(*size):
            name, kw = sc.case("floor_box", size, screen)
            want = ref.ssao(**kw)
            for subset in sc.OUTPUT_SUBSETS:
                got = post.host_ssao(want=subset, fill=FILL, **kw)
                for k in ("raw", "blurred", "ao_pixel"):
                    if k in subset:
                        assert got[k].tobytes() == want[k].astype(got[k].dtype).tobytes(), (name, subset, k)
                    else:
                        assert got[k] is None
                assert int(got["stats"]["samples_in_range"]) == want["stats"]["samples_in_range"]
            assert post.host_ssao(want_stats=False, **kw)["stats"] is None


def test_degenerate_noise_and_the_nan_byte():
    # A3: a (0, 0) noise texel makes the basis NaN; every sample's proj is then NaN and fails A5's range test, as in the shader:
    # nothing is added, the byte is 255
    name, kw = sc.case("floor_box", (9, 9), (18, 18), "zero_noise")
    got = post.host_ssao(**kw)
    assert (got["raw"] == 255).all() and int(got["stats"]["unoccluded_pixels"]) == 81 == int(got["stats"]["pixels"])
    assert int(got["stats"]["nonfinite_pixels"]) == 0 and int(got["stats"]["samples_in_range"]) == 0
    # A6: a NaN occlusion (min_radius 0 and a sample at its own surface: 0 / 0) stores 0 and counts
    got = post.host_ssao(**sc.case("floor_box", (17, 15), (35, 31), sample_count=2, min_radius=0.0, max_radius=0.0)[1])
    nan = int(got["stats"]["nonfinite_pixels"])
    assert nan > 0 and int((got["raw"] == 0).sum()) >= nan
    # -128 clamps to the value of -127
    kw = sc.case("floor_box", (9, 9), (18, 18), "snorm_clamp")[1]
    a = post.host_ssao(**kw)
    b = post.host_ssao(**dict(kw, noise=np.full((4, 4, 2), -127, np.int8)))
    assert a["raw"].tobytes() == b["raw"].tobytes() and int(a["stats"]["samples_in_range"]) > 0


# -- 2. A4's table against float64, every (i, sample_count)
def test_the_sample_table_against_float64():
    _, samples = post.ssao_tables(3, samples_size=100)
    worst, flips = 0.0, 0
    for count in range(1, 65):
        got = post.host_ssao_table(samples, count, 0.1, 0.5)
        assert got.tobytes() == ref.table(samples, count, 0.1, 0.5).tobytes(), count
        want = ref.table(samples, count, 0.1, 0.5, np.float64)
        worst = max(worst, float(np.abs(got[:, :3] - want[:, :3]).max()))
        # the radius: NearestRepeat's floor(fi * size) is a hard comparison, so float32 and float64 may pick neighbouring texels
        fi32, fi64 = np.arange(count, dtype=F) / F(count), np.arange(count) / count
        same = np.floor(fi32 * F(100)).astype(int) == np.floor(fi64 * 100).astype(int)
        flips += int((~same).sum())
        assert np.abs(got[same, 3] - want[same, 3]).max() <= 4 * 2.0 ** -24  # mix: two products and a sum of values at most 0.5
        assert np.abs(np.sqrt((got[:, :3].astype(np.float64) ** 2).sum(-1)) - 1.0).max() <= 4e-7  # unit directions
        assert (got[:, 2] > 0).all() and (got[:, 3] >= F(0.1)).all() and (got[:, 3] <= F(0.5)).all()
    print(f"A4's table: largest absolute error of a direction against float64 {worst:.3g}; {flips} of {64 * 65 // 2} samples pick another texel")
    # Vulkan's own bound for sin and cos, 2^-11, times sinTheta <= 1: a condition, not a measurement (H6's routines measure far
    # below it); 1e-6 covers the roundings of fi, 1 - fi, the square, the root (ill-conditioned near fi = 0) and the product
    assert worst <= 2.0 ** -11 + 1e-6 and flips < 64 * 65 // 2 // 10


# -- 3. A5's knife edges, on the mirror's own functions
def test_the_range_test_at_its_edges():
    up, down = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(-np.inf))  # noqa: E731
    inside = [(0.0, 0.5, 0.5), (1.0, 0.5, 0.5), (0.5, 0.0, 1.0), (0.5, 1.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-0.0, 0.5, 0.5), (down(1.0), up(0.0), 0.5)]
    outside = [(down(0.0), 0.5, 0.5), (up(1.0), 0.5, 0.5), (0.5, down(0.0), 0.5), (0.5, up(1.0), 0.5), (0.5, 0.5, down(0.0)), (0.5, 0.5, up(1.0)),
               (np.nan, 0.5, 0.5), (0.5, np.nan, 0.5), (0.5, 0.5, np.nan), (np.inf, 0.5, 0.5), (0.5, -np.inf, 0.5)]
    assert post.host_ssao_in_range(np.array(inside, F)).all() and not post.host_ssao_in_range(np.array(outside, F)).any()


def test_range_check_at_its_edges():
    rc = post.host_ssao_range_check
    # sample_depth 0.002 is a distance of 5; proj.w is the sample's own distance
    d = F(0.002)
    lin = F(0.01) / d
    assert rc(0.0, d, lin + F(1.0)) == 0.0                      # an argument of 0
    assert rc(1.0, d, lin + F(1.0)) == 1.0 == rc(1.0, d, lin - F(1.0))  # exactly 1
    assert rc(1.0, d, lin + F(0.5)) == 1.0                      # above 1
    assert rc(0.1, d, lin) == 1.0                               # x / 0 = +inf clamps to 1
    assert np.isnan(rc(0.0, d, lin))                            # 0 / 0
    assert rc(0.1, F(0.0), F(5.0)) == 0.0                       # an uncovered texel: 0.01 / 0 = inf, 0.1 / inf = 0
    # lin lies in [4, 8): adding 0.5 or 1 to it is exact, so are the differences, and 0.25 / 0.5, 0.25 / 1 are exact
    assert 4.0 <= lin < 7.0
    assert rc(0.25, d, lin + F(0.5)) == F(0.5) and rc(0.25, d, lin + F(1.0)) == F(0.15625)  # t = 0.5 and 0.25: strictly inside
    x = np.nextafter(F(1.0), F(0.0))                            # one ulp below 1: strictly inside
    assert 0.0 < rc(x, d, lin + F(1.0)) <= 1.0


def test_the_searched_edge_cases():
    # the same edges through the whole call: a sample with a proj component exactly 1, one exactly 0, and each one step outside,
    # on the mirror and on the restatement (tests/test_ssao_gpu.py runs the same cases on the device)
    cases = sc.edge_cases()
    assert len(cases) == 2 * len(sc.EDGE_SEARCHES)
    seen = dict.fromkeys(("proj_at_zero", "proj_at_one", "proj_below_zero", "proj_above_one"), 0)
    for (name_in, kw_in), (name_out, kw_out) in zip(cases[0::2], cases[1::2]):
        assert np.nextafter(F(kw_in["min_radius"]), F(np.inf)) == F(kw_out["min_radius"]), "neighbouring radii"
        c_in, c_out = sc.census(kw_in), sc.census(kw_out)
        moved = c_out["out_of_range"] - c_in["out_of_range"]
        assert moved > 0
        # the samples that leave sit exactly on an edge before and one step outside after
        assert c_in["proj_at_zero"] + c_in["proj_at_one"] == moved == c_out["proj_below_zero"] + c_out["proj_above_one"], (name_in, c_in, c_out)
        assert c_in["proj_at_zero"] == c_out["proj_below_zero"] and c_in["proj_at_one"] == c_out["proj_above_one"]
        for k in seen:
            seen[k] += c_in[k] + c_out[k]
        for name, kw in ((name_in, kw_in), (name_out, kw_out)):
            assert_equal(name, post.host_ssao(**kw), ref.ssao(**kw))
    print("searched edges:", seen)
    assert all(v > 0 for v in seen.values()), seen


# -- 4. the census: every branch, verdict and edge is exercised somewhere
def test_the_census():
    total = dict.fromkeys(post.SSAO_CENSUS, 0)
    per_image = {k: dict.fromkeys(post.SSAO_CENSUS, 0) for k in sc.IMAGES}
    for name, kw in sc.all_cases() + sc.settings_cases() + sc.edge_cases():
        c = sc.census(kw)
        for k, v in c.items():
            total[k] += v
            per_image[name.split()[0]][k] += v
    print("census:", total)
    assert all(v > 0 for v in total.values()), total
    fb = per_image["floor_box"]
    assert all(fb[k] > 0 for k in post.SSAO_CENSUS[:9]), fb  # the four branches, in / out of range, occluded / not, range_check inside (0, 1)
    assert per_image["plane"]["right_up"] == per_image["plane"]["right_down"] == 0  # every horizontal |dz| ties: left
    assert per_image["plane"]["tie_horizontal"] > 0 and per_image["uncovered"]["in_range"] == 0
    assert total["depth_equal"] > 0 and total["range_nan"] > 0 and total["range_zero"] > 0 and total["range_one"] > 0


def test_the_wrapped_neighbour_decides_column_0():
    # A1: the left neighbour of column 0 is pixel 0xFFFFFFFF, whose uv clamps to the far edge and whose x is enormous and POSITIVE.
    # Where A2 takes it (on a plane facing the camera every |dz| ties, and a tie takes left / up) the cross product changes
    # sign, the hemisphere points into the surface and the pixel darkens: column 0 and row 0 against their neighbours.  With a
    # signed pixel column 0 would look like column 1.  The restatement states the unsigned conversion on its own.
    for size, screen in (((32, 18), (64, 36)), ((64, 36), (64, 36))):
        kw = sc.case("plane", size, screen)[1]
        got = post.host_ssao(**kw)["raw"]
        assert got.tobytes() == ref.ssao(**kw)["raw"].tobytes()
        assert got[1:, 0].mean() < 100 and got[1:, 1].mean() > 200 and got[0, 1:].mean() < 100 and got[1, 1:].mean() > 200, size


# -- 5. against the GLSL in float64: profiles/ssao_cpu.json keeps the figures, over the case matrix and over the scene
def held(recorded, measured, figures, where):
    for k in figures:
        figure = Decimal(recorded[k])
        bound = figure + Decimal(1).scaleb(figure.as_tuple().exponent)  # one unit of the last printed digit
        print(f"{where} {k}: {measured[k]:.6g} (recorded {recorded[k]}, held at {bound})")
        assert measured[k] <= float(bound), (where, k)


def test_the_figures_against_float64(oracle):
    t = tool()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "ssao_cpu.json")))
    cases = t.measure_cases()
    held(recorded["printed"]["case_matrix"], cases, t.FIGURES, "case matrix")
    assert cases["nan_one_way_pixels"] <= recorded["case_matrix"]["nan_one_way_pixels"]  # a count: held as it is
    # the 100-instance scene at 320 x 180 and 160 x 90, full and half resolution: the figures README and DESIGN quote
    scene, census = t.measure_scene(oracle)
    held(recorded["printed"]["scene"], scene, t.FIGURES, "scene")
    assert scene["nan_one_way_pixels"] == 0 == recorded["scene"]["nan_one_way_pixels"] and scene["bytes"] == 90000
    assert [c["ssao"] for c in census] == [[320, 180], [160, 90], [160, 90], [80, 45]] and census == recorded["census"]


# -- 6. what the device answers with ORBIT_E_INVALID
def test_the_argument_errors():
    depth = sc.depth_image("plane", 8, 4)
    proj, inv = sc.camera(8, 4)
    noise, samples = post.ssao_tables(1)

    def job(**kw):
        raw, blurred, ao, stats = np.zeros(8, np.uint8), np.zeros(8, np.uint8), np.zeros(32, F), np.zeros(1, L.SSAO_STATS)
        keep = dict(depth=depth, noise=noise, samples=samples, raw=raw, blurred=blurred, ao_pixel=ao, stats=stats)
        j = _lib.Ssao()
        for k, v in keep.items():
            setattr(j, k, v.ctypes.data)
        _lib.fill_ssao(j, proj, inv, 8, 4, 4, 2, 4, 64, 32, 0.1, 0.5)
        for k, v in kw.items():
            setattr(j, k, v(keep) if callable(v) else v)
        return j, keep

    fn = passes.lib().orbit_host_ssao
    fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_void_p]
    j, keep = job()
    assert fn(C.byref(j), None) == 0
    at = lambda name, off=0: (lambda keep: keep[name].ctypes.data + off)  # noqa: E731
    bad = [dict(depth=None), dict(noise=None), dict(samples=None), dict(raw=None, blurred=None, ao_pixel=None), dict(raw=None), dict(blurred=None),
           dict(depth=at("depth", 2)), dict(ao_pixel=at("ao_pixel", 2)), dict(samples=at("samples", 1)), dict(noise=at("noise", 1)), dict(stats=at("stats", 4)),
           dict(screen_w=0), dict(screen_h=0), dict(screen_w=_lib.RASTER_MAX_DIM + 1), dict(ssao_w=0), dict(ssao_h=0), dict(ssao_w=9), dict(ssao_h=5),
           dict(noise_size=0), dict(noise_size=_lib.SSAO_MAX_NOISE_SIZE + 1), dict(samples_size=0), dict(samples_size=_lib.SSAO_MAX_SAMPLES_SIZE + 1),
           dict(sample_count=0), dict(sample_count=_lib.SSAO_MAX_SAMPLES + 1),
           dict(min_radius=-0.1), dict(max_radius=-1.0), dict(min_radius=math.nan), dict(max_radius=math.inf), dict(flags=1), dict(flags=1 << 31),
           dict(raw=at("depth")), dict(blurred=at("noise")), dict(ao_pixel=at("samples")), dict(stats=at("depth")), dict(blurred=at("raw")),
           dict(ao_pixel=at("blurred")), dict(stats=at("ao_pixel"))]
    for kw in bad:
        j, keep = job(**kw)
        assert fn(C.byref(j), None) == passes.HOST_PANIC, kw
        assert passes.lib().orbit_host_last_error().decode().startswith("ssao:"), kw
    assert fn(None, None) == passes.HOST_PANIC
    # the device entry point decides the same before it looks at the context
    lib = _lib.load()
    for kw in bad:
        j, keep = job(**kw)
        assert lib.orbit_ssao(None, C.byref(j), None) == _lib.E_INVALID and lib.orbit_last_error(None).decode().startswith("ssao:"), kw
    j, keep = job()
    assert lib.orbit_ssao(None, C.byref(j), None) == _lib.E_INVALID and lib.orbit_last_error(None).decode() == "ssao: ctx is NULL"


def test_resolution_and_tables():
    assert post.ssao_resolution(1920, 1080) == (960, 540) and post.ssao_resolution(1921, 1081) == (960, 540)
    assert post.ssao_resolution(1920, 1080, True) == (1920, 1080)
    n, s = post.ssao_tables(9)
    assert n.shape == (4, 4, 2) and n.dtype == np.int8 and s.shape == (64, 4) and s.dtype == np.uint8
    assert post.ssao_tables(9)[0].tobytes() == n.tobytes() and post.ssao_tables(10)[1].tobytes() != s.tobytes()
    assert post.SSAO_DEFAULTS == dict(sample_count=32, min_radius=0.1, max_radius=0.5, full_res=False)
