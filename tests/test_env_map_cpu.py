"""The host mirror of orbit_env_map and orbit_env_sample (include/orbit_abi_ext.h E0-E12, DESIGN.md §4.30;
orbit_amd.env_map.host_env_map / host_env_sample, the reference of tests/test_env_map_gpu.py) against tests/env_map_ref.py,
the independent numpy restatement of the env_map shaders, brdf_integration.frag and the loader: every half of the four
products and every counter over tests/env_map_cases.py, each product alone and from a caller's sky cube; E1 derived two
ways for all six layers; E0's rounding; the sampler on the hostile directions; the census of what the matrix exercises;
the figures against the GLSL in float64 and the routines' errors (profiles/env_map_cpu.json keeps them; held at the
recorded value plus one unit of its last printed digit); the argument errors on the mirror and on the entry point; the
layout call; the sanitizer program.  No GPU."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import subprocess
from decimal import Decimal

import numpy as np
import pytest

import env_map_cases as ec
import env_map_ref as ref
from orbit_amd import _lib, passes
from orbit_amd import env_map as em

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCTS = ("sky", "irradiance", "prefiltered", "brdf")
CASES = ec.chain_cases()


def tool():
    spec = importlib.util.spec_from_file_location("count_env_map", os.path.join(ROOT, "tools", "count_env_map.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def restated(kw, sky=None, census=None):
    return ref.env_map(pano=None if sky is not None else kw["equirect"], sky_words=sky, census=census,
                       **{k: v for k, v in kw.items() if k != "equirect"})


def assert_equal(name, got, want):
    for k in PRODUCTS:
        if want[k] is None:
            assert got[k] is None or k == "sky", (name, k)
            continue
        diff = np.flatnonzero(got[k] != want[k])
        assert len(diff) == 0, f"{name}: {len(diff)} halves of {k} differ, first {diff[0]}: mirror {got[k][diff[0]]:#x}, restated {want[k][diff[0]]:#x}"
    assert {k: int(got["stats"][k]) for k in want["stats"]} == want["stats"], name
    assert int(got["stats"]["_pad"]) == 0


@pytest.fixture(scope="module")
def matrix():
    """every case once through the mirror (with its census) and the restatement (with its own)"""
    out = {}
    for name, kw in CASES:
        census = dict.fromkeys(em.CENSUS, 0)
        out[name] = (em.host_env_map(want_census=True, fill=0xA5A5, **kw), restated(kw, census=census), census)
    return out


# -- 1. mirror = restatement
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_mirror_equals_restatement(matrix, name):
    got, want, _ = matrix[name]
    assert_equal(name, got, want)


@pytest.mark.parametrize("product", PRODUCTS)
def test_each_product_alone_and_from_a_callers_sky(matrix, product):
    name, kw = CASES[3]
    whole = matrix[name][0]
    alone = {k: (0 if k.endswith("_size") and k[:-5] in PRODUCTS[1:] and k[:-5] != product else v) for k, v in kw.items()}
    if product == "brdf":
        alone["sky_size"] = 0
    got = em.host_env_map(**alone)
    assert [k for k in PRODUCTS if got[k] is not None] == sorted({"sky", product} - ({"sky"} if product == "brdf" else set()), key=PRODUCTS.index)
    assert np.array_equal(got[product], whole[product])
    if product in ("irradiance", "prefiltered"):
        sky_before = whole["sky"].copy()
        got = em.host_env_map(sky=sky_before, **{k: v for k, v in alone.items() if k != "equirect"})
        assert np.array_equal(got["sky"], sky_before), "a caller's sky cube was written"
        assert_equal(name, got, restated(alone, sky=sky_before))
        assert np.array_equal(got[product], whole[product])


# -- 2. E1 both ways, E0's rounding, the layout
def test_texel_directions_both_ways():
    for face in range(6):
        V = ref.look_at_rh(*ref.VIEWS[face])
        for n in (1, 2, 3, 5, 16):
            want = ref.local_pos(face, n, F)
            for py in range(n):
                for px in range(n):
                    got = em.host_direction(face, px, py, n)
                    cx, cy = F(F(2.0) * F(px + 0.5)) / F(n) - F(1.0), F(1.0) - F(F(2.0) * F(px * 0 + py + 0.5)) / F(n)
                    by_matrix = V.T @ np.array([cx, cy, 1.0])  # transpose(V) * (cx, cy, 1), in float64: exact here
                    assert np.array_equal(got, by_matrix.astype(F)), (face, n, px, py, got, by_matrix)
                    assert got.tobytes() == np.array([c[py, px] for c in want], F).tobytes()  # and the signs of the zeros
                    # what covers the target is the cube's face at view z = +1: the point maps back to (cx, cy, 1)
                    assert np.allclose(V @ got.astype(np.float64), [cx, cy, 1.0], atol=1e-7)
    # against Vulkan's face table the texel's own direction lands on the layer opposite in x and z: the rotation about Y
    for face, seen in zip(range(6), (1, 0, 2, 3, 5, 4)):
        d = em.host_direction(face, 1, 2, 5)
        assert int(ref.face_select([np.float64(c) for c in d])[0]) == seen


def test_half_rounding_and_layout():
    # E0: every finite fp16 value, the midpoint to its upper neighbour and a step of fp32 either side of both, the values
    # around 65504 / 65520, below the smallest subnormal and the non-finite ones, against numpy's own round-to-nearest-even
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    mid = (h + np.append(h[1:], 65536.0)) / 2  # exact in float32: 12 significant bits at most
    x = np.concatenate([h, mid]).astype(F)
    x = np.concatenate([x, np.nextafter(x, F(np.inf)), np.nextafter(x, F(-np.inf)), F([65519.996, 65520.0, 1e30, 3.4e38, 2.0 ** -25, 2.9e-8, 1e-40])])
    x = np.concatenate([x, -x, F([np.inf, -np.inf, np.nan])])
    got = em.host_half(x)
    want, bad = ref.to_half(x)
    fin = ~bad
    assert bad.sum() == 3 and np.isnan(got[bad]).all()
    assert np.array_equal(got[fin].view(np.uint32), want[fin].astype(F).view(np.uint32)), x[fin][got[fin].view(np.uint32) != want[fin].astype(F).view(np.uint32)][:5]
    assert got[fin].max() == 65504.0 and got[fin].min() == -65504.0
    # the layout against the restatement's, and the refused shapes
    for sky, irr, pre, levels, brdf in ((16, 8, 17, 5, 17), (1, 1, 1, 5, 1), (4096, 32, 512, 5, 512), (0, 0, 5, 13, 0), (1024, 0, 0, 0, 0)):
        lay = em.layout(sky, irr, pre, levels, brdf)
        sizes, offsets = ref.layout(sky, sky.bit_length())
        assert lay["sky_sizes"] == (sizes if sky else []) and lay["sky_offsets"] == list(offsets[:-1] if sky else []) and lay["sky_texels"] == (offsets[-1] if sky else 0)
        sizes, offsets = ref.layout(pre, levels if pre else 0)
        assert lay["prefiltered_sizes"] == sizes and lay["prefiltered_offsets"] == list(offsets[:-1]) and lay["prefiltered_texels"] == offsets[-1]
        assert lay["irradiance_texels"] == 6 * irr * irr and lay["brdf_texels"] == brdf * brdf
    for args in ((3, 0, 0, 0, 0), (8192, 0, 0, 0, 0), (0, 4097, 0, 0, 0), (0, 0, 4, 0, 0), (0, 0, 4, 14, 0), (0, 0, 0, 0, 4097)):
        with pytest.raises(_lib.OrbitError):
            em.layout(*args)
    assert _lib.load().orbit_env_map_layout(4, 0, 0, 0, 0, None) == _lib.E_INVALID


# -- 3. the sampler on the hostile directions
@pytest.mark.parametrize("size,levels", ec.SAMPLE_CUBES)
def test_sampler_equals_restatement(size, levels):
    cube = ec.noise_cube(size, levels)
    d, lods = ec.sample_directions(levels)
    got = em.host_env_sample(cube, size, levels, d, lods, want_census=True)
    rgb, bad = ref.Cube(cube, size, levels, F).sample([d[:, 0], d[:, 1], d[:, 2]], lods)
    diff = np.flatnonzero((got["rgb"].view(np.uint32) != rgb.astype(F).view(np.uint32)).any(-1))
    assert len(diff) == 0, f"{len(diff)} directions differ, first {d[diff[0]]} lod {lods[diff[0]]}: mirror {got['rgb'][diff[0]]}, restated {rgb[diff[0]]}"
    assert got["bad_directions"] == int(bad.sum()) == 6 * 8
    census = got["census"]
    assert (census[em.CENSUS_MAJOR] > 0).all(), "a layer is never the major axis"
    assert (census[em.CENSUS_EDGE] > 0).all() and (census[em.CENSUS_CORNER] > 0).all(), "an edge or corner neighbour is never read"
    assert (census[em.CENSUS["two_level_taps"]] > 0) == (levels > 1)
    # explicit level numbers are exact: lod m returns level m's bilinear value alone, and beyond the last level the last
    whole = np.flatnonzero(lods == np.floor(lods))
    for m in sorted(set(int(v) for v in lods[whole] if 0 <= v < levels)):
        at = whole[lods[whole] == m]
        alone = ref.Cube(cube, size, levels, F)._level(m, *_face_st(d[at]))
        ok = ~bad[at]
        assert np.array_equal(got["rgb"][at][ok].view(np.uint32), alone.astype(F)[ok].view(np.uint32))


def _face_st(d):
    safe = np.where(np.isfinite(d).all(-1, keepdims=True) & (d != 0).any(-1, keepdims=True), d, F(1.0))
    face, sc, tc, ma = ref.face_select([safe[:, 0], safe[:, 1], safe[:, 2]])
    return face, (F(0.5) * sc) / ma + F(0.5), (F(0.5) * tc) / ma + F(0.5)


# -- 4. the census: what the matrix exercises
def test_census(matrix):
    total = np.zeros(em.CENSUS_SIZE, np.uint64)
    mine = dict.fromkeys(em.CENSUS, 0)
    nonfinite = dict.fromkeys(("sky_nonfinite", "prefiltered_nonfinite", "bad_directions"), 0)
    for name, (got, _, census) in matrix.items():
        total += got["census"]
        for k in ("z_up", "x_up", "ndl_not_positive", "weight_zero_texels", "roughness_zero_texels"):
            assert int(got["census"][em.CENSUS[k]]) == census[k], (name, k)  # the mirror's count is the restatement's
            mine[k] += census[k]
        for k in nonfinite:
            nonfinite[k] += int(got["stats"][k])
    assert (total[em.CENSUS_MAJOR] > 0).all(), "a layer is never the major axis"
    assert (total[em.CENSUS_EDGE] > 0).all() and (total[em.CENSUS_CORNER] > 0).all(), "an edge or corner neighbour is never read"
    for k in ("z_up", "x_up", "ndl_not_positive", "roughness_zero_texels", "two_level_taps", "nan_frame_texels"):
        assert total[em.CENSUS[k]] > 0, k
    # both NaN sources: the odd irradiance sizes' frame (2 texels per odd size: the centres of the +-Y layers) ...
    odd = sum(1 for _, kw in CASES if kw["irradiance_size"] % 2)
    assert total[em.CENSUS["nan_frame_texels"]] == 2 * odd and nonfinite["bad_directions"] > 0
    # ... and the hostile panorama's NaN texels.  totalWeight == 0 cannot occur under E6 as written: sample 0 has Xi = (0, 0),
    # so cosTheta = 1, H = N and dotNL = 1 whatever the roughness; every texel's weight is at least 1.  The counter stays, and
    # the matrix (sample counts 1 and 2, roughness 1 among them) shows it at 0 with dotNL <= 0 samples beside it
    assert total[em.CENSUS["weight_zero_texels"]] == 0 == nonfinite["prefiltered_nonfinite"]
    assert nonfinite["sky_nonfinite"] > 0


def test_panorama_gradients_show_the_rotation_and_the_flip():
    # gradient_u: red grows with u.  The sky cube's +X layer (layer 0) holds in_local_pos = (-1, ..): u = atan(z, -1) near
    # +-pi, the panorama's seam, not its centre: the rotation by 180 degrees about Y.  Layer 1 holds the centre (u = 0.5)
    got = em.host_env_map(equirect=ec.panorama("gradient_u"), sky_size=4)
    level0 = got["sky"][:6 * 16 * 4].view(np.float16).reshape(6, 4, 4, 4).astype(F)
    assert np.abs(level0[1, 1:3, 1:3, 0] - 0.5).max() < 0.05 and np.abs(level0[0, 1:3, 1:3, 0] - 0.5).min() > 0.3
    # gradient_v: blue grows downwards in the panorama; uv.y = 1 - uv.y puts the panorama's top row at asin = +pi / 2: layer 2 (+Y)
    pano = ec.panorama("gradient_v")
    got = em.host_env_map(equirect=pano, sky_size=4)
    level0 = got["sky"][:6 * 16 * 4].view(np.float16).reshape(6, 4, 4, 4).astype(F)
    assert level0[2, :, :, 2].mean() < 0.5 < 1.5 < level0[3, :, :, 2].mean()


# -- 5. the figures against float64 and the routines' errors, held at the recorded values
def held(name, value, recorded):
    if recorded == 0:  # a recorded zero has no last digit to give way by: nothing may appear
        assert value == 0, f"{name}: {value} where 0 is recorded"
        return
    d = Decimal(repr(recorded))
    bound = float(d + Decimal(1).scaleb(d.as_tuple().exponent))
    assert value <= bound, f"{name}: {value} above the recorded {recorded} plus one unit of its last digit"


def test_figures_against_float64():
    t = tool()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "env_map_cpu.json")))
    routines = t.routine_errors()
    for k, v in routines.items():
        print(k, v)
        held(k, v, recorded["routines"][k])
    for over, figures in (("matrix", t.matrix_figures()), ("chain", t.chain_figures())):
        for product, row in figures.items():
            for k, v in row.items():
                print(over, product, k, v)
                held(f"{over}.{product}.{k}", v, recorded[over][product][k])
    assert recorded["chain_over"] == dict(t.CHAIN, panorama="256 x 128, seeded")
    # E5's constant lod against lods from 2 x 2 quad differences
    quad = t.quad_lod_distance()
    assert quad["over"] == recorded["constant_lod_against_quad_lod"]["over"]
    for k in ("max_abs", "mean_abs", "max_rel"):
        print("constant_lod_against_quad_lod", k, quad[k])
        held(f"constant_lod_against_quad_lod.{k}", quad[k], recorded["constant_lod_against_quad_lod"][k])
    assert quad["max_abs"] > 0, "the two lods never part: the comparison compares nothing"


# -- 6. the argument errors, on the mirror and on the entry point without a device
def test_the_errors():
    bufs = {k: np.zeros(4096, np.uint8) for k in ("equirect", "sky", "irradiance", "prefiltered", "brdf", "stats")}
    good = dict({k: v.ctypes.data for k, v in bufs.items()}, equirect_w=4, equirect_h=2, sky_size=4, irradiance_size=2, prefiltered_size=4,
                prefiltered_levels=2, brdf_size=4, sample_count=4, sample_delta=0.5, brdf_sample_count=4)
    assert all(v % 16 == 0 for k, v in good.items() if k in bufs)
    lib = _lib.load()
    assert em.host_env_map_raw(em.env_map_job(**good)) == _lib.OK
    bad = [dict(sky_size=3), dict(sky_size=0), dict(sky_size=8192), dict(irradiance_size=0), dict(irradiance_size=4097), dict(prefiltered_size=0),
           dict(prefiltered_levels=0), dict(prefiltered_levels=14), dict(sample_count=0), dict(sample_count=65537), dict(brdf_size=0),
           dict(brdf_sample_count=0), dict(brdf_sample_count=65537), dict(sample_delta=0.0), dict(sample_delta=-0.5),
           dict(sample_delta=float("nan")), dict(sample_delta=float("inf")), dict(sample_delta=0.00005), dict(sample_delta=0.0049), dict(sky=good["sky"] + 4),
           dict(equirect=good["equirect"] + 8), dict(irradiance=good["irradiance"] + 2), dict(prefiltered=good["prefiltered"] + 4),
           dict(brdf=good["brdf"] + 2), dict(stats=good["stats"] + 4), dict(flags=1), dict(equirect_w=0), dict(equirect_h=0), dict(sky=None),
           dict(irradiance=good["prefiltered"]), dict(stats=good["sky"]),
           # ranges, not only first bytes: sky 4 is 1008 B, irradiance 2 is 192 B, prefiltered 4 x 2 is 960 B, the table 64 B
           dict(prefiltered=good["sky"] + 1000), dict(irradiance=good["sky"] + 8), dict(stats=good["brdf"] + 56), dict(sky=good["equirect"] + 120),
           dict(brdf=good["prefiltered"] + 956), dict(sky=None, irradiance=None, prefiltered=None, brdf=None)]
    for change in bad:
        job = em.env_map_job(**{**good, **change})
        assert em.host_env_map_raw(job) == passes.HOST_PANIC, change  # the mirror's Panic
        assert lib.orbit_env_map(None, C.byref(job), None) == _lib.E_INVALID, change  # the job is looked at before the context
        assert b"env_map:" in lib.orbit_last_error(None)
    # a good job and no context: refused for the context
    assert lib.orbit_env_map(None, C.byref(em.env_map_job(**good)), None) == _lib.E_INVALID and b"ctx is NULL" in lib.orbit_last_error(None)
    assert lib.orbit_env_map(None, None, None) == _lib.E_INVALID
    # NULL products are not made, and what is not asked for is not checked: a table alone needs no sky size
    only_table = em.env_map_job(None, None, None, None, good["brdf"], None, brdf_size=4, brdf_sample_count=4)
    assert em.host_env_map_raw(only_table) == _lib.OK
    sample = dict(cube=good["sky"], directions=good["equirect"], lods=good["irradiance"], rgb=good["prefiltered"], bad_directions=good["stats"],
                  size=4, levels=2, n=4)
    assert em.host_env_sample_raw(em.env_sample_job(**sample)) == _lib.OK
    assert em.host_env_sample_raw(em.env_sample_job(**{**sample, "n": 0, "directions": None, "lods": None, "rgb": None})) == _lib.OK
    for change in (dict(size=0), dict(size=4097), dict(levels=0), dict(levels=14), dict(cube=None), dict(rgb=None), dict(directions=None),
                   dict(lods=None), dict(cube=sample["cube"] + 4), dict(rgb=sample["rgb"] + 2), dict(bad_directions=sample["bad_directions"] + 4),
                   dict(flags=2), dict(rgb=sample["lods"]), dict(bad_directions=sample["cube"]),
                   # ranges: the cube is 960 B, directions and rgb 48 B, lods 16 B
                   dict(rgb=sample["cube"] + 952), dict(rgb=sample["directions"] + 44), dict(bad_directions=sample["lods"] + 8),
                   dict(bad_directions=sample["rgb"] + 40)):
        job = em.env_sample_job(**{**sample, **change})
        assert em.host_env_sample_raw(job) == passes.HOST_PANIC, change
        assert lib.orbit_env_sample(None, C.byref(job), None) == _lib.E_INVALID and b"env_sample:" in lib.orbit_last_error(None), change
    assert lib.orbit_env_sample(None, C.byref(em.env_sample_job(**sample)), None) == _lib.E_INVALID


# -- 7. the sanitizer program: a stand-alone host binary, built and run here
def test_sanitizer_program_runs_clean(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "sanitize_env_map"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(ROOT, "orbit_amd", "host"), os.path.join(ROOT, "tools", "sanitize_env_map.cpp"),
                            os.path.join(ROOT, "orbit_amd", "host", "orbit_env_map.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, (done.stdout[-1000:], done.stderr[-3000:])
    assert "refused" in done.stdout
