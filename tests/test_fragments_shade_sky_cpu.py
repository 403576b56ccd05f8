"""orbit_fragments_shade_sky's host mirror (orbit_amd.raster.host_fragments_shade_sky over csrc/sky_common.h; include/orbit_abi_ext.h
K1-K10) against the independent numpy restatement tests/fragments_shade_sky_ref.py: every colour float and
every counter over the case matrix of tests/fragments_shade_sky_cases.py; the census that shows every branch of K1-K9 taken;
each optional input alone; K10's equality with orbit_host_fragments_shade_shadowed; the skybox basis against the
reference's matrix product; the argument errors on the mirror and on the entry point without a device; the struct layout;
the recorded float64 figures; the sanitizer program.  No GPU."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import subprocess
from decimal import Decimal

import numpy as np
import pytest

import fragments_shade_shadowed_cases as sc
import fragments_shade_sky_cases as kc
import fragments_shade_sky_ref as ref
from orbit_amd import _lib, camera, env_map, passes, raster
from orbit_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "lights_walked", "shadow_factor", "cascade")
BLOCKS = ("stats", "shadow_stats", "sky_stats")


@pytest.fixture(scope="module")
def matrix(oracle):
    """[(case, the mirror's outputs with its census)], computed once"""
    return [(c, kc.mirror(c, want_census=True)) for c in kc.all_cases(oracle)]


def assert_equal(name, got, want, blocks=BLOCKS):
    for k in blocks:
        assert got[k].tobytes() == want[k].tobytes(), f"{name}: {k}: mirror {got[k]} != restatement {want[k]}"
    assert got["status"] == want["status"], name
    for k in PLANES:
        diff = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(diff) == 0, f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}: {got[k][tuple(diff[0])]!r} != {want[k][tuple(diff[0])]!r}"


# -- 1. mirror equals restatement on every colour float and every counter over the matrix
def test_mirror_equals_restatement(oracle, matrix):
    lit = boxed = 0
    for case, got in matrix:
        assert_equal(case.name, got, kc.restated(case, oracle))
        assert np.isfinite(got["color"]).all(), case.name  # L8
        lit, boxed = lit + int(got["sky_stats"]["sky_lit_pixels"]), boxed + int(got["sky_stats"]["skybox_pixels"])
    assert lit > 1500 and boxed > 300


def test_the_matrix_holds_what_the_issue_names(oracle):
    cases = kc.all_cases(oracle)
    shapes = {c.case.visibility.shape[::-1] for c in cases}
    assert {(1, 1), (8, 8), (9, 7), (73, 33)} <= shapes
    envs = [c.env for c in cases if c.env is not None]
    assert {e["irradiance_size"] for e in envs} == set(kc.IRRADIANCE_SIZES)
    assert {e["prefiltered_size"] for e in envs} == set(kc.PREFILTERED_SIZES) and {e["prefiltered_levels"] for e in envs} == set(kc.PREFILTERED_LEVELS)
    assert {e["brdf_size"] for e in envs} == set(kc.TABLE_SIZES)
    assert {c.sky["size"] for c in cases if c.sky is not None} == set(kc.SKY_SIZES)
    assert {c.skybox_lod for c in cases if c.sky is not None} >= {0.0, 0.5, 20.0}
    assert any(c.ao is None for c in cases) and any(c.ao is not None and np.isnan(c.ao).any() and (c.ao == -1).any() and (c.ao == 2).any() for c in cases)
    assert {True, False} == {c.staged for c in cases}


# -- 2. the census: every branch of K1-K9 is taken by the matrix
def test_census(matrix):
    total = np.zeros(raster.SKY_CENSUS_SIZE, np.uint64)
    for _, got in matrix:
        total += got["census"]
    for name, index in raster.SKY_CENSUS.items():
        assert total[index] > 0, f"no case takes {name}"
    assert (total[env_map.CENSUS_MAJOR] > 0).all(), "a layer no sampled direction has as its major axis"
    assert (total[env_map.CENSUS_EDGE] > 0).all(), "an edge no tap crosses"
    assert (total[env_map.CENSUS_CORNER] > 0).all(), "a corner no tap meets"
    assert total[env_map.CENSUS["two_level_taps"]] > 0
    # K5's whole lod (roughness 0.25 under 5 levels) takes E4's one-level path: in such a call the two-level count stays below the samples
    by_name = {c.name: g for c, g in matrix}
    directions = by_name["sky_directions_tile8"]
    assert 0 < directions["census"][env_map.CENSUS["two_level_taps"]] < directions["sky_stats"]["sky_evaluations"]
    assert total[raster.SKY_CENSUS_SIZE - 12:].sum() == 0  # the reserved tail


# -- 3. each optional input alone: environment only, skybox only, neither
@pytest.mark.parametrize("without", (("sky",), ("env",), ("env", "sky")))
def test_each_optional_input_alone(oracle, matrix, without):
    for case, full in matrix:
        if (case.env is None and "env" not in without) or (case.sky is None and "sky" not in without):
            continue
        part = case.without(*without)
        got = kc.mirror(part)
        assert_equal(f"{case.name} without {without}", got, kc.restated(part, oracle))
        covered = case.case.visibility != 0
        if "env" not in without:  # the lit pixels do not depend on the sky cube
            assert got["color"][covered].tobytes() == full["color"][covered].tobytes(), case.name
            assert int(got["sky_stats"]["skybox_pixels"]) == 0
        if "sky" not in without:  # nor the skybox on the environment
            assert got["color"][~covered].tobytes() == full["color"][~covered].tobytes(), case.name
            assert int(got["sky_stats"]["sky_evaluations"]) == 0
        if "env" in without and case.env is not None and int(full["sky_stats"]["sky_lit_pixels"]):
            assert int(got["stats"]["unserved_pixels"]) >= int(full["sky_stats"]["sky_lit_pixels"])  # K1: counted as before


# -- 4. K10: with neither, the bytes of orbit_host_fragments_shade_shadowed
def test_without_environment_and_sky_it_is_the_shadowed_call(oracle, matrix):
    shadowed_cases = [kc.SkyCase(s) for s in sc.all_cases(oracle)] + [kc.SkyCase(s) for s, _ in sc.tampers(oracle)]
    compared = 0
    for case in [c.without("env", "sky") for c, _ in matrix] + shadowed_cases:
        for mode in (0, 8):
            for clear in (True, False):
                new = kc.mirror(case, render_mode=mode, clear=clear, fill=0x5A5A5A5A)
                old = sc.mirror(case.shadow, render_mode=mode, clear=clear, fill=0x5A5A5A5A)
                for k in PLANES + ("stats", "shadow_stats"):
                    assert new[k].tobytes() == old[k].tobytes(), (case.name, mode, clear, k)
                assert new["status"] == old["status"] and not any(new["sky_stats"].tolist()), case.name
                compared += 1
    assert compared > 200


def test_render_mode_8_evaluates_nothing_of_k(oracle, matrix):
    for case, _ in matrix:
        got = kc.mirror(case, render_mode=8, clear=False, fill=0x5A5A5A5A, want_census=True)
        assert_equal(f"{case.name} heat map", got, kc.restated(case, oracle, render_mode=8, clear=False, fill=0x5A5A5A5A))
        assert not any(got["sky_stats"].tolist()) and not got["census"].any(), case.name
        old = sc.mirror(case.shadow, render_mode=8, clear=False, fill=0x5A5A5A5A)
        assert got["color"].tobytes() == old["color"].tobytes(), case.name  # uncovered pixels are left as before


# -- 5. the skybox basis against the reference's matrix product
@pytest.mark.parametrize("q", ((0, 0, 0, 1), (0, 0.7071068, 0, 0.7071068), (0.5, 0.5, 0.5, 0.5), (-0.2, 0.55, 0.1, 0.8), (0.3, -0.4, 0.5, -0.7)))
@pytest.mark.parametrize("fov_deg,aspect", ((90.0, 16.0 / 9.0), (45.0, 1.0), (120.0, 0.75)))
def test_skybox_basis(q, fov_deg, aspect):
    q = np.asarray(q, np.float64)
    q = np.float32(q / np.linalg.norm(q))
    got = camera.skybox_basis(q, fov_deg, aspect)
    want = ref.skybox_matrix_basis(q, float(np.deg2rad(np.float32(fov_deg))), aspect)
    for g, w, name in zip(got, want, ("sky_x", "sky_y", "sky_z")):
        assert g.dtype == np.float32 and g.shape == (3,)
        assert np.abs(g - w).max() <= 8 * 2.0 ** -24 * max(1.0, np.abs(w).max()), (name, g, w)  # a few float32 roundings of products of q
    # the ray of a pixel is the direction the reference's vertex shader interpolates: (matrix * (d, 1)).xy / w = (cx, cy)
    cx, cy = 0.375, -0.625
    d = cx * want[0] + cy * want[1] + want[2]
    f = 1.0 / np.tan(0.5 * float(np.deg2rad(np.float32(fov_deg))))
    x, y, z, w = (float(v) for v in q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    v = R.T @ d
    assert abs(f / aspect * v[0] / -v[2] - cx) < 1e-6 and abs(f * v[1] / -v[2] - cy) < 1e-6


# -- 6. the argument errors, on the mirror and on the entry point without a device
def test_the_errors(oracle):
    case = kc.SkyCase(kc.base_case("errors_9x7", oracle, 9, 7, 4, 5, ([kc.SKY, kc.SUN], [12])), kc.make_env(6, 8, 16, 5, 17), kc.make_sky(7, 16),
                      ao=kc.ao_plane(np.random.default_rng(8), 7, 9))
    a, k = case.args()
    lib = _lib.load()
    host = passes.lib().orbit_host_fragments_shade_sky
    host.restype, host.argtypes = C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]
    keep = []

    def job(**over):
        """the case's block over fresh arrays (kept alive in `keep`) with `over` set last; a callable value is given the block"""
        j, arrays = raster.host_fragments_shade_sky(*a, **dict(k, return_job=True))
        keep.append(arrays)
        for name, value in over.items():
            target = j if hasattr(j, name) else j.shadowed if hasattr(j.shadowed, name) else j.shadowed.shade
            setattr(target, name, value(j) if callable(value) else value)
        return j

    good = job()
    assert host(C.byref(good), None, None) == _lib.OK
    base = lambda j: j.shadowed.shade  # noqa: E731
    off = lambda field, n, of=(lambda j: j): (lambda j: getattr(of(j), field) + n)  # noqa: E731
    bad = [dict(brdf=None), dict(irradiance=None), dict(prefiltered=None), dict(irradiance=None, prefiltered=None), dict(irradiance_size=0),
           dict(irradiance_size=4097), dict(prefiltered_size=0), dict(prefiltered_size=4097), dict(brdf_size=0), dict(brdf_size=4097),
           dict(prefiltered_levels=0), dict(prefiltered_levels=14), dict(sky_size=0), dict(sky_size=4097), dict(sky_levels=0), dict(sky_levels=14),
           dict(skybox_lod=float("nan")), dict(skybox_lod=float("inf")), dict(skybox_lod=float("-inf")), dict(irradiance=off("irradiance", 4)),
           dict(prefiltered=off("prefiltered", 4)), dict(sky=off("sky", 4)), dict(brdf=off("brdf", 2)), dict(ao=off("ao", 2)),
           dict(sky_stats=off("sky_stats", 4)),
           # an output sharing a byte with an input, by ranges: the 9 x 7 colour plane is 1008 B, the irradiance cube of 8 is 3072 B, the table of 17 is 1156 B
           dict(color=off("irradiance", 0)), dict(color=off("irradiance", 3064)), dict(sky_stats=off("sky", 0)),
           dict(sky_stats=off("brdf", 1152)), dict(lights_walked=off("ao", 4 * 62)), dict(shadow_factor=off("prefiltered", 8)),
           dict(cascade=off("visibility", 8 * 62, base)), dict(ao=off("color", 16, base)), dict(stats=off("world_pos", 16 * 62, base)),
           dict(sky_stats=off("materials", 0, base)),
           # everything the shadowed call rejects
           dict(render_mode=1), dict(width=0), dict(height=32769), dict(tile_size_px=0), dict(flags=8), dict(flags=6), dict(color=None),
           dict(visibility=None), dict(shadow_resolution=0), dict(shadows=None), dict(materials=off("materials", 8, base)),
           dict(visibility=off("visibility", 4, base))]
    assert case.env["irradiance_size"] == 8 and case.env["brdf_size"] == 17 and case.ao is not None
    for change in bad:
        j = job(**change)
        assert host(C.byref(j), None, None) == passes.HOST_PANIC, change  # the mirror's Panic
        assert lib.orbit_fragments_shade_sky(None, C.byref(j), None) == _lib.E_INVALID, change  # the job is looked at before the context
        assert b"fragments_shade_sky:" in lib.orbit_last_error(None), change
    # a good job and no context: refused for the context
    assert lib.orbit_fragments_shade_sky(None, C.byref(good), None) == _lib.E_INVALID and b"ctx is NULL" in lib.orbit_last_error(None)
    assert lib.orbit_fragments_shade_sky(None, None, None) == _lib.E_INVALID
    # what is not given is not checked: no environment needs no sizes, no sky no levels and no finite lod
    for change in (dict(irradiance=None, prefiltered=None, brdf=None, irradiance_size=0, prefiltered_levels=99),
                   dict(sky=None, sky_size=0, sky_levels=0, skybox_lod=float("nan")), dict(ao=None), dict(sky_stats=None)):
        assert host(C.byref(job(**change)), None, None) == _lib.OK, change


# -- 7. the struct layout
def test_struct_layout():
    J = _lib.FragmentsShadeSky
    assert C.sizeof(J) == 344 and C.sizeof(_lib.FragmentsShadeShadowed) == 232 and L.SKY_STATS.itemsize == 32
    want = dict(shadowed=0, irradiance=232, prefiltered=240, brdf=248, sky=256, ao=264, sky_stats=272, irradiance_size=280, prefiltered_size=284,
                prefiltered_levels=288, brdf_size=292, sky_size=296, sky_levels=300, skybox_lod=304, sky_x=308, sky_y=320, sky_z=332)
    assert {n: getattr(J, n).offset for n in want} == want
    assert [L.SKY_STATS.fields[n][1] for n in ("sky_evaluations", "sky_lit_pixels", "skybox_pixels", "bad_directions")] == [0, 4, 8, 16]
    header = open(os.path.join(ROOT, "include", "orbit_abi_ext.h")).read()
    assert "sizeof(OrbitFragmentsShadeSky) == 344" in header and "sizeof(OrbitSkyStats) == 32" in header
    assert _lib.load().orbit_abi_version() == 6


# -- 8. the float64 figures of tools/count_fragments_shade_sky.py, held at the recorded values
def tool():
    spec = importlib.util.spec_from_file_location("count_fragments_shade_sky", os.path.join(ROOT, "tools", "count_fragments_shade_sky.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def held(name, value, recorded):
    """value <= recorded plus one unit of its last printed digit; a recorded 0 is held at 0"""
    if recorded == 0:
        assert value == 0, f"{name}: {value}, recorded 0"
        return
    d = Decimal(repr(recorded))
    bound = float(d + Decimal(1).scaleb(d.as_tuple().exponent))
    assert value <= bound, f"{name}: {value} above the recorded {recorded} plus one unit of its last digit"


def test_figures_against_float64(oracle):
    t = tool()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "fragments_shade_sky_cpu.json")))
    scene, counters = t.scene_figures(oracle)
    assert counters == recorded["scene_counters"] and counters["sky_lit_pixels"] == counters["written_pixels"] > 40000 and counters["skybox_pixels"] > 5000
    assert recorded["scene_over"] == dict(t.SCENE_ENV, frame=recorded["scene_over"]["frame"], panorama="64 x 32, seeded")
    for over, figures in (("scene", scene), ("matrix", t.matrix_figures(oracle))):
        for part in ("lit", "skybox"):
            assert figures[part]["pixels"] == recorded[over][part]["pixels"] > 0
            for k in ("max_abs", "max_rel", "share_above_2_pow_minus_10"):
                for channel in range(3):
                    print(over, part, k, channel, figures[part][k][channel])
                    held(f"{over}.{part}.{k}[{channel}]", figures[part][k][channel], recorded[over][part][k][channel])


# -- 9. the sanitizer program: a stand-alone host binary, built and run here
def test_sanitizer_program_runs_clean(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "sanitize_shade_sky"
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(ROOT, "orbit_amd", "host"), os.path.join(ROOT, "tools", "sanitize_shade_sky.cpp"),
                            os.path.join(ROOT, "orbit_amd", "host", "orbit_raster.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, (done.stdout[-1000:], done.stderr[-3000:])
    assert "refused" in done.stdout and "corner taps 0," not in done.stdout
