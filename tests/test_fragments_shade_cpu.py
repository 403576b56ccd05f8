"""orbit_fragments_shade's host mirror (orbit_amd.raster.host_fragments_shade, the device call's pin) against the numpy
restatement of L1-L9 (tests/fragments_shade_ref.py), byte for byte, on the hand-built cases and tampers of
tests/fragments_shade_cases.py; the argument errors; the host log2 against the oracle's; and, on the 100-instance scene at
320 x 180 over the host chain, the derived property that shading from the cluster lists equals shading from all lights,
and the accuracy figures of profiles/fragments_shade_cpu.json.  No GPU."""
import importlib.util
import json
import os

import numpy as np
import pytest

import fragments_shade_cases as fc
import fragments_shade_ref as ref
import raster_scene as rs
from orbit_amd import _lib, passes, raster

FILL = 0xA5A5A5A5  # what the call does not write keeps it: the guards of a host array
KEYS = ("color", "lights_walked", "stats")


@pytest.fixture(scope="module")
def cases(oracle):
    return fc.all_cases(oracle)


@pytest.fixture(scope="module")
def tampers(oracle):
    return fc.tampers(oracle)


def count_tool():
    spec = importlib.util.spec_from_file_location("count_fragments_shade", os.path.join(rs.ROOT, "tools", "count_fragments_shade.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@pytest.fixture(scope="module")
def frame(oracle):
    return count_tool().host_frame(oracle)


def assert_equal(name, got, want):
    assert got["status"] == want["status"], f"{name}: status {got['status']}, restated {want['status']}"
    assert got["stats"].tobytes() == want["stats"].tobytes(), f"{name}: stats {got['stats']}, restated {want['stats']}"
    for k in ("color", "lights_walked"):
        diff = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(diff) == 0, f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}: {got[k][tuple(diff[0])]!r} != {want[k][tuple(diff[0])]!r}"


# -- 1. mirror = restatement, byte for byte, between guards, with and without the clear, both render modes
@pytest.mark.parametrize("render_mode", (0, 8))
@pytest.mark.parametrize("clear", (False, True))
def test_the_mirror_equals_the_restatement(oracle, cases, tampers, clear, render_mode):
    totals = np.zeros(8, np.int64)
    for case in cases + [c for c, _ in tampers]:
        got = fc.mirror(case, clear=clear, render_mode=render_mode, fill=FILL)
        assert_equal(f"{case.name} (clear={clear}, mode {render_mode})", got, fc.restated(case, oracle, clear=clear, render_mode=render_mode, fill=FILL))
        st = got["stats"]
        assert int(st["covered_pixels"]) == int(st["written_pixels"]) + int(st["unshaded_pixels"]) + int(st["stale_pixels"])  # L9
        unwritten = ~ref.shade(oracle, *case.args()[0], **{k: v for k, v in case.over.items()})["live"]
        assert (got["color"].view(np.uint32)[unwritten] == (0 if clear else FILL)).all(), case.name
        totals += np.array([int(st[k]) for k in ref.STATS])
    covered, written, unshaded, stale, outside, degenerate, textured, unserved = totals
    assert written > 3000 and unshaded >= 2 and stale > 300 and outside > 300 and textured > 300
    assert (degenerate >= 2 and unserved > 300) if render_mode == 0 else (degenerate == unserved == 0)


def test_the_census_covers_what_the_issue_names(oracle, cases):
    shapes = {c.visibility.shape[::-1] for c in cases}
    assert set(fc.TARGETS) <= shapes and {c.tile for c in cases} == set(fc.TILES)
    walked = np.concatenate([fc.mirror(c)["lights_walked"][c.visibility != 0] for c in cases])
    assert {0, 1, 63, 64, 65, 256} <= set(walked.tolist()) and walked.max() == 256
    assert any((c.image[:, 1] == 300).any() for c in cases)  # a count of 300 walks 256
    for distinct in (1, 2, 32):
        c = next(q for q in cases if q.name == f"{distinct}_slices_tile8")
        assert len(np.unique(ref.slices(oracle, c.visibility, fc.Z_NEAR, c.zs, c.zb))) == distinct


# -- 2. each tamper counts exactly its pixels stale
def test_each_tamper_counts_exactly_its_pixels_stale(oracle, tampers):
    for case, spec in tampers:
        want = fc.stale_pixels(case, spec, oracle)
        assert want.any(), case.name
        got = fc.mirror(case, clear=True)
        assert got["status"] == _lib.E_RANGE and int(got["stats"]["stale_pixels"]) == int(want.sum()), case.name
        covered = case.visibility != 0
        assert (got["color"][want] == 0).all() and (got["color"][covered & ~want][:, 3] == 1.0).all(), case.name
    names = {c.name.rsplit("_tile", 1)[0] for c, _ in tampers}
    assert {"material_is_material_count", "offset_plus_n_one_past_capacity"} <= names
    assert {f"bad_index_at_{p}" for p in (0, 63, 64, 255)} <= names


# -- 3. NULL lights_walked / stats; the forms' flags change nothing on the host
def test_null_outputs_and_forms(cases):
    for case in cases[::5]:
        full = fc.mirror(case, fill=FILL, clear=False)
        for kw in (dict(want_walked=False), dict(want_stats=False), dict(form="per_lane")) + ((dict(form="staged"),) if case.staged else ()):
            got = fc.mirror(case, fill=FILL, clear=False, **kw)
            assert got["color"].tobytes() == full["color"].tobytes() and got["status"] == full["status"], (case.name, kw)
            assert (got["lights_walked"] is None) == ("want_walked" in kw) and (got["stats"] is None) == ("want_stats" in kw)


# -- 4. every argument error is a panic of the mirror
def test_argument_errors(cases):
    case = next(c for c in cases if c.name == "shape_9x9_tile4")
    a, _ = case.args()

    def panics(positional=None, **changed):
        args, kw = list(a), {}
        for k, v in list((positional or {}).items()) + list(changed.items()):
            if isinstance(k, int):
                args[k] = v
            else:
                kw[k] = v
        with pytest.raises(passes.Panic, match="fragments_shade"):
            raster.host_fragments_shade(*args, **kw)

    for cc in ((0, 3, 12), (3, 0, 12), (3, 3, 0), (3, 3, 33)):
        big = np.zeros((max(cc[0] * cc[1] * cc[2], 1), 2), np.uint32)
        panics({6: big, 8: cc})
    panics({9: 0})
    panics(render_mode=1)
    panics(render_mode=9)
    panics(form=8)
    panics(form=_lib.SHADE_FORCE_PER_LANE | _lib.SHADE_FORCE_STAGED)
    panics(form="staged")  # tile_size_px 4
    j = _lib.FragmentsShade()  # NULL pointers, zero sizes
    assert raster.lib().orbit_host_fragments_shade(None, None) == passes.HOST_PANIC
    import ctypes as C

    assert raster.lib().orbit_host_fragments_shade(C.byref(j), None) == passes.HOST_PANIC
    with pytest.raises(ValueError):
        raster.host_fragments_shade(*a, index_capacity=1 << 20)
    assert raster.host_fragments_shade(*a)["status"] == 0


# -- 5. the host log2 = the oracle's; the host slice = the restatement's
def test_host_log2_equals_the_oracle(oracle):
    zs, zb = fc.grid(oracle)
    edges = fc.knife_edge_depths(oracle, zs, zb)
    assert sum(t < k for _, k, t in edges) >= 4 and sum(t >= k for _, k, t in edges) >= 4
    rng = np.random.default_rng(5)
    values = [np.float32(fc.Z_NEAR) / d for d, _, _ in edges] + list(fc.special_depths()) + list(rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32))
    values += [np.float32(v) for v in (0.0, -0.0, 1.0, 2.0, 1.41421354, 1.4142135, np.inf, -np.inf, 1e-45, 3.4e38)]
    for v in values:
        want, got = np.float32(oracle.log2f(float(v))), raster.host_shade_log2(v)
        assert want.tobytes() == got.tobytes() or (np.isnan(want) and np.isnan(got)), (v, want, got)
    for d, k, t in edges:
        assert raster.host_shade_slice(fc.Z_NEAR, d, zs, zb) == (k if t >= k else k - 1), (d, k, t)
    depths = np.concatenate([np.array([d for d, _, _ in edges], np.float32), fc.special_depths()])
    vis = (depths.view(np.uint32).astype(np.uint64) << np.uint64(32) | np.uint64(1)).reshape(1, -1)
    want = ref.slices(oracle, vis, fc.Z_NEAR, zs, zb).reshape(-1)
    assert [raster.host_shade_slice(fc.Z_NEAR, d, zs, zb) for d in depths] == [min(int(s), 0xFFFFFFFF) for s in want]


# -- 6. lights_walked = the image's clamped count
def test_lights_walked_is_the_clamped_count(oracle, cases):
    for case in cases:
        got = fc.mirror(case, clear=True)
        c = ref.classify(oracle, case.visibility, case.material, case.materials, case.lights, case.image, case.index_buffer, case.cluster_count,
                         case.tile, case.zs, case.zb, fc.Z_NEAR)
        h, w = case.visibility.shape
        sl = c["slice"].reshape(h, w)
        for y, x in zip(*np.nonzero(c["live"].reshape(h, w))):
            cx, cy, cz = case.cluster_count
            inside = x // case.tile < cx and y // case.tile < cy and sl[y, x] < cz
            count = min(int(case.image[case.cluster(x, y, int(sl[y, x])), 1]), 256) if inside else 0
            assert int(got["lights_walked"][y, x]) == count, (case.name, x, y)


# -- 7. clustered = all lights, on the scene's frame over the host chain
def test_clustered_shading_equals_all_lights(frame):
    """Derived, not measured: beyond sqrt(1.05) R0 ~ 0.976 R, with R0 = sqrt(intensity / cutoff) and R = outer_radius = 1.05
    R0, L5's attenuation max(intensity / d2 - cutoff d2 / R^2, 0) is exactly +0 (the first term is below the second), so a
    light the cull left out of a cluster (its sphere of radius R misses the cluster's box) adds (.. x (lc x +0)) x ndl = +0
    to a finite sum, in every list order."""
    tool = count_tool()
    n = len(frame["lights"])
    real = raster.host_fragments_shade(*frame["args"], fill=FILL, clear=False)
    st = real["stats"]
    # the conditions of the property
    assert frame["dropped"] == 0 and n <= 256 and int(frame["image"][:, 1].max()) <= 256
    assert real["status"] == 0 and int(st["stale_pixels"]) == int(st["unshaded_pixels"]) == int(st["degenerate_pixels"]) == 0
    assert int(st["written_pixels"]) == int((frame["frame"]["visibility"] != 0).sum()) > 40000
    every = raster.host_fragments_shade(*tool.all_lights_args(frame["args"], n), fill=FILL, clear=False)
    assert int(every["stats"]["written_pixels"]) == int(st["written_pixels"]) and every["status"] == 0
    diff = np.argwhere(real["color"].view(np.uint32) != every["color"].view(np.uint32))
    assert len(diff) == 0, f"{len(diff)} words differ, first at {diff[0]}"
    walked = real["lights_walked"][frame["frame"]["visibility"] != 0]
    assert 0 < walked.mean() < n and walked.max() > 8  # the lists cull, and light: not vacuous
    lit = real["color"][frame["frame"]["visibility"] != 0][:, :3].max(axis=1)
    assert (lit > 0).mean() > 0.5


# -- 8. the accuracy figures of profiles/fragments_shade_cpu.json
def test_accuracy_against_the_float64_glsl(oracle, cases, frame):
    """Largest relative error of color.rgb against forward.frag evaluated in float64 (true pow(x, 5.0), double log2) from the
    same planes; allowed: twice the recorded figure, rounded up to a power of two (units of 2^-24), as §4.24 does."""
    tool = count_tool()
    with open(os.path.join(rs.ROOT, "profiles", "fragments_shade_cpu.json")) as fh:
        recorded = json.loads(fh.read())
    allowed = 2.0 ** np.ceil(np.log2(2.0 * recorded["max_relative_error"]))
    worst, compared, differs, clamped = tool.accuracy(oracle, frame["args"])
    for c in cases:
        a, kw = c.args()
        e, n, d, q = tool.accuracy(oracle, a, kw)
        worst, compared, differs, clamped = max(worst, e), compared + n, differs + d, clamped + q
    print(f"max_relative_error {worst:.4g} x 2^-24 over {compared} pixels (allowed {allowed:g}); slice_differs {differs}; near_clamp_pixels {clamped}")
    assert compared > 40000 and differs > 0 and worst <= allowed
