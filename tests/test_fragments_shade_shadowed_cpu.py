"""orbit_fragments_shade_shadowed's host mirror (orbit_amd.raster.host_fragments_shade_shadowed, the device call's pin)
against the numpy restatement of H1-H10 (tests/fragments_shade_shadowed_ref.py), byte for byte, on the hand-built cases
and tampers of tests/fragments_shade_shadowed_cases.py; the argument errors; with no shadowed light the mirror of
orbit_fragments_shade on its whole census; a floor, a box and a sun whose cascades come from orbit_host_shadow_cascade and
whose maps the host raster draws; and the project's sine and cosine against float64 over every angle a 4096 x 4096 target
produces.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

import fragments_shade_cases as fc
import fragments_shade_shadowed_cases as sc
import fragments_shade_shadowed_ref as ref
import raster_cases as rc
import raster_scene as rs
from orbit_amd import _lib, passes, raster
from orbit_amd import layouts as L

FILL = 0xA5A5A5A5  # what the call does not write keeps it: the guards of a host array
KEYS = ("color", "lights_walked", "shadow_factor", "cascade")
PROFILE = os.path.join(rs.ROOT, "profiles", "fragments_shade_shadowed_cpu.json")


@pytest.fixture(scope="module")
def cases(oracle):
    return sc.all_cases(oracle)


@pytest.fixture(scope="module")
def tampers(oracle):
    return sc.tampers(oracle)


def assert_equal(name, got, want, keys=KEYS):
    assert got["status"] == want["status"], f"{name}: status {got['status']}, restated {want['status']}"
    for k in ("stats", "shadow_stats"):
        if got[k] is not None:
            assert got[k].tobytes() == want[k].tobytes(), f"{name}: {k} {got[k]}, restated {want[k]}"
    for k in keys:
        if got[k] is None:
            continue
        diff = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(diff) == 0, f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}: {got[k][tuple(diff[0])]!r} != {want[k][tuple(diff[0])]!r}"


# -- 1. mirror = restatement, byte for byte, between guards, with and without the clear, both render modes
@pytest.mark.parametrize("render_mode", (0, 8))
@pytest.mark.parametrize("clear", (False, True))
def test_the_mirror_equals_the_restatement(oracle, cases, tampers, clear, render_mode):
    shadow = np.zeros(4, np.int64)
    blockers, cascades = set(), set()
    for case in cases + [c for c, _ in tampers]:
        got = sc.mirror(case, clear=clear, render_mode=render_mode, fill=FILL)
        want = sc.restated(case, oracle, clear=clear, render_mode=render_mode, fill=FILL)
        assert_equal(f"{case.name} (clear={clear}, mode {render_mode})", got, want)
        shadow += np.array([int(v) for v in got["shadow_stats"]])
        blockers |= set(np.unique(want["blockers"]).tolist())
        cascades |= set(np.unique(got["cascade"]).tolist())
    if render_mode == 8:
        assert not shadow.any()
        return
    # the census reaches what it is there for: every blocker count (1 and 11 among them), every cascade, pixels no cascade holds
    assert blockers >= set(range(13)) and {0, 1, 2, 3, 4, 0xFFFFFFFF} <= cascades | ({FILL} if not clear else set())
    assert shadow[0] > 3000 and shadow[1] >= 8 and 500 < shadow[2] < shadow[0] and shadow[3] > shadow[0]


def test_what_the_cases_claim(oracle, cases):
    by_name = {c.name: c for c in cases}
    for tile in (8, 4):
        for tag, factor in (("no_blockers", 1.0), ("all_blockers", 0.0)):  # a constant map gives blocker count 0 or 12, nothing else
            got = sc.mirror(by_name[f"constant_{tag}_tile{tile}"])
            assert (got["shadow_factor"] == factor).all() and got["shadow_stats"]["early_out_pixels"] == got["shadow_stats"]["shadowed_pixels"] == 81
        want = sc.restated(by_name[f"z_equals_texel_tile{tile}"], oracle)  # z == t is lit for >= and no blocker for >
        assert want["shadow_stats"]["early_out_pixels"] == 0 and ((want["lit"] > 0) & (want["lit"] < 128)).any()
        got = sc.mirror(by_name[f"cascade_edges_tile{tile}"])
        c = got["cascade"]
        # q exactly at -1, 0, 1: inside cascade 0; one ulp beyond: not; the c.w = 0 cascade never holds; NaN and far pixels: none
        assert list(c[0, :2]) == [0, 0] and list(c[1, 1:4]) == [0, 0, 0] and c[0, 7] == 0, c[:2]
        assert all(v == 2 for v in c[0, 2:7]) and c[1, 0] == 2 and not (c == 1).any(), c[:2]
        # (2, 3) has world_pos.w = 0, so c.w = 0 in every cascade: none; (2, 4) has w = 2: q = c / 2, inside cascade 2
        assert list(c[2, :4]) == [4, 4, 4, 4] and c[2, 4] == 2 and got["shadow_stats"]["no_cascade_pixels"] >= 4, c[2]
        pos = sc.mirror(by_name[f"positions_tile{tile}"])  # two shadowed lights: the first's factor, both counted
        two = pos["lights_walked"] == 3
        assert two.any() and int(pos["shadow_stats"]["shadow_evaluations"]) == int((pos["lights_walked"] == 256).sum() + 2 * two.sum())


def test_null_outputs_and_no_clear(oracle, cases):
    by_name = {c.name: c for c in cases}
    for name in ("shadow_shape_65x8_tile8_res64", "shadow_shape_9x9_tile4_res1", "cascade_edges_tile8"):
        full = sc.mirror(by_name[name], clear=False, fill=FILL)
        for off in ("want_walked", "want_stats", "want_factor", "want_cascade", "want_shadow_stats"):
            assert_equal(f"{name} with {off}=False", sc.mirror(by_name[name], clear=False, fill=FILL, **{off: False}), full)
        second = sc.mirror(by_name[name], clear=False, into=full)  # onto an earlier call's planes: the same bytes again
        assert_equal(f"{name} into", second, full)


# -- 2. tampers: each counts exactly its own pixels stale
def test_tampers_count_their_own_pixels(oracle, tampers):
    kinds = 0
    for case, spec in tampers:
        got = sc.mirror(case, clear=True)
        want = sc.stale_pixels(case, spec, oracle)
        stale = (case.case.visibility != 0) & (got["cascade"] == 0xFFFFFFFF) & (got["color"][..., 3] == 0)
        assert int(got["stats"]["stale_pixels"]) == int(want.sum()), (case.name, got["stats"])
        assert (stale == want).all(), case.name
        assert got["status"] == (_lib.E_RANGE if want.any() else 0), case.name
        kinds += bool(want.any())
    assert kinds == 6


# -- 3. every argument error
def test_argument_errors(oracle, cases):
    case = next(c for c in cases if c.name == "shadow_shape_9x9_tile4_res1")
    a, kw = case.args()

    def bad(at=None, value=None, **over):
        args = list(a)
        if at is not None:
            args[at] = value
        with pytest.raises((passes.Panic, ValueError)):  # the mirror's own check, or the wrapper's where it sees the arrays
            raster.host_fragments_shade_shadowed(*args, **dict(kw, **over))

    assert raster.host_fragments_shade_shadowed(*a, **kw)["status"] == 0
    bad(render_mode=1), bad(form=8), bad(form=6), bad(form="staged")
    bad(at=8, value=(0, 3, 12)), bad(at=8, value=(3, 3, 33)), bad(at=9, value=0)
    bad(at=15, value=None, shadow_count=2), bad(at=16, value=None, shadow_map_count=4)  # shadow_count > 0 with shadows or shadow_maps NULL
    bad(at=17, value=0, shadow_map_count=4), bad(at=17, value=32769, shadow_map_count=0)
    bad(at=17, value=32768, shadow_map_count=3)  # 3 * 2^30 floats
    # shadow_count == 0 is valid with nothing behind the pointers: every shadowed light makes its pixel stale
    args = list(a)
    args[15] = args[16] = None
    args[17] = 0
    none = raster.host_fragments_shade_shadowed(*args, **kw)
    walked = ref.shade(oracle, *a, **{k: v for k, v in kw.items()}, shadow_count=0)
    assert none["status"] == _lib.E_RANGE and none["stats"].tobytes() == walked["stats"].tobytes() and none["stats"]["stale_pixels"] > 0


# -- 4. with no shadowed light: orbit_fragments_shade's mirror, byte for byte, on its whole census
@pytest.mark.parametrize("render_mode", (0, 8))
def test_without_shadowed_lights_it_is_the_old_call(oracle, render_mode):
    rows, maps = sc.rows_of(sc.row()), np.zeros((1, 1, 1), np.float32)
    written = 0
    for case in fc.all_cases(oracle) + [c for c, _ in fc.tampers(oracle)]:
        case = case.copy(case.name)
        case.lights["shadow_data_index"] = 0xFFFFFFFF
        a, kw = case.args(clear=False, fill=FILL, render_mode=render_mode)
        old = raster.host_fragments_shade(*a, **kw)
        for count in (0, 1):
            new = raster.host_fragments_shade_shadowed(*a, rows if count else None, maps if count else None, 1, 0.3, 0.0, -0.02, **kw)
            for k in ("color", "lights_walked", "stats"):
                assert new[k].tobytes() == old[k].tobytes(), (case.name, k)
            assert new["status"] == old["status"] and not any(new["shadow_stats"]), case.name
            assert set(np.unique(new["cascade"]).tolist()) <= {FILL, 0xFFFFFFFF}  # H10's defaults where written
        written += int(old["stats"]["written_pixels"])
    assert written > 2000


# -- 5. a floor, a box, one sun: cascades from orbit_host_shadow_cascade, maps from the host raster
def test_a_box_on_a_floor_casts_its_shadow(oracle):
    res, w, h = 256, 61, 120
    cam_pos, cam_q, fov, near, aspect = (0.0, 2.0, 0.0), (0.0, 0.0, 0.0, 1.0), float(np.pi / 2), 0.01, 16.0 / 9.0
    sun_q = (-0.5, 0.0, 0.0, float(np.sqrt(0.75)))  # 60 degrees down, travelling towards -z: direction = q . (0, 0, 1)
    direction = (0.0, float(np.sqrt(0.75)), 0.5)
    cascades = [passes.shadow_cascade(sun_q, cam_pos, cam_q, fov, near, aspect, k, shadow_resolution=res)[1:] for k in range(4)]
    floor = [((-40, 0, 40), (40, 0, 40), (40, 0, -40)), ((-40, 0, 40), (40, 0, -40), (-40, 0, -40))]
    x0, x1, z0, z1 = -0.5, 0.5, -4.5, -3.5
    box = []
    for (ax, ay, az), (bx, by, bz), (cx, cy, cz), (dx, dy, dz) in (
            ((x0, 1, z1), (x1, 1, z1), (x1, 1, z0), (x0, 1, z0)), ((x0, 0, z1), (x1, 0, z1), (x1, 1, z1), (x0, 1, z1)),
            ((x0, 0, z0), (x1, 0, z0), (x1, 1, z0), (x0, 1, z0)), ((x0, 0, z0), (x0, 0, z1), (x0, 1, z1), (x0, 1, z0)),
            ((x1, 0, z0), (x1, 0, z1), (x1, 1, z1), (x1, 1, z0))):
        box += [((ax, ay, az), (bx, by, bz), (cx, cy, cz)), ((ax, ay, az), (cx, cy, cz), (dx, dy, dz))]
    packed = rc.Packed(rc.Case("floor_and_box", [rc.poly(floor), rc.poly(box)], width=res, height=res, view_proj=cascades[0][0], cull_none=True))
    kw, pa = packed.args()
    atlas = raster.host_shadow_atlas(*pa[:6], [m for m, _ in cascades], res, cull_none=True, **kw)
    assert all((atlas[k] > 0).any() for k in range(4))
    # the planes: pixel (row, column) is the floor point x = (column - 30) * 0.05, z = -1 - row * 0.25, seen from above
    zs, zb = fc.grid(oracle)
    ys, xs = np.mgrid[0:h, 0:w]
    case = fc.Case("floor", np.full((h, w), fc.depth_of_slice(zs, zb, 4), np.float32), 8, zs, zb, seed=1,
                   lists={c: [0] for c in range(-(-w // 8) * -(-h // 8) * 12)}, default_lengths=(0,), cluster_count=(-(-w // 8), -(-h // 8), 12),
                   lights=sc.make_lights(np.random.default_rng(1)), view_pos=cam_pos)
    case.world_pos[..., 0], case.world_pos[..., 1], case.world_pos[..., 2] = (xs - 30) * 0.05, 0.0, -1.0 - ys * 0.25
    case.normal[:] = (0.0, 1.0, 0.0)
    case.lights["light_type"][0], case.lights["shadow_data_index"][0] = L.LIGHT_TYPE_DIRECTIONAL, sc.BASE
    case.lights["direction"][0], case.lights["inner_radius"][0] = direction, 0.5
    rows = raster.shadow_rows([m for m, _ in cascades], [s for _, s in cascades])
    got = sc.mirror(sc.ShadowCase(case, rows, atlas, settings=dict(normal_bias_scale=2.0, oriented_bias=-0.1)))
    assert got["status"] == 0 and got["stats"]["written_pixels"] == w * h
    factor, cascade = got["shadow_factor"], got["cascade"]
    z_of = lambda z: int(round((-1.0 - z) / 0.25))  # noqa: E731
    # the shadow on the floor: |x| <= 0.5, z in [-5.08, -3.5]; well inside it, well outside it, and its edge
    assert (factor[z_of(-4.0):z_of(-4.75) + 1, 30 - 5:30 + 6] == 0).all(), factor[z_of(-4.0):z_of(-4.75) + 1, 25:36]
    assert (factor[z_of(-3.0), :] == 1).all() and (factor[z_of(-6.5), :] == 1).all() and (factor[:z_of(-20.0), :8] == 1).all()
    edge = factor[z_of(-3.25):z_of(-5.5) + 1, 30 - 14:30 + 15]
    assert ((edge > 0) & (edge < 1)).any(), edge
    centre = cascade[:, 30].astype(np.int64)
    assert (np.diff(centre) >= 0).all() and centre[0] == 0 and centre.max() >= 2, centre


# -- 6. sinc / cosc against float64 sin / cos over every theta the seeds of a 4096 x 4096 target produce
def test_the_sine_and_cosine(oracle):
    worst, strip = 0.0, 256
    for y0 in range(0, 4096, strip):
        theta, s, c = raster.host_shadow_rotation(0, y0, 4096, strip)
        if y0 == 0:  # the restatement's angle, sine and cosine are the mirror's, bit for bit
            ys, xs = np.mgrid[0:8, 0:4096]
            t = ref.theta_of(xs.reshape(-1), ys.reshape(-1))
            rs_, rc_ = ref.sincos(t)
            assert t.tobytes() == theta[:8].tobytes() and rs_.tobytes() == s[:8].tobytes() and rc_.tobytes() == c[:8].tobytes()
        assert theta.min() >= 0 and theta.max() < 6.2832
        t64 = theta.astype(np.float64)
        worst = max(worst, float(np.abs(s - np.sin(t64)).max()), float(np.abs(c - np.cos(t64)).max()))
    print(f"sinc / cosc: largest absolute error {worst:.4g} = 2^{math.log2(worst):.2f}")
    assert worst < 2.0 ** -11  # Vulkan's own bound for sin and cos: a condition, not a measurement
    with open(PROFILE) as f:
        measured = json.load(f)["sincos_max_abs_error"]
    assert worst < 2.0 ** math.ceil(math.log2(2.0 * measured)), (worst, measured)
