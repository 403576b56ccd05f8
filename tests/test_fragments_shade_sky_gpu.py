"""orbit_fragments_shade_sky on the device (include/orbit_abi_ext.h K1-K10) against the host mirror
(orbit_amd.raster.host_fragments_shade_sky, which tests/test_fragments_shade_sky_cpu.py holds to the numpy restatement):
every hand-built case, byte for byte, with both forms of the walk where the grid is eligible and with the library's
choice, with and without ORBIT_SHADE_CLEAR, between guards, inputs unchanged, under grid caps of 1, 2 and none; NULL
outputs; render_mode 8; K10's equality with the device's own orbit_fragments_shade_shadowed on the shadowed test's cases;
the argument errors; the first call of a fresh context captured into a graph and replayed; one chained frame, orbit_env_map
-> orbit_ssao -> the new call -> orbit_bloom -> orbit_post_process, against the mirrors' chain.  No test provokes a fault:
every cube, table and plane is read inside its bounds by construction, and stale rows are ordinary data the checks reject."""
import importlib.util
import os

import numpy as np
import pytest

import fragments_shade_shadowed_cases as sc
import fragments_shade_sky_cases as kc
import raster_cases as rc
import raster_scene as rs
from orbit_amd import _lib
from orbit_amd import layouts as L
from test_gpu_parity import dev, host
from test_raster_depth_gpu import Guarded, latched

pytestmark = pytest.mark.gpu
FILL = 0x01010101 * rc.SENTINEL  # the mirror's outputs start as the guards' bytes do
PLANES = ("color", "lights_walked", "shadow_factor", "cascade")
BLOCKS = dict(stats=L.SHADE_STATS, shadow_stats=L.SHADOW_STATS, sky_stats=L.SKY_STATS)
OPTIONAL = ("lights_walked", "stats", "shadow_factor", "cascade", "shadow_stats", "sky_stats")


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def engine(torch_mod):
    from orbit_amd.engine import Engine

    e = Engine(0, max_entities=4096, max_dispatches=100000, max_draws=200000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(oracle):
    return kc.all_cases(oracle)


@pytest.fixture(scope="module")
def mirrors():
    """the mirror's outputs per (case, clear, render_mode), computed once and left unchanged"""
    return {}


def mirror(mirrors, case, clear=False, render_mode=0):
    key = (case.name, case.env is None, case.sky is None, clear, render_mode)
    if key not in mirrors:
        mirrors[key] = kc.mirror(case, clear=clear, render_mode=render_mode, fill=FILL)
    return mirrors[key]


def forms_of(case):
    return (None, "per_lane", "staged") if case.staged else (None, "per_lane")


def sky_keywords(case, pointers):
    """the call's sky arguments: pointers = {name: address or None} of irradiance, prefiltered, brdf, sky, ao"""
    e, s = case.env or {}, case.sky or {}
    return dict(irradiance=pointers["irradiance"], irradiance_size=e.get("irradiance_size", 0), prefiltered=pointers["prefiltered"],
                prefiltered_size=e.get("prefiltered_size", 0), prefiltered_levels=e.get("prefiltered_levels", 0), brdf=pointers["brdf"],
                brdf_size=e.get("brdf_size", 0), sky=pointers["sky"], sky_size=s.get("size", 0), sky_levels=s.get("levels", 0),
                skybox_lod=case.skybox_lod, basis=case.basis, ao=pointers["ao"])


def sky_arrays(case):
    e, s = case.env or {}, case.sky or {}
    return dict(irradiance=e.get("irradiance"), prefiltered=e.get("prefiltered"), brdf=e.get("brdf"), sky=s.get("cube"),
                ao=None if case.ao is None else np.ascontiguousarray(case.ao, np.float32))


def run(torch, engine, case, clear=False, form=None, render_mode=0, without=()):
    """One orbit_fragments_shade_sky call on guarded copies -> the dict of raster.host_fragments_shade_sky (status: what the
    context latched); `without`: the optional outputs passed as NULL."""
    a, kw = case.args()
    vis, wp, nrm, mat, mats, lights, image, index_buffer, cc, tile, zs, zb, cutoff, z_near, view_pos, rows, maps, res, brs, nbs, ob = a
    h, w = vis.shape
    inputs = [Guarded(torch, x) for x in (vis, wp, nrm, mat, mats, lights, image, index_buffer, rows, maps)]
    g_vis, g_wp, g_nrm, g_mat, g_mats, g_lights, g_image, g_index, g_rows, g_maps = inputs
    extra = {k: None if v is None else Guarded(torch, v) for k, v in sky_arrays(case).items()}
    sizes = dict(color=16 * w * h, lights_walked=4 * w * h, stats=32, shadow_factor=4 * w * h, cascade=4 * w * h, shadow_stats=16, sky_stats=32)
    out = {k: Guarded(torch, np.zeros(0, np.uint8), nbytes=n) for k, n in sizes.items()}
    ptr = lambda k: None if k in without else out[k].ptr  # noqa: E731
    engine.fragments_shade_sky(g_vis.ptr, w, h, g_wp.ptr, g_nrm.ptr, g_mat.ptr, g_mats.ptr, len(mats), g_lights.ptr, len(lights), g_image.ptr,
                               g_index.ptr, (np.ascontiguousarray(index_buffer).view(np.uint8).size - 4) // 4, cc, tile, zs, zb, cutoff, z_near,
                               view_pos, out["color"].ptr, g_rows.ptr, len(rows), g_maps.ptr, len(maps), res, brs, nbs, ob,
                               **sky_keywords(case, {k: None if g is None else g.ptr for k, g in extra.items()}), sky_stats=ptr("sky_stats"),
                               shadow_index_base=kw["shadow_index_base"], shadow_factor=ptr("shadow_factor"), cascade=ptr("cascade"),
                               shadow_stats=ptr("shadow_stats"), lights_walked=ptr("lights_walked"), stats=ptr("stats"), render_mode=render_mode,
                               clear=clear, form=form)
    torch.cuda.synchronize()
    for g in inputs + [g for g in extra.values() if g is not None]:
        g.unchanged()
    for k in without:
        out[k].unchanged()
    views = dict(color=(np.float32, (h, w, 4)), lights_walked=(np.uint32, (h, w)), shadow_factor=(np.float32, (h, w)), cascade=(np.uint32, (h, w)))
    got = {k: None if k in without else out[k].read().view(t).reshape(s) for k, (t, s) in views.items()}
    for k, dtype in BLOCKS.items():
        got[k] = None if k in without else out[k].read().view(dtype)[0]
    return dict(got, status=latched(engine))


def assert_equal(name, got, want):
    for k in BLOCKS:
        if got[k] is not None:
            assert got[k].tobytes() == want[k].tobytes(), f"{name}: device {k} {got[k]} != host {want[k]}"
    assert got["status"] == want["status"], f"{name}: latched {got['status']}, the mirror says {want['status']}"
    for k in PLANES:
        if got[k] is None:
            continue
        diff = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(diff) == 0, (f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}: device {got[k][tuple(diff[0])]!r}, "
                                f"host {want[k][tuple(diff[0])]!r}")


# -- 1. every case, each form, with and without CLEAR: bytes, counters, latched status, guards, inputs
@pytest.mark.parametrize("clear", (False, True))
@pytest.mark.parametrize("form", (None, "per_lane", "staged"))
def test_every_case_equals_the_host_mirror(torch_mod, engine, cases, mirrors, clear, form):
    assert latched(engine) == 0
    lit = boxed = bad = stale = 0
    for case in cases:
        if form not in forms_of(case):
            continue
        got = run(torch_mod, engine, case, clear=clear, form=form)
        assert_equal(f"{case.name} (clear={clear}, form={form})", got, mirror(mirrors, case, clear=clear))
        sk = got["sky_stats"]
        lit, boxed, bad = lit + int(sk["sky_lit_pixels"]), boxed + int(sk["skybox_pixels"]), bad + int(sk["bad_directions"])
        stale += int(got["stats"]["stale_pixels"])
    assert lit > 1000 and boxed > 300 and bad > 60 and stale > 50  # (staged runs the eligible half)


# -- 2. each optional input alone: the kernel built without the environment, the call without the skybox launch
@pytest.mark.parametrize("without_inputs", (("sky",), ("env",), ("env", "sky")))
def test_each_optional_input_alone(torch_mod, engine, cases, mirrors, without_inputs):
    by_name = {c.name: c for c in cases}
    for name in ("sky_shape_8x8_tile8", "sky_shape_9x7_tile4", "skybox_checkerboard", "sky_tiles_73x33"):
        part = by_name[name].without(*without_inputs)
        for form in forms_of(part):
            assert_equal(f"{name} without {without_inputs} (form={form})", run(torch_mod, engine, part, clear=True, form=form),
                         mirror(mirrors, part, clear=True))


# -- 3. NULL optional outputs, one at a time and all six
def test_null_outputs(torch_mod, engine, cases, mirrors):
    by_name = {c.name: c for c in cases}
    for name in ("sky_shape_9x7_tile8", "sky_shape_8x8_tile4", "skybox_zero_basis"):
        for form in forms_of(by_name[name]):
            for clear in (False, True):
                full = mirror(mirrors, by_name[name], clear=clear)
                for without in [(k,) for k in OPTIONAL] + [OPTIONAL]:
                    assert_equal(f"{name} without {without}", run(torch_mod, engine, by_name[name], clear=clear, form=form, without=without), full)


# -- 4. render_mode 8: nothing of K runs, uncovered pixels stay as they were
def test_the_heat_map(torch_mod, engine, cases, mirrors):
    for case in cases:
        for form in forms_of(case):
            got = run(torch_mod, engine, case, clear=False, form=form, render_mode=8)
            assert_equal(f"{case.name} heat map (form={form})", got, mirror(mirrors, case, clear=False, render_mode=8))
            assert not any(got["sky_stats"].tolist()) and not any(got["shadow_stats"].tolist())


# -- 5. grids of one and two workgroups, and the uncapped one again
@pytest.mark.parametrize("cap", (1, 2, 0))
def test_capped_grids_walk_every_tile(torch_mod, engine, cases, mirrors, cap):
    by_name = {c.name: c for c in cases}
    engine.set_visibility_grid(cap)
    try:
        for name in ("sky_tiles_73x33", "sky_lists_tile8", "sky_lists_tile4", "skybox_all_uncovered", "sky_shape_9x7_tile4"):
            for form in forms_of(by_name[name]):
                for clear in (False, True):
                    assert_equal(f"{name}, cap {cap} (clear={clear}, form={form})", run(torch_mod, engine, by_name[name], clear=clear, form=form),
                                 mirror(mirrors, by_name[name], clear=clear))
    finally:
        engine.set_visibility_grid(0)


def device_job(torch, case):
    """the case's inputs on the device and zeroed outputs -> (inputs: 10 tensors, sky inputs: dict, outputs: dict, arguments)"""
    a, kw = case.args()
    h, w = a[0].shape
    bufs = [dev(torch, x) for x in a[:8]] + [dev(torch, a[15]), dev(torch, a[16])]
    extra = {k: None if v is None else dev(torch, v) for k, v in sky_arrays(case).items()}
    sizes = dict(color=16 * w * h, lights_walked=4 * w * h, stats=32, shadow_factor=4 * w * h, cascade=4 * w * h, shadow_stats=16, sky_stats=32)
    outs = {k: torch.zeros(n, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
    return bufs, extra, outs, a, kw


def call(engine, case, ptrs, sky_ptrs, o, a, kw, w=None, h=None, over=None, **opts):
    """orbit_fragments_shade_sky on raw addresses -> the error code, 0 for none"""
    ic = (np.ascontiguousarray(a[7]).view(np.uint8).size - 4) // 4
    h0, w0 = a[0].shape
    sky = dict(sky_keywords(case, sky_ptrs), **(over or {}))
    try:
        engine.fragments_shade_sky(ptrs[0], w0 if w is None else w, h0 if h is None else h, ptrs[1], ptrs[2], ptrs[3], ptrs[4], len(a[4]), ptrs[5],
                                   len(a[5]), ptrs[6], ptrs[7], ic, a[8], a[9], a[10], a[11], a[12], a[13], a[14], o["color"], ptrs[8], len(a[15]),
                                   ptrs[9], len(a[16]), a[17], a[18], a[19], a[20], **sky, sky_stats=o["sky_stats"],
                                   shadow_index_base=kw["shadow_index_base"], shadow_factor=o["shadow_factor"], cascade=o["cascade"],
                                   shadow_stats=o["shadow_stats"], lights_walked=o["lights_walked"], stats=o["stats"], **opts)
    except _lib.OrbitError as e:
        assert "fragments_shade_sky:" in str(e), str(e)
        return e.code
    return 0


# -- 6. the argument errors, each checked before the context is looked at
def test_argument_errors(torch_mod, engine, oracle):
    torch = torch_mod
    case = kc.SkyCase(kc.base_case("errors_9x7", oracle, 9, 7, 4, 5, ([kc.SKY, kc.SUN], [12])), kc.make_env(6, 8, 16, 5, 17), kc.make_sky(7, 16),
                      ao=kc.ao_plane(np.random.default_rng(8), 7, 9))
    bufs, extra, outs, a, kw = device_job(torch, case)
    ptrs, sky_ptrs, o = [b.data_ptr() for b in bufs], {k: t.data_ptr() for k, t in extra.items()}, {k: t.data_ptr() for k, t in outs.items()}
    go = lambda p=ptrs, s=sky_ptrs, out=o, **kws: call(engine, case, p, s, out, a, kw, **kws)  # noqa: E731
    assert go() == 0
    E = _lib.E_INVALID
    for k in range(10):  # everything the shadowed call rejects: NULL, misaligned, an output that is an input
        assert go(ptrs[:k] + [None] + ptrs[k + 1:]) == E, k
        assert go(ptrs[:k] + [ptrs[k] + (4 if k in (0, 4, 5, 6, 8) else 2)] + ptrs[k + 1:]) == E, k
        for name in ("color", "shadow_factor", "cascade", "sky_stats"):
            assert go(out=dict(o, **{name: ptrs[k]})) == E, (k, name)
    assert go(out=dict(o, color=None)) == go(w=0) == go(h=0) == go(w=32769) == go(render_mode=1) == go(form=6) == go(form=8) == E
    for name in o:
        assert go(out=dict(o, **{name: o[name] + 2})) == E, name
    assert go(out=dict(o, sky_stats=o["sky_stats"] + 4)) == E  # 8-B aligned
    for name in ("irradiance", "prefiltered", "brdf"):  # the environment in part, misaligned
        assert go(s=dict(sky_ptrs, **{name: None})) == E, name
        assert go(s=dict(sky_ptrs, **{name: sky_ptrs[name] + (2 if name == "brdf" else 4)})) == E, name
    assert go(s=dict(sky_ptrs, sky=sky_ptrs["sky"] + 4)) == go(s=dict(sky_ptrs, ao=sky_ptrs["ao"] + 2)) == E
    for field, values in (("irradiance_size", (0, 4097)), ("prefiltered_size", (0, 4097)), ("brdf_size", (0, 4097)), ("prefiltered_levels", (0, 14)),
                          ("sky_size", (0, 4097)), ("sky_levels", (0, 14)), ("skybox_lod", (float("nan"), float("inf"), float("-inf")))):
        for v in values:
            assert go(over={field: v}) == E, (field, v)
    # an output sharing a byte with an input, by ranges: inside the cube's last texel, the table's last texel, the ao plane's last float
    assert go(out=dict(o, sky_stats=sky_ptrs["irradiance"] + 3064)) == go(out=dict(o, sky_stats=sky_ptrs["brdf"] + 1152)) == E
    assert go(out=dict(o, lights_walked=sky_ptrs["ao"] + 4 * 62)) == go(out=dict(o, color=sky_ptrs["sky"] + 8)) == E
    assert go(s=dict(sky_ptrs, ao=o["color"] + 16)) == go(s=dict(sky_ptrs, sky=o["shadow_factor"])) == E
    # what is not given is not checked
    none = dict(sky_ptrs, irradiance=None, prefiltered=None, brdf=None)
    assert go(s=none, over=dict(irradiance_size=0, prefiltered_levels=99)) == 0
    assert go(s=dict(sky_ptrs, sky=None), over=dict(sky_size=0, sky_levels=0, skybox_lod=float("nan"))) == 0
    assert go(s=dict(sky_ptrs, ao=None)) == 0 and go() == 0
    torch.cuda.synchronize()
    assert latched(engine) == 0


# -- 7. K10: with the environment and sky NULL, the device bytes of orbit_fragments_shade_shadowed on the shadowed test's cases
def test_without_environment_and_sky_it_is_the_shadowed_call(torch_mod, engine, oracle):
    torch = torch_mod
    picked = [c for c in sc.all_cases(oracle) + [c for c, _ in sc.tampers(oracle)]]
    compared = 0
    for shadow in picked:
        case = kc.SkyCase(shadow)
        bufs, extra, _, a, kw = device_job(torch, case)
        h, w = a[0].shape
        ic = (np.ascontiguousarray(a[7]).view(np.uint8).size - 4) // 4
        for form in forms_of(case):
            for mode in (0, 8):
                old, new = ([torch.full((n,), 9, dtype=torch.uint8, device="cuda") for n in (16 * w * h, 4 * w * h, 32, 4 * w * h, 4 * w * h, 16)]
                            for _ in range(2))
                sky_stats = torch.full((32,), 9, dtype=torch.uint8, device="cuda")
                common = (bufs[0], w, h, bufs[1], bufs[2], bufs[3], bufs[4], len(a[4]), bufs[5], len(a[5]), bufs[6], bufs[7], ic, a[8], a[9], a[10],
                          a[11], a[12], a[13], a[14])
                tail = (bufs[8], len(a[15]), bufs[9], len(a[16]), a[17], a[18], a[19], a[20])
                outs = lambda t: dict(lights_walked=t[1], stats=t[2], shadow_factor=t[3], cascade=t[4], shadow_stats=t[5])  # noqa: E731
                engine.fragments_shade_shadowed(*common, old[0], *tail, shadow_index_base=kw["shadow_index_base"], render_mode=mode, form=form, **outs(old))
                assert latched(engine) in (0, _lib.E_RANGE)
                engine.fragments_shade_sky(*common, new[0], *tail, shadow_index_base=kw["shadow_index_base"], render_mode=mode, form=form,
                                           sky_stats=sky_stats, **outs(new))
                torch.cuda.synchronize()
                for t_old, t_new in zip(old, new):
                    assert host(t_old).tobytes() == host(t_new).tobytes(), (case.name, form, mode)
                assert not host(sky_stats).any()
                latched(engine)
                compared += 1
    assert compared > 100


# -- 8. captured into a graph as the first call of a fresh context, replayed twice on changed buffers
def test_the_first_call_captures_into_a_graph(torch_mod, cases, mirrors):
    torch = torch_mod
    from orbit_amd.engine import Engine

    base = next(c for c in cases if c.name == "sky_shape_9x7_tile8")
    other = kc.SkyCase(base.shadow.copy("other planes, another environment"), kc.make_env(1234, *[base.env[k] for k in
                       ("irradiance_size", "prefiltered_size", "prefiltered_levels", "brdf_size")]), kc.make_sky(1235, base.sky["size"]),
                       base.skybox_lod, base.basis, None if base.ao is None else base.ao[::-1].copy())
    other.case.world_pos = base.case.world_pos[::-1].copy()
    assert base.env is not None and base.sky is not None
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        bufs, extra, outs, a, kw = device_job(torch, base)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            code = call(eng, base, bufs, extra, outs, a, kw, clear=True)
        assert code == 0
        for c in (base, other, base):  # replayed: new planes and images, the first ones again
            ca = c.args()[0]
            for t, x in zip(bufs, list(ca[:8]) + [ca[15], ca[16]]):
                t.copy_(dev(torch, x))
            for k, v in sky_arrays(c).items():
                if v is not None:
                    extra[k].copy_(dev(torch, v))
            want = kc.mirror(c, clear=True)
            for replay in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert latched(eng) == want["status"], c.name
                for k in PLANES + tuple(BLOCKS):
                    assert host(outs[k]).tobytes() == want[k].tobytes(), (c.name, k, replay)
        assert int(want["sky_stats"]["sky_lit_pixels"]) > 20 and int(want["sky_stats"]["skybox_pixels"]) > 0
    finally:
        eng.close()


# -- 9. one chained frame on the device: orbit_env_map -> orbit_ssao -> orbit_fragments_shade_sky -> orbit_bloom -> orbit_post_process
def test_the_chained_frame(torch_mod, engine, oracle):
    spec = importlib.util.spec_from_file_location("render_frame", os.path.join(rs.ROOT, "tools", "render_frame.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    sky_tool = tool._tool("count_fragments_shade_sky")
    assert latched(engine) == 0
    f = sky_tool.host_frame(oracle)  # the frame of the shadowed test, 320 x 180, with the sky light, the environment and the skybox
    want = tool.host_sky_picture(f, sky_tool, 4.0, True)
    got = tool.device_sky_picture(f, sky_tool, 4.0, True, engine)
    equal = tool.sky_equal(f, want, got)
    assert all(equal.values()) and len(equal) == 11, equal
    sk = want[1]["sky_stats"]
    assert int(sk["sky_lit_pixels"]) == int(want[1]["stats"]["written_pixels"]) > 40000 and int(sk["skybox_pixels"]) > 5000
    assert int(want[1]["stats"]["unserved_pixels"]) == 0
