"""orbit_surface_fragments on the CPU (include/orbit_abi_ext.h F1-F8): the host mirror that is the GPU
tests' reference equals the independent restatement (tests/surface_fragments_ref.py) on every byte of every output, the
counters and the status of every case of tests/surface_fragments_cases.py, between sentinel guards, with the inputs
unchanged and with vertex and meshlet buffers that end with their last legal byte; material against a separate decode;
the written set is the surface call's; what is not written keeps its fill, or the clear's; every float agrees with a
float64 evaluation of the same definition and view_proj x world_pos lands on the pixel's centre, within twice what
tools/count_surface_fragments.py measured (profiles/surface_fragments_cpu.json), as does uv_grad with the finite
difference of uv; each tamper counts exactly its pixels as stale; unshaded pixels leave the status OK; the degenerate
inputs give F7's zeros; each argument error answers ORBIT_E_INVALID with its own message, without a device;
pack_mesh_vertices follows the reference's packing."""
import ctypes as C
import importlib.util
import json
import math
import os

import numpy as np
import pytest

import raster_cases as rc
import surface_drawn_cases as dc
import surface_fragments_cases as fc
import surface_fragments_ref as ref
import visibility_surface_cases as sc
from orbit_amd import _lib, assets, raster
from orbit_amd import layouts as L
from orbit_amd.passes import lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL, GUARD = rc.SENTINEL, rc.GUARD
FILL = 0x01010101 * SENTINEL  # what the call does not write keeps the guards' bytes
KEYS = tuple(n for n, _, _ in raster.FRAGMENT_OUTPUTS)
PER_PIXEL = {n: (per, dtype) for n, per, dtype in raster.FRAGMENT_OUTPUTS}
PARTS = 6  # the census in slices, so that no test case takes more than a few seconds
STATS = ("covered_pixels", "written_pixels", "foreign_pixels", "unshaded_pixels", "stale_pixels", "degenerate_pixels")


def tool():
    spec = importlib.util.spec_from_file_location("count_surface_fragments", os.path.join(ROOT, "tools", "count_surface_fragments.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def measured():
    """profiles/surface_fragments_cpu.json -> {figure: twice the measured value, rounded up to a power of two}"""
    with open(os.path.join(ROOT, "profiles", "surface_fragments_cpu.json")) as fh:
        row = json.loads(fh.readline())
    return {k: 2.0 ** math.ceil(math.log2(2.0 * row[k])) for k in ("max_relative_error", "max_relative_error_wide", "max_reprojection_error_narrow",
                                                                    "max_reprojection_error_wide", "max_uv_grad_difference")}


def between_guards(a=None, nbytes=None):
    a = np.zeros(0, np.uint8) if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    n = len(a) if nbytes is None else nbytes
    whole = np.full((n + 15) // 16 * 16 + 2 * GUARD, SENTINEL, np.uint8)
    whole[GUARD:GUARD + len(a)] = a
    assert (whole.ctypes.data + GUARD) % 16 == 0
    return whole, whole[GUARD:GUARD + n]


def guarded_mirror(c, clear=False, want=KEYS, with_grad=True):
    """orbit_host_surface_fragments on case c with every input and output between 256-B sentinel guards -> the outputs, after
    asserting that no guard byte and no input byte changed.  Outputs start as sentinel bytes."""
    (vis, words, mc, meshlets, surface, vb, vcount, ent), kw = c.args()
    h, w = vis.shape
    given = (vis, words, meshlets, surface["bary"], surface["grad"], surface["triangle"], vb, ent)
    inputs = [between_guards(a) for a in given]
    before = [whole.copy() for whole, _ in inputs]
    outs = {k: between_guards(nbytes=4 * PER_PIXEL[k][0] * w * h) for k in KEYS}
    stats = between_guards(nbytes=32)
    at = lambda pair: pair[0].ctypes.data + GUARD  # noqa: E731
    j = _lib.SurfaceFragments()
    j.visibility, j.draw_commands, j.meshlets, j.bary, j.grad, j.triangle, j.vertices, j.entity_data = (at(q) for q in inputs)
    if not with_grad:
        j.grad = None
    for k in KEYS:
        setattr(j, k, at(outs[k]) if k in want else None)
    j.stats = at(stats)
    j.vertex_count, j.meshlet_count, j.max_commands, j.entity_count = vcount, kw["meshlet_count"], mc, kw["entity_count"]
    j.vertex_stride, j.position_offset, j.normal_offset, j.uv_offset, j.tangent_offset = 32, 0, 12, 16, 24
    j.width, j.height, j.flags, j.command_base = w, h, _lib.FRAGMENTS_CLEAR if clear else 0, kw["command_base"]
    status = C.c_int32(0)
    assert lib().orbit_host_surface_fragments(C.byref(j), C.byref(status)) == 0, c.name
    for (whole, _), was in zip(inputs, before):
        assert whole.tobytes() == was.tobytes(), f"{c.name}: an input or its guards were written"
    for name, (whole, payload) in list(outs.items()) + [("stats", stats)]:
        assert (whole[:GUARD] == SENTINEL).all() and (whole[GUARD + len(payload):] == SENTINEL).all(), f"{c.name}: a guard byte of {name} was written"
        if name != "stats" and name not in want:
            assert (payload == SENTINEL).all(), f"{c.name}: {name} was not given and was written"
    got = {k: outs[k][1].view(PER_PIXEL[k][1]).reshape(h, w, -1).copy() if k in want else None for k in KEYS}
    return dict(got, stats=stats[1].view(L.SURFACE_FRAGMENT_STATS)[0].copy(), status=status.value)


def restate(c, clear=False, **over):
    a, kw = c.args(fill=FILL, clear=clear, **over)
    return ref.fragments(*a, **kw)


def assert_equal(name, got, want):
    assert {k: int(got["stats"][k]) for k in STATS} == {k: want["stats"][k] for k in STATS}, name
    assert int(got["stats"]["_pad0"]) == int(got["stats"]["_pad1"]) == 0
    assert got["status"] == want["status"], name
    for k in KEYS:
        if got[k] is None or want[k] is None:
            continue
        diff = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(diff) == 0, (f"{name}: {k}: {len(diff)} words differ, first at {diff[0]}: mirror {got[k][tuple(diff[0])]!r}, "
                                f"restatement {want[k][tuple(diff[0])]!r}")


@pytest.fixture(scope="module")
def cases():
    return fc.all_cases()


@pytest.fixture(scope="module")
def restated(cases):
    """{name: the restatement's result without the clear}; computed once, shared, left unchanged"""
    return {c.name: restate(c) for c in cases}


# -- 1. mirror = restatement, byte for byte
def test_the_census_is_complete(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    shapes = {c.visibility.shape[::-1] for c in cases}
    assert {(1, 1), (7, 3), (8, 8), (9, 9), (65, 8)} <= shapes
    for must in ("whole_1x1", "whole_7x3", "whole_8x8", "whole_9x9", "whole_65x8", "tile_of_64_65x9", "w_1_1_4", "two_lists_base_cap",
                 "one_out_full_65x9@8", "cut_with_a_wide_piece_65x9@40", "64_keys_cut_and_wide_65x9@40", "fan_of_wide_triangles@32"):
        assert must in names, must
    assert any(n.startswith("clip_") and n.endswith("@40") for n in names) and len(fc.both_flag_cases()) > 5
    tile = next(c for c in cases if c.name == "tile_of_64_65x9")
    t = tile.surface["triangle"][0:8, 8:16].reshape(64, 4)
    assert len({tuple(r[1:]) for r in t}) == 64 and set(t[:, 0]) == {0, 1, 2, 3}


def test_the_census_reaches_written_and_unshaded_pixels(restated):
    written = sum(r["stats"]["written_pixels"] for r in restated.values())
    unshaded = sum(r["stats"]["unshaded_pixels"] for r in restated.values())
    assert written > 100000 and unshaded > 1000  # (degenerate pixels: test_degenerate_inputs_give_zeros_and_a_count)


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("clear", (False, True))
def test_the_mirror_equals_the_restatement(cases, restated, clear, part):
    for c in cases[part::PARTS]:
        want = restated[c.name] if not clear else restate(c, clear=True)
        assert_equal(f"{c.name} (clear={clear})", guarded_mirror(c, clear=clear), want)
        st = want["stats"]
        assert st["covered_pixels"] == st["written_pixels"] + st["foreign_pixels"] + st["unshaded_pixels"] + st["stale_pixels"]
        assert st["stale_pixels"] == 0 and want["status"] == 0, c.name


def test_null_outputs_change_no_counter_and_no_other_output(cases, restated):
    for name in ("tile_of_64_65x9", "whole_9x9", "w_2_pow_minus_120"):
        c = next(q for q in cases if q.name == name)
        for k in KEYS:
            rest = tuple(q for q in KEYS if q != k)
            assert_equal(f"{name} without {k}", guarded_mirror(c, want=rest), restated[name])
            assert_equal(f"{name} {k} alone", guarded_mirror(c, want=(k,)), restated[name])
        no_grad = guarded_mirror(c, want=tuple(q for q in KEYS if q != "uv_grad"), with_grad=False)
        assert_equal(f"{name} without grad", no_grad, restated[name])


# -- 2. independent checks on every written pixel
def test_material_written_set_and_fill(cases, restated):
    for c in cases:
        got = guarded_mirror(c)
        h, w = c.visibility.shape
        words = c.words.view(np.uint32)
        base, n = c.kw["command_base"], min(int(words[0]), c.max_commands)
        meshlet_rows = np.zeros(c.kw["meshlet_count"] * 32, np.uint8)
        meshlet_rows[:len(c.meshlets)] = c.meshlets
        materials = meshlet_rows.view(L.MESHLET)["material_index"]
        surface_written = c.surface["triangle"][..., 0] != 0xFFFFFFFF
        k = ((c.visibility >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64) - base
        own = (c.visibility != 0) & (k >= 0) & (k < n)
        written = own & surface_written
        assert ((got["material"][..., 0] != FILL) == written).all(), c.name
        kw_ = k[written]
        assert (got["material"][..., 0][written] == materials[words[1 + 7 * kw_ + 6]]).all() and (materials[words[1 + 7 * kw_ + 6]] == 7 + 3 * kw_).all(), c.name
        # the surface call's written set under the same base (its clear leaves 0xFFFFFFFF elsewhere: foreign pixels too)
        assert (written == surface_written).all() and (surface_written <= own).all(), c.name
        assert int(got["stats"]["written_pixels"]) == int(written.sum())
        for k in KEYS:
            assert (got[k].view(np.uint32)[~written] == FILL).all(), (c.name, k)
        cleared = guarded_mirror(c, clear=True)
        for k in KEYS:
            assert (cleared[k].view(np.uint32)[~written] == (0xFFFFFFFF if k == "material" else 0)).all(), (c.name, k)
            assert (cleared[k].view(np.uint32)[written] == got[k].view(np.uint32)[written]).all(), (c.name, k)


# -- 3, 4. accuracy: within twice what tools/count_surface_fragments.py measured
@pytest.mark.parametrize("part", range(PARTS))
def test_accuracy_within_twice_the_measured(cases, restated, part):
    t, bound = tool(), measured()
    worst = dict.fromkeys(bound, 0.0)
    for c in cases[part::PARTS]:
        for k, v in t.accuracy(c, view_proj=c.source.packed.case.view_proj, got=restated[c.name]).items():
            worst[k] = max(worst[k], v)
    print("measured on this part of the census:", worst, "bounds:", bound)
    for k in bound:
        assert worst[k] <= bound[k], (k, worst[k], bound[k])
    assert worst["max_relative_error"] > 0 and worst["max_uv_grad_difference"] > 0


# -- 5. stale and unshaded
def stale_cases():
    base = next(c for c in fc.shape_cases() if c.name == "tile_of_64_65x9")
    tri = base.surface["triangle"]
    out = []

    def edit(y, x, col, value):
        t = tri.copy()
        t[y, x, col] = value
        return dict(triangle=t)

    out.append(fc.tamper(base, "entity_is_entity_count", 1, surface=edit(2, 9, 0, base.kw["entity_count"])))
    out.append(fc.tamper(base, "entity_of_another_command", 1, surface=edit(2, 9, 0, (int(tri[2, 9, 0]) + 1) % 4)))
    out.append(fc.tamper(base, "g_is_vertex_count", 1, surface=edit(3, 12, 2, base.vertex_count)))
    words = base.words.copy()
    k = ((int(base.visibility[5, 10]) >> 8) & 0xFFFFFF) - base.kw["command_base"]
    words[1 + 7 * k + 6] = base.kw["meshlet_count"]
    out.append(fc.tamper(base, "meshlet_index_is_meshlet_count", 1, words=words))
    # legal ends: the last vertex and the last meshlet, whose rows end the buffers
    out.append(fc.tamper(base, "g_is_last_vertex", 0, surface=edit(3, 12, 2, base.vertex_count - 1)))
    words = base.words.copy()
    words[1 + 7 * k + 6] = base.kw["meshlet_count"] - 1
    out.append(fc.tamper(base, "meshlet_index_is_last", 0, words=words))
    return out


def test_each_tamper_counts_exactly_its_pixels():
    for c in stale_cases():
        clean, got = guarded_mirror(c.clean), guarded_mirror(c)
        assert_equal(c.name, got, restate(c))
        assert int(got["stats"]["stale_pixels"]) == c.stale and got["status"] == (_lib.E_RANGE if c.stale else 0), c.name
        assert int(got["stats"]["written_pixels"]) == int(clean["stats"]["written_pixels"]) - c.stale
        changed = np.zeros(c.visibility.shape, bool)
        for k in KEYS:
            changed |= (got[k].view(np.uint32) != clean[k].view(np.uint32)).any(axis=2)
        assert int(changed.sum()) == 1, c.name  # the tampered pixel: unwritten when stale, other values when legal
        if c.stale:
            y, x = np.argwhere(changed)[0]
            assert all((got[k].view(np.uint32)[y, x] == FILL).all() for k in KEYS)


def test_unshaded_pixels_leave_the_status_ok():
    base = next(c for c in fc.shape_cases() if c.name == "tile_of_64_65x9")
    t = base.surface["triangle"].copy()
    t[1, 8:12] = 0xFFFFFFFF
    c = fc.tamper(base, "four_left_out", 0, surface=dict(triangle=t))
    got = guarded_mirror(c)
    assert_equal(c.name, got, restate(c))
    assert int(got["stats"]["unshaded_pixels"]) == 4 and got["status"] == 0 and int(got["stats"]["written_pixels"]) == 60
    # a buffer drawn with the flags but surfaced by the old call: unshaded = the old call's unsupported
    seen = 0
    for src in dc.hand_cases()[:6] + dc.wide_cases()[:4]:
        (vis, words, mc, data, vb, vcount, ent, vp), kw = src.args()
        kw.pop("raster_flags")
        old = raster.host_visibility_surface(vis, words, mc, data, vb, vcount, ent, vp, clear=True, **kw)
        c = fc.of(src, surface_over=0)
        got = guarded_mirror(c)
        assert_equal(c.name, got, restate(c))
        assert int(got["stats"]["unshaded_pixels"]) == int(old["stats"]["unsupported_pixels"]) and got["status"] == 0, src.name
        seen += int(old["stats"]["unsupported_pixels"])
    assert seen > 1000


# -- 6. degenerates
def test_degenerate_inputs_give_zeros_and_a_count():
    base = next(c for c in fc.shape_cases() if c.name == "whole_9x9")
    rows = base.vertices.copy()
    g = [int(v) for v in base.surface["triangle"][4, 4, 1:]]

    def with_rows(name, edit_rows):
        r = rows.copy()
        edit_rows(r)
        return fc.tamper(base, name, 0, vertices=r)

    def zero(offset, nbytes):
        def f(r):
            for v in g:
                r[32 * v + offset:32 * v + offset + nbytes] = 0
        return f

    c = with_rows("zero_normal", zero(12, 3))
    got = guarded_mirror(c)
    assert_equal(c.name, got, restate(c))
    assert int(got["stats"]["degenerate_pixels"]) == int(got["stats"]["written_pixels"]) == 81
    assert not got["normal"].any() and got["tangent"].any() and got["world_pos"].any()
    c = with_rows("zero_tangent", zero(24, 3))
    got = guarded_mirror(c)
    assert_equal(c.name, got, restate(c))
    assert int(got["stats"]["degenerate_pixels"]) == 81 and not got["tangent"][..., :3].any() and got["tangent"][..., 3].any()

    def minus_128(r):
        r[32 * g[0] + 12] = r[32 * g[1] + 25] = r[32 * g[2] + 27] = 0x80
    c = with_rows("int8_minus_128", minus_128)
    got = guarded_mirror(c)
    assert_equal(c.name, got, restate(c))
    assert int(got["stats"]["degenerate_pixels"]) == 0
    # tangent.w of corner 2 is -128 / 127 (as the product with 0x3C010204 gives it), not clamped: at l2 = 1 it would arrive whole
    w2 = F(-128.0) * np.array([0x3C010204], np.uint32).view(F)[0]
    assert w2 < F(-1.0)
    bary = base.surface["bary"].copy()
    bary[4, 4] = (0.0, 1.0)
    got = guarded_mirror(fc.tamper(c, "int8_minus_128_at_corner_2", 0, surface=dict(bary=bary)))
    assert got["tangent"][4, 4, 3] == w2

    bary = base.surface["bary"].copy()
    bary[0, 0], bary[0, 1], bary[0, 2] = (np.nan, 0.25), (0.25, np.inf), (-np.inf, 0.5)
    c = fc.tamper(base, "non_finite_bary", 0, surface=dict(bary=bary))
    got = guarded_mirror(c)
    assert_equal(c.name, got, restate(c))
    assert int(got["stats"]["degenerate_pixels"]) == 3 and int(got["stats"]["written_pixels"]) == 81
    for x in range(3):
        assert not got["world_pos"][0, x].any() and not got["uv"][0, x].any() and got["material"][0, x, 0] != FILL
    assert got["uv_grad"][0, 0].any()  # (uv_grad does not read bary)

    bary = base.surface["bary"].copy()
    one_up = np.nextafter(F(0.5), F(1.0))
    bary[4, 4] = (one_up, one_up)  # l1 + l2 slightly above 1: l0 = -2^-23 becomes +0.0f
    c = fc.tamper(base, "l0_below_zero", 0, surface=dict(bary=bary))
    got, want = guarded_mirror(c), restate(c)
    assert_equal(c.name, got, want)
    corners = want["detail"]["corners"]
    p = list(zip(*want["written"])).index((4, 4))
    expect = F(corners[1]["uv"][p, 0] * one_up) + F(corners[2]["uv"][p, 0] * one_up)  # a_0 * (+0.0f) adds nothing
    assert got["uv"][4, 4, 0] == expect and int(got["stats"]["degenerate_pixels"]) == 0


# -- 7. argument errors, without a device
def test_each_argument_error_has_its_own_message_without_a_device():
    lib_ = _lib.load()
    buf = np.zeros(64, np.uint64)
    at = buf.ctypes.data
    pointers = ("visibility", "draw_commands", "meshlets", "bary", "grad", "triangle", "vertices", "entity_data", "world_pos", "normal",
                "tangent", "uv", "uv_grad", "material", "stats")

    def call(**over):
        j = _lib.SurfaceFragments()
        for q, name in enumerate(pointers):
            setattr(j, name, at + 16 * q)
        j.vertex_count, j.meshlet_count, j.max_commands, j.entity_count = 3, 1, 1, 1
        j.vertex_stride, j.position_offset, j.normal_offset, j.uv_offset, j.tangent_offset = 32, 0, 12, 16, 24
        j.width, j.height, j.flags, j.command_base = 1, 1, 0, 0
        for k, v in over.items():
            setattr(j, k, v)
        rc_ = lib_.orbit_surface_fragments(None, C.byref(j), None)
        return rc_, lib_.orbit_last_error(None).decode()

    assert lib_.orbit_surface_fragments(None, None, None) == _lib.E_INVALID
    assert "surface_fragments: job is NULL" in lib_.orbit_last_error(None).decode()
    for over in (dict(), dict(flags=1), dict(grad=None, uv_grad=None), dict(stats=None), dict(vertex_count=1 << 32),
                 dict(vertex_stride=28), dict(world_pos=None, normal=None, tangent=None, uv=None, uv_grad=None)):
        assert call(**over) == (_lib.E_INVALID, "surface_fragments: ctx is NULL"), over
    top = _lib.VIS_MAX_COMMANDS
    outputs = pointers[8:14]
    for over, reason in (
            [(dict([(k, None)]), "NULL buffer") for k in ("visibility", "draw_commands", "meshlets", "bary", "triangle", "vertices", "entity_data")]
            + [(dict.fromkeys(outputs), "no output"), (dict(grad=None), "uv_grad needs grad")]
            + [(dict(visibility=at + 4), "8-B aligned"), (dict(entity_data=at + 8), "16-B aligned")]
            + [(dict([(k, at + 16 * q + 2)]), "4-B aligned") for q, k in enumerate(pointers) if k not in ("visibility", "entity_data")]
            + [(dict([(k, 6)]), "multiples of 4") for k in ("vertex_stride", "position_offset", "normal_offset", "uv_offset", "tangent_offset")]
            + [(dict(vertex_stride=24), "below an attribute's end"), (dict(position_offset=24), "below an attribute's end"),
               (dict(normal_offset=32), "below an attribute's end"), (dict(uv_offset=28), "below an attribute's end"),
               (dict(tangent_offset=32), "below an attribute's end")]
            + [(dict(width=0), "target"), (dict(height=0), "target"), (dict(width=_lib.RASTER_MAX_DIM + 1), "target"),
               (dict(height=_lib.RASTER_MAX_DIM + 1), "target")]
            + [(dict(command_base=top, max_commands=1), "24 bits of id"), (dict(command_base=1, max_commands=top), "24 bits of id")]
            + [(dict(vertex_count=(1 << 32) + 1), "2^32"), (dict(flags=2), "flags 0x2"), (dict(flags=1 << 31), "flags 0x80000000")]
            + [(dict([(o, at + 16 * q)]), "an output is an input") for o in outputs for q in range(8)]):
        rc_, text = call(**over)
        assert rc_ == _lib.E_INVALID and text.startswith("surface_fragments: ") and reason in text and "ctx is NULL" not in text, (over, text)
    assert not buf.any()  # nothing was written
    # the mirror answers the argument errors that it can see with a panic
    c = fc.shape_cases()[0]
    a, kw = c.args()
    for over in (dict(vertex_stride=24), dict(uv_offset=6), dict(want=())):
        with pytest.raises(Exception, match="surface_fragments"):
            raster.host_surface_fragments(*a, **dict(kw, **over))


# -- 8. pack_mesh_vertices
def test_pack_mesh_vertices_follows_the_reference():
    values = np.array([1.0, -1.0, 1.5, -7.0, np.nan, 0.999, -0.999, 0.5, 1.0 / 127.0, 0.0078, -0.0, np.inf, -np.inf, 126.9 / 127.0], F)
    expect = np.array([127, -127, 127, -127, 0, 126, -126, 63, 1, 0, 0, 127, -127, 126], np.int8)
    assert (assets.pack_snorm8(values) == expect).all()
    n = len(values)
    pos = np.arange(3 * n, dtype=F).reshape(n, 3)
    normals = np.stack([values, np.roll(values, 1), np.roll(values, 2)], axis=1)
    tangents = np.stack([np.roll(values, 3), values, np.roll(values, 5), np.roll(values, 7)], axis=1)
    uvs = np.arange(2 * n, dtype=F).reshape(n, 2) * F(0.25)
    rows = assets.pack_mesh_vertices(pos, normals, uvs, tangents)
    assert rows.dtype == L.MESH_VERTEX and rows.dtype.itemsize == 32 and len(rows) == n
    assert [rows.dtype.fields[k][1] for k in ("position", "normal", "uv", "tangent", "_padding")] == [0, 12, 16, 24, 28]
    assert (rows["position"] == pos).all() and (rows["uv"] == uvs).all() and not rows["_padding"].any() and not rows["normal"][:, 3].any()
    assert (rows["normal"][:, 0] == expect).all() and (rows["tangent"][:, 1] == expect).all() and (rows["tangent"][:, 3] == np.roll(expect, 7)).all()


def test_a_stride_32_buffer_gives_the_stride_12_bytes():
    for src in (sc.perspective_case(), dc.hand_cases()[1], next(c for c in dc.wide_cases() if c.name.startswith("fan_of_wide_triangles"))):
        (vis, words, mc, data, vb, vcount, ent, vp), kw = src.args()
        flags = kw.pop("raster_flags", 0)
        assert kw["vertex_stride"] == 12
        c = fc.of(src)
        rows = np.zeros(vcount * 32, np.uint8)
        rows[:len(c.vertices)] = c.vertices
        kw32 = dict(kw, vertex_stride=32, position_offset=0)
        base = kw32.pop("command_base")
        pc = src.packed.case
        vis32 = raster.host_raster_visibility(words, mc, data, rows, vcount, ent, vp, pc.width, pc.height, command_base=base,
                                              cull_none=pc.cull_none, clip_near=bool(flags & dc.CLIP), wide_guard=bool(flags & dc.WIDE), **kw32)[0]
        assert vis32.tobytes() == vis.tobytes(), src.name
        got = raster.host_visibility_surface_drawn(vis32, words, mc, data, rows, vcount, ent, vp, raster_flags=flags, clear=True, command_base=base, **kw32)
        for k in ("bary", "grad", "triangle"):
            assert got[k].tobytes() == c.surface[k].tobytes(), (src.name, k)
