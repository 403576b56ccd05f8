"""orbit_visibility_surface on the CPU (include/orbit_abi_ext.h S1-S7): the host mirror that is the GPU
tests' reference equals the independent numpy restatement (tests/visibility_surface_ref.py) on every byte of every
output of every case of tests/visibility_surface_cases.py — guards and unwritten pixels included; on every written
pixel 0.0f <= l1, l2 <= 1.0f as bit patterns and l1 + l2 <= 1 + 2^-22; every l agrees with the exact rational value to
8 * 2^-24 (relative); the ids match an independent decode; the counters add up; the cases reach what they claim; the
clip buffers hold unsupported pixels under status OK; each stale case counts exactly the tampered pixels and changes
nothing else; the layouts match the header; each argument error answers ORBIT_E_INVALID with its own message, without a
device; the 100-instance scene's two-pass frame, one call per list into shared outputs."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import raster_cases as rc
import raster_scene as rs
import visibility_surface_cases as sc
import visibility_surface_ref as ref
from orbit_amd import _lib, raster
from orbit_amd import layouts as L
from orbit_amd.passes import lib

F = np.float32
SENTINEL = rc.SENTINEL
FILL = 0x01010101 * SENTINEL  # what the call does not write keeps the guards' bytes
KEYS = ("bary", "grad", "triangle")
ONE = int(F(1.0).view(np.uint32))
GUARD = rc.GUARD
PER_PIXEL = dict(bary=(2, F), grad=(4, F), triangle=(4, np.uint32))


def between_guards(a=None, nbytes=None):
    """A copy of `a` (or nbytes sentinel bytes) with GUARD sentinel bytes in front and behind -> (whole, payload view)"""
    a = np.zeros(0, np.uint8) if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    n = len(a) if nbytes is None else nbytes
    whole = np.full(n + 2 * GUARD, SENTINEL, np.uint8)
    whole[GUARD:GUARD + len(a)] = a
    assert (whole.ctypes.data + GUARD) % 16 == 0
    return whole, whole[GUARD:GUARD + n]


def guarded_mirror(c, clear=False, want=KEYS, want_stats=True):
    """orbit_host_visibility_surface on case c with every input and output between 256-B sentinel guards -> the dict of
    raster.host_visibility_surface, after asserting that no guard byte and no input byte changed.  Outputs start as
    sentinel bytes: what the call does not write keeps them."""
    (vis, words, mc, data, vb, vcount, ent, vp), kw = c.args()
    h, w = vis.shape
    inputs = [between_guards(a) for a in (vis, words, np.ascontiguousarray(data, np.uint32), vb, ent)]
    before = [whole.copy() for whole, _ in inputs]
    outs = {k: between_guards(nbytes=4 * PER_PIXEL[k][0] * w * h) for k in KEYS}
    stats = between_guards(nbytes=32)
    at = lambda pair: pair[1].ctypes.data if len(pair[1]) else pair[0].ctypes.data + GUARD  # noqa: E731
    j = _lib.VisibilitySurface()
    j.visibility, j.draw_commands, j.meshlet_data, j.vertices, j.entity_data = (at(q) for q in inputs)
    for k in want:
        setattr(j, k, at(outs[k]))
    if want_stats:
        j.stats = at(stats)
    j.meshlet_data_words, j.vertex_count, j.max_commands = kw["meshlet_data_words"], vcount, mc
    j.entity_count, j.vertex_stride, j.position_offset = kw["entity_count"], kw["vertex_stride"], kw["position_offset"]
    j.width, j.height, j.flags, j.command_base = w, h, _lib.SURFACE_CLEAR if clear else 0, kw["command_base"]
    j.view_proj = (C.c_float * 16)(*np.asarray(vp, F).reshape(16))
    status = C.c_int32(0)
    assert lib().orbit_host_visibility_surface(C.byref(j), C.byref(status)) == 0, c.name
    for (whole, _), was in zip(inputs, before):
        assert whole.tobytes() == was.tobytes(), f"{c.name}: an input or its guards were written"
    for name, (whole, payload) in list(outs.items()) + [("stats", stats)]:
        assert (whole[:GUARD] == SENTINEL).all() and (whole[GUARD + len(payload):] == SENTINEL).all(), f"{c.name}: a guard byte of {name} was written"
        if name not in want and not (name == "stats" and want_stats):
            assert (payload == SENTINEL).all(), f"{c.name}: {name} was not given and was written"
    got = {k: outs[k][1].view(PER_PIXEL[k][1]).reshape(h, w, -1).copy() if k in want else None for k in KEYS}
    return dict(got, stats=stats[1].view(L.SURFACE_STATS)[0].copy() if want_stats else None, status=status.value)


@pytest.fixture(scope="module")
def cases():
    return sc.all_cases()


@pytest.fixture(scope="module")
def mirrored(cases):
    """{name: the host mirror's outputs}, every buffer between sentinel guards, every output filled with the sentinel
    first and not cleared: what the call does not write keeps the sentinel; computed once"""
    return {c.name: guarded_mirror(c) for c in cases}


def stats_dict(row):
    return {k: int(row[k]) for k in ref.STAT_NAMES}


def test_the_census_is_complete(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for must in ("64_keys_in_a_tile", "t_0_63_64_255", "list_65", "list_257", "wound_front", "wound_mirror", "vertex_on_centre_2",
                 "shared_edge", "w_1_1_4", "w_2_pow_minus_120", "foreshortened", "range_ends", "ids_in_n_to_max", "list_count_zero",
                 "list_count_above_max", "base_top_of_24_bits", "stale_depth_bit", "stale_moved_word", "stale_t_is_nt",
                 "stale_257_triangles", "stale_r9_corner_is_vcount", "two_lists_base_cap", "nt_256", "clip_lone_out_vertex_0"):
        assert must in names, must
    hand = sc.hand_cases() + sc.stale_cases()[:3]
    assert {c.visibility.shape[::-1] for c in hand} <= set(sc.HAND_SIZES)


def test_the_mirror_equals_the_restatement_byte_for_byte(cases, mirrored):
    for c in cases:
        a, kw = c.args(fill=FILL, clear=False)
        want, got = ref.surface(*a, **kw), mirrored[c.name]
        assert stats_dict(got["stats"]) == want["stats"], c.name
        assert got["status"] == want["status"] == (ref.E_RANGE if want["stats"]["stale_pixels"] else 0), c.name
        for k in KEYS:
            diff = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
            assert len(diff) == 0, (f"{c.name}: {k}: {len(diff)} words differ, first at {diff[0]}: mirror "
                                    f"{got[k][tuple(diff[0])]!r}, restatement {want[k][tuple(diff[0])]!r}")
        # what is not written keeps the fill: exactly the written pixels differ from it in `triangle`
        written = (got["triangle"].view(np.uint32) != FILL).any(axis=2)
        assert int(written.sum()) == want["stats"]["written_pixels"], c.name


def test_the_cases_reach_what_they_claim(cases, mirrored):
    for c in cases:
        st = stats_dict(mirrored[c.name]["stats"])
        for k, v in c.expect.items():
            assert st[k] == v, (c.name, k, st)
        # S7
        assert st["covered_pixels"] == st["written_pixels"] + st["foreign_pixels"] + st["unsupported_pixels"] + st["stale_pixels"], c.name
        assert st["covered_pixels"] == int((c.visibility != 0).sum()), c.name
    by = {c.name: stats_dict(mirrored[c.name]["stats"]) for c in cases}
    assert by["w_2_pow_minus_120"]["degenerate_pixels"] == by["w_2_pow_minus_120"]["written_pixels"] > 10
    assert 0 < by["foreshortened"]["degenerate_pixels"] < by["foreshortened"]["written_pixels"]
    assert by["nt_256"]["written_pixels"] > 100 and by["back_face_kept"]["written_pixels"] == 90
    assert sum(st["written_pixels"] for st in by.values()) > 10000


def test_partial_outputs_and_no_clear_write_the_same_pixels(cases, mirrored):
    """Each output alone gives the bytes it has beside the others; without CLEAR the unwritten pixels keep the fill, with
    it they hold 0.0 and 0xFFFFFFFF; the counters depend on neither."""
    for c in cases:
        if c.name not in ("w_1_1_4", "foreshortened", "two_lists_base_cap", "stale_depth_bit", "clip_lone_out_vertex_0"):
            continue
        full = mirrored[c.name]
        for k in KEYS:
            one = guarded_mirror(c, want=(k,))
            assert one[k].tobytes() == full[k].tobytes() and one["stats"].tobytes() == full["stats"].tobytes(), (c.name, k)
            assert all(one[q] is None for q in KEYS if q != k)
        a, kw = c.args(fill=FILL, clear=True)
        wiped = guarded_mirror(c, clear=True)
        want = ref.surface(*a, **kw)
        plain = raster.host_visibility_surface(*a, **kw)  # the Python form of the same call: the same bytes
        assert all(plain[k].tobytes() == wiped[k].tobytes() for k in KEYS) and plain["stats"].tobytes() == wiped["stats"].tobytes()
        assert wiped["stats"].tobytes() == full["stats"].tobytes()
        written = (full["triangle"].view(np.uint32) != FILL).any(axis=2)
        assert int(written.sum()) == int(full["stats"]["written_pixels"])
        for k, cleared in (("bary", 0), ("grad", 0), ("triangle", 0xFFFFFFFF)):
            assert wiped[k].tobytes() == want[k].tobytes()
            assert (wiped[k].view(np.uint32)[written] == full[k].view(np.uint32)[written]).all()
            assert (full[k].view(np.uint32)[~written] == FILL).all() and (wiped[k].view(np.uint32)[~written] == cleared).all()
        assert guarded_mirror(c, want_stats=False)["stats"] is None


def decode(c, y, x):
    """An independent decode of pixel (y, x) of case c -> (entity, [g0, g1, g2], three float32 positions)"""
    pk = c.packed
    word = int(c.visibility[y, x])
    k, t = ((word >> 8) & 0xFFFFFF) - c.command_base, word & 255
    words = pk.words if c.words is None else c.words
    cmd = words[1 + 7 * k:8 + 7 * k]
    first_index, index_base, entity, vertex_base = int(cmd[2]), int(cmd[3]), int(cmd[4]), int(cmd[5])
    corners = pk.meshlet_data.view(np.uint8)[first_index + 3 * t:first_index + 3 * t + 3]
    g = [vertex_base + int(pk.meshlet_data[index_base + int(q)]) for q in corners]
    pos = [pk.vertices[v * pk.stride + pk.offset:][:12].view(F) for v in g]
    return entity, g, pos


def snapped_corners(c, y, x, memo):
    """(X, Y, W) of the owning triangle's three corners: the snapped integers the definition uses and the float clip w as
    a Fraction — computed here from the model positions with float32 steps (R2-R4); once per (command, triangle)."""
    key = int(c.visibility[y, x]) & 0xFFFFFFFF
    if key not in memo:
        pk = c.packed
        entity, g, pos = decode(c, y, x)
        mvp = ref._mvp(np.asarray(pk.case.view_proj, F), np.asarray(pk.entities[entity]["model_matrix"], F).reshape(16))
        X, Y, W = [], [], []
        for p in pos:
            cx, cy, _, w = (F(F(F(mvp[r] * p[0]) + F(mvp[4 + r] * p[1])) + F(mvp[8 + r] * p[2])) + F(mvp[12 + r] * F(1)) for r in range(4))
            w = F(w)
            X.append(int(np.rint(F(F(F(F(F(cx) / w) * F(0.5)) + F(0.5)) * F(pk.case.width)) * F(256))))
            Y.append(int(np.rint(F(F(F(F(F(cy) / w) * F(-0.5)) + F(0.5)) * F(pk.case.height)) * F(256))))
            W.append(Fraction(float(w)))
        memo[key] = X, Y, W
    return memo[key]


def exact_lambdas(c, y, x, memo):
    """The exact rational (l1, l2) of pixel (y, x): E_j / w_j over their sum; and the affine pair E_j / A beside it."""
    X, Y, W = snapped_corners(c, y, x, memo)
    px, py = 256 * x + 128, 256 * y + 128
    edge = lambda u, v: (X[v] - X[u]) * (py - Y[u]) - (Y[v] - Y[u]) * (px - X[u])  # noqa: E731  (weight of the third corner)
    e = [edge(1, 2), edge(2, 0), edge(0, 1)]  # of corners 0, 1, 2; all of one sign inside
    q = [Fraction(e[i]) / W[i] for i in range(3)]
    s = sum(q)
    return q[1] / s, q[2] / s, Fraction(e[1], sum(e)), Fraction(e[2], sum(e))


WIDE = 100_000  # written pixels above which a case's rational check goes through the float64 sieve below


def sieved(c, bary, ys, xs, memo, bound):
    """The pixels of a large one-key-per-many-pixels case that float64 cannot decide.  The exact value is a quotient of
    sums of non-negative terms, so float64 (every step within 2^-52, nothing cancels) gives it to better than 2^-48
    relative; a pixel whose l lies within bound - 2^-40 of that value satisfies the exact bound, and only the others
    need rational arithmetic.  Every pixel is decided; none is sampled."""
    undecided = np.zeros(len(ys), bool)
    keys = (c.visibility[ys, xs] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    for key in np.unique(keys):
        sel = np.flatnonzero(keys == key)
        X, Y, W = snapped_corners(c, int(ys[sel[0]]), int(xs[sel[0]]), memo)
        px, py = 256.0 * xs[sel] + 128, 256.0 * ys[sel] + 128  # (integers below 2^53: exact)
        edge = lambda u, v: (X[v] - X[u]) * (py - Y[u]) - (Y[v] - Y[u]) * (px - X[u])  # noqa: E731
        q = [edge(1, 2) / float(W[0]), edge(2, 0) / float(W[1]), edge(0, 1) / float(W[2])]
        total = q[0] + q[1] + q[2]
        for i in (1, 2):
            exact = q[i] / total
            near = np.abs(bary[ys[sel], xs[sel], i - 1].astype(np.float64) - exact) <= (float(bound) - 2.0 ** -40) * exact
            undecided[sel] |= ~near | (exact < 2.0 ** -90)
    return undecided


def test_written_lambdas_lie_in_0_1_and_match_the_exact_rational_value(cases, mirrored):
    """Every written pixel of every case (those whose every pixel is degenerate aside: S5 wrote zeros there)."""
    bound, checked, affine_differs, worst = Fraction(8, 2 ** 24), 0, 0, Fraction(0)
    for c in cases:
        got = mirrored[c.name]
        bary = got["bary"]
        bits = bary.view(np.uint32)
        written = (got["triangle"].view(np.uint32) != FILL).any(axis=2)
        # 0.0f <= l <= 1.0f on the bit patterns: no sign bit, nothing above 1.0f
        assert (bits[written] <= ONE).all(), c.name
        assert (bary[written].astype(np.float64).sum(axis=1) <= 1 + 2.0 ** -22).all(), c.name
        assert np.isfinite(got["grad"][written]).all(), c.name
        if int(got["stats"]["degenerate_pixels"]) == int(got["stats"]["written_pixels"]):
            continue
        ys, xs = np.nonzero(written)
        memo = {}
        if len(ys) > WIDE:
            checked += len(ys)
            keep = sieved(c, bary, ys, xs, memo, bound)
            keep[::997] = True  # (and a spread of them through the rational path all the same)
            ys, xs = ys[keep], xs[keep]
            checked -= len(ys)
        for y, x in zip(ys.tolist(), xs.tolist()):
            l1, l2, a1, a2 = exact_lambdas(c, y, x, memo)
            for value, exact in ((bary[y, x, 0], l1), (bary[y, x, 1], l2)):
                value = Fraction(float(value))
                if exact < Fraction(1, 2 ** 100):
                    assert abs(value - exact) < Fraction(1, 2 ** 100), (c.name, y, x)
                else:
                    assert abs(value - exact) <= bound * exact, (c.name, y, x, float(value), float(exact))
                    worst = max(worst, abs(value - exact) / exact)
            checked += 1
            if c.name == "w_1_1_4" and abs(l1 - a1) > Fraction(1, 100):
                affine_differs += 1
    print(f"rational check: {checked} pixels, largest relative error {float(worst * 2 ** 24):.3f} * 2^-24")
    assert checked > 2_000_000 and affine_differs > 5


def test_ids_match_an_independent_decode(cases, mirrored):
    """S6 on every written pixel of every case, decoded here from the word, the command and meshlet_data."""
    total = 0
    for c in cases:
        tri = mirrored[c.name]["triangle"]
        ys, xs = np.nonzero((tri != FILL).any(axis=2))
        if len(ys) == 0:
            continue
        pk = c.packed
        word = c.visibility[ys, xs]
        k = ((word >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64) - c.command_base
        t = (word & np.uint64(255)).astype(np.int64)
        words = pk.words if c.words is None else c.words
        cmd = np.asarray(words[1:]).reshape(-1, 7).astype(np.int64)[k]
        corner = np.stack([pk.meshlet_data.view(np.uint8)[cmd[:, 2] + 3 * t + q] for q in range(3)], axis=1).astype(np.int64)
        g = cmd[:, 5:6] + pk.meshlet_data[cmd[:, 3:4] + corner]
        assert (tri[ys, xs, 0] == cmd[:, 4]).all() and (tri[ys, xs, 1:] == g).all(), c.name
        total += len(ys)
        y, x = int(ys[0]), int(xs[0])  # (and the scalar decode the rational check uses, against the same)
        entity, gs, _ = decode(c, y, x)
        assert list(tri[y, x]) == [entity] + gs, c.name
    assert total > 2_000_000


def test_exact_zeros_and_ones_and_the_swap(mirrored):
    for k, want in enumerate(((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))):
        got = mirrored[f"vertex_on_centre_{k}"]["bary"][1, 2]
        assert got.view(np.uint32).tolist() == np.array(want, F).view(np.uint32).tolist(), (k, got)
    edge = mirrored["shared_edge"]
    for q in range(9, 24):  # (8, 8) is the shared vertex itself; the diagonal's samples: the corner opposite it weighs exactly 0 on whichever side owns it
        t = int(next(c for c in sc.rasterised_cases() if c.name == "shared_edge").visibility[q, q]) & 255
        assert edge["bary"][q, q, t].view(np.uint32) == 0 and edge["bary"][q, q, 1 - t] > 0
    front, mirror = mirrored["wound_front"], mirrored["wound_mirror"]
    assert int(front["stats"]["written_pixels"]) == int(mirror["stats"]["written_pixels"]) > 50
    assert front["bary"][..., 0].tobytes() == mirror["bary"][..., 1].tobytes()
    assert front["bary"][..., 1].tobytes() == mirror["bary"][..., 0].tobytes()
    assert front["grad"][..., [0, 2]].tobytes() == mirror["grad"][..., [1, 3]].tobytes()


def test_degenerate_pixels_are_written_as_zeros(cases, mirrored):
    got = mirrored["w_2_pow_minus_120"]
    written = (got["triangle"].view(np.uint32) != FILL).any(axis=2)
    assert not got["bary"].view(np.uint32)[written].any() and not got["grad"].view(np.uint32)[written].any()
    case = next(c for c in cases if c.name == "w_2_pow_minus_120")
    tiny = np.finfo(F).tiny
    values = np.concatenate([case.packed.vertices.view(F)[9:], np.asarray(case.packed.case.view_proj, F)])
    assert ((values == 0) | (np.abs(values) >= tiny)).all()  # no denormal in the inputs
    got = mirrored["foreshortened"]
    written = (got["triangle"].view(np.uint32) != FILL).any(axis=2)
    zeroed_x = written & ~got["grad"].view(np.uint32)[..., :2].any(axis=2)
    assert int(zeroed_x.sum()) == int(got["stats"]["degenerate_pixels"]) > 0
    assert got["grad"][..., 2:][zeroed_x].any()  # (the y axis of the same pixels is kept)


def test_clip_buffers_hold_unsupported_pixels_under_status_ok(cases, mirrored):
    unsupported = written = 0
    for c in cases:
        if not c.name.startswith("clip_"):
            continue
        got = mirrored[c.name]
        assert got["status"] == 0 and int(got["stats"]["stale_pixels"]) == 0, c.name
        unsupported += int(got["stats"]["unsupported_pixels"])
        written += int(got["stats"]["written_pixels"])
    assert unsupported > 1000 and written > 100


def test_each_stale_case_counts_the_tampered_pixels_and_changes_nothing_else(cases, mirrored):
    stale = [c for c in cases if c.stale]
    assert len(stale) >= 9
    for c in stale:
        got = mirrored[c.name]
        clean = guarded_mirror(c.clean)
        assert clean["status"] == 0 and got["status"] == _lib.E_RANGE, c.name
        assert int(got["stats"]["stale_pixels"]) == len(c.stale), c.name
        for k in KEYS:
            same = got[k].view(np.uint32) == clean[k].view(np.uint32)
            for y, x in c.stale:
                assert (got[k].view(np.uint32)[y, x] == FILL).all(), (c.name, k)
                same[y, x] = True
            assert same.all(), (c.name, k)


def test_layouts_match_the_header():
    assert C.sizeof(_lib.VisibilitySurface) == 184 and L.SURFACE_STATS.itemsize == 32
    for name, offset in (("bary", 40), ("stats", 64), ("meshlet_data_words", 72), ("max_commands", 88), ("command_base", 116),
                         ("view_proj", 120)):
        assert getattr(_lib.VisibilitySurface, name).offset == offset, name
    assert _lib.SURFACE_CLEAR == 1


def test_each_argument_error_has_its_own_message_without_a_device():
    lib = _lib.load()
    buf = np.zeros(64, np.uint64)
    at = buf.ctypes.data  # 16-B aligned: numpy's allocations are
    assert at % 16 == 0

    def call(**kw):
        j = _lib.VisibilitySurface()
        j.visibility = j.draw_commands = j.meshlet_data = j.vertices = j.entity_data = at
        j.bary = j.grad = j.triangle = j.stats = at
        j.vertex_stride, j.width, j.height, j.max_commands, j.flags = 12, 4, 4, 1, _lib.SURFACE_CLEAR
        for k, v in kw.items():
            setattr(j, k, v)
        rc_ = lib.orbit_visibility_surface(None, C.byref(j), None)
        return rc_, lib.orbit_last_error(None).decode()

    assert lib.orbit_visibility_surface(None, None, None) == _lib.E_INVALID and "job is NULL" in lib.orbit_last_error(None).decode()
    for over in (dict(), dict(flags=0), dict(bary=None, grad=None), dict(triangle=None, stats=None, vertex_count=1 << 40),
                 dict(vertex_count=1 << 32), dict(command_base=_lib.VIS_MAX_COMMANDS - 1), dict(width=_lib.RASTER_MAX_DIM, height=1),
                 dict(vertex_stride=32, position_offset=20)):
        assert call(**over) == (_lib.E_INVALID, "visibility_surface: ctx is NULL"), over
    top = _lib.VIS_MAX_COMMANDS
    for over, reason in (
            [(dict([(k, None)]), "NULL buffer") for k in ("visibility", "draw_commands", "meshlet_data", "vertices", "entity_data")]
            + [(dict(bary=None, grad=None, triangle=None), "no output")]
            + [(dict(visibility=at + 4), "aligned"), (dict(entity_data=at + 8), "aligned")]
            + [(dict([(k, at + 2)]), "aligned") for k in ("draw_commands", "meshlet_data", "vertices", "bary", "grad", "triangle", "stats")]
            + [(dict(vertex_stride=8), "vertex_stride"), (dict(vertex_stride=14), "vertex_stride"),
               (dict(vertex_stride=16, position_offset=8), "vertex_stride"), (dict(vertex_stride=16, position_offset=2), "vertex_stride"),
               (dict(width=0), "target"), (dict(height=0), "target"), (dict(width=_lib.RASTER_MAX_DIM + 1), "target"),
               (dict(height=_lib.RASTER_MAX_DIM + 1), "target"), (dict(command_base=top), "24 bits"),
               (dict(command_base=top - 1, max_commands=2), "24 bits"), (dict(max_commands=top + 1), "24 bits"),
               (dict(vertex_count=(1 << 32) + 1), "2^32"),
               (dict(flags=2), "flags"), (dict(flags=_lib.RASTER_CLIP_NEAR | 1), "flags"), (dict(flags=_lib.RASTER_WIDE_GUARD), "flags"),
               (dict(flags=1 << 31), "flags")]):
        rc_, text = call(**over)
        assert rc_ == _lib.E_INVALID and reason in text and "ctx is NULL" not in text, (over, text)
    assert not buf.any()  # nothing was written
    # the mirror answers the same argument errors with a panic
    c = sc.perspective_case()
    a, kw = c.args()
    with pytest.raises(Exception):
        raster.host_visibility_surface(*a, **dict(kw, want=()))
    with pytest.raises(Exception):
        raster.host_visibility_surface(*a, **dict(kw, vertex_stride=14))


def test_the_scenes_two_pass_frame_one_call_per_list(oracle):
    """The 100-instance glTF scene at 320 x 180, both frames of two_pass_frame: the early list at base 0 and the late one
    at base = the capacity, one call each into shared outputs (the second without CLEAR).  Everything the resolve sees
    covered is written, nothing is stale or unsupported, and `triangle` is the visibility word's decode."""
    scene = rs.glb_scene(100)
    w, h, cap = 320, 180, scene.cap_c
    cams = [rs.camera(w, h), rs.camera(w, h, (1.5, 1.2, 5.0))]
    frames = rs.two_pass_frame(scene, oracle, cams[0], cams[1], w, h)
    total = 0
    for f, cam in enumerate(cams):
        frame, vp = frames[f], rs.view_proj(cam)
        common = (scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities, vp)
        vis = None
        for k, name in enumerate(("draw1", "draw2")):
            vis = raster.host_raster_visibility(frame[name], cap, *common, w, h, visibility=vis, command_base=k * cap, clear=k == 0)[0]
        assert (vis >> np.uint64(32)).astype(np.uint32).tobytes() == frame["depth2"].tobytes()
        out, written = None, 0
        for k, name in enumerate(("draw1", "draw2")):
            out = raster.host_visibility_surface(vis, frame[name], cap, *common, command_base=k * cap, clear=k == 0, into=out)
            assert out["status"] == 0 and int(out["stats"]["stale_pixels"]) == int(out["stats"]["unsupported_pixels"]) == 0
            assert int(out["stats"]["degenerate_pixels"]) == 0
            written += int(out["stats"]["written_pixels"])
        covered = int(raster.host_visibility_resolve(vis, 0, 2 * cap)[2]["covered_pixels"])
        assert written == covered == int((vis != 0).sum()) > w * h // 4
        total += written
        # S6 against the word's own decode, every covered pixel at once
        ys, xs = np.nonzero(vis)
        ids = ((vis[ys, xs] >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64)
        t = (vis[ys, xs] & np.uint64(255)).astype(np.int64)
        late = ids >= cap
        lists = [np.ascontiguousarray(frame[n]).view(np.uint8).reshape(-1)[4:].view(np.uint32)[:7 * cap].reshape(-1, 7)
                 for n in ("draw1", "draw2")]
        cmd = np.where(late[:, None], lists[1][np.clip(ids - cap, 0, cap - 1)], lists[0][np.clip(ids, 0, cap - 1)]).astype(np.int64)
        corners = np.stack([scene.meshlet_data.view(np.uint8)[cmd[:, 2] + 3 * t + q] for q in range(3)], axis=1).astype(np.int64)
        g = cmd[:, 5:6] + scene.meshlet_data[cmd[:, 3:4] + corners]
        assert (out["triangle"][ys, xs, 0] == cmd[:, 4]).all() and (out["triangle"][ys, xs, 1:] == g).all()
        unwritten = vis == 0
        assert (out["triangle"][unwritten] == 0xFFFFFFFF).all() and not out["bary"].view(np.uint32)[unwritten].any()
        assert (out["bary"].view(np.uint32)[~unwritten] <= ONE).all()
        # the rational value of every written pixel (tools/count_visible_surface.py's own loop): within the issue's bound
        worst = surface_tool().max_relative_error(vis, out, scene, vp, w, h)
        assert worst <= 8.0, (f, worst)
    assert total > 40000


def surface_tool():
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("count_visible_surface", os.path.join(rs.ROOT, "tools", "count_visible_surface.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool
