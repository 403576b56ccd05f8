"""Inputs for the raster calls with ORBIT_RASTER_WIDE_GUARD (include/orbit_abi_ext.h R4w, R5w-R7w): hand-built
meshlets at the edges of the wide rule, on raster_cases.Case / Packed, each with what it CLAIMS — counters known in
closed form and the route it must take, read from the extras of the restatement tests/raster_wide_ref.py.  As in the
other case files the expected bytes are never computed here: the GPU tests' reference is the host mirror, which
tests/test_raster_wide_cpu.py holds to the restatement; census() checks the claims against the restatement.

Most cases are written in SNAPPED coordinates: at(xf, yf, w) is the model position that the projection sub_proj()
(clip = (x, y, 1/8, z): w is the model's z, the depth is 1 / (8 w)) carries to X = xf, Y = yf of R4 / R4w, found by
inverting R4 and checked with the restatement's own snap().  The clipping cases use raster_cases.w_from_z_proj and
raster_clip_cases.exact_proj as tests/raster_clip_cases.py does."""
from dataclasses import dataclass

import numpy as np

import raster_cases as rc
import raster_wide_ref as wref
from raster_cases import poly, w_from_z_proj
from raster_clip_cases import exact_proj
from raster_vis_cases import VisCase

F = np.float32
W, H = 64, 48
CX, CY = 128 * W, 128 * H  # the snapped centre of the 64 x 48 target
BELOW_2_60 = int(np.nextafter(F(2.0 ** 60), F(0)))


@dataclass
class WideCase(VisCase):
    clip_near: bool = False
    wide: object = None  # f(extras, stats, visibility) -> bool on the restatement's extras: the route the case is there for


def sub_proj():
    return exact_proj()


def nan_proj():
    """sub_proj with clip.x = 2 x - 2 y: two products that overflow to +inf and -inf sum to NaN while z and w stay finite"""
    m = sub_proj()
    m[0], m[4] = 2, -2
    return m


def at(xf, yf, w=1.0, width=W, height=H):
    """the model position that snaps to (xf, yf) at clip w = `w` (a power of two) under sub_proj()"""
    w = F(w)

    def solve(target, size, sign):
        guess = F(sign * (target / (128.0 * size) - 1.0))
        cands = [guess]
        for _ in range(4):
            cands += [np.nextafter(cands[-1], F(np.inf))]
        c = guess
        for _ in range(4):
            c = np.nextafter(c, F(-np.inf))
            cands.append(c)
        for c in cands:
            v = F(F(F(c * F(0.5 * sign)) + F(0.5)) * F(size)) * F(256)
            if int(np.rint(v)) == target:
                return F(c * w)
        raise AssertionError(f"no fp32 coordinate snaps to {target}")

    x, y = solve(xf, width, 1), solve(yf, height, -1)
    X, Y, kind = wref.snap(x, y, w, width, height, True)
    assert (X, Y) == (xf, yf) and kind != wref.OUT, (xf, yf, X, Y, kind)
    return (float(x), float(y), float(w))


# --------------------------------------------------------------------------------------------- running a packed case
def flags_of(pk, wide=True, clear=True, clip_near=None):
    clip_near = getattr(pk.case, "clip_near", False) if clip_near is None else clip_near
    return (pk.flags | (wref.CLEAR if clear else 0) | (wref.CLIP_NEAR if clip_near else 0) | (wref.WIDE_GUARD if wide else 0))


def restated_vis(pk, visibility=None, clear=True, wide=True, clip_near=None, **opts):
    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    return wref.raster(words, mc, data, vb, vc, ent, vp, w, h, visibility=visibility,
                       command_base=getattr(pk.case, "command_base", 0), flags=flags_of(pk, wide, clear, clip_near), **kw, **opts)


def restated_depth(pk, depth=None, clear=True, wide=True, clip_near=None):
    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    return wref.raster_depth(words, mc, data, vb, vc, ent, vp, w, h, depth=depth, flags=flags_of(pk, wide, clear, clip_near), **kw)


def host_vis(pk, visibility=None, clear=True, wide=True, clip_near=None):
    from orbit_amd import raster

    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    clip_near = getattr(pk.case, "clip_near", False) if clip_near is None else clip_near
    return raster.host_raster_visibility(words, mc, data, vb, vc, ent, vp, w, h, visibility=visibility,
                                         command_base=getattr(pk.case, "command_base", 0), clear=clear,
                                         cull_none=pk.case.cull_none, clip_near=clip_near, wide_guard=wide, **kw)


def host_depth(pk, depth=None, clear=True, wide=True, clip_near=None):
    from orbit_amd import raster

    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    clip_near = getattr(pk.case, "clip_near", False) if clip_near is None else clip_near
    return raster.host_raster_depth(words, mc, data, vb, vc, ent, vp, w, h, depth=depth, clear=clear,
                                    cull_none=pk.case.cull_none, clip_near=clip_near, wide_guard=wide, **kw)


# --------------------------------------------------------------------------------------------------------- geometry
def _covered(vis):
    return int((np.asarray(vis) != 0).sum())


def _wide_drawn(n=1, **more):
    return lambda e, s, vis: e["wide_drawn"] == n and s["fragments"] > 0 and all(e[k] == v for k, v in more.items())


def _watertight(e, s, vis):
    return s["fragments"] == _covered(vis) > 0


# two on-screen corners beside the far one: with the far vertex LAST the triangle (A, B, far) is front-facing (A < 0 in
# y-down snapped coordinates) for a far vertex to the right
A, B = (1024, 1024), (1024, 11000)
BIG = 2 ** 30


def build_cases():
    cases = []
    ps = sub_proj()
    add = lambda *a, **k: cases.append(WideCase(*a, **{"view_proj": ps, "cull_none": True, **k}))  # noqa: E731
    one = dict(triangles=1, clip_skipped=0)
    # ------------------------------------------------------------------------------------------------- band edges
    # (x = 1023 - 2^-14 gives xf = 2^23 - 0.5 exactly: below the band's edge, and rint ties it to the even 2^23)
    add("band_edge_narrow_side", [poly([((1023 - 2.0 ** -14, 0.0, 1.0), at(*A), at(*B))])], stats=dict(one, guard_skipped=0),
        wide=lambda e, s, vis: e["wide_pieces"] == 0 and e["wave_pieces"] == 1 and s["fragments"] > 0,
        what="|xf| = 2^23 - 0.5: narrow, R5-R8 as without the flag")
    add("band_edge_wide_side", [poly([(at(2 ** 23, CY), at(*A), at(*B))])], stats=dict(one, guard_skipped=0),
        wide=_wide_drawn(max_coord_bits=24), what="|xf| = 2^23: the first wide coordinate")
    add("band_top_below_2_60", [poly([(at(BELOW_2_60, CY), at(*A), at(*B))])], stats=dict(one, guard_skipped=0),
        wide=_wide_drawn(max_coord_bits=60), what="the largest float below 2^60: still wide")
    add("band_top_2_60_is_out", [poly([((2.0 ** 47, 0.0, 1.0), at(*A), at(*B))])], stats=dict(one, guard_skipped=1, fragments=0),
        covered_count=0, wide=lambda e, s, vis: e["out_of_band_pieces"] == 1 and e["wide_pieces"] == 0,
        what="xf = 2^60 itself: out of band, guard_skipped")
    add("infinite_xf_is_out", [poly([((3.0e38, 0.0, 0.5), at(*A), at(*B))])], stats=dict(one, guard_skipped=1, fragments=0),
        covered_count=0, wide=lambda e, s, vis: e["out_of_band_pieces"] == 1, what="x / w overflows to infinity: guard_skipped")
    add("nan_xf_is_out", [poly([((3.0e38, 3.0e38, 1.0), (-0.9, 0.9, 1.0), (-0.9, -0.9, 1.0))])], view_proj=nan_proj(),
        stats=dict(one, guard_skipped=1, fragments=0), covered_count=0, wide=lambda e, s, vis: e["out_of_band_pieces"] == 1,
        what="clip.x = inf - inf = NaN with z and w finite: R3 passes, R4w does not")
    # ------------------------------------------------------------------------------- position of the wide vertex
    far = dict(x_only=(BIG, CY), y_only=(CX, BIG), both=(BIG, 2 ** 29), negative_side=(-BIG, -2 ** 28))
    for name, f in far.items():
        near = ((1024, 1024), (15000, 1024)) if name == "y_only" else (A, B)
        tri = (at(*near[0], w=1.0), at(*near[1], w=2.0), at(*f, w=0.5))  # three depths: the plane's anchor matters
        for k in range(3):
            add(f"wide_{name}_corner_{k}", [poly([tri[-k:] + tri[:-k] if k else tri])], stats=dict(one, guard_skipped=0, no_coverage=0),
                wide=_wide_drawn(), what=f"one wide vertex ({name}), as corner {k} of the triangle")
    add("two_wide_vertices", [poly([(at(CX, 1024), at(BIG, 2 ** 29, w=2.0), at(-BIG, 2 ** 29, w=0.5))])],
        stats=dict(one, guard_skipped=0), wide=_wide_drawn(), what="two wide vertices, the narrow one on the screen")
    add("three_wide_enclose_the_target", [poly([(at(-BIG, -BIG), at(-BIG, 2 ** 31, w=2.0), at(2 ** 31, -BIG, w=0.5))])],
        stats=dict(one, guard_skipped=0, fragments=W * H), covered_count=W * H, wide=_wide_drawn(),
        what="three wide vertices around the whole target: every pixel is covered")
    # ---------------------------------------------------------------------------------------- more than 64 bits
    add("edge_products_beyond_64_bits", [poly([(at(-2 ** 50, -2 ** 49), at(-2 ** 48, 2 ** 52, w=2.0), at(2 ** 51, -2 ** 50, w=0.5))])],
        stats=dict(one, guard_skipped=0, fragments=W * H), covered_count=W * H,
        wide=lambda e, s, vis: e["beyond_64_bits"] == 1 and e["wrap_differs"] == 1,
        what="products near 2^100: wrapped to 64 bits the coverage is another one (the restatement checks it)")
    # ---------------------------------------------------------------------------------------- exact zero, facing
    add("collinear_wide_is_exactly_zero", [poly([(at(2 ** 23 + 1, 2 ** 24 + 2), at(2 ** 40, 2 ** 41), at(2 ** 58, 2 ** 59))])],
        stats=dict(one, guard_skipped=0, no_coverage=1, fragments=0), covered_count=0,
        wide=lambda e, s, vis: e["wide_no_coverage"] == 1, what="three wide vertices on y = 2 x: A == 0 in 128-bit integers")
    # x = 9 y and x = 3 y through a NARROW vertex and two wide ones: the differences from the narrow vertex need more
    # than 53 bits (X2 - X0 has 55 and 56), so a float64 evaluation rounds them, and the two products no longer cancel
    add("collinear_wide_zero_only_in_integers",
        [poly([(at(-638541, -70949), at(28929461059584, 3214384562176, w=2.0), at(29133897040134144, 3237099671126016, w=0.5))]),
         poly([(at(2377686, 792562), at(8213635327328256, 2737878442442752, w=2.0), at(71736742801047552, 23912247600349184, w=0.5))])],
        stats=dict(triangles=2, guard_skipped=0, no_coverage=2, back_facing=0, fragments=0), covered_count=0,
        wide=lambda e, s, vis: e["wide_no_coverage"] == 2 and e["double_area_wrong"] == 2,
        what="exactly collinear with one narrow vertex: A == 0 in 128-bit integers where the same expression in double "
             "is 1.8e13 and 3.6e16; an area kept in double would draw or cull them")
    add("nearly_collinear_wide_is_not_zero", [poly([(at(0, 0), at(2 ** 40, 2 ** 40), at(2 ** 58, 2 ** 58 + 2 ** 35))]),
                                             poly([(at(0, 0), at(2 ** 58, 2 ** 58 - 2 ** 35), at(2 ** 40, 2 ** 40))])],
        stats=dict(triangles=2, guard_skipped=0, no_coverage=1, back_facing=0, fragments=H), covered_count=H,
        wide=lambda e, s, vis: e["wide_drawn"] == 1 and e["wide_no_coverage"] == 0 and e["beyond_64_bits"] == 2,
        what="one ulp of a 2^58 coordinate off the diagonal, either side: A is 2^-23 of its products and not zero; the "
             "slivers hold only the samples ON the diagonal, which the top-left rule gives to one of them")
    back = (at(*B), at(*A), at(BIG, CY))
    add("back_facing_wide_dropped", [poly([back])], cull_none=False, stats=dict(one, back_facing=1, fragments=0), covered_count=0,
        wide=lambda e, s, vis: e["wide_back_facing"] == 1, what="A > 0 in 128 bits: back_facing")
    add("back_facing_wide_kept", [poly([back])], stats=dict(one, back_facing=0), wide=_wide_drawn(), what="CULL_NONE draws it, swapped")
    add("front_facing_wide_culled_call", [poly([tuple(reversed(back))])], cull_none=False, stats=dict(one, back_facing=0),
        wide=_wide_drawn(), what="the same triangle front-facing, back-face culling on")
    add("wide_wholly_off_target", [poly([(at(2 ** 24, 1024), at(2 ** 24, 11000), at(BIG, CY))])],
        stats=dict(one, no_coverage=1, fragments=0), covered_count=0, wide=lambda e, s, vis: e["wide_off_target"] == 1,
        what="x_lo > x_hi after the clamp: no_coverage")
    # -------------------------------------------------------------------------------------------- top-left rule
    yc, xc = 256 * 20 + 128, 256 * 30 + 128
    h_near, h_far = (256 * 4 + 128, yc), (BIG, yc)
    add("horizontal_edge_through_centres", [poly([(at(*h_near), at(*h_far), at(256 * 4 + 128, yc - 256 * 9)),
                                                  (at(*h_near), at(256 * 4 + 128, yc + 256 * 9), at(*h_far))])],
        stats=dict(triangles=2, no_coverage=0), wide=lambda e, s, vis: e["wide_drawn"] == 2 and _watertight(e, s, vis),
        what="a horizontal edge through sample centres to a wide end, shared from above and below: row 20 goes to one side")
    add("horizontal_edge_other_orientation", [poly([(at(*h_far), at(*h_near), at(256 * 4 + 128, yc - 256 * 9)),
                                                    (at(*h_far), at(256 * 4 + 128, yc + 256 * 9), at(*h_near))])],
        stats=dict(triangles=2, no_coverage=0), wide=lambda e, s, vis: e["wide_drawn"] == 2 and _watertight(e, s, vis),
        what="the same two triangles wound the other way round")
    v_near, v_far = (xc, 256 * 3 + 128), (xc, BIG)
    add("vertical_edge_through_centres", [poly([(at(*v_near), at(*v_far), at(xc - 256 * 9, 256 * 3 + 128)),
                                                (at(*v_near), at(xc + 256 * 9, 256 * 3 + 128), at(*v_far))])],
        stats=dict(triangles=2, no_coverage=0), wide=lambda e, s, vis: e["wide_drawn"] == 2 and _watertight(e, s, vis),
        what="a vertical edge through sample centres to a wide end, shared from the left and the right")
    add("vertical_edge_other_orientation", [poly([(at(*v_far), at(*v_near), at(xc - 256 * 9, 256 * 3 + 128)),
                                                  (at(*v_far), at(xc + 256 * 9, 256 * 3 + 128), at(*v_near))])],
        stats=dict(triangles=2, no_coverage=0), wide=lambda e, s, vis: e["wide_drawn"] == 2 and _watertight(e, s, vis),
        what="the same wound the other way round")
    # -------------------------------------------------------------------------------------------- watertightness
    ring = [(BIG, 0), (2 ** 29, BIG), (-2 ** 29, BIG), (-BIG, 0), (-2 ** 29, -BIG), (2 ** 29, -BIG)]
    hub = at(CX + 37, CY - 21)
    add("fan_of_wide_triangles", [poly([(hub, at(*ring[k], w=2.0), at(*ring[(k + 1) % 6], w=2.0)) for k in range(6)])],
        stats=dict(triangles=6, fragments=W * H, no_coverage=0), covered_count=W * H,
        wide=lambda e, s, vis: e["wide_drawn"] == 6 and _watertight(e, s, vis),
        what="six wide triangles around an on-screen vertex: six shared edges with a wide end, every sample once")
    a, b, c, d = (2000, 2000), (2000, 9000), (9000, 2500), (9500, 9300)
    add("strip_of_narrow_and_wide", [poly([(at(*a), at(*b), at(*c)), (at(*b), at(*d), at(*c)), (at(*c), at(*d), at(BIG, 2 ** 28, w=2.0)),
                                           (at(*a), at(-BIG, 2 ** 27, w=2.0), at(*b))])],
        stats=dict(triangles=4, no_coverage=0),
        wide=lambda e, s, vis: e["wide_drawn"] == 2 and e["wave_pieces"] == 2 and _watertight(e, s, vis),
        what="two narrow triangles between two wide ones: the shared edges c-d and a-b have narrow ends on both sides")
    # --------------------------------------------------------------------------------------------------- routes
    add("wide_sliver_in_a_small_box", [poly([(at(-BIG, 100), at(1000, 100), at(1000, 1000))])], stats=dict(one, no_coverage=0),
        wide=_wide_drawn(wide_small_box=1), what="a wide triangle whose clamped box holds 4 x 4 samples: still the wide route")
    add("wide_over_most_of_256x144", [poly([(at(-BIG, 2 ** 20, w=1.0, width=256, height=144), at(2 ** 16, -BIG, w=2.0, width=256, height=144),
                                            at(2 ** 17, BIG, w=0.5, width=256, height=144))])],
        width=256, height=144, stats=dict(one, no_coverage=0),
        wide=lambda e, s, vis: e["wide_drawn"] == 1 and _covered(vis) > 256 * 144 // 2,
        what="a wide triangle over most of a target of 4 x 3 blocks of 64 x 64 (the last row and column of blocks partial)")
    add("wide_wedge_of_256x144", [poly([(at(2000, 30000, width=256, height=144), at(BIG, 2 ** 28, w=2.0, width=256, height=144),
                                        at(BIG, 2 ** 28 + 2 ** 26, w=0.5, width=256, height=144))])],
        width=256, height=144, stats=dict(one, no_coverage=0),
        wide=lambda e, s, vis: e["wide_drawn"] == 1 and 0 < _covered(vis) < 256 * 144 // 8,
        what="a wedge: a box of most of the target, a coverage of a few tiles of it")
    small = (at(5000, 5000), at(5000, 5600), at(5600, 5000))
    wide_tri = (at(*A), at(*B), at(BIG, CY, w=0.5))
    add("wide_in_the_second_chunk", [poly([small] * 64 + [wide_tri, (at(*B), at(*A, w=2.0), at(-BIG, CY))])],
        stats=dict(triangles=66, guard_skipped=0), wide=_wide_drawn(2), what="66 triangles, the two wide ones at index 64 and 65")
    add("nt_256_wide_last", [poly([small] * 255 + [wide_tri])], stats=dict(triangles=256, range_errors=0, guard_skipped=0),
        wide=_wide_drawn(), winners=lambda won, e, s, err: won.get((0, 255), 0) > 0 and err == [0],
        what="256 triangles: the wide one carries index 255 into the low byte")
    top = (1 << 24) - 1
    add("command_base_top_of_24_bits", [poly([wide_tri])], command_base=top, stats=dict(one, guard_skipped=0), wide=_wide_drawn(),
        winners=lambda won, e, s, err: list(won) == [(top, 0)] and won[(top, 0)] == s["fragments"],
        what="command_base = 2^24 - 1: a wide triangle's word carries the top id")
    # ------------------------------------------------------------------------------------------ with CLIP_NEAR
    pw = w_from_z_proj()
    IN, OUT = 0.2, 0.05
    add("one_in_new_vertices_wide", [poly([((0.0, 0.0, IN), (300.0, -30.0, OUT), (300.0, 30.0, OUT))])], view_proj=pw, clip_near=True,
        stats=dict(one, guard_skipped=0), wide=lambda e, s, vis: e["one_in"] == 1 and e["wide_drawn"] == 1 and s["fragments"] > 0,
        what="raster_clip_cases' guard_piece_none_draws opened up: both new vertices are wide, the piece is drawn now")
    add("one_out_one_narrow_one_wide_piece", [poly([((300.0, 0.0, OUT), (-0.02, -0.1, IN), (-0.02, 0.1, 0.101))])], view_proj=pw,
        clip_near=True, stats=dict(one, guard_skipped=0),
        wide=lambda e, s, vis: e["one_out"] == 1 and e["mixed_pieces"] == 1 and _watertight(e, s, vis),
        what="the shape of raster_clip_cases' guard_piece_other_draws: piece (b, c, Q) is narrow, piece (b, Q, P) wide, the diagonal shared")
    add("one_out_both_pieces_wide", [poly([((0.0, -0.05, -0.05), (-3000.0, -0.05, 0.5), (3000.0, -0.05, 0.5))])], view_proj=pw, clip_near=True,
        stats=dict(one, guard_skipped=0), wide=lambda e, s, vis: e["one_out"] == 1 and e["wide_drawn"] == 2 and _watertight(e, s, vis),
        what="a floor through the eye's plane, 6000 units wide: both pieces wide")
    t_cross = ((-65536.0, -0.0625, 0.25), (131072.0, -0.0625, 0.0), (-65536.0, 0.125, 0.0))  # t = 1/2 on both edges
    t_whole = ((-65536.0, -0.0625, 0.25), (32768.0, -0.0625, 0.125), (-65536.0, 0.03125, 0.125))  # its piece, written down
    for name, tris in (("tie_wide_piece_loses_to_later_triangle", (t_cross, t_whole)),
                       ("tie_wide_piece_wins_over_earlier_triangle", (t_whole, t_cross))):
        add(name, [poly([tris[0]]), poly([tris[1]])], view_proj=exact_proj(), clip_near=True, cull_none=False,
            stats=dict(triangles=2, clip_skipped=0, back_facing=0, guard_skipped=0),
            wide=lambda e, s, vis: e["one_in"] == 1 and e["wide_drawn"] == 2 and s["fragments"] == 2 * _covered(vis) > 0,
            winners=lambda won, e, s, err: list(won) == [(1, 0)],
            what="an exact wide piece and the same wide triangle unclipped: equal depth on every sample, the larger id wins")
    return cases


def all_cases():
    return build_cases()


ROUTES = ("band_edge", "out_of_band", "wide_one", "wide_two", "wide_three", "beyond_64_bits", "exact_zero", "zero_not_in_double", "back_facing",
          "off_target", "small_box", "second_chunk", "clipped_one_in", "clipped_one_out", "mixed_pieces", "tie")


def routes_of(case, extras, stats):
    """the classes of ROUTES that `case` exercises, from the restatement's extras"""
    e, out = extras, set()
    if case.name.startswith("band_"):
        out.add("band_edge")
    if e["out_of_band_pieces"]:
        out.add("out_of_band")
    for key, names in (("wide_one", ("corner_",)), ("wide_two", ("two_wide",)), ("wide_three", ("three_wide", "beyond_64"))):
        if any(n in case.name for n in names) and e["wide_drawn"]:
            out.add(key)
    for key, route in (("beyond_64_bits", "beyond_64_bits"), ("wide_no_coverage", "exact_zero"), ("wide_back_facing", "back_facing"),
                       ("wide_off_target", "off_target"), ("double_area_wrong", "zero_not_in_double"), ("wide_small_box", "small_box"), ("mixed_pieces", "mixed_pieces")):
        if e[key]:
            out.add(route)
    if e["wide_drawn"] and stats["triangles"] > 64:
        out.add("second_chunk")
    if e["one_in"] and e["wide_pieces"]:
        out.add("clipped_one_in")
    if e["one_out"] and e["wide_pieces"]:
        out.add("clipped_one_out")
    if case.name.startswith("tie_"):
        out.add("tie")
    return out


def check_claims(case, visibility, stats, errors, extras):
    """-> list of what `case` claims and does not reach: raster_cases' claims on the high halves, the route on the
    restatement's `extras` (None: not checked), the winners on the words."""
    depth = wref.depth_of(visibility)
    base = rc.Case(**{k: getattr(case, k) for k in rc.Case.__dataclass_fields__})
    base.extra = None
    missed = rc.check_claims(base, depth, stats, errors, None)
    if case.wide is not None and extras is not None and not case.wide(extras, stats, np.asarray(visibility)):
        missed.append(f"the route it is there for was not taken: {extras}")
    if case.winners is not None:
        from raster_vis_ref import winners

        won = winners(visibility, case.command_base, len(case.meshlets))
        if not case.winners(won, extras, stats, list(errors)):
            missed.append(f"the winners are not the claimed ones: {won}")
    return missed


def census(cases=None, verbose=True):
    """-> ({name: [missed claims]}, the set of ROUTES reached); prints one line per case"""
    out, reached = {}, set()
    for c in all_cases() if cases is None else cases:
        vis, stats, errors, extras = restated_vis(rc.Packed(c), check_wrap=True)
        out[c.name] = check_claims(c, vis, stats, errors, extras)
        routes = routes_of(c, extras, stats)
        reached |= routes
        if verbose:
            line = ", ".join(f"{k}={v}" for k, v in stats.items() if v)
            print(f"{c.name:44s} {line}  {sorted(routes)}  -- {c.what}" + (f"  MISSED: {out[c.name]}" if out[c.name] else ""))
    return out, reached


if __name__ == "__main__":
    print(sorted(set(ROUTES) - census()[1]))
