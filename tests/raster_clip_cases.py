"""Inputs for the raster calls with ORBIT_RASTER_CLIP_NEAR (include/orbit_abi_ext.h R3c): hand-built meshlets at the
edges of the clipping rule, on raster_cases.Case / Packed, each with what it CLAIMS — counters known in closed form and
the route it must take.  As in raster_cases, the expected bytes are never computed here: the GPU tests' reference is
the host mirror, which tests/test_raster_clip_cpu.py holds to the restatement tests/raster_clip_ref.py; census() checks
the claims against the restatement.

Most cases use raster_cases.w_from_z_proj: clip = (x, y, 0.1, z), so a model position is (x, y, w), the near plane is
w = 0.1, w < 0.1 is in front of it and w <= 0 behind the eye; y is up.  EXACT_PROJ is the same with near 0.125, where
the new vertices of suitable triangles are exact and can be written down as model positions."""
from dataclasses import dataclass

import numpy as np

import raster_cases as rc
import raster_clip_ref as cref
from raster_cases import Meshlet, poly, w_from_z_proj
from raster_vis_cases import VisCase

F = np.float32


@dataclass
class ClipCase(VisCase):
    clip: object = None  # f(extras, stats, visibility) -> bool on the restatement's extras: the route the case is there for


def exact_proj():
    m = np.zeros(16, F)
    m[0], m[5], m[11], m[14] = 1, 1, 1, F(0.125)
    return m


def zw_proj():
    """clip = (x, x / 4, y, z): a model position's y is clip z and its z is clip w, independent of each other"""
    m = np.zeros(16, F)
    m[0], m[1], m[6], m[11] = 1, F(0.25), 1, 1
    return m


# --------------------------------------------------------------------------------------------- running a packed case
def flags_of(pk, clip_near=True, clear=True):
    return pk.flags | (cref.CLEAR if clear else 0) | (cref.CLIP_NEAR if clip_near else 0)


def restated_vis(pk, visibility=None, clear=True, clip_near=True):
    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    return cref.raster(words, mc, data, vb, vc, ent, vp, w, h, visibility=visibility,
                       command_base=getattr(pk.case, "command_base", 0), flags=flags_of(pk, clip_near, clear), **kw)


def restated_depth(pk, depth=None, clear=True, clip_near=True):
    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    return cref.raster_depth(words, mc, data, vb, vc, ent, vp, w, h, depth=depth, flags=flags_of(pk, clip_near, clear), **kw)


def host_vis(pk, visibility=None, clear=True, clip_near=True):
    from orbit_amd import raster

    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    return raster.host_raster_visibility(words, mc, data, vb, vc, ent, vp, w, h, visibility=visibility,
                                         command_base=getattr(pk.case, "command_base", 0), clear=clear,
                                         cull_none=pk.case.cull_none, clip_near=clip_near, **kw)


def host_depth(pk, depth=None, clear=True, clip_near=True):
    from orbit_amd import raster

    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    return raster.host_raster_depth(words, mc, data, vb, vc, ent, vp, w, h, depth=depth, clear=clear,
                                    cull_none=pk.case.cull_none, clip_near=clip_near, **kw)


# --------------------------------------------------------------------------------------------------------- geometry
IN, OUT = 0.2, 0.05  # w of a vertex behind / in front of the near plane 0.1
# front-facing under w_from_z_proj for any positive w (y up in clip space): screen corners at x / w, y / w
BASE = ((-0.04, -0.04), (0.04, -0.04), (-0.04, 0.04))
ALL_OUT = tuple((x, y, OUT) for x, y in BASE)


def crossing(ws, base=BASE):
    return tuple((x, y, w) for (x, y), w in zip(base, ws))


def _drawn(one_in=0, one_out=0):
    return lambda e, s, vis: (e["one_in"], e["one_out"]) == (one_in, one_out) and s["fragments"] > 0


def _watertight(e, s, vis):
    return s["fragments"] == int((vis != 0).sum()) > 0


def _cascade_caster():
    """A triangle of the cascade's light space: two vertices inside its depth range, the third moved along the
    projection's z axis to z = 1.5, in front of the cascade's near plane (w = 1 everywhere)."""
    m = np.asarray(rc._cascade_view_proj(), np.float64).reshape(4, 4).T  # rows
    p = np.array([0.0, 2.0, -2.0])
    grad = m[2, :3]
    z0 = m[2, :3] @ p + m[2, 3]
    assert 0 < z0 < 1
    third = p + grad * (1.5 - z0) / (grad @ grad) + np.array([0.0, 0.6, 0.0]) - grad * (grad @ [0.0, 0.6, 0.0]) / (grad @ grad)
    return [poly([(tuple(p + (-0.5, -0.3, 0.0)), tuple(p + (0.5, -0.3, 0.0)), tuple(third))])]


def build_cases():
    cases = []
    pw = w_from_z_proj()
    add = lambda *a, **k: cases.append(ClipCase(*a, **{"view_proj": pw, **k}))  # noqa: E731
    for k in range(3):
        ws = [OUT] * 3
        ws[k] = IN
        add(f"lone_in_vertex_{k}", [poly([crossing(ws)])], stats=dict(triangles=1, clip_skipped=0, back_facing=0, no_coverage=0),
            clip=_drawn(one_in=1), what=f"vertex {k} is the only one behind the near plane: one piece")
        ws = [IN] * 3
        ws[k] = OUT
        add(f"lone_out_vertex_{k}", [poly([crossing(ws)])], stats=dict(triangles=1, clip_skipped=0, back_facing=0, no_coverage=0),
            clip=_drawn(one_out=1), what=f"vertex {k} is the only one in front of the near plane: two pieces")
    a, b, c, d = (-0.04, -0.04, IN), (0.04, -0.04, IN), (0.03, 0.03, OUT), (-0.03, 0.03, OUT)
    add("shared_crossing_edge", [poly([(a, b, c), (a, c, d)])], cull_none=True, stats=dict(triangles=2, clip_skipped=0),
        clip=lambda e, s, vis: (e["one_in"], e["one_out"]) == (1, 1) and _watertight(e, s, vis),
        what="two triangles share the crossing edge a-c, cut from its in end both times: every sample once")
    eye = (0.0, -0.05, -0.1)
    ring = [(x, -0.05, 0.3) for x in (-0.2, -0.1, 0.0, 0.1, 0.2)]
    add("fan_around_a_vertex_behind_the_eye", [poly([(eye, ring[k], ring[k + 1]) for k in range(4)])], cull_none=True,
        stats=dict(triangles=4, clip_skipped=0), clip=lambda e, s, vis: e["one_out"] == 4 and _watertight(e, s, vis),
        what="a floor fan around a vertex with w < 0: eight pieces, three shared crossing edges, every sample once")
    add("all_three_out", [poly([ALL_OUT])], stats=dict(triangles=1, clip_skipped=1, fragments=0), covered_count=0,
        what="no vertex in: still clip_skipped")
    near = F(0.1)
    add("on_the_plane_others_in", [poly([crossing((near, IN, IN))])], stats=dict(triangles=1, clip_skipped=0),
        clip=_drawn(), what="z == w passes R3: the triangle is untouched")
    add("on_the_plane_another_out", [poly([crossing((IN, near, OUT))]), poly([crossing((near, OUT, OUT))])],
        stats=dict(triangles=2, clip_skipped=0, no_coverage=1),
        clip=lambda e, s, vis: (e["one_in"], e["one_out"]) == (1, 1) and s["fragments"] > 0,
        what="t = 0 from a vertex on the plane: the new vertex is that vertex; with two out the piece has no area")
    nearer = np.nextafter(F(0.1), F(0))
    add("z_above_w_by_one_ulp_clipped", [poly([crossing((near, near, nearer), ((-0.01, -0.01), (0.01, -0.01), (-0.01, 0.01)))]),
                                         poly([crossing((IN, IN, nearer))])],
        stats=dict(triangles=2, clip_skipped=0, no_coverage=1), clip=lambda e, s, vis: e["one_out"] == 2 and s["fragments"] > 0,
        what="z one ulp above w is out: cut at t = 0 (no area left) and at t just below 1")
    nan, inf = np.nan, np.inf
    add("nan_and_inf_stay_skipped", [poly([crossing((IN, IN, OUT)), ((nan, -0.04, IN), (0.04, -0.04, IN), (-0.04, 0.04, OUT)),
                                           ((-0.04, inf, IN), (0.04, -0.04, IN), (-0.04, 0.04, OUT)),
                                           ((-0.04, -0.04, IN), (0.04, -0.04, IN), (-0.04, 0.04, -inf))])],
        stats=dict(triangles=4, clip_skipped=3), clip=_drawn(one_out=1), what="a NaN or infinite clip coordinate: not eligible")
    add("beyond_far_beside_near_crossing", [poly([((-0.5, -0.5, 0.5), (0.5, -0.5, 1.5), (-0.5, 0.5, -0.25))])],
        view_proj=rc.IDENTITY, stats=dict(triangles=1, clip_skipped=1, fragments=0),
        what="clip = position: one vertex in, one in front of near (z > w), one with z < 0 — not eligible")
    add("den_not_positive", [poly([((0.1, 0.1, 1.0), (0.2, 0.5, 0.5), (0.3, 0.0, 0.0))])], view_proj=zw_proj(),
        stats=dict(triangles=1, clip_skipped=1, fragments=0),
        what="in vertex on the plane (b = 0) and out vertex at z = w = 0 (b = 0): den = 0, the triangle is skipped")
    add("guard_piece_other_draws", [poly([((300.0, 0.0, OUT), (0.0, -0.05, IN), (0.0, 0.05, 0.11))])], cull_none=True,
        stats=dict(triangles=1, clip_skipped=0, guard_skipped=0), clip=_drawn(one_out=1),
        what="N(b, a) leaves the guard band, N(c, a) does not: piece (b, c, Q) draws, the triangle counts as drawn")
    add("guard_piece_none_draws", [poly([((0.0, 0.0, IN), (300.0, -0.05, OUT), (300.0, 0.05, OUT))])], cull_none=True,
        stats=dict(triangles=1, clip_skipped=0, guard_skipped=1, fragments=0), covered_count=0,
        what="both new vertices leave the guard band: guard_skipped, the safe side")
    back = tuple(reversed(crossing((IN, IN, OUT))))
    add("back_facing_crossing_dropped", [poly([back])], stats=dict(triangles=1, clip_skipped=0, back_facing=1, fragments=0),
        what="the pieces keep the orientation: both back-facing, counted once")
    add("back_facing_crossing_kept", [poly([back])], cull_none=True, stats=dict(triangles=1, back_facing=0, clip_skipped=0),
        clip=_drawn(one_out=1), what="CULL_NONE draws them")
    add("lane_piece_and_wave_piece", [poly([((-0.1613, 0.01875, OUT), (-0.1105, 0.01683, 0.101), (0.16875, -0.075, 0.3))])], cull_none=True,
        stats=dict(triangles=1, clip_skipped=0), clip=lambda e, s, vis: e["both_routes"] == 1 and s["fragments"] > 0,
        what="two pieces, one with a box of at most 16 samples (clamped at the left edge), one larger")
    add("both_pieces_by_the_wave_256x144", [poly([((0.0, -0.1, -0.05), (-0.6, -0.1, 0.5), (0.6, -0.1, 0.5)),
                                                  ((0.0, 0.1, -0.05), (0.6, 0.1, 0.5), (-0.6, 0.1, 0.5))])],
        width=256, height=144, cull_none=True, stats=dict(triangles=2, clip_skipped=0),
        clip=lambda e, s, vis: e["one_out"] == 2 and e["wave_pieces"] == 4 and e["lane_pieces"] == 0
        and int((vis != 0).sum()) > 256 * 144 // 2,
        what="a floor and a ceiling through the eye's plane: four large pieces over most of the target")
    small = crossing((IN, IN, IN), ((-0.01, -0.01), (0.01, -0.01), (-0.01, 0.01)))
    add("crossing_in_the_second_chunk", [poly([small] * 64 + [crossing(w) for w in ((IN, OUT, OUT), (OUT, IN, OUT), (OUT, OUT, IN),
                                                                                   (OUT, IN, IN), (IN, OUT, IN), (IN, IN, OUT))])],
        stats=dict(triangles=70, clip_skipped=0, back_facing=0),
        clip=lambda e, s, vis: (e["one_in"], e["one_out"]) == (3, 3), what="70 triangles, the six crossing ones at index >= 64")
    add("cascade_caster_in_front_of_near", _cascade_caster, view_proj=rc._cascade_view_proj, cull_none=True,
        stats=dict(triangles=1, clip_skipped=0), clip=_drawn(one_out=1),
        what="the orthographic cascade projection (w = 1): a caster reaching z > 1 is cut, not dropped")
    # ------------------------------------------------------------------------------------------- the visibility word
    pe = exact_proj()
    t_cross = ((-0.0625, -0.0625, 0.25), (0.125, -0.0625, 0.0), (-0.0625, 0.125, 0.0))  # t = 1/2 on both edges
    t_whole = ((-0.0625, -0.0625, 0.25), (0.03125, -0.0625, 0.125), (-0.0625, 0.03125, 0.125))  # its piece, written down
    for name, tris, winner in (("tie_piece_loses_to_later_triangle", (t_cross, t_whole), 1),
                               ("tie_piece_wins_over_earlier_triangle", (t_whole, t_cross), 1)):
        add(name, [poly([tris[0]]), poly([tris[1]])], view_proj=pe, stats=dict(triangles=2, clip_skipped=0, back_facing=0),
            clip=lambda e, s, vis: e["one_in"] == 1 and s["fragments"] == 2 * int((vis != 0).sum()) > 0,
            winners=lambda won, e, s, err, k=winner: list(won) == [(k, 0)],
            what="an exact piece (w = 0 out vertices, t = 1/2) and the same triangle unclipped: equal depth, the larger id wins")
    add("pieces_carry_the_triangles_index", [poly([ALL_OUT] * 5 + [crossing((IN, OUT, IN))])], command_base=1000,
        stats=dict(triangles=6, clip_skipped=5, no_coverage=0),
        clip=lambda e, s, vis: e["one_out"] == 1 and e["lane_pieces"] + e["wave_pieces"] == 2,
        winners=lambda won, e, s, err: list(won) == [(1000, 5)] and won[(1000, 5)] == s["fragments"],
        what="both pieces of triangle 5 write t = 5 under command_base 1000")
    return cases


def all_cases():
    return build_cases()


def check_claims(case, visibility, stats, errors, extras):
    """-> list of what `case` claims and does not reach: raster_cases' claims on the high halves, the route on the
    restatement's `extras` (None: not checked), the winners on the words."""
    depth = cref.depth_of(visibility)
    base = rc.Case(**{k: getattr(case, k) for k in rc.Case.__dataclass_fields__})
    base.extra = None
    missed = rc.check_claims(base, depth, stats, errors, None)
    if case.clip is not None and extras is not None and not case.clip(extras, stats, np.asarray(visibility)):
        missed.append(f"the route it is there for was not taken: {extras}")
    if case.winners is not None:
        from raster_vis_ref import winners

        won = winners(visibility, case.command_base, len(case.meshlets))
        if not case.winners(won, extras, stats, list(errors)):
            missed.append(f"the winners are not the claimed ones: {won}")
    return missed


def census(cases=None, verbose=True):
    out = {}
    for c in all_cases() if cases is None else cases:
        vis, stats, errors, extras = restated_vis(rc.Packed(c))
        out[c.name] = check_claims(c, vis, stats, errors, extras)
        if verbose:
            line = ", ".join(f"{k}={v}" for k, v in stats.items() if v)
            print(f"{c.name:40s} {line}  {extras}  -- {c.what}" + (f"  MISSED: {out[c.name]}" if out[c.name] else ""))
    return out


if __name__ == "__main__":
    census()
