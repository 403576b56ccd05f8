"""Inputs for orbit_raster_visibility and orbit_visibility_resolve (include/orbit_abi_ext.h V1-V4): the census of
tests/raster_cases.py at command_base 0, and the smallest inputs at which what the visibility call ADDS can go wrong —
ties, the 8 bits of the triangle index, the 24 bits of the command id, two lists in one buffer, the lane and the wave
walk losing to each other — plus buffers for the resolve built directly, without the rasteriser.  As in raster_cases,
the expected bytes are never computed here: the GPU tests' reference is the host mirror
(orbit_amd.raster.host_raster_visibility / host_visibility_resolve), which tests/test_raster_visibility_cpu.py holds to
the numpy restatement tests/raster_vis_ref.py; what a case CLAIMS is checked against the restatement by census()."""
from dataclasses import dataclass

import numpy as np

import raster_cases as rc
import raster_vis_ref as vref
from raster_cases import LEG10, Meshlet, poly, rect, strip_255

F = np.float32


@dataclass
class VisCase(rc.Case):
    command_base: int = 0
    winners: object = None  # f(won: {(command, triangle): pixels}, extras, stats, errors) -> bool: what the ids must show


def host(pk, visibility=None, clear=True, command_base=None):
    """the host mirror on a packed case -> (visibility (h, w) uint64, stats row, command_error)"""
    from orbit_amd import raster

    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    base = getattr(pk.case, "command_base", 0) if command_base is None else command_base
    return raster.host_raster_visibility(words, mc, data, vb, vc, ent, vp, w, h, visibility=visibility, command_base=base,
                                         clear=clear, cull_none=pk.case.cull_none, **kw)


def restated(pk, visibility=None, clear=True, command_base=None):
    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    base = getattr(pk.case, "command_base", 0) if command_base is None else command_base
    return vref.raster(words, mc, data, vb, vc, ent, vp, w, h, visibility=visibility, command_base=base,
                       flags=pk.flags | (vref.CLEAR if clear else 0), **kw)


def strip_256():
    """strip_255's 255 vertices with one triangle more: triangle 255 repeats triangle 2 (255 % 253), so wherever
    triangle 2 is seen, the tie goes to index 255 — the top value of the low byte."""
    m = strip_255()
    j = 255 % 253
    return Meshlet(m.positions, np.concatenate([m.corners, np.array([[j, j + 1, j + 2]], np.uint8)]))


def strip_257():
    m = strip_256()
    return Meshlet(m.positions, np.concatenate([m.corners, m.corners[:1]]))


# lane-path tiles: a rectangle from x.25 to (x + 4).25 holds exactly the 4 x 4 samples x.5 .. (x + 3).5, and so does
# the box of each of its two triangles (16 samples: the lane walk)
def tile(x, y, z):
    return rect(x + 0.25, y + 0.25, x + 4.25, y + 4.25)[0], z


def new_cases():
    cases = []
    add = lambda *a, **k: cases.append(VisCase(*a, **k))  # noqa: E731
    add("tie_between_commands", [poly([LEG10]), poly([LEG10]), poly([LEG10])], stats=dict(triangles=3, fragments=135),
        covered_count=45, winners=lambda won, e, s, err: won == {(2, 0): 45},
        what="the same triangle in three commands: equal depth everywhere, the largest command id owns every pixel")
    add("tie_inside_a_command", [poly([LEG10, LEG10, ((34, 4), (34, 14), (44, 4))])], stats=dict(triangles=3, fragments=135),
        covered_count=90, winners=lambda won, e, s, err: won == {(0, 1): 45, (0, 2): 45},
        what="the same triangle twice inside one command: the larger triangle index wins")
    add("nt_256", [strip_256()], stats=dict(triangles=256, range_errors=0, back_facing=0),
        winners=lambda won, e, s, err: won.get((0, 255), 0) > 0 and (0, 2) not in won and err == [0],
        what="256 triangles from 255 vertices: index 255 survives in the low byte and takes triangle 2's pixels")
    add("nt_257_between_neighbours", [poly([LEG10]), strip_257(), poly([((4, 24), (4, 34), (14, 24))])],
        stats=dict(commands=3, range_errors=1, triangles=2, fragments=90), covered_count=90, covered=[(5, 5), (5, 25)],
        winners=lambda won, e, s, err: err == [0, 1, 0] and won == {(0, 0): 45, (2, 0): 45},
        what="257 triangles do not fit the low byte: the command is skipped whole, the ones around it are drawn")
    n = 3
    top = vref.MAX_COMMANDS - n
    add("command_base_top_of_24_bits", [poly([LEG10]), poly([((34, 4), (34, 14), (44, 4))]), poly([((4, 24), (4, 34), (14, 24))])],
        command_base=top, stats=dict(triangles=3, fragments=135), covered_count=135,
        winners=lambda won, e, s, err: won == {(top, 0): 45, (top + 1, 0): 45, (top + 2, 0): 45},
        what="command_base = 2^24 - n: ids up to 2^24 - 1, the top bit of the 24")
    # a wave-path triangle (box 7 x 4 = 28 samples, 12 inside) wholly behind two lane-path tiles, in the last command
    wave_tri = ((8.5, 8.5), (8.5, 11.5), (14.5, 8.5))
    add("wave_path_loses_to_lane_path", [poly(tile(8, 8, 0.6)[0] + tile(12, 8, 0.6)[0], z=0.6), poly([wave_tri], z=0.3)],
        stats=dict(triangles=5, no_coverage=0), covered_count=32,
        winners=lambda won, e, s, err: (e["lane_triangles"], e["wave_triangles"]) == (4, 1) and s["fragments"] > 32
        and sum(won.values()) == 32 and all(c == 0 for c, _ in won),
        what="a triangle walked by the wave writes fragments and keeps none: lane-walked triangles are in front of all")
    add("lane_path_loses_to_wave_path", [poly(rect(4.5, 4.5, 20.5, 20.5)[0], z=0.6), poly(tile(8, 8, 0.3)[0], z=0.3)],
        stats=dict(triangles=4, fragments=256 + 16), covered_count=256,
        winners=lambda won, e, s, err: (e["lane_triangles"], e["wave_triangles"]) == (2, 2) and sum(won.values()) == 256
        and all(c == 0 for c, _ in won),
        what="the reverse: lane-walked triangles wholly behind wave-walked ones keep no pixel")
    return cases


def census_as_vis_cases():
    return [VisCase(**{k: getattr(c, k) for k in rc.Case.__dataclass_fields__}) for c in rc.all_cases()]


def all_cases():
    return census_as_vis_cases() + new_cases()


def check_claims(case, visibility, stats, errors, extras):
    """-> list of what `case` claims and does not reach; the depth claims of raster_cases on the high halves."""
    depth = (np.asarray(visibility, np.uint64) >> np.uint64(32)).astype(np.uint32).view(F)
    base = rc.Case(**{k: getattr(case, k) for k in rc.Case.__dataclass_fields__})
    base.extra = None  # (the census' `extra` reads the depth restatement's extras; tests/test_raster_depth_cpu.py holds it)
    missed = rc.check_claims(base, depth, stats, errors, None)
    if case.winners is not None and not case.winners(extras["won"], extras, stats, list(errors)):
        missed.append(f"the winners are not the claimed ones: {extras['won']}")
    return missed


def census(cases=None, verbose=True):
    out = {}
    for c in new_cases() if cases is None else cases:
        vis, stats, errors, extras = restated(rc.Packed(c))
        out[c.name] = check_claims(c, vis, stats, errors, extras)
        if verbose:
            line = ", ".join(f"{k}={v}" for k, v in stats.items() if v)
            print(f"{c.name:32s} {line}  lane/wave={extras['lane_triangles']}/{extras['wave_triangles']}  -- {c.what}"
                  + (f"  MISSED: {out[c.name]}" if out[c.name] else ""))
    return out


# -------------------------------------------------------------------------------------- two lists in one buffer
def two_lists():
    """List A (CLEAR, base 0) and list B (merged, base = A's capacity) overlap: B is nearer where they do.
    -> (case A, case B, cap)"""
    a = VisCase("list_a", [poly(rect(8.5, 8.5, 24.5, 24.5)[0], z=0.5), poly([((40, 30), (40, 40), (50, 30))], z=0.7)], what="the early list")
    b = VisCase("list_b", [poly(rect(16.5, 16.5, 32.5, 32.5)[0], z=0.6), poly([((40, 4), (40, 14), (50, 4))], z=0.2)],
                what="the late list")
    cap = 4  # A's capacity: more than A holds, so B's ids start behind a gap
    b.command_base = cap
    return a, b, cap


# -------------------------------------------------------------------------------------- buffers for the resolve
RESOLVE_SIZES = ((1, 1), (7, 5), (64, 1), (65, 9), (320, 180))


def _word(depth, command, triangle):
    return (np.asarray(depth, F).view(np.uint32).astype(np.uint64) << np.uint64(32)
            | (np.asarray(command, np.uint64) << np.uint64(8)) | np.asarray(triangle, np.uint64))


def resolve_buffers():
    """-> [(name, visibility (h, w) uint64, command_base, max_commands)]: partial 8 x 8 tiles on both edges, one command
    for a whole wave, 64 distinct commands in a wave, nothing covered, nothing owned, and ids on and next to both ends."""
    out = []
    for w, h in RESOLVE_SIZES:
        n = w * h
        p = np.arange(n, dtype=np.int64)
        depth = (F(0.25) + (p % 7).astype(F) / F(16)).astype(F)
        tri = (p % 256).astype(np.uint64)
        shape = lambda a: a.reshape(h, w)  # noqa: E731
        out.append((f"one_command_{w}x{h}", shape(_word(depth, np.full(n, 9), tri)), 5, 8))
        out.append((f"all_distinct_{w}x{h}", shape(_word(depth, 100 + p, tri)), 100, n))
        out.append((f"uncovered_{w}x{h}", np.zeros((h, w), np.uint64), 0, 16))
        out.append((f"all_foreign_{w}x{h}", shape(_word(depth, 40 + p % 5, tri)), 64, 32))
        base, count = 1000, 50  # ids base - 1, base, base + count - 1, base + count in turn, some pixels uncovered
        ids = np.array([base - 1, base, base + count - 1, base + count])[p % 4]
        words = _word(depth, ids, tri)
        words[p % 5 == 3] = 0
        out.append((f"range_ends_{w}x{h}", shape(words), base, count))
    w, h = 65, 9
    p = np.arange(w * h, dtype=np.int64)
    out.append(("top_of_24_bits", _word(np.full(w * h, 1.0, F), vref.MAX_COMMANDS - 1 - p % 3, 255).reshape(h, w),
                vref.MAX_COMMANDS - 2, 2))
    out.append(("no_commands", _word(np.full(w * h, 0.5, F), p % 3, 0).reshape(h, w), 1, 0))
    return out


if __name__ == "__main__":
    census()
