"""Inputs aimed at the compute rasteriser's WALKER (orbit_amd/csrc/raster_walk.h), the one file the device does not share
with the host mirror: the switch between the lane walk and the wave walk at 16 samples, the wave walk's 8 x 8 tiles of
the BOX, a wave-walked triangle that covers nothing, chunks of 64 triangles, the vertex loop's rounds of 64, sums that
wrap in 32 bits, the pieces form (ORBIT_RASTER_CLIP_NEAR / ORBIT_RASTER_WIDE_GUARD) on shapes that cross neither plane
nor band, and command lists for a grid capped by orbit_ctx_set_raster_grid, where one wave takes several commands and
carries its LDS vertices, its kept mvp and its counters from one to the next.

As in raster_cases, the expected bytes are never computed here: the GPU tests' reference is the host mirror, which
tests/test_raster_walk_cpu.py holds to the numpy restatements (raster_ref, raster_vis_ref, raster_clip_ref,
raster_wide_ref, as the flags need).  What a case CLAIMS — counters in closed form, how many triangles go to the lane
and how many to the wave, which ids own pixels — is checked by check_claims(): against the restatement on the CPU, so
that a case which does not take the route it is there for fails without a GPU, and against the device's output.

Targets are 64 x 48 under raster_cases.pixel_proj unless stated.  A box of exactly w x h samples at (x, y) comes from
corners at x + .25 .. x + w + .25 and y + .25 .. y + h + .25 (raster_vis_cases.tile)."""
from dataclasses import dataclass, field

import numpy as np

import raster_cases as rc
import raster_clip_cases as cc
import raster_vis_cases as vc
import raster_vis_ref as vref
import raster_wide_cases as wc
from raster_cases import LEG10, Meshlet, poly, rect
from raster_vis_cases import VisCase

F = np.float32
W, H = 64, 48
FLAG_SETS = ((False, False), (True, False), (False, True), (True, True))  # (clip_near, wide_guard)


@dataclass
class WalkCase(VisCase):
    routes: tuple = None        # (lane-walked, wave-walked) drawn triangles (pieces, under CLIP_NEAR)
    clip_near: bool = False     # the case's own flag; the pieces runs add flags to cases that have none
    pieces: bool = False        # run again under CLIP_NEAR, WIDE_GUARD and both: same bytes, same counters
    faults: dict = field(default_factory=dict)  # a capped list's range-failed commands: {position: kind}
    crossing: tuple = ()        # a capped list's commands with a triangle across the near plane


# --------------------------------------------------------------------------------------------- running a packed case
def _clip(pk, clip_near):
    return pk.case.clip_near if clip_near is None else clip_near


def host_vis(pk, clip_near=None, wide=False):
    return wc.host_vis(pk, wide=wide, clip_near=_clip(pk, clip_near))


def host_depth(pk, clip_near=None, wide=False):
    return wc.host_depth(pk, wide=wide, clip_near=_clip(pk, clip_near))


def restated_vis(pk, clip_near=None, wide=False):
    """the restatement the flags need -> (visibility, stats, errors, extras)"""
    clip_near = _clip(pk, clip_near)
    if wide:
        return wc.restated_vis(pk, wide=True, clip_near=clip_near)
    return cc.restated_vis(pk, clip_near=True) if clip_near else vc.restated(pk)


def restated_depth(pk, clip_near=None, wide=False):
    clip_near = _clip(pk, clip_near)
    if wide:
        return wc.restated_depth(pk, wide=True, clip_near=clip_near)
    return cc.restated_depth(pk, clip_near=True) if clip_near else pk.restated()


def routes_of(extras):
    """(lane-walked, wave-walked) of whichever restatement's extras"""
    if "lane_triangles" in extras:
        return extras["lane_triangles"], extras["wave_triangles"]
    return extras["lane_pieces"], extras["wave_pieces"]


# --------------------------------------------------------------------------------------------------------- geometry
def box(x, y, w, h):
    """two triangles sharing the diagonal of the w x h samples at (x, y); the box of each is the w x h samples"""
    return rect(x + 0.25, y + 0.25, x + w + 0.25, y + h + 0.25)[0]


def corner(x, y, w, h):
    """one front-facing right triangle, the right angle at the top left: its box is the w x h samples at (x, y)"""
    return ((x + 0.25, y + 0.25), (x + 0.25, y + h + 0.25), (x + w + 0.25, y + 0.25))


def corner_bottom_right(x, y, w, h):
    """the right angle at the bottom right: the first sample of the box is outside"""
    return ((x + w + 0.25, y + h + 0.25), (x + w + 0.25, y + 0.25), (x + 0.25, y + h + 0.25))


def at_depth(tris, z):
    return [tuple((p[0], p[1], z) for p in t) for t in tris]


# wave next to lane, smallest first: (1, 16) ... (4, 4) hold 16 samples (the lane), every other one more (the wave)
LADDER = ((1, 17), (1, 16), (17, 1), (16, 1), (2, 9), (2, 8), (9, 2), (8, 2), (3, 6), (4, 4), (6, 3), (7, 9), (8, 8), (9, 9),
          (15, 17), (16, 16), (17, 17), (1, 40), (40, 1))
RESIDUES = (0, 1, 7)  # of the boxes' origins modulo 8, in x and in y: the wave walk's tiles are the box's own


def pack(boxes, r):
    """First fit of `boxes` on origins = r (mod 8) in x and y, no two overlapping -> pages of (x, y, w, h), a page a target"""
    pages = [(np.zeros((H, W), bool), [])]
    for w, h in boxes:
        assert r + w <= W and r + h <= H
        for n in range(len(pages) + 1):
            if n == len(pages):
                pages.append((np.zeros((H, W), bool), []))
            taken, placed = pages[n]
            spots = [(x, y) for y in range(r, H - h + 1, 8) for x in range(r, W - w + 1, 8) if not taken[y:y + h, x:x + w].any()]
            if spots:
                x, y = spots[0]
                taken[y:y + h, x:x + w] = True
                placed.append((x, y, w, h))
                break
    return [placed for _, placed in pages]


def ladder_cases():
    """Every box of LADDER once as two triangles sharing the diagonal and once as one right triangle, at each residue
    of the origin; four boxes to a command (so lane-walked and wave-walked triangles share a chunk), each box at its
    own depth on its own pixels."""
    cases = []
    for r in RESIDUES:
        for page, placed in enumerate(pack(LADDER, r)):
            groups = [placed[k:k + 4] for k in range(0, len(placed), 4)]
            lane = sum(w * h <= 16 for _, _, w, h in placed)
            samples = sum(w * h for _, _, w, h in placed)
            depth = lambda c, k: 0.1 + 0.03 * (4 * c + k)  # noqa: E731

            def sides_sum(won, e, s, err, groups=groups, samples=samples):
                return all(won.get((c, 2 * k), 0) + won.get((c, 2 * k + 1), 0) == w * h and won.get((c, 2 * k), 0) > 0
                           and won.get((c, 2 * k + 1), 0) > 0
                           for c, g in enumerate(groups) for k, (_, _, w, h) in enumerate(g)) and sum(won.values()) == samples

            cases.append(WalkCase(
                f"ladder_rects_origin_{r}_page_{page}",
                [poly(sum((at_depth(box(*b), depth(c, k)) for k, b in enumerate(g)), [])) for c, g in enumerate(groups)],
                stats=dict(commands=len(groups), triangles=2 * len(placed), fragments=samples, no_coverage=0, back_facing=0,
                           range_errors=0),
                covered_count=samples, routes=(2 * lane, 2 * (len(placed) - lane)), winners=sides_sum, pieces=True,
                what=f"boxes {[(w, h) for _, _, w, h in placed]} at origins = {r} (mod 8), two triangles each: every sample once"))

            def all_own(won, e, s, err, groups=groups):
                return sorted(won) == [(c, k) for c, g in enumerate(groups) for k in range(len(g))]

            cases.append(WalkCase(
                f"ladder_corners_origin_{r}_page_{page}",
                [poly(sum((at_depth([corner(*b)], depth(c, k)) for k, b in enumerate(g)), [])) for c, g in enumerate(groups)],
                stats=dict(commands=len(groups), triangles=len(placed), no_coverage=0, back_facing=0, range_errors=0),
                routes=(lane, len(placed) - lane), winners=all_own, pieces=True,
                what="the same boxes as one right triangle each"))
    return cases


SPECIAL = (0, 63, 64, 127, 128, 191, 192, 255)  # the first and last lane of each chunk of 64
TILES = [vc.tile(4 * k, 24, 0.2)[0][j] for k in range(6) for j in range(2)]  # twelve lane-walked triangles, z = 0.2


def chunk_meshlet(nt, wave_at):
    """nt triangles from few vertices: lane-walked 4 x 4 tiles (twelve, in turn) but for the positions in `wave_at`
    {t: (x, y, z)}: wave-walked 3 x 6 right triangles at (x, y)"""
    tris = []
    for t in range(nt):
        if t in wave_at:
            x, y, z = wave_at[t]
            tris += at_depth([corner(x, y, 3, 6)], z)
        else:
            tris += at_depth([TILES[t % 12]], 0.2)
    return poly(tris)


def chunk_cases():
    cases = []
    corner_samples = 3 + 3 + 2 + 2 + 1 + 1  # of a 3 x 6 right triangle: samples (i, j) with (i + .25) / 3 + (j + .25) / 6 < 1
    for nt in (64, 65, 128, 129, 192, 256):
        special = [t for t in SPECIAL if t < nt]
        wave_at = {t: (2 + 7 * k, 2, 0.3 + 0.05 * k) for k, t in enumerate(special)}

        def named(won, e, s, err, special=special):
            return [t for (c, t), n in sorted(won.items()) if n == corner_samples and c == 0] == special and all(
                n in (6, 10) for (_, t), n in won.items() if t not in special)  # (a tile's two triangles own 10 and 6)

        cases.append(WalkCase(f"chunks_nt_{nt}", [chunk_meshlet(nt, wave_at)],
                              stats=dict(commands=1, triangles=nt, no_coverage=0, back_facing=0, range_errors=0),
                              routes=(nt - len(special), len(special)), winners=named, pieces=True,
                              what=f"{nt} triangles in one command; the ones at {special} go to the wave, alone on their pixels"))
    cases.append(WalkCase("chunk_tie_at_70_and_71", [chunk_meshlet(72, {70: (30, 2, 0.4), 71: (30, 2, 0.4)})],
                          stats=dict(triangles=72, no_coverage=0, range_errors=0), routes=(70, 2),
                          winners=lambda won, e, s, err: won.get((0, 71)) == corner_samples and (0, 70) not in won,
                          what="two wave-walked triangles of the second chunk on the same samples at the same depth: the larger id owns them"))
    return cases


def vertex_meshlet(vcount, x, y):
    """vcount vertices of which vertex 0 and the last two form LEG10 moved to (x, y); the rest lie on a line"""
    pos = np.stack([1 + np.arange(vcount) % 60, np.full(vcount, 40.0), np.full(vcount, 0.5)], axis=1).astype(F)
    tri = np.array(LEG10, F) + F([x - 4, y - 4])
    pos[0, :2], pos[-2, :2], pos[-1, :2] = tri[0], tri[1], tri[2]
    corners = [[0, vcount - 2, vcount - 1]] + ([[1, vcount // 2, vcount - 3]] if vcount > 4 else [])  # (collinear: no coverage)
    return Meshlet(pos, np.array(corners, np.uint8))


def vertex_count_cases():
    cases = []
    counts = (63, 64, 65, 128, 255)
    cases.append(WalkCase("vertex_counts", [Meshlet(np.array([[5, 30, 0.5]], F), np.array([[0, 0, 0]], np.uint8))]
                          + [vertex_meshlet(n, 2 + 12 * k, 2) for k, n in enumerate(counts)],
                          stats=dict(commands=6, triangles=11, no_coverage=6, fragments=45 * 5, range_errors=0), covered_count=45 * 5,
                          winners=lambda won, e, s, err: won == {(k + 1, 0): 45 for k in range(5)},
                          what="vcount = 1, 63, 64, 65, 128, 255: the covering triangle uses the first and the last two vertices"))
    cases.append(WalkCase("no_triangles", [poly([LEG10]), Meshlet(np.array([[5, 5, 0.5]] * 3, F), np.zeros((0, 3), np.uint8)),
                                           Meshlet(np.array([[5, 5, 0.5]] * 3, F), np.zeros((0, 3), np.uint8))],
                          stats=dict(commands=3, triangles=1, range_errors=0, fragments=45), covered_count=45,
                          winners=lambda won, e, s, err: err == [0, 0, 0] and won == {(0, 0): 45},
                          what="nt = 0, in the middle of the data and as its last words: a valid command that draws nothing"))
    for n in (4, 5):
        def more_indices(p, n=n):
            p.commands[1]["cmd_index_count"] = n
        cases.append(WalkCase(f"index_count_{n}", [poly([LEG10]), poly([((34, 4), (34, 14), (44, 4))]), poly([((4, 24), (4, 34), (14, 24))])],
                              mutate=more_indices, stats=dict(commands=3, triangles=3, fragments=135, range_errors=0), covered_count=135,
                              winners=lambda won, e, s, err: won == {(0, 0): 45, (1, 0): 45, (2, 0): 45},
                              what=f"index_count = {n}: one triangle, the remainder is ignored"))
    return cases


# -------------------------------------------------------------------------- R9 faults, written into command k of a list
def _vcount(p, k):
    return int(p.commands[k]["cmd_first_index"]) // 4 - int(p.commands[k]["cmd_vertex_offset"])


def _corner_bytes_beyond(p, k):
    nv = _vcount(p, k)
    p.commands[k]["cmd_first_index"] = p.meshlet_data_words * 4
    p.commands[k]["cmd_vertex_offset"] = p.meshlet_data_words - nv


def _index_words_beyond(p, k):
    nv = _vcount(p, k)
    p.commands[k]["cmd_first_index"] = (p.meshlet_data_words + 1) * 4
    p.commands[k]["cmd_vertex_offset"] = p.meshlet_data_words + 1 - nv
    p.commands[k]["cmd_index_count"] = 0


def _first_below_offset(p, k):
    p.commands[k]["cmd_vertex_offset"] = int(p.commands[k]["cmd_first_index"]) // 4 + 1


def _negative_offset(p, k):
    p.commands[k]["cmd_vertex_offset"] = -1


def _vcount_256(p, k):  # (the data in front is padded so that 256 index words are in range)
    pad = 256
    p.meshlet_data = np.concatenate([np.zeros(pad, np.uint32), p.meshlet_data])
    p.meshlet_data_words += pad
    for c in p.commands:
        c["cmd_first_index"] += 4 * pad
        c["cmd_vertex_offset"] += pad
    p.commands[k]["cmd_vertex_offset"] = int(p.commands[k]["cmd_first_index"]) // 4 - 256


def _corner_is_vcount(p, k):
    p.meshlet_data.view(np.uint8)[int(p.commands[k]["cmd_first_index"]) + 2] = _vcount(p, k)


def _vertex_word(p, k):  # the command's LAST index word: the lanes in front of it have written their vertices to LDS
    last = int(p.commands[k]["cmd_vertex_offset"]) + _vcount(p, k) - 1
    p.meshlet_data[last] = p.vertex_count - int(p.commands[k]["meshlet_vertex_offset"])


def _entity(p, k):
    p.commands[k]["cmd_first_instance"] = p.entity_count


def _wrapping_sum(p, k):
    """meshlet_vertex_offset + word = 2^32 + a valid vertex: R9 compares the SUM with vertex_count"""
    first = int(p.commands[k]["meshlet_vertex_offset"])
    assert first > 0
    word = int(p.commands[k]["cmd_vertex_offset"])
    valid = first + int(p.meshlet_data[word])
    p.meshlet_data[word] = (1 << 32) + valid - first - first
    assert first + int(p.meshlet_data[word]) == (1 << 32) + valid - first and valid - first < p.vertex_count


def _stale_corners(p, k):
    """a second triangle of corners (200, 201, 202) in a command of fewer vertices: in range of a 255-vertex command's"""
    first = int(p.commands[k]["cmd_first_index"])
    assert int(p.commands[k]["cmd_index_count"]) == 6 and _vcount(p, k) < 200
    p.meshlet_data.view(np.uint8)[first + 3:first + 6] = (200, 201, 202)


FAULTS = dict(corner_bytes_beyond_data=_corner_bytes_beyond, index_words_beyond_data=_index_words_beyond,
              first_index_below_offset=_first_below_offset, negative_vertex_offset=_negative_offset, vcount_256=_vcount_256,
              corner_is_vcount=_corner_is_vcount, vertex_word=_vertex_word, entity_is_entity_count=_entity,
              wrapping_sum=_wrapping_sum, stale_corners=_stale_corners)
R9_WAYS = tuple(k for k in FAULTS if k not in ("wrapping_sum", "stale_corners"))  # the ways of raster_cases.py


def write_faults(faults):
    def mutate(p):
        for k, kind in sorted(faults.items(), key=lambda kv: kv[1] != "vcount_256"):  # (the one that moves the data goes first)
            if kind in FAULTS:
                FAULTS[kind](p, k)
    return mutate


def wrap_cases():
    return [WalkCase("r9_wrapping_sum", [poly([LEG10]), poly([((34, 4), (34, 14), (44, 4))]), poly([((4, 24), (4, 34), (14, 24))])],
                     mutate=write_faults({1: "wrapping_sum"}), faults={1: "wrapping_sum"},
                     stats=dict(commands=3, range_errors=1, triangles=2, fragments=90), covered_count=90, covered=[(5, 5), (5, 25)],
                     uncovered=[(35, 5)], winners=lambda won, e, s, err: err == [0, 1, 0] and won == {(0, 0): 45, (2, 0): 45},
                     what="meshlet_vertex_offset + index word >= 2^32 with low 32 bits that name a valid vertex: out of range (R9)")]


def walker_cases():
    cases = ladder_cases()
    add = lambda *a, **k: cases.append(WalkCase(*a, **k))  # noqa: E731
    for n in (8, 16):
        add(f"lane_0_owns_nothing_{n}x{n}", [poly(vc.tile(40, 40, 0.3)[0] + [corner_bottom_right(9, 9, n, n)])],
            stats=dict(triangles=3, no_coverage=0, back_facing=0), routes=(2, 1), uncovered=[(9, 9)], covered=[(8 + n, 8 + n)],
            winners=lambda won, e, s, err: won.get((0, 2), 0) > n, pieces=True,
            what="the right angle at the bottom right: the box's first sample, lane 0's, is outside; the triangle covers")
    sliver = ((10.0, 10.5), (16.0, 16.5), (16.04, 16.5))
    add("empty_sliver_by_the_wave", [poly([sliver])], cull_none=True, stats=dict(triangles=1, no_coverage=1, fragments=0, back_facing=0),
        routes=(0, 1), covered_count=0, pieces=True,
        what="a sliver along the diagonal y = x + 1/2, between the centres: a box of 42 samples, none inside")
    add("empty_sliver_beside_a_covering_triangle", [poly(vc.tile(40, 40, 0.3)[0] + [sliver, corner(20, 20, 9, 9), sliver])], cull_none=True,
        stats=dict(triangles=5, no_coverage=2, back_facing=0), routes=(2, 3), pieces=True,
        winners=lambda won, e, s, err: sorted(won) == [(0, 0), (0, 1), (0, 3)],
        what="the sliver in front of and behind a covering wave-walked triangle, in one chunk")
    add("wave_walked_depth_not_positive", [poly(at_depth(box(9, 9, 9, 9), 0.0) + at_depth([corner(30, 9, 9, 9)], 0.5))],
        stats=dict(triangles=3, no_coverage=0, fragments=45), routes=(0, 3), covered_count=45, uncovered=[(9, 9), (13, 13)], pieces=True,
        what="a 9 x 9 box at d = 0: its inside samples count as covered and are no fragments")
    cases += chunk_cases() + vertex_count_cases() + wrap_cases()
    # -- a clip case of its own: a lane with two pieces, both by the wave, beside another lane's wave-walked triangle
    big, small = ((-0.1, -0.1), (0.1, -0.1), (-0.1, 0.1)), ((0.02, 0.02), (0.1, 0.02), (0.02, 0.1))
    tiny = ((-0.19, 0.17), (-0.18, 0.17), (-0.19, 0.18))
    add("two_wave_pieces_beside_a_wave_triangle",
        [poly([cc.crossing((cc.IN,) * 3, tiny), cc.crossing((cc.IN,) * 3, small), cc.crossing((cc.IN, cc.IN, cc.OUT), big)], entity=0)],
        view_proj=rc.w_from_z_proj(), clip_near=True, command_base=7,
        stats=dict(triangles=3, clip_skipped=0, back_facing=0, no_coverage=0, guard_skipped=0), routes=(1, 3),
        winners=lambda won, e, s, err: {k for k in won} >= {(7, 1), (7, 2)} and sum(won.values()) > 64,
        what="triangle 2 has one vertex in front of the near plane: two pieces, both wave-walked, both write t = 2, counted once")
    return cases


# ------------------------------------------------------------------------------------------- lists for a capped grid
WAVES = 4  # of a workgroup


def cell(i):
    return 5 * (i % 12), 7 * (i // 12)


def small(i):
    """command i of a list: on its own pixels at its own depth; even i two lane-walked triangles, odd i two wave-walked"""
    x, y = cell(i)
    z = 0.1 + 0.02 * i
    return poly(at_depth(box(x, y, 4, 4) if i % 2 == 0 else box(x, y, 3, 6), z))


def with_255_vertices(i):
    """command i with 255 vertices: 0, 253, 254 and 200, 201, 202 are two covering triangles in its cell"""
    x, y = cell(i)
    pos = np.stack([x + 1 + np.arange(255) % 3, np.full(255, y + 6.5), np.full(255, 0.1 + 0.02 * i)], axis=1).astype(F)
    a, b = np.array(corner(x, y, 4, 4), F), np.array(corner_bottom_right(x, y, 4, 4), F)
    pos[[0, 253, 254], :2], pos[[200, 201, 202], :2] = a, b
    return Meshlet(pos, np.array([[0, 253, 254], [200, 201, 202]], np.uint8))


def with_3_vertices(i):
    """command i with three vertices: the same lane-walked triangle twice"""
    x, y = cell(i)
    return poly(at_depth([corner(x, y, 4, 4)] * 2, 0.1 + 0.02 * i))


def with_257_triangles(i):
    m = small(i)
    return Meshlet(m.positions, np.concatenate([m.corners] * 128 + [m.corners[:1]]))


def assignment(count, cap):
    """-> per wave of a grid of `cap` workgroups the commands it takes, in order: wave k takes k, k + 4 cap, ..."""
    waves = WAVES * cap
    return [list(range(k, count, waves)) for k in range(waves)]


def grid_list(name, n, faults=None, special=None, **kw):
    faults = faults or {}
    special = special or {}
    meshlets = [special[i](i) if i in special else small(i) for i in range(n)]
    assert all(len(meshlets[i].corners) == 257 for i, v in faults.items() if v == "nt_257")  # (no mutation: the meshlet's own)
    return WalkCase(name, meshlets, mutate=write_faults(faults), faults=faults, **kw)


def crossing_list(n):
    """n commands of three entities with different model matrices, each with a triangle across the near plane"""
    def model(sx, tx, ty):
        m = np.eye(4, dtype=F)
        m[0, 0], m[1, 1], m[0, 3], m[1, 3] = sx, sx, tx, ty
        return m.T.reshape(16).copy()
    entities = [model(1.0, 0.0, 0.0), model(0.5, 0.06, -0.03), model(0.75, -0.05, 0.04)]
    ws = ((cc.IN, cc.IN, cc.OUT), (cc.IN, cc.OUT, cc.OUT), (cc.OUT, cc.IN, cc.IN))
    meshlets = [poly([cc.crossing(ws[i % 3], tuple((x + 0.01 * (i // 3), y) for x, y in cc.BASE))], entity=i % 3) for i in range(n)]
    return WalkCase(f"grid_crossing_{n}", meshlets, view_proj=rc.w_from_z_proj(), entities=entities, clip_near=True,
                    crossing=tuple(range(n)), stats=dict(commands=n, triangles=n, clip_skipped=0, range_errors=0),
                    what="every command of another entity than the one before it in its wave, each cut at the near plane")


def grid_lists():
    lists = [grid_list(f"grid_{n}", n, stats=dict(commands=n, triangles=2 * n, range_errors=0, fragments=n // 2 * 18 + (n + 1) // 2 * 16),
                       what=f"{n} small commands") for n in (1, 2, 3, 4, 5, 8)]
    # wave 0 of one workgroup takes 0, 4, 8: good, range-failed, good — one list per way
    for kind in R9_WAYS + ("wrapping_sum",):
        lists.append(grid_list(f"grid_9_{kind}", 9, {4: kind}, stats=dict(commands=9, range_errors=1),
                               what=f"command 4 fails its ranges ({kind}) between two good ones of its wave"))
    lists.append(grid_list("grid_9_nt_257", 9, {4: "nt_257"}, {4: with_257_triangles}, stats=dict(commands=9),
                           what="command 4 has 257 triangles: a range error of the visibility call, drawn by the depth call"))
    # of two workgroups wave 0 takes 0, 8, 16, 24, 32, wave 1 takes 1, 9, 17, 25, ...
    lists.append(grid_list("grid_33_mixed", 33, {8: "vertex_word", 9: "corner_is_vcount", 10: "nt_257", 11: "entity_is_entity_count",
                                                 12: "wrapping_sum", 13: "vcount_256", 14: "corner_bytes_beyond_data",
                                                 15: "index_words_beyond_data", 24: "first_index_below_offset"},
                           {10: with_257_triangles}, stats=dict(commands=33),
                           what="every way to fail between good commands of a wave under a cap of two workgroups (and of one)"))
    lists.append(grid_list("grid_9_large_then_small", 9, {4: "stale_corners", 8: "stale_corners"},
                           {0: with_255_vertices, 4: with_3_vertices, 8: with_3_vertices}, stats=dict(commands=9, range_errors=2),
                           what="a 255-vertex command, then in the same wave 3-vertex commands whose corners 200, 201, 202 name the "
                                "first one's vertices: range errors that draw nothing"))
    lists += [crossing_list(5), crossing_list(9)]
    lists.append(grid_list("grid_9_clamped_at_6", 9, count=1000, max_commands=6, stats=dict(commands=6, triangles=12, range_errors=0),
                           what="listed 1000 > max_commands 6: of one workgroup waves 0 and 1 take a second command, waves 2 and 3 do not"))
    lists.append(grid_list("grid_33_clamped_at_11", 33, count=34, max_commands=11, stats=dict(commands=11, triangles=22, range_errors=0),
                           what="the same for two workgroups: the clamp falls between waves 2 and 3 of the second round"))
    ways = ("vertex_word", "corner_is_vcount", "entity_is_entity_count", "negative_vertex_offset", "wrapping_sum")
    lists.append(grid_list("grid_9_all_failed", 9, {k: ways[k % 5] for k in range(9)},
                           stats=dict(commands=9, triangles=0, fragments=0, range_errors=9), covered_count=0,
                           what="every command fails its ranges: nothing is drawn, nothing is counted but commands and errors"))
    return lists


CAPS = (1, 2, 0)  # workgroups; 0 = the resident grid
ARRANGEMENTS = ("a", "c", "d", "e", "f") + tuple(f"b:{k}" for k in R9_WAYS + ("nt_257", "wrapping_sum"))
# (33 commands hold nine commands with good neighbours eight in front and behind: this one way is left to one workgroup)
NOT_UNDER_TWO_WORKGROUPS = ("b:negative_vertex_offset",)


def arrangements(pk, errors, cap):
    """What the host-side assignment of `pk`'s list to the waves of `cap` workgroups holds, of ARRANGEMENTS:
      a  a wave without a command beside waves with one
      b:<kind>  one wave takes a good, a range-failed (<kind>) and a good command, in this order, one after the other
      c  one wave takes a good 255-vertex command and later a command of fewer vertices with a corner that would be in
         range of the first, with no larger command in between
      d  one wave takes, one after the other, two commands of entities with different model matrices, each with a
         triangle across the near plane, under CLIP_NEAR
      e  listed > max_commands and the clamp falls inside a round after the first: some waves take a command in it,
         others do not
      f  every command fails its ranges, and a wave takes two of them
    `errors`: the mirror's command_error of the call."""
    case = pk.case
    listed = int(pk.words[0])
    count = min(listed, pk.max_commands)
    errors = [int(e) for e in errors]
    assert len(errors) == count
    waves = assignment(count, cap)
    found = set()
    if any(not w for w in waves) and any(w for w in waves):
        found.add("a")
    if listed > pk.max_commands and count > len(waves) and count % len(waves) != 0:
        found.add("e")
    if count and all(errors) and any(len(w) > 1 for w in waves):
        found.add("f")
    data_bytes = pk.meshlet_data.view(np.uint8)
    for w in waves:
        for a, b, c in zip(w, w[1:], w[2:]):
            if (errors[a], errors[b], errors[c]) == (0, 1, 0) and b in case.faults:
                found.add(f"b:{case.faults[b]}")
        for a, b in zip(w, w[1:]):
            if (case.clip_near and a in case.crossing and b in case.crossing and not errors[a] and not errors[b]
                    and pk.entities[int(pk.commands[a]["cmd_first_instance"])]["model_matrix"].tobytes()
                    != pk.entities[int(pk.commands[b]["cmd_first_instance"])]["model_matrix"].tobytes()):
                found.add("d")
        held = 0  # vertices of the wave's LDS that a good command has written
        for k in w:
            first, nt = int(pk.commands[k]["cmd_first_index"]), int(pk.commands[k]["cmd_index_count"]) // 3
            nv = _vcount(pk, k)
            if case.faults.get(k) == "stale_corners":
                top = int(data_bytes[first:first + 3 * nt].max())
                if held == 255 and nv <= top < held and errors[k]:
                    found.add("c")
            elif not errors[k]:
                held = max(held, nv)
    return found


def all_cases():
    return walker_cases()


PIECES_CASES = [c.name for c in walker_cases() if c.pieces]


def check_claims(case, visibility, stats, errors, extras=None):
    """-> list of what `case` claims and does not reach: raster_cases' claims on the high halves, the winners on the
    words, and — with a restatement's extras — the triangles that went to the lane and to the wave."""
    depth = (np.asarray(visibility, np.uint64) >> np.uint64(32)).astype(np.uint32).view(F)
    base = rc.Case(**{k: getattr(case, k) for k in rc.Case.__dataclass_fields__})
    base.extra = None
    missed = rc.check_claims(base, depth, stats, errors, None)
    if case.routes is not None and extras is not None and tuple(routes_of(extras)) != tuple(case.routes):
        missed.append(f"lane / wave = {routes_of(extras)}, claimed {case.routes}")
    if case.winners is not None:
        won = vref.winners(visibility, case.command_base, len(case.meshlets))
        if not case.winners(won, extras, stats, list(errors)):
            missed.append(f"the winners are not the claimed ones: {won}")
    return missed


def census(cases=None, verbose=True):
    out = {}
    for c in (walker_cases() + grid_lists()) if cases is None else cases:
        vis, stats, errors, extras = restated_vis(rc.Packed(c))
        out[c.name] = check_claims(c, vis, stats, errors, extras)
        if verbose:
            line = ", ".join(f"{k}={v}" for k, v in stats.items() if v)
            print(f"{c.name:42s} {line}  lane/wave={routes_of(extras)}  -- {c.what}" + (f"  MISSED: {out[c.name]}" if out[c.name] else ""))
    return out


if __name__ == "__main__":
    census()
