"""Inputs that make the two later readers of a finished visibility buffer — orbit_visibility_surface_drawn (read with raster
flags) and orbit_surface_fragments — run their tile loop MORE THAN ONCE per wave, with something else in every trip
(DESIGN.md §4.22): visibility_tile_cases' tile programme a second time, with the kinds that only a buffer drawn with
ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD (flags 40) holds.  As in the sibling case files the expected bytes are
never computed here: the GPU tests' reference is the host mirror (orbit_amd.raster.host_visibility_surface_drawn,
host_surface_fragments), which tests/test_surface_tiles_cpu.py holds to the numpy restatements; a programme states only
counters known in closed form (`expect`).

A target is cut into 8 x 8 pixel tiles, tile = ty * tiles_x + tx, and every tile is given a KIND.  Those of
visibility_tile_cases that are kept: E (empty), O (one key on all 64 pixels), K (64 keys), F (foreign ids, by hand),
Px (the partial column: a single-pixel triangle per pixel), Py (the partial row: the entity whose w is 2^-100, every
pixel degenerate).  New, with a key that has candidates (SLOW: surface_triangle_drawn makes records for it):
  C1    one key on all 64 pixels, a one-in cut: one piece, count == 1
  C2    one key, a one-out cut whose quad is the tile: the two pieces' diagonal crosses it, pixels of candidate 0 and of 1
  C2a   one key, a one-out cut of which only piece 0 reaches the tile: count == 2 and nobody needs candidate 1
  Wd    one key, a wide triangle: a sliver over the tile to a vertex 2^24 sub-pixels to its left
  KS    64 single-pixel keys, every second a cut triangle and every eighth a wide one (surface_drawn_cases' 64_keys_cut_and_wide)
  K1    64 single-pixel keys, key 27 a cut triangle: 63 fast keys and one slow
  KA    64 single-pixel keys, every eighth a wide triangle and the others cut ones: all slow
  CPx   C2's key in the one-pixel-wide last column, CPy in the one-pixel-high last row: the other lanes are not `own`
  Sm    a small one-out cut inside the tile, and its word copied by hand to the tile's first pixel, outside both pieces:
        no candidate owns it, `miss` is stale (surface_drawn_cases' stale_moved_outside_both_pieces)
  Un    one key on all 64 pixels, a one-out cut whose piece (b, Q, P) leaves the guard band and owns the tile
        (surface_drawn_cases' cut_with_a_wide_piece).  The SAME buffer is read twice: with flags 40 the tile is written
        (cut and wide), with flags 8 the piece is not a candidate and the pixels are unsupported.  One buffer serves both
        reads: read with flags 8, the Wd tiles and the wide keys of KS and KA are unsupported as well, with a fixed verdict
and without one:
  Big   one command of 24 triangles on 72 vertices, triangles 0 and 23 over the tile's two halves: both validation loops
        of the command (vcount, 3 * nt) take a second round of 64
For the fragments reader only — the drawn reader sees an O tile —, the surface call's records tampered with afterwards:
  T     `triangle`: a vertex id = vertex_count on the upper half, the other entity's id on the lower: fragment-stale
  U     `triangle` = 0xFFFFFFFF: unshaded
  TU    rows 0-2 untouched, rows 3-4 as U, rows 5-7 as T: written, unshaded and stale lanes in one tile
  N     `bary` = NaN on the upper half, +inf on the lower: written and degenerate (F7)

Every tile's list is drawn ALONE by the host mirror's raster (raster_wide_cases.host_vis' route, flags 40, CULL_NONE,
raster_cases.w_from_z_proj, command_base = BASE moved to the tile's first command, so that the words name the commands
as the whole list does), and the tile's own pixels are taken from that buffer: the spill-to-zero tampering of
visibility_tile_cases, tile by tile.  (Depth alone cannot keep a cut triangle's spill out of its neighbours: whatever
its vertices' w, a piece reaches depth 1, the nearest there is, at its cut edge.  The fast kinds still lie at
depth_of(tile) and the C2 quad holds no sample outside its tile, so that a whole list drawn at once — the device chain,
the natural grid — keeps most of its tiles.)  Then the F
words and the Sm word are written by hand.

arrangements() works from the kinds and visibility_tile_cases.assignment alone and returns which of ARRANGEMENTS some
wave meets; RULES is its table: a name and the kinds of consecutive trips of one wave.
  slow>fast>slow  fast>slow  E>slow  F>slow      tile_slow and the records after a tile without, an empty and a foreign one
  cand1>no_cand1>cand1                            the candidate-1 ballot: non-zero, zero (C2a or C1), non-zero
  KA>O>KS                                         64 setup lanes make slow records, then 1 makes a fast one, then 64
  K1_after_no_slow                                one slow record among 63 fast ones, after a tile that made none
  partial_slow>full  CPy_last                     a slow key on 8 lanes (or 1), then all 64; CPy as the last of several
  Sm>C2  Un>C1  Wd>C2                             a stale miss, an unsupported miss (flags 8), a wide candidate, then cut ones
  Big>O>Big                                       the validation loops' second round, none, the second round
  h:idle_wave                                     a wave without a tile beside one with
  U>O  T>O  E>O  F>O  Px>O  mixed>full            (fragments) unshaded, stale, no, foreign, 8 lanes, then all 64 written
  i:drawn.<counter>  i:frag.<counter>             the counter receives a share from two trips of one wave and from two waves
                                                  (drawn.unsupported_pixels: of the read with flags 8; with 40 it stays 0)
The three targets of programmes() together hold all of them under a cap of 1 and of 2 workgroups."""
from dataclasses import dataclass, field

import numpy as np

import raster_cases as rc
import surface_drawn_cases as dc
import surface_fragments_cases as fc
import visibility_tile_cases as tc
from raster_cases import poly, w_from_z_proj
from raster_vis_cases import _word
from raster_wide_cases import WideCase
from visibility_tile_cases import BASE, CAPS, RESIDENT, TINY_W, assignment, depth_of, parse  # noqa: F401

F = np.float32
IN, OUT = dc.IN, dc.OUT
SM_W = 0.3     # the Sm cut's in vertices: behind the near plane's w = 0.1
CUT_W = 0.15   # the in vertices of the whole-tile cuts: depth 2/3, nearer than every fast tile (depth_of < 0.65)
DRAWN_COUNTERS = ("covered_pixels", "written_pixels", "foreign_pixels", "unsupported_pixels", "stale_pixels", "degenerate_pixels",
                  "cut_pixels", "wide_pixels")       # OrbitSurfaceStats
FRAG_COUNTERS = ("covered_pixels", "written_pixels", "foreign_pixels", "unshaded_pixels", "stale_pixels", "degenerate_pixels")  # OrbitFragmentStats

SLOW_FULL = ("C1", "C2", "C2a", "Wd", "KS", "K1", "KA", "Un")   # all 64 pixels owned, at least one key with candidates
SLOW = SLOW_FULL + ("Sm", "CPx", "CPy")
FAST_FULL = ("O", "K", "Big", "T", "U", "TU", "N")               # all 64 pixels owned, no key with candidates
NO_SLOW = FAST_FULL + ("E", "F", "Px", "Py")
FULL = SLOW_FULL + FAST_FULL
KINDS = SLOW + NO_SLOW

# the counters a tile of a kind gives a non-zero share to: drawn.* of the read with flags 40 (drawn.unsupported_pixels: of
# the read with flags 8), frag.* of the fragments call over the flags-40 surface
_D = ("drawn.covered_pixels", "drawn.written_pixels")
_FR = ("frag.covered_pixels", "frag.written_pixels")
_CUT, _WIDE, _UNS = ("drawn.cut_pixels",), ("drawn.wide_pixels",), ("drawn.unsupported_pixels",)
_FOREIGN = ("drawn.covered_pixels", "drawn.foreign_pixels", "frag.covered_pixels", "frag.foreign_pixels")
SHARES = {"E": (), "F": _FOREIGN, "O": _D + _FR, "K": _D + _FR, "Big": _D + _FR, "Px": _D + _FR,
          "Py": _D + _FR + ("drawn.degenerate_pixels",),
          "C1": _D + _FR + _CUT, "C2": _D + _FR + _CUT, "C2a": _D + _FR + _CUT, "CPx": _D + _FR + _CUT, "CPy": _D + _FR + _CUT,
          "K1": _D + _FR + _CUT, "Wd": _D + _FR + _WIDE + _UNS, "KS": _D + _FR + _CUT + _WIDE + _UNS, "KA": _D + _FR + _CUT + _WIDE + _UNS,
          "Un": _D + _FR + _CUT + _WIDE + _UNS, "Sm": _D + _FR + _CUT + ("drawn.stale_pixels", "frag.unshaded_pixels"),
          "T": _D + ("frag.covered_pixels", "frag.stale_pixels"), "U": _D + ("frag.covered_pixels", "frag.unshaded_pixels"),
          "TU": _D + _FR + ("frag.unshaded_pixels", "frag.stale_pixels"), "N": _D + _FR + ("frag.degenerate_pixels",)}
COUNTERS = tuple(f"drawn.{c}" for c in DRAWN_COUNTERS) + tuple(f"frag.{c}" for c in FRAG_COUNTERS)
assert set(SHARES) == set(KINDS) and {c for v in SHARES.values() for c in v} == set(COUNTERS)

# name, the kinds of consecutive trips of one wave (a tuple: any of them)
RULES = (("slow>fast>slow", ("C2", "O", "C2")), ("fast>slow", (FAST_FULL, SLOW)), ("E>slow", ("E", SLOW)), ("F>slow", ("F", SLOW)),
         ("cand1>no_cand1>cand1", ("C2", ("C2a", "C1"), "C2")), ("KA>O>KS", ("KA", "O", "KS")), ("K1_after_no_slow", (NO_SLOW, "K1")),
         ("partial_slow>full", ("CPx", FULL)), ("Sm>C2", ("Sm", "C2")), ("Un>C1", ("Un", "C1")), ("Big>O>Big", ("Big", "O", "Big")),
         ("Wd>C2", ("Wd", "C2")), ("U>O", ("U", "O")), ("T>O", ("T", "O")), ("E>O", ("E", "O")), ("F>O", ("F", "O")), ("Px>O", ("Px", "O")),
         ("mixed>full", ("TU", FULL)))
ARRANGEMENTS = tuple(n for n, _ in RULES) + ("CPy_last", "h:idle_wave") + tuple(f"i:{c}" for c in COUNTERS)


def arrangements(kinds, tiles, cap, resident=RESIDENT, rules=RULES, shares=SHARES):
    """What the assignment of `tiles` tiles of `kinds` to the waves of a grid capped at `cap` workgroups holds, of
    ARRANGEMENTS (the module's docstring); nothing is rasterised."""
    assert len(kinds) == tiles
    found = set()
    waves = assignment(tiles, cap, resident)
    if any(not w for w in waves) and any(w for w in waves):
        found.add("h:idle_wave")
    sharing = {c: set() for v in shares.values() for c in v}
    for g, w in enumerate(waves):
        seq = [kinds[t] for t in w]
        for name, pattern in rules:
            for i in range(len(seq) - len(pattern) + 1):
                if all(k == p if isinstance(p, str) else k in p for k, p in zip(seq[i:], pattern)):
                    found.add(name)
        if len(seq) > 1 and seq[-1] == "CPy":
            found.add("CPy_last")
        for c in sharing:
            trips = sum(1 for k in seq if c in shares[k])
            if trips:
                sharing[c].add((g, trips > 1))
    for c, waves_of in sharing.items():
        if len(waves_of) > 1 and any(twice for _, twice in waves_of):
            found.add(f"i:{c}")
    return found


# ------------------------------------------------------------------------------------------------ the programme
@dataclass
class Programme:
    name: str
    width: int
    height: int
    kinds: tuple
    visibility: np.ndarray = None   # (h, w) uint64: drawn tile by tile, then tampered with
    packed: object = None           # rc.Packed of the list
    surface: object = None          # dc.DrawnCase read with flags 40
    surface8: object = None         # the same buffer read with flags 8
    frag: object = None             # fc.FragCase over `surface`, T / U / TU / N tampered
    expect: dict = field(default_factory=dict)  # {"drawn", "drawn8", "frag": {counter: value}}
    stale: bool = False             # the drawn reader latches ORBIT_E_RANGE (an Sm tile)
    frag_stale: bool = False        # the fragments reader does (a T or TU tile)
    tamper_free: bool = False       # no word and no record written by hand: a device can draw and read the list itself

    @property
    def tiles(self):
        return ((self.width + 7) // 8) * ((self.height + 7) // 8)

    @property
    def max_commands(self):
        return self.packed.max_commands


def _fraction(w_in, w_out):
    """where on the screen, from the in vertex to the out one, the new vertex of an edge from clip w_in to w_out lies: the
    near plane is w = 0.1 (w_from_z_proj), R3c's t = (w_in - 0.1) / (w_in - w_out), and the screen weighs the ends by their w"""
    return (w_in - 0.1) / (w_in - w_out) * w_out / 0.1


def _cut_over(s, x0, y0):
    """a one-in cut whose piece (a, N(a, b), N(a, c)) lies over the whole tile, as visibility_tile_cases' O triangle does
    (surface_drawn_cases.cut_pixel_triangle's construction, the in vertex at CUT_W)"""
    a, nb, nc = (x0 - 0.5, y0 - 0.5), (x0 - 0.5, y0 + 17.5), (x0 + 17.5, y0 - 0.5)
    f = _fraction(CUT_W, OUT)
    far = lambda n: (a[0] + (n[0] - a[0]) / f, a[1] + (n[1] - a[1]) / f)  # noqa: E731
    return (s(*a, CUT_W), s(*far(nb), OUT), s(*far(nc), OUT))


def _cut_square(s, x0, y0):
    """a one-out cut whose quad (b, c, Q, P) is the tile and a quarter of a pixel around it, so that it holds no sample of a
    neighbouring tile: b and c a quarter below the tile's lower corners, the out vertex a 2500 pixels above at w = 0.001, the
    new vertices P = N(b, a), Q = N(c, a) a quarter above the tile (the sides lean by a hundredth of a pixel).  Piece 0 =
    (b, c, Q) is the half below the diagonal b-Q, piece 1 = (b, Q, P) the half above"""
    up = 8.5 / _fraction(CUT_W, 0.001)
    return (s(x0 + 4.0, y0 + 8.25 - up, 0.001), s(x0 - 0.25, y0 + 8.25, CUT_W), s(x0 + 8.25, y0 + 8.25, CUT_W))


def _one_out(s, cx, cy, scale, w_in=IN):
    """surface_drawn_cases.ONE_OUT, ndc (0, 0) at screen (cx, cy) and an ndc unit `scale` pixels long: the quad (b, c, Q, P) =
    (-3, -3), (3, -3), (2, 3), (-2, 3); piece 0 = (b, c, Q), piece 1 = (b, Q, P)"""
    return (s(cx, cy - 15.0 * scale, OUT), s(cx - 3.0 * scale, cy + 3.0 * scale, w_in), s(cx + 3.0 * scale, cy + 3.0 * scale, w_in))


def programme(name, width, height, kinds):
    tiles_x, tiles_y = (width + 7) // 8, (height + 7) // 8
    assert len(kinds) == tiles_x * tiles_y and width <= 80 and height <= 40 and set(kinds) <= set(KINDS), name
    s = lambda sx, sy, w: dc.on_screen(sx, sy, w, width, height)  # noqa: E731
    px = lambda x, y, w: dc.pixel_triangle(x, y, w, width, height)  # noqa: E731
    meshlets, first = [], []  # first[tile]: its first command
    for tile, kind in enumerate(kinds):
        x0, y0 = 8 * (tile % tiles_x), 8 * (tile // tiles_x)
        w = 0.1 / depth_of(tile)  # the depth is 0.1 / w
        pw, ph = min(8, width - x0), min(8, height - y0)  # the tile's pixels inside the target
        assert pw == ph == 8 or kind in ("E", "F", "Px", "Py", "CPx", "CPy", "C2"), (name, tile, kind)
        assert (kind != "CPx" or pw == 1) and (kind != "CPy" or ph == 1), (name, tile, kind)
        first.append(len(meshlets))
        add = lambda tris, entity=0: meshlets.append(poly(tris, entity=entity))  # noqa: E731
        over = (s(x0 - 0.5, y0 - 0.5, w), s(x0 - 0.5, y0 + 17.5, w), s(x0 + 17.5, y0 - 0.5, w))
        if kind in ("O", "T", "U", "TU", "N"):
            add([over])
        elif kind == "K":
            for q in range(64):
                add([px(x0 + q % 8, y0 + q // 8, w)])
        elif kind == "Px":
            add([px(x0, y0 + q, w) for q in range(ph)])
        elif kind == "Py":  # (corner 1 at the tile: the quotient that S3 divides by s is the one that overflows)
            add([(s(x0 + 30000.0, y0 + 0.25, w), s(x0 + 0.25, y0 + 0.25, w), s(x0 + 0.25, y0 + 30000.0, w))], entity=1)
        elif kind == "C1":
            add([_cut_over(s, x0, y0)])
        elif kind in ("C2", "CPx", "CPy"):  # the diagonal b-Q runs from the tile's lower left corner to its upper right one
            add([_cut_square(s, x0, y0)])
        elif kind == "C2a":  # piece 0 = (b, c, Q) = (-28, 16), (20, 16), (12, -32) from the tile's corner: the tile lies inside it
            add([_one_out(s, x0 - 4.0, y0 - 8.0, 8.0)])
        elif kind == "Wd":   # 10 pixels high at the tile, to a vertex 2^24 sub-pixels to its left; behind the cut triangles
            add([(s(x0 + 9.0, y0 - 1.0, 0.4), s(x0 + 9.0, y0 + 9.0, 0.4), s(x0 - 65536.0, y0 + 4.0, 0.4))])
        elif kind in ("KS", "K1", "KA"):
            for q in range(64):
                x, y = x0 + q % 8, y0 + q // 8
                how = {"KS": "wide" if q % 8 == 0 else "cut" if q % 2 else "fast", "K1": "cut" if q == 27 else "fast",
                       "KA": "wide" if q % 8 == 0 else "cut"}[kind]
                add([{"fast": lambda: px(x, y, w), "cut": lambda: dc.cut_pixel_triangle(x, y, width, height),
                      "wide": lambda: dc.wide_sliver(x, y, width, height)}[how]()])
        elif kind == "Sm":   # the quad (b, c, Q, P) = (1, 7), (7, 7), (6, 1), (2, 1) from the tile's corner
            add([_one_out(s, x0 + 4.0, y0 + 4.0, 1.0, SM_W)])
        elif kind == "Un":   # surface_drawn_cases' cut_with_a_wide_piece: piece (b, Q, P) is the lower right of the TARGET and wide
            add([((300.0, 0.0, OUT), (-0.18, -0.18, IN), (-0.09, 0.09, 0.1 + 2e-5))])
        elif kind == "Big":  # 22 triangles off the target between the two that share the tile
            off = [tuple(s(-100.0 - 3.0 * q + dx, -50.0 + dy, w) for dx, dy in ((0.0, 0.0), (0.0, 1.0), (1.0, 0.0))) for q in range(22)]
            low = (s(x0 - 0.5, y0 - 0.5, w), s(x0 - 0.5, y0 + 8.5, w), s(x0 + 8.5, y0 + 8.5, w))
            high = (s(x0 - 0.5, y0 - 0.5, w), s(x0 + 8.5, y0 + 8.5, w), s(x0 + 8.5, y0 - 0.5, w))
            m = poly([low] + off + [high])  # triangle 23's own vertex is index word 69, its corner bytes are 69 to 71
            assert len(m.positions) == 70 and len(m.corners) == 24 and int(m.corners[23].max()) == 69
            meshlets.append(m)
    first.append(len(meshlets))
    n = len(meshlets)
    case = WideCase(name, meshlets, width=width, height=height, view_proj=w_from_z_proj(), entities=[rc.IDENTITY, TINY_W],
                    command_base=BASE, clip_near=True, cull_none=True)
    pk = rc.Packed(case)
    kw, (words, mc, data, vb, vcount, ent, vp, _, _) = pk.args()
    assert mc == n
    from orbit_amd import raster

    # every tile's commands drawn alone; the words name them as the whole list does; the tile's own pixels taken
    vis = np.zeros((height, width), np.uint64)
    for tile, kind in enumerate(kinds):
        k0, k1 = first[tile], first[tile + 1]
        if k0 == k1:
            continue
        x0, y0 = 8 * (tile % tiles_x), 8 * (tile // tiles_x)
        sub = np.concatenate([np.array([k1 - k0], np.uint32), words[1 + 7 * k0:1 + 7 * k1]])
        alone, stats, errors = raster.host_raster_visibility(sub, k1 - k0, data, vb, vcount, ent, vp, width, height, command_base=BASE + k0,
                                                             clear=True, cull_none=True, clip_near=True, wide_guard=True, **kw)
        assert not errors.any() and int(stats["clip_skipped"]) == int(stats["guard_skipped"]) == 0, (name, tile, kind)
        own = alone[y0:y0 + 8, x0:x0 + 8]
        vis[y0:y0 + 8, x0:x0 + 8] = own
        if kind in FULL or kind in ("CPx", "CPy", "Py"):
            assert own.all(), (name, tile, kind)
        if kind in ("O", "T", "U", "TU", "N", "C1", "C2", "C2a", "Wd", "Un", "CPx", "CPy", "Py"):
            assert len(np.unique(own & np.uint64(0xFFFFFFFF))) == 1, (name, tile, kind)
        if kind in ("K", "KS", "K1", "KA"):
            assert len(np.unique(own & np.uint64(0xFFFFFFFF))) == 64, (name, tile, kind)
        if kind == "Big":
            assert sorted(np.unique(own & np.uint64(255))) == [0, 23], (name, tile)
    # by hand: the foreign words, and the Sm word copied outside both pieces
    stale = []
    for tile, kind in enumerate(kinds):
        x0, y0 = 8 * (tile % tiles_x), 8 * (tile // tiles_x)
        pw, ph = min(8, width - x0), min(8, height - y0)
        if kind == "F":
            for q in range(pw * ph):
                y, x = y0 + q // pw, x0 + q % pw
                vis[y, x] = _word(F(0.5), BASE - 1 if (x + y) % 2 else BASE + n, q % 3)
        if kind == "Sm":
            assert vis[y0, x0] == 0 and vis[y0 + 4, x0 + 4] != 0
            vis[y0, x0] = vis[y0 + 4, x0 + 4]
            stale.append((y0, x0))
    count = lambda *which: sum(1 for q in kinds if q in which)  # noqa: E731
    in_target = lambda *which: sum(min(8, width - 8 * (q % tiles_x)) * min(8, height - 8 * (q // tiles_x))  # noqa: E731
                                   for q, kd in enumerate(kinds) if kd in which)
    column = sum(min(8, height - 8 * (q // tiles_x)) for q, kd in enumerate(kinds) if kd == "Px")
    covered = int((vis != 0).sum())
    foreign = in_target("F")
    owned = covered - foreign
    # (the Sm cut's pixel count, the KS / KA tiles' split between cut and wide keys and the C2 pieces' are not stated: sums only)
    assert covered == in_target(*FULL, "CPx", "CPy", "Py", "F", "C2") + column + int(sum(
        (vis[8 * (q // tiles_x):8 * (q // tiles_x) + 8, 8 * (q % tiles_x):8 * (q % tiles_x) + 8] != 0).sum() for q, kd in enumerate(kinds) if kd == "Sm")), name
    drawn = dict(covered_pixels=covered, foreign_pixels=foreign, stale_pixels=len(stale), unsupported_pixels=0,
                 written_pixels=owned - len(stale), degenerate_pixels=in_target("Py"))
    if not count("KS", "KA", "K1", "Sm"):  # whole tiles of one cut or one wide key (Un: both)
        drawn.update(cut_pixels=in_target("C1", "C2", "C2a", "CPx", "CPy", "Un"), wide_pixels=in_target("Wd", "Un"))
    drawn8 = dict(covered_pixels=covered, foreign_pixels=foreign, stale_pixels=len(stale), wide_pixels=0)
    if not count("KS", "KA"):
        unsupported = in_target("Wd", "Un")
        drawn8.update(unsupported_pixels=unsupported, written_pixels=owned - len(stale) - unsupported)
    unshaded = len(stale) + 64 * count("U") + 16 * count("TU")
    frag_stale = 64 * count("T") + 24 * count("TU")
    frag = dict(covered_pixels=covered, foreign_pixels=foreign, unshaded_pixels=unshaded, stale_pixels=frag_stale,
                written_pixels=owned - unshaded - frag_stale, degenerate_pixels=64 * count("N"))
    p = Programme(name, width, height, tuple(kinds), vis, pk, expect=dict(drawn=drawn, drawn8=drawn8, frag=frag), stale=bool(stale),
                  frag_stale=frag_stale > 0, tamper_free=not count("F", "Sm", "T", "U", "TU", "N"))
    p.surface = dc.read(name, vis, pk, BASE, dc.BOTH, expect=drawn, stale=stale)
    p.surface8 = dc.read(name, vis, pk, BASE, dc.CLIP, expect=drawn8, stale=stale)
    p.frag = frag_case(p)
    return p


def frag_case(p):
    """fc.of() over the programme's flags-40 surface case, the T, U, TU and N tiles' records tampered with"""
    clean = fc.of(p.surface)
    tiles_x = (p.width + 7) // 8
    tri, bary = clean.surface["triangle"].copy(), clean.surface["bary"].copy()
    for tile, kind in enumerate(p.kinds):
        x0, y0 = 8 * (tile % tiles_x), 8 * (tile // tiles_x)
        assert kind not in ("T", "U", "TU", "N") or (tri[y0:y0 + 8, x0:x0 + 8, 0] == 0).all()  # written, entity 0
        if kind == "U":
            tri[y0:y0 + 8, x0:x0 + 8] = 0xFFFFFFFF
        if kind == "T":
            tri[y0:y0 + 4, x0:x0 + 8, 2] = clean.vertex_count
            tri[y0 + 4:y0 + 8, x0:x0 + 8, 0] = 1
        if kind == "TU":
            tri[y0 + 3:y0 + 5, x0:x0 + 8] = 0xFFFFFFFF
            tri[y0 + 5:y0 + 6, x0:x0 + 8, 3] = clean.vertex_count
            tri[y0 + 6:y0 + 8, x0:x0 + 8, 0] = 1
        if kind == "N":
            bary[y0:y0 + 4, x0:x0 + 8] = np.nan
            bary[y0 + 4:y0 + 8, x0:x0 + 8] = np.inf
    assert clean.kw["entity_count"] == 2
    return fc.tamper(clean, p.name, p.expect["frag"]["stale_pixels"], surface=dict(triangle=tri, bary=bary))


# 73 x 33: 10 x 5 tiles, column 9 one pixel wide, row 4 one pixel high.  64 x 32: 8 x 4 whole tiles.  The two layouts were found
# by a search over arrangements() — random kinds, one tile changed at a time, kept when the two caps' sets did not shrink —
# under the conditions that the last column holds Px and CPx, the last row Py and CPy, and Un lies in columns 7, 8 of rows 1 to 3
# (the lower right of the target, which its wide piece owns); tests/test_surface_tiles_cpu.py asserts what they hold
MAIN_W, MAIN_H = 73, 33
MAIN_KINDS = parse((
    "TU  N   TU  Sm  E   E   C2  U   Big CPx",
    "C2a F   O   K   C2  KA  Big K1  Un  Px",
    "TU  Wd  C1  O   O   C2  C1  K1  T   Px",
    "C2  KS  Big U   Sm  Sm  K1  O   F   CPx",
    "Py  Py  Py  CPy Py  CPy CPy Py  Py  CPy",
))
SECOND_W, SECOND_H = 64, 32
SECOND_KINDS = parse((
    "K1  N   Wd  U   C2  N   Sm  KA",
    "T   E   C2  O   O   F   C2  KS",
    "O   E   F   Big C2  O   KS  E",
    "O   Wd  F   K   C2  N   O   N",
))


def programmes():
    """-> [Programme]: the 73 x 33 target; the 64 x 32 target; a 7 x 5 target of one partial C2 tile, three waves without one"""
    return [programme("surface_tiles_73x33", MAIN_W, MAIN_H, MAIN_KINDS), programme("surface_tiles_64x32", SECOND_W, SECOND_H, SECOND_KINDS),
            programme("one_slow_tile_7x5", 7, 5, ("C2",))]


AT_ONCE = {"F": "E", "Sm": "C2", "T": "O", "U": "O", "TU": "O", "N": "O", "C2a": "C2", "Un": "C1"}


def tamper_free_programme():
    """A list that a device draws and reads itself (the chain): the main layout without its hand-written kinds — F becomes E,
    Sm becomes C2, T, U, TU and N become O — and without the two kinds whose spill would win most of the target when the
    whole list is drawn at once: C2a becomes C2 and Un becomes C1.  What is left to spill are the C1 pieces, into the tiles
    to their right and below."""
    return programme("surface_tiles_tamper_free", MAIN_W, MAIN_H, tuple(AT_ONCE.get(k, k) for k in MAIN_KINDS))


def arrangements_of(layouts, cap, resident=RESIDENT):
    """layouts: [(kinds, tiles)] or [Programme]"""
    pairs = [(p.kinds, p.tiles) if isinstance(p, Programme) else p for p in layouts]
    return set().union(*(arrangements(k, t, cap, resident) for k, t in pairs))


LAYOUTS = ((MAIN_KINDS, 50), (SECOND_KINDS, 32), (("C2",), 1))
UNCAPPED = ("h:idle_wave",)  # what is left when every wave takes one tile


def old_programmes_as_frag_cases():
    """visibility_tile_cases.programmes() through fc.of(): their S:* and X tiles are unshaded tiles (the surface call left
    them out); read without raster flags, as they were drawn with CLIP_NEAR alone and hold no supported cut key"""
    out = []
    for p in tc.programmes():
        src = dc.read(p.name, p.visibility, p.packed, BASE, 0, stale=list(p.surface.stale))
        out.append(fc.of(src))
    return out


# ------------------------------------------------------------------------------------------------ the natural grid
def natural_programme():
    """tamper_free_programme() for the natural grid: Py becomes CPy as well (a Py triangle is 30 000 pixels wide: on a large
    target it would draw over the other instances)"""
    swap = dict(AT_ONCE, Py="CPy")
    return programme("surface_tiles_natural", MAIN_W, MAIN_H, tuple(swap.get(k, k) for k in MAIN_KINDS))


def instanced(prog, width, height, waves):
    """visibility_tile_cases.instanced for a programme under w_from_z_proj: prog's meshes four times at that function's
    places — the target's top right corner, the left of its middle row, its bottom left and its bottom right corner —, each
    by an entity whose model matrix carries the programme's ndc to the place's: x' = a x + c z, y' = b y + d z with
    a = prog.width / width, b = prog.height / height (a model position is (ndc x * w, ndc y * w, w)); entity 2 i + 1 is the
    same times 2^-100.  -> (rc.Packed, [(name, offset x, offset y, trip of its first tile, trip of its last tile)])"""
    assert prog.width <= width // 4 and prog.height <= height // 4
    tiles_x = (width + 7) // 8
    mid_y = 8 * ((height // 8) // 2)
    places = (("top_right", width - prog.width, 0), ("middle", 8 * ((width // 8) // 2 - prog.width // 8), mid_y),
              ("bottom_left", 0, height - prog.height), ("bottom_right", width - prog.width, height - prog.height))
    entities, meshlets, where = [], [], []
    for i, (name, dx, dy) in enumerate(places):
        assert dx % 8 == 0 and dy % 8 == 0
        m = np.eye(4, dtype=F)
        m[0, 0], m[0, 2] = F(prog.width) / F(width), F(2 * dx + prog.width) / F(width) - F(1)
        m[1, 1], m[1, 2] = F(prog.height) / F(height), F(1) - F(2 * dy + prog.height) / F(height)
        entities += [np.ascontiguousarray(m.T.reshape(16)), np.ascontiguousarray((m * F(2.0) ** F(-100)).T.reshape(16))]
        meshlets += [rc.Meshlet(q.positions, q.corners, 2 * i + q.entity) for q in prog.packed.case.meshlets]
        first = (dy // 8) * tiles_x + dx // 8
        last = ((dy + prog.height - 1) // 8) * tiles_x + (dx + prog.width - 1) // 8
        where.append((name, dx, dy, first // waves, last // waves))
    case = WideCase(f"{prog.name}_four_times", meshlets, width=width, height=height, view_proj=w_from_z_proj(), entities=entities,
                    command_base=BASE, clip_near=True, cull_none=True)
    return rc.Packed(case), where
