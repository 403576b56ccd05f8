"""Inputs that make the two shade calls — orbit_fragments_shade and orbit_fragments_shade_shadowed — run their tile loop MORE
THAN ONCE per wave, with something else in every trip: the tile programmes of visibility_tile_cases and
surface_tile_cases a third time, for the calls that read planes and tables only.  No raster is needed: a programme is a
fragments_shade_cases.Case (and a fragments_shade_shadowed_cases.ShadowCase over it) whose depths, materials, lists and lights
are chosen tile by tile.  As in the sibling files the expected bytes are never stored: the GPU tests' reference is the host
mirror, which tests/test_shade_tiles_cpu.py holds to the numpy restatements; a programme states only the counters known in
closed form (`expect`).

A target is cut into 8 x 8 pixel WAVE TILES, tile = ty * tiles_x + tx, and every tile is given a KIND.  A list is made of
point lights (8 to 31 of the light table) unless said otherwise; one slice is slice 4.
  E        uncovered: every word 0
  L<n>     one slice whose cluster's list has n lights: L0, L1, L63, L64, L65, L129, L256
  L300     a list of 300 and a count word of 300: the walk stops at 256 (ORBIT_SHADE_MAX_WALK)
  S2 S32   2 and 32 distinct slices in the tile, each cluster with a list of its own; by the order in which the staged walk
           takes the slices the lengths are 129, 1 and 65, 1, 64, 3, 129, 0, 63, 2, ...: a long list, then a short one
  B<p>     p = 0, 63, 64, 255: rows 0-3 lie in slice 4, whose list of 256 holds light_count at position p, rows 4-7 in slice
           9 with a clean list: the upper half is stale, the lower half written
  BC       one slice (31) whose list ends one past index_capacity: the index buffer is cut off there.  Stale
  U        material 0xFFFFFFFF on every pixel: unshaded
  MU       rows 0-2 written, rows 3-4 unshaded, rows 5-7 material == material_count: stale
  O        the tile's cluster column lies beyond cluster_count: outside, no list, the slice loop is not entered
  Oz       depths whose slices are 32 and 40, not below cluster_count.z: outside
  D        every D tile's list holds the eight lights 32 to 39; the k-th D tile's pixel (1, 1) lies at light 32 + k, and the
           first D tile's pixel (2, 2) is the view position (fragments_shade_cases.light_case's devices): degenerate
  T        materials 5 and 6, the textured ones
  Un       the sky light and the shadowed directional light 1 in the list: unserved for orbit_fragments_shade; the other
           call serves light 1 and still counts the sky
  Px Py    the one-pixel-wide last column's and the one-pixel-high last row's tile, covered, a list of 5
  PxL65    the partial column with a list of 65: two chunks of the staged walk
and, meant for orbit_fragments_shade_shadowed (the other call shades them as lists that hold a shadowed light: unserved):
  SH       light 1 twice in the list (row 0: a 64 x 64 map of 2s and -1s read at its corners, see shadow_tables; every cascade holds every pixel): two evaluations
  SH0 SH12 light 4 (row 1, a map of -1: no tap is a blocker) resp. light 5 (row 2, a map of 2: all 12 are): the early out
  SHn      light 6 (row 3, whose matrices hold no pixel): no cascade
  SHb      light 7, whose shadow_data_index is shadow_index_base + shadow_count (H1), at position 65 of its list: stale for
           the shadowed call — found by the staging lane of the second chunk in one form, by every lane in the other
  SHm      rows 0-3 in slice 4 with light 1 in the list, rows 4-7 in slice 9 without a shadowed light

With tile_size_px 8 a wave tile is a cluster column; with 16 four wave tiles share one, so the kinds are given per column
(and BC, which needs the last list of the buffer, is left out); with 4 a wave tile holds four columns, each cluster with a
list of its own of the kind's length.  A list's lights are drawn from a generator seeded by the cluster.

Which tiles a wave takes is visibility_tile_cases.assignment's closed formula.  arrangements() works from the kinds and
that formula alone and returns which of ARRANGEMENTS some wave meets; RULES is its table: a name and the kinds of
consecutive trips of one wave.
  long>short  S32>L1          the staged table's rows past the list's length still hold the trip before's
  bad>clean  clean>bad>clean  `bad`, the stale verdict and the latch, then (and before) a tile that is written
  E>L  L>E>L                  the uniform `continue` on an uncovered tile
  O>L  Oz>L                   no lane inside, then a walk
  U>L  MU>full                unshaded and stale lanes, then all 64 written
  partial>full                8 lanes (or 1) store, then all 64
  L300>L0  D>L  Un>L          four chunks then none; non-finite sums and the unserved mark, then a clean tile
  SH>no_shadow>SH             the shadowed call's wave-uniform branch around its cross-lane sum: taken, skipped, taken
  SH0>SH  SHb>SH  SHn>SH  SHm>full   the early out, a stale row, no cascade, a half-shadowed tile, then an evaluated one
  h:idle_wave                 a wave without a tile beside one with
  i:<call>.<counter>          the counter receives a share from two trips of one wave and from two waves: shade.* are
                              OrbitShadeStats of orbit_fragments_shade, shadowed.* of the other call, shadow.* OrbitShadowStats
The layouts of LAYOUTS together hold all of them under a cap of 1 and of 2 workgroups."""
from dataclasses import dataclass, field

import numpy as np

import fragments_shade_cases as fc
import fragments_shade_shadowed_cases as sc
from orbit_amd import layouts as L
from visibility_tile_cases import CAPS, RESIDENT, assignment, natural_target, parse  # noqa: F401

F = np.float32
NONE = fc.NONE
CZ = 32
S0, S1, S_LAST = 4, 9, 31
POINTS = (8, 32)                      # the light table's rows a plain list draws from
D_LIGHTS = tuple(range(32, 40))
SKY, SH_LIGHT, SH0_LIGHT, SH12_LIGHT, SHN_LIGHT, SHB_LIGHT = 2, 1, 4, 5, 6, 7
UNTEXTURED = (0, 1, 2, 3, 4, 7, 8, 9, 10, 11)
MAP_SEED = 3                          # of row 0's map

L_KINDS = ("L0", "L1", "L63", "L64", "L65", "L129", "L256", "L300")
LENGTH = {k: int(k[1:]) for k in L_KINDS}
B_KINDS = ("B0", "B63", "B64", "B255")
SH_KINDS = ("SH", "SH0", "SH12", "SHn", "SHb", "SHm")
PARTIAL = ("Px", "PxL65", "Py")
KINDS = ("E",) + L_KINDS + ("S2", "S32") + B_KINDS + ("BC", "U", "MU", "O", "Oz", "D", "T", "Un") + PARTIAL + SH_KINDS
S2_LENGTHS, S32_LENGTHS = (129, 1), (65, 1, 64, 3, 129, 0, 63, 2)

LNZ = tuple(k for k in L_KINDS if k != "L0")                                  # "L" of the rules: a walk that is not empty
NO_SHADOW = L_KINDS + ("S2", "S32", "T", "D", "Oz", "O")                      # all 64 written, no shadowed light walked
FULL = NO_SHADOW + ("Un", "SH", "SH0", "SH12", "SHn", "SHm")                  # all 64 written by both calls
BAD = B_KINDS + ("BC",)
RULES = (("long>short", (("L256", "L129", "L65"), ("L1", "L63"))), ("S32>L1", ("S32", "L1")), ("bad>clean", (BAD, FULL)),
         ("clean>bad>clean", (FULL, BAD, FULL)), ("E>L", ("E", LNZ)), ("L>E>L", (LNZ, "E", LNZ)), ("O>L", ("O", LNZ)), ("Oz>L", ("Oz", LNZ)),
         ("U>L", ("U", LNZ)), ("MU>full", ("MU", FULL)), ("partial>full", (("Px", "PxL65"), FULL)), ("L300>L0", ("L300", "L0")),
         ("D>L", ("D", LNZ)), ("Un>L", ("Un", LNZ)), ("SH>no_shadow>SH", ("SH", NO_SHADOW, "SH")), ("SH0>SH", (("SH0", "SH12"), "SH")),
         ("SHb>SH", ("SHb", "SH")), ("SHn>SH", ("SHn", "SH")), ("SHm>full", ("SHm", FULL)))

SHADE_COUNTERS = ("covered_pixels", "written_pixels", "unshaded_pixels", "stale_pixels", "outside_pixels", "degenerate_pixels", "textured_pixels",
                  "unserved_pixels")                                                                  # OrbitShadeStats
SHADOW_COUNTERS = ("shadowed_pixels", "no_cascade_pixels", "early_out_pixels", "shadow_evaluations")  # OrbitShadowStats


def tile_counts(kind, area, first_d=False):
    """What one tile of `kind` with `area` pixels inside the target adds to the counters, render_mode 0 -> {"shade": ...,
    "shadowed": ... (OrbitShadeStats of the two calls), "shadow": ... (OrbitShadowStats)}; everything not named is 0"""
    covered = 0 if kind == "E" else area
    unshaded = {"U": area, "MU": 16}.get(kind, 0)
    stale = 32 if kind in B_KINDS else {"BC": 64, "MU": 24}.get(kind, 0)
    shadow_stale = 64 if kind == "SHb" else 0
    walks_shadowed = {"Un": area, "SH": 64, "SH0": 64, "SH12": 64, "SHn": 64, "SHm": 32}.get(kind, 0)  # written pixels that walk a served row
    out = {}
    for call, extra in (("shade", 0), ("shadowed", shadow_stale)):
        out[call] = dict(covered_pixels=covered, unshaded_pixels=unshaded, stale_pixels=stale + extra, written_pixels=covered - unshaded - stale - extra,
                         outside_pixels=area if kind in ("O", "Oz") else 0, textured_pixels=64 if kind == "T" else 0,
                         degenerate_pixels=(2 if first_d else 1) if kind == "D" else 0)
    out["shade"]["unserved_pixels"] = walks_shadowed + (64 if kind == "SHb" else 0)
    out["shadowed"]["unserved_pixels"] = area if kind == "Un" else 0  # the sky
    out["shadow"] = dict(shadowed_pixels=walks_shadowed, no_cascade_pixels=64 if kind == "SHn" else 0,
                         early_out_pixels=64 if kind in ("SH0", "SH12") else 0, shadow_evaluations=walks_shadowed * (2 if kind == "SH" else 1))
    return out


# the counters a kind gives a non-zero share to (render_mode 0), from tile_counts
SHARES = {k: tuple(f"{call}.{c}" for call, row in tile_counts(k, 64).items() for c, v in row.items() if v) for k in KINDS}
COUNTERS = tuple(f"{call}.{c}" for call in ("shade", "shadowed") for c in SHADE_COUNTERS) + tuple(f"shadow.{c}" for c in SHADOW_COUNTERS)
assert {c for v in SHARES.values() for c in v} == set(COUNTERS)
ARRANGEMENTS = tuple(n for n, _ in RULES) + ("h:idle_wave",) + tuple(f"i:{c}" for c in COUNTERS)


def arrangements(kinds, tiles, cap, resident=RESIDENT):
    """What the assignment of `tiles` tiles of `kinds` to the waves of a grid capped at `cap` workgroups holds, of
    ARRANGEMENTS (the module's docstring); nothing is shaded."""
    assert len(kinds) == tiles
    found = set()
    waves = assignment(tiles, cap, resident)
    if any(not w for w in waves) and any(w for w in waves):
        found.add("h:idle_wave")
    sharing = {c: set() for c in COUNTERS}
    for g, w in enumerate(waves):
        seq = [kinds[t] for t in w]
        for name, pattern in RULES:
            for i in range(len(seq) - len(pattern) + 1):
                if all(k == p if isinstance(p, str) else k in p for k, p in zip(seq[i:], pattern)):
                    found.add(name)
        for c in COUNTERS:
            trips = sum(1 for k in seq if c in SHARES[k])
            if trips:
                sharing[c].add((g, trips > 1))
    for c, waves_of in sharing.items():
        if len(waves_of) > 1 and any(twice for _, twice in waves_of):
            found.add(f"i:{c}")
    return found


# ------------------------------------------------------------------------------------------------ the tables
def make_lights():
    """fragments_shade_cases.make_lights (0 directional, 2 sky, 3 a type that is ignored, points) with the shadowed directional
    lights 1, 4, 5, 6 on rows 0 to 3 and 7 on row 4 = shadow_count"""
    l = fc.make_lights(np.random.default_rng(77), 40)
    for light, row in ((SH_LIGHT, 0), (SH0_LIGHT, 1), (SH12_LIGHT, 2), (SHN_LIGHT, 3), (SHB_LIGHT, 4)):
        l["light_type"][light], l["shadow_data_index"][light], l["inner_radius"][light] = L.LIGHT_TYPE_DIRECTIONAL, sc.BASE + row, 0.3
    return l


def shadow_tables():
    """-> (rows, maps): four rows whose cascades all hold every pixel (row 3: none does) over map 0 (texels of 2 and of -1), 1 (-1) and 2 (2).
    Row 0's world size is 0.02, so its blocker search spreads the 12 taps over 750 times the map: every tap is clamped to a
    corner texel, the corner of the quadrant its rotated offset lies in.  The first 12 Poisson offsets leave no half plane
    empty, so under every rotation two adjacent quadrants hold a tap, and adjacent corners differ: the blocker count of a
    pixel that evaluates row 0 is neither 0 nor 12, whatever its position"""
    held, nothing = [sc.ortho(0.2)] * 4, [sc.ortho(0.2, bx=50.0)] * 4
    rows = sc.rows_of(sc.row(held, world_sizes=(0.02,) * 4, map_indices=(0, 0, 0, 0)), sc.row(held, map_indices=(1, 1, 1, 1)), sc.row(held, map_indices=(2, 2, 2, 2)),
                      sc.row(nothing, map_indices=(0, 1, 2, 0)))
    maps = np.zeros((3, 64, 64), F)
    maps[0] = np.where(np.random.default_rng(MAP_SEED).uniform(0, 1, (64, 64)) < 0.5, F(2.0), F(-1.0))  # a blocker for every z, or for none
    maps[0, 0, 0] = maps[0, 63, 63] = 2.0
    maps[0, 0, 63] = maps[0, 63, 0] = -1.0
    maps[1], maps[2] = -1.0, 2.0
    return rows, maps


def _plain(n):
    return lambda r: r.integers(POINTS[0], POINTS[1], n).tolist()


def _with(before, lights, after=0):
    return lambda r: r.integers(POINTS[0], POINTS[1], before).tolist() + list(lights) + r.integers(POINTS[0], POINTS[1], after).tolist()


def _bad(pos, light_count=40):
    def walk(r):
        out = r.integers(POINTS[0], POINTS[1], 256).tolist()
        out[pos] = light_count
        return out
    return walk


def _sh(r):
    return r.integers(POINTS[0], POINTS[1], 3).tolist() + [SH_LIGHT] + r.integers(POINTS[0], POINTS[1], 2).tolist() + [SH_LIGHT]


# a one-slice kind's list (slice S0; BC: S_LAST)
ONE_SLICE = dict({k: _plain(n) for k, n in LENGTH.items()}, BC=_plain(5), U=_plain(5), MU=_plain(5), O=_plain(5), T=_plain(5), Px=_plain(5),
                 Py=_plain(5), PxL65=_plain(65), D=_with(0, D_LIGHTS, 2), Un=_with(0, (SKY, SH_LIGHT), 3), SH=_sh, SH0=_with(2, (SH0_LIGHT,)),
                 SH12=_with(0, (SH12_LIGHT,), 2), SHn=_with(1, (SHN_LIGHT,), 1), SHb=_with(65, (SHB_LIGHT,), 2))


def lane_slices(kind):
    """-> the slice of each of the tile's 64 lanes (lane = 8 * row + column), or None for an uncovered tile"""
    lane = np.arange(64)
    if kind == "E":
        return None
    if kind == "S2":
        return np.where((lane * 7 + 3) % 2 == 1, S0, S1)
    if kind == "S32":
        return (lane * 7 + 3) % 32
    if kind in B_KINDS or kind == "SHm":
        return np.where(lane < 32, S0, S1)
    if kind == "Oz":
        return np.where((lane // 8) % 2 == 0, 32, 40)
    return np.full(64, S_LAST if kind == "BC" else S0)


def slice_lists(kind, order):
    """-> {slice: a function of a generator that makes the cluster's list} for a tile whose lanes, in the target, meet the
    slices in `order`"""
    if kind == "S2":
        return {s: _plain(S2_LENGTHS[i % 2]) for i, s in enumerate(order)}
    if kind == "S32":
        return {s: _plain(S32_LENGTHS[i % 8]) for i, s in enumerate(order)}
    if kind in B_KINDS:
        return {S0: _bad(int(kind[1:])), S1: _plain(5)}
    if kind == "SHm":
        return {S0: _with(2, (SH_LIGHT,)), S1: _plain(5)}
    if kind == "Oz":
        return {}
    return {order[0]: ONE_SLICE[kind]}


# ------------------------------------------------------------------------------------------------ the programme
@dataclass
class Programme:
    name: str
    width: int
    height: int
    tile: int                       # tile_size_px
    kinds: tuple                    # per wave tile
    case: object = None             # fc.Case: orbit_fragments_shade's inputs
    shadow: object = None           # sc.ShadowCase over it: orbit_fragments_shade_shadowed's
    expect: dict = field(default_factory=dict)   # {"shade", "shadowed", "shadow": {counter: value}}, render_mode 0
    expect8: dict = field(default_factory=dict)  # the same for render_mode 8
    stale_mask: dict = field(default_factory=dict)  # {"shade", "shadowed": (h, w) bool}: the pixels that are stale

    @property
    def tiles(self):
        return ((self.width + 7) // 8) * ((self.height + 7) // 8)

    def stale(self, call):
        return bool(self.stale_mask[call].any())

    def tile_box(self, t):
        tiles_x = (self.width + 7) // 8
        x0, y0 = 8 * (t % tiles_x), 8 * (t // tiles_x)
        return slice(y0, min(y0 + 8, self.height)), slice(x0, min(x0 + 8, self.width))


def programme(oracle, name, width, height, tile, kinds, cluster_count=None, seed=1):
    tiles_x, tiles_y = (width + 7) // 8, (height + 7) // 8
    assert len(kinds) == tiles_x * tiles_y and set(kinds) <= set(KINDS), name
    zs, zb = fc.grid(oracle)
    cx, cy, cz = cluster_count or (-(-width // tile), -(-height // tile), CZ)
    assert cz == CZ
    depth = np.zeros((height, width), F)
    lists, walked, bc_clusters = {}, set(), []
    for t, kind in enumerate(kinds):
        x0, y0 = 8 * (t % tiles_x), 8 * (t // tiles_x)
        pw, ph = min(8, width - x0), min(8, height - y0)
        assert pw == ph == 8 or kind in PARTIAL + L_KINDS + ("E", "O"), (name, t, kind)
        assert (kind not in ("Px", "PxL65") or pw == 1) and (kind != "Py" or ph == 1), (name, t, kind)
        sl = lane_slices(kind)
        if sl is None:
            continue
        sl = sl.reshape(8, 8)[:ph, :pw]
        depth[y0:y0 + ph, x0:x0 + pw] = np.array([fc.depth_of_slice(zs, zb, int(s)) for s in sl.reshape(-1)], F).reshape(ph, pw)
        order = list(dict.fromkeys(int(s) for s in sl.reshape(-1)))
        columns = sorted({((x0 + dx) // tile, (y0 + dy) // tile) for dy in range(ph) for dx in range(pw)})
        assert (kind == "O") == any(tx >= cx or ty >= cy for tx, ty in columns), (name, t, kind)
        for s, make in slice_lists(kind, order).items():
            for tx, ty in columns:
                if tx >= cx or ty >= cy:
                    continue
                c = tx + ty * cx + s * cx * cy
                walk = make(np.random.default_rng([seed, c]))
                assert lists.setdefault(c, walk) == walk, (name, t, kind)  # (tile_size_px 16: the column's four wave tiles agree)
                walked.add(c)
                if kind == "BC":
                    bc_clusters.append(c)
    case = fc.Case(name, depth, tile, zs, zb, seed=seed, lists=lists, default_lengths=(0,), cluster_count=(cx, cy, cz), lights=make_lights())
    assert len(case.materials) == 12 and len(case.lights) == 40
    rng = np.random.default_rng(seed + 1)
    case.material = np.asarray(UNTEXTURED, np.uint32)[rng.integers(0, len(UNTEXTURED), (height, width))]
    d_tiles = 0
    for t, kind in enumerate(kinds):
        x0, y0 = 8 * (t % tiles_x), 8 * (t // tiles_x)
        if kind == "U":
            case.material[y0:y0 + 8, x0:x0 + 8] = NONE
        if kind == "MU":
            case.material[y0 + 3:y0 + 5, x0:x0 + 8], case.material[y0 + 5:y0 + 8, x0:x0 + 8] = NONE, len(case.materials)
        if kind == "T":
            case.material[y0:y0 + 8, x0:x0 + 8] = np.where((np.arange(8)[:, None] + np.arange(8)[None, :]) % 2 == 0, 5, 6)
        if kind == "D":
            assert d_tiles < len(D_LIGHTS), name
            case.lights["position"][D_LIGHTS[d_tiles]] = case.world_pos[y0 + 1, x0 + 1, :3]
            if d_tiles == 0:
                case.view_pos = tuple(float(v) for v in case.world_pos[y0 + 2, x0 + 2, :3])
            d_tiles += 1
    if bc_clusters:  # the index buffer ends one index short of the first BC list's end; nothing else that is walked lies behind
        capacity = int(min(case.image[c, 0] + case.image[c, 1] for c in bc_clusters)) - 1
        assert all(c in bc_clusters or int(case.image[c, 0] + case.image[c, 1]) <= capacity for c in walked), name
        case.index_buffer = case.index_buffer[:4 + 4 * capacity].copy()
    rows, maps = shadow_tables()
    p = Programme(name, width, height, tile, tuple(kinds), case, sc.ShadowCase(case, rows, maps))
    # the closed forms
    for mode, into in ((0, p.expect), (8, p.expect8)):
        total = {"shade": dict.fromkeys(SHADE_COUNTERS, 0), "shadowed": dict.fromkeys(SHADE_COUNTERS, 0), "shadow": dict.fromkeys(SHADOW_COUNTERS, 0)}
        first_d = True
        for t, kind in enumerate(kinds):
            rows_, cols_ = p.tile_box(t)
            area = (rows_.stop - rows_.start) * (cols_.stop - cols_.start)
            for call, row in tile_counts(kind, area, first_d and kind == "D").items():
                for c, v in row.items():
                    total[call][c] += v
            first_d = first_d and kind != "D"
        if mode == 8:  # L7 of mode 8: no sum, no light term; H9: nothing of H but the row check
            for call in ("shade", "shadowed"):
                total[call]["degenerate_pixels"] = total[call]["unserved_pixels"] = 0
            total["shadow"] = dict.fromkeys(SHADOW_COUNTERS, 0)
        into.update(total)
    for call in ("shade", "shadowed"):
        mask = np.zeros((height, width), bool)
        for t, kind in enumerate(kinds):
            rows_, cols_ = p.tile_box(t)
            y0, x0 = rows_.start, cols_.start
            if kind in B_KINDS:
                mask[y0:y0 + 4, x0:x0 + 8] = True
            if kind == "MU":
                mask[y0 + 5:y0 + 8, x0:x0 + 8] = True
            if kind == "BC" or (kind == "SHb" and call == "shadowed"):
                mask[rows_, cols_] = True
        p.stale_mask[call] = mask
    return p


# The layouts.  73 x 33: 10 x 5 wave tiles, column 9 one pixel wide, row 4 one pixel high; under a cap of 1 wave g takes tiles g,
# g + 4, ..., under a cap of 2 g, g + 8, ...  Both were found by a search over arrangements() — random kinds, one tile changed at a
# time, kept when the number of arrangements held under the two caps did not shrink — under the conditions that the last column holds
# Px and PxL65, the last row Py, that every S32 tile lies in a tile row above every BC tile (BC's list must be the last one walked)
# and that no layout holds more than eight D tiles; tests/test_shade_tiles_cpu.py asserts what they hold.
MAIN_W, MAIN_H = 73, 33
MAIN_KINDS = parse((
    "Un    SH12  L256  L63   S32   SH    SH    SH0   L1    PxL65",
    "SHn   SHb   L1    L300  BC    SH    Oz    SHn   L1    Px",
    "L1    SH    Oz    SHm   L1    SHn   U     Oz    E     Px",
    "SHn   SH12  L65   SH    L1    D     L300  L63   Oz    PxL65",
    "Py    Py    Py    Py    Py    Py    Py    Py    Py    Py",
))
SHADOW_KINDS = parse((
    "MU    L65   L256  T     D     SHb   L256  Un    T     Px",
    "SHb   L300  SH    SH    L300  B63   S2    D     L0    PxL65",
    "E     L1    L0    Un    B64   Un    L0    D     D     Px",
    "B0    B255  Oz    L65   U     T     L300  SH0   L129  PxL65",
    "Py    Py    Py    Py    Py    Py    Py    Py    Py    Py",
))
# 64 x 32 with tile_size_px 16: 8 x 4 wave tiles, 4 x 2 cluster columns of four wave tiles each, chosen by hand
SECOND_W, SECOND_H = 64, 32
SECOND_COLUMNS = parse((
    "L256 L1  S32 B63",
    "E    SH  MU  L65",
))
# 72 x 16 under cluster_count (8, 2): 9 x 2 wave tiles, the last column beyond the image.  With tile_size_px 8 a column beyond the
# image of the 73 x 33 target could only be its partial one, whose tiles are wanted with lists
STRIP_W, STRIP_H = 72, 16
STRIP_KINDS = parse((
    "L1  L64 L0  L63 L65 SH  L1  L129 O",
    "L63 T   L1  L1  Oz  L0  L64 L1   O",
))


def column_kinds(columns, tiles_x=8, tiles_y=4, per=2):
    """the wave tiles' kinds of a layout given per cluster column of per x per wave tiles"""
    return tuple(columns[(ty // per) * (tiles_x // per) + tx // per] for ty in range(tiles_y) for tx in range(tiles_x))


SECOND_KINDS = column_kinds(SECOND_COLUMNS)
LAYOUTS = ((MAIN_KINDS, 50), (SHADOW_KINDS, 50), (SECOND_KINDS, 32), (STRIP_KINDS, 18), (("L65",), 1))
UNCAPPED = ("h:idle_wave",)  # what is left when every wave takes one tile


def programmes(oracle):
    """-> [Programme]: the two 73 x 33 layouts with tile_size_px 8; the 64 x 32 one with 16; the first 73 x 33 layout again with 4;
    the 72 x 16 strip; a 7 x 5 target of one tile, three waves without one"""
    return [programme(oracle, "shade_tiles_73x33", MAIN_W, MAIN_H, 8, MAIN_KINDS, seed=1),
            programme(oracle, "shade_tiles_shadow_73x33", MAIN_W, MAIN_H, 8, SHADOW_KINDS, seed=2),
            programme(oracle, "shade_tiles_64x32_tile16", SECOND_W, SECOND_H, 16, SECOND_KINDS, seed=3),
            programme(oracle, "shade_tiles_73x33_tile4", MAIN_W, MAIN_H, 4, MAIN_KINDS, seed=4),
            programme(oracle, "shade_tiles_strip_72x16", STRIP_W, STRIP_H, 8, STRIP_KINDS, cluster_count=(8, 2, CZ), seed=5),
            programme(oracle, "one_tile_7x5", 7, 5, 8, ("L65",), seed=6)]


def arrangements_of(layouts, cap, resident=RESIDENT):
    return set().union(*(arrangements(k, t, cap, resident) for k, t in layouts))


# what has no place in a list that a whole frame could produce: nothing stale, nothing tampered with
TAMPER_FREE = dict({k: "L64" for k in B_KINDS}, BC="L1", MU="U", SHb="SH")


def tamper_free_programme(oracle, seed=7):
    """The first layout without its stale kinds, for the chain on the device: B<p> becomes L64, BC L1, MU U and SHb SH.  With the
    first programme's seed (1) it has that programme's planes, tables and view position, and other lists where the kinds differ"""
    return programme(oracle, "shade_tiles_tamper_free", MAIN_W, MAIN_H, 8, tuple(TAMPER_FREE.get(k, k) for k in MAIN_KINDS), seed=seed)


# ------------------------------------------------------------------------------------------------ the natural grid
def natural_programme(oracle):
    """The first 73 x 33 layout without BC, whose list must be the last of the whole index buffer (it becomes L1)"""
    return programme(oracle, "shade_tiles_natural", MAIN_W, MAIN_H, 8, tuple("L1" if k == "BC" else k for k in MAIN_KINDS), seed=8)


def instanced(prog, width, height, waves):
    """prog four or five times on a width x height target that is uncovered everywhere else, at visibility_tile_cases.instanced's places:
    the target's top right corner — the first trip, the partial column —, the left of its middle row — a middle trip —, its
    bottom left corner — the partial row — and its bottom right corner, the last tile of the last trip.  The planes are
    copied, the (offset, count) pairs of the programme's clusters are copied to the clusters of the place (the index buffer is
    the programme's own), every other cluster's list is empty.
    -> (fc.Case, sc.ShadowCase, [(name, offset x, offset y, trip of its first tile, trip of its last tile)])"""
    assert prog.tile == 8 and prog.width <= width // 4 and prog.height <= height // 4 and prog.width % 8 == width % 8 and prog.height % 8 == height % 8
    tiles_x = (width + 7) // 8
    mid_y = 8 * ((height // 8) // 2)
    places = (("top_right", width - prog.width, 0), ("middle", 8 * ((width // 8) // 2 - prog.width // 8), mid_y),
              ("bottom_left", 0, height - prog.height), ("bottom_right", width - prog.width, height - prog.height))
    # and, where it fits, a fifth time one trip behind the first: tile for tile on the waves that took the top right copy, so
    # that every wave there meets the same kind in two trips
    ry, c = divmod((width - prog.width) // 8 + waves, tiles_x)
    box = lambda dx, dy: (dx, dy, dx + prog.width, dy + prog.height)  # noqa: E731
    apart = lambda a, b: a[2] <= b[0] or b[2] <= a[0] or a[3] <= b[1] or b[3] <= a[1]  # noqa: E731
    if c + (prog.width + 7) // 8 <= tiles_x and 8 * ry + prog.height <= height and all(apart(box(8 * c, 8 * ry), box(dx, dy)) for _, dx, dy in places):
        places += (("same_waves", 8 * c, 8 * ry),)
    src = prog.case
    big = src.copy(f"{prog.name}_several_times")
    big.visibility = np.zeros((height, width), np.uint64)
    big.world_pos, big.normal = np.zeros((height, width, 4), F), np.zeros((height, width, 3), F)
    big.material = np.zeros((height, width), np.uint32)
    cx, cy, cz = -(-width // 8), -(-height // 8), CZ
    big.cluster_count = (cx, cy, cz)
    image = np.zeros((cz, cy, cx, 2), np.uint32)
    pcx, pcy, _ = src.cluster_count
    small = src.image.reshape(cz, pcy, pcx, 2)
    where = []
    for name, dx, dy in places:
        assert dx % 8 == 0 and dy % 8 == 0
        rows, cols = slice(dy, dy + prog.height), slice(dx, dx + prog.width)
        big.visibility[rows, cols], big.world_pos[rows, cols], big.normal[rows, cols] = src.visibility, src.world_pos, src.normal
        big.material[rows, cols] = src.material
        image[:, dy // 8:dy // 8 + pcy, dx // 8:dx // 8 + pcx] = small
        first = (dy // 8) * tiles_x + dx // 8
        last = ((dy + prog.height - 1) // 8) * tiles_x + (dx + prog.width - 1) // 8
        where.append((name, dx, dy, first // waves, last // waves))
    big.image = np.ascontiguousarray(image.reshape(-1, 2))
    return big, sc.ShadowCase(big, prog.shadow.rows, prog.shadow.maps), where
